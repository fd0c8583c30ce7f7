"""End to end on the GPU for an ANNOTATED raw scan: the fixture room's vertices, three times over with 2 mm of jitter and
twenty unannotated points 50 m away, carry one semantic and one instance id per raw point (float64, as the reference's
`.npy` files hold them) through pbnet_amd.mesh.decode_points(pitch, outlier_ratio, sem_label, ins_label).  The labels of
the kept points must be vote_labels over the decode's own raw_index, keep one semantic label per instance, and feed
save_decoded -> scene_io -> SceneCache -> DeviceMerge (a validation and a training batch)."""
import os

import numpy as np
import pytest
import torch

import vote_ref
from pbnet_amd import mesh, scene_io
from pbnet_amd.config import get_config
from pbnet_amd.loader import DeviceMerge, MergeDraws, SceneCache
from test_mesh_e2e_gpu import DEV, _labels

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
K, PITCH, RATIO, N_FAR = 16, 0.03, 2.0, 20
VOTED = ("sem_label", "ins_label", "votes", "members", "ins_old_id")


def _host(d):
    return {k: v.cpu().numpy() for k, v in d.items()}


@pytest.fixture(scope="module")
def scan():
    g = np.load(os.path.join(HERE, "golden", "mesh_room.npz"))
    rng = np.random.default_rng(3)
    v = g["vertices"]
    xyz = np.concatenate([v + rng.normal(scale=0.002, size=v.shape) for _ in range(3)] + [rng.uniform(50.0, 60.0, (N_FAR, 3))])
    colours = np.concatenate([g["colours"]] * 3 + [rng.integers(0, 256, (N_FAR, 3)).astype(np.uint8)])
    sem0, ins0 = _labels(v.shape[0])                         # float64; one semantic label per instance by construction
    sem = np.concatenate([sem0] * 3 + [np.full(N_FAR, -100.0)])
    ins = np.concatenate([ins0] * 3 + [np.full(N_FAR, -100.0)])
    raw = (xyz.astype(np.float32), colours)
    dec = mesh.decode_points(raw, device=DEV, k=K, pitch=PITCH, outlier_ratio=RATIO, sem_label=sem, ins_label=ins)
    assert all(t.is_cuda for t in dec.values())
    return raw, sem.astype(np.int32), ins.astype(np.int32), _host(dec)


def test_labels_are_the_vote_over_the_decodes_own_raw_index(scan):
    _, sem, ins, d = scan
    assert sorted(d) == sorted(("count", "nl", "raw_index", "rgb", "sup", "xyz") + VOTED)
    m = d["xyz"].shape[0]
    to = lambda a: torch.from_numpy(a).to(DEV)
    v = _host(mesh.vote_labels(to(d["raw_index"]), to(sem), to(ins), m=m))
    want = vote_ref.vote(d["raw_index"], sem, ins, m)
    for k in VOTED:
        src = "old_id" if k == "ins_old_id" else k
        assert d[k].dtype == want[src].dtype and d[k].shape == want[src].shape, k
        assert np.array_equal(d[k], v[src]) and np.array_equal(d[k], want[src]), k
    assert np.array_equal(d["members"], np.bincount(d["raw_index"][d["raw_index"] >= 0], minlength=m))
    assert (d["votes"] < d["members"]).any()                 # rows on a label border exist


def test_instances_keep_one_semantic_label_and_dense_ascending_ids(scan):
    _, sem, ins, d = scan
    live = d["ins_label"] >= 0
    n_ins = d["ins_old_id"].shape[0]
    assert n_ins > 10 and np.array_equal(np.unique(d["ins_label"][live]), np.arange(n_ins))
    assert np.all(np.diff(d["ins_old_id"]) > 0) and set(d["ins_old_id"].tolist()) <= set(ins[ins >= 0].tolist())
    assert np.all(d["ins_label"][~live] == -100)
    for i in range(n_ins):
        assert np.unique(d["sem_label"][d["ins_label"] == i]).shape[0] == 1, i
    # every winner is a pair that exists in the raw data
    raw_pairs = set(zip(sem.tolist(), ins.tolist()))
    old = np.where(live, d["ins_old_id"][np.maximum(d["ins_label"], 0)], -100)
    assert set(zip(d["sem_label"].tolist(), old.tolist())) <= raw_pairs


def test_carry_labels_gives_unanimous_rows_their_raw_pair_back(scan):
    _, sem, ins, d = scan
    raw = torch.from_numpy(d["raw_index"]).to(DEV)
    live = d["ins_label"] >= 0
    old = np.where(live, d["ins_old_id"][np.maximum(d["ins_label"], 0)], -100)
    pair = torch.from_numpy(np.stack([d["sem_label"], old], 1)).to(DEV)
    back = mesh.carry_labels(pair, raw, fill=-1).cpu().numpy()
    r = d["raw_index"]
    sure = (r >= 0) & (d["votes"] == d["members"])[np.maximum(r, 0)]
    assert sure.mean() > 0.5
    assert np.array_equal(back[sure, 0], np.where(sem < 0, -100, sem)[sure])
    assert np.array_equal(back[sure, 1], np.where(ins < 0, -100, ins)[sure])
    assert np.all(back[r < 0] == -1) and (r < 0).sum() >= N_FAR


def test_without_pitch_the_labels_pass_through_up_to_compaction():
    g = np.load(os.path.join(HERE, "golden", "mesh_room.npz"))
    sem0, ins0 = _labels(g["vertices"].shape[0])
    d = _host(mesh.decode_points((g["vertices"], g["colours"]), device=DEV, k=K, sem_label=sem0.astype(np.int64),
                                 ins_label=torch.from_numpy(ins0.astype(np.int32))))
    plain = _host(mesh.decode_points((g["vertices"], g["colours"]), device=DEV, k=K))
    assert sorted(d) == ["ins_label", "ins_old_id", "nl", "rgb", "sem_label", "sup", "xyz"]
    for k in plain:
        assert d[k].dtype == plain[k].dtype and d[k].tobytes() == plain[k].tobytes(), k
    assert d["sem_label"].dtype == np.int64 and np.array_equal(d["sem_label"], sem0.astype(np.int64))
    live = ins0 >= 0
    assert np.array_equal(d["ins_label"] >= 0, live) and np.all(d["ins_label"][~live] == -100)
    assert np.array_equal(d["ins_old_id"][d["ins_label"][live]], ins0[live].astype(np.int64))
    assert np.array_equal(d["ins_old_id"], np.unique(ins0[live]).astype(np.int64))


def test_without_the_keywords_the_dict_is_todays(scan):
    raw, _, _, d = scan
    plain = _host(mesh.decode_points(raw, device=DEV, k=K, pitch=PITCH, outlier_ratio=RATIO))
    assert sorted(plain) == ["count", "nl", "raw_index", "rgb", "sup", "xyz"]
    for k in plain:
        assert d[k].dtype == plain[k].dtype and d[k].shape == plain[k].shape and d[k].tobytes() == plain[k].tobytes(), k


def test_refused_labels(scan):
    raw, sem, ins, _ = scan
    with pytest.raises(ValueError):
        mesh.decode_points(raw, device=DEV, k=K, pitch=PITCH, sem_label=np.where(sem == 19, 20, sem), ins_label=ins)
    with pytest.raises(ValueError):
        mesh.decode_points(raw, device=DEV, k=K, pitch=PITCH, sem_label=sem, ins_label=np.where(ins == 3, 1 << 21, ins))


def test_the_training_chain_runs_from_the_saved_scene(scan, tmp_path):
    _, _, _, d = scan
    name = "scan0000_00"
    mesh.save_decoded(str(tmp_path), name, d)
    assert sorted(os.listdir(tmp_path)) == ["%s_%s.npy" % (name, k) for k in ("ins_label", "nl", "rgb", "sem_label", "sup", "xyz")]
    scene = scene_io.load_scene(str(tmp_path), name, with_mesh=False)
    scene["sup"] = np.load(scene_io.scene_path(str(tmp_path), name, "sup"))
    assert scene["sem_label"].dtype == np.float64 and np.array_equal(scene["ins_label"], d["ins_label"])
    cache = SceneCache({name: scene}, DEV, train=[name], val=[name])
    n_ins = d["ins_old_id"].shape[0]
    val = DeviceMerge(cache, get_config(test=True), seed=5).val_merge([0], MergeDraws.draw_val(torch.Generator().manual_seed(5), 1))
    train = DeviceMerge(cache, get_config(batch_size=1), seed=5).train_merge([0])
    for batch, copies in ((val, 3), (train, None)):
        pn = batch["instance_pointnum"].cpu().numpy()
        assert pn.shape[0] > 0 and np.all(pn > 0)
        assert torch.isfinite(batch["inst_info"]).all() and batch["xyz_original"].shape[0] > 0
        if copies:                                           # validation keeps every point: every instance, `copies` times
            assert pn.shape[0] == copies * n_ins
