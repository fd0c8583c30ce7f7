"""End to end on the GPU for decode_points(orient="graph"): on the sheet whose tangent plane passes through the cloud's mean
(tests/orient_ref.py sheet_at_mean) the decode must be the chain point_normals -> orient_normals -> segment_point written
out by hand, leave the sheet with one sign and no more superpoints than before, pass through save_decoded and SceneCache,
and change nothing when the argument is absent; and on a small synthetic room the device's orientation of the device's own
normals must equal the restatement run on those same normals."""
import os

import numpy as np
import pytest
import torch

import orient_ref as R
from pbnet_amd import mesh, synth
from test_mesh_e2e_gpu import DEV, _labels, _run

pytestmark = pytest.mark.gpu

K = 16
SHEET = slice(0, R.SHEET_POINTS)


def _host(d):
    return {k: v.cpu().numpy() for k, v in d.items()}


@pytest.fixture(scope="module")
def sheet():
    xyz = R.sheet_at_mean_points()
    colours = np.random.default_rng(6).integers(0, 256, xyz.shape).astype(np.uint8)
    src = (xyz, colours)
    return src, _host(mesh.decode_points(src, device=DEV, k=K, orient="graph", return_graph=True)), \
        _host(mesh.decode_points(src, device=DEV, k=K, orient=None)), _host(mesh.decode_points(src, device=DEV, k=K))


def test_decode_is_the_chain_written_out_by_hand(sheet):
    _, d, _, _ = sheet
    assert sorted(d) == ["d2", "flipped", "idx", "nl", "rgb", "sup", "tree", "xyz"]
    x, idx = torch.from_numpy(d["xyz"]).to(DEV), torch.from_numpy(d["idx"]).to(DEV)
    o = mesh.orient_normals(mesh.point_normals(x, idx), idx)
    assert d["nl"].tobytes() == o["nl"].cpu().numpy().tobytes()
    assert d["flipped"].dtype == bool and np.array_equal(d["flipped"], o["flipped"].cpu().numpy())
    assert d["tree"].dtype == np.int32 and np.array_equal(d["tree"], o["tree"].cpu().numpy())
    sup = mesh.segment_point(x, o["nl"], mesh.knn_edges(idx))
    assert d["sup"].dtype == np.int64 and np.array_equal(d["sup"], sup.cpu().numpy())


def test_sheet_gets_one_sign_and_no_more_superpoints(sheet):
    _, d, plain, _ = sheet
    before = plain["nl"][SHEET, 2]
    assert 0.1 <= (before > 0).mean() <= 0.9                                 # towards the mean: the signs are noise
    assert np.unique(np.sign(d["nl"][SHEET, 2])).size == 1 and np.all(d["nl"][SHEET, 2] != 0)
    assert np.array_equal(np.abs(d["nl"]).view(np.uint32), np.abs(plain["nl"]).view(np.uint32))   # signs only
    assert np.unique(d["sup"][SHEET]).size <= np.unique(plain["sup"][SHEET]).size
    assert np.unique(d["tree"][SHEET]).size == 1


def test_without_the_argument_nothing_changes(sheet):
    _, _, none, absent = sheet
    assert sorted(none) == sorted(absent) == ["nl", "rgb", "sup", "xyz"]
    for k in none:
        assert none[k].dtype == absent[k].dtype and none[k].tobytes() == absent[k].tobytes(), k
    src = sheet[0]
    with pytest.raises(ValueError):
        mesh.decode_points(src, device=DEV, k=K, orient="viewpoint")
    with pytest.raises(ValueError):
        mesh.decode_points(src, device=DEV, k=K, orient=True)


def test_save_decoded_and_scene_cache_take_the_result(sheet, tmp_path):
    _, d, _, _ = sheet
    scene = {k: v for k, v in d.items() if k not in ("idx", "d2")}
    mesh.save_decoded(str(tmp_path), "scan0000_00", scene)
    assert sorted(os.listdir(tmp_path)) == ["scan0000_00_%s.npy" % k for k in ("nl", "rgb", "sup", "xyz")]
    sem, ins = _labels(d["xyz"].shape[0])
    batch, _ = _run(dict(scene, sem_label=sem, ins_label=ins))               # SceneCache takes the dict with its extra keys
    assert batch["xyz_original"].shape[0] > 0 and torch.isfinite(batch["xyz_original"]).all()


def test_room_orientation_of_the_devices_own_normals_is_the_restatement():
    pts = synth.synth_room(pitch=0.165)["xyz"]
    assert 2000 <= pts.shape[0] <= 4500
    x = torch.from_numpy((pts - pts.mean(0)).astype(np.float32)).to(DEV)
    idx, _ = mesh.knn_graph(x, k=K)
    nl = mesh.point_normals(x, idx)
    got = mesh.orient_normals(nl, idx)
    want = R.orient(nl.cpu().numpy(), idx.cpu().numpy())
    for k in ("nl", "flipped", "tree", "stats"):
        assert got[k].cpu().numpy().tobytes() == want[k].tobytes(), k
    assert want["stats"][0] >= 1 and want["stats"][1] <= pts.shape[0] // 2
