"""End to end on the GPU for a raw scan filtered by RADIUS: the annotated scan of tests/test_vote_gpu.py (the 3 000-point
room six times over with 4 mm of jitter and 1 % far points) goes through
pbnet_amd.mesh.decode_points(pitch, outlier_radius, outlier_min_pts).  Its front must be the chain thin_points ->
radius_outlier_mask -> radius_raw_index written out by hand and must build no kNN graph over the unfiltered points; its
kept points, given to the plain decode_points, must produce the same bytes; the labels must be the vote over its own
raw_index; SceneCache -> DeviceMerge must take the result; and without the new keywords decode_points is what it was."""
import numpy as np
import pytest
import torch

import vote_cases
import vote_ref
from pbnet_amd import mesh
from test_mesh_e2e_gpu import DEV, _labels, _run

pytestmark = pytest.mark.gpu

K, PITCH, RADIUS, MIN_PTS, RATIO = 16, 0.02, 0.15, 4, 2.0
VOTED = ("sem_label", "ins_label", "votes", "members", "ins_old_id")


def _host(d):
    return {k: v.cpu().numpy() for k, v in d.items()}


def _to(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@pytest.fixture(scope="module")
def scan():
    xyz, sem, ins = vote_cases.room_scan()
    colours = np.random.default_rng(4).integers(0, 256, xyz.shape).astype(np.uint8)
    calls = []
    real = mesh.knn_graph

    def counting(x, *a, **kw):
        calls.append(int(x.shape[0]))
        return real(x, *a, **kw)
    mesh.knn_graph = counting
    try:
        dec = mesh.decode_points((xyz, colours), device=DEV, k=K, pitch=PITCH, outlier_radius=RADIUS, outlier_min_pts=MIN_PTS,
                                 return_kept=True, sem_label=sem, ins_label=ins)
        new_calls = list(calls)
        del calls[:]
        old = mesh.decode_points((xyz, colours), device=DEV, k=K, pitch=PITCH, outlier_ratio=RATIO)
        old_calls = list(calls)
    finally:
        mesh.knn_graph = real
    assert all(t.is_cuda for t in dec.values())
    return (xyz, colours, sem, ins), _host(dec), new_calls, _host(old), old_calls


def test_front_is_the_chain_written_out_by_hand(scan):
    (xyz, colours, _, _), d, _, _, _ = scan
    assert sorted(d) == sorted(("count", "kept_rgb", "kept_xyz", "nl", "raw_index", "rgb", "sup", "xyz") + VOTED)
    th = mesh.thin_points(_to(xyz), _to(colours.astype(np.float32)), PITCH)
    keep = mesh.radius_outlier_mask(th["xyz"], RADIUS, MIN_PTS)
    raw = mesh.radius_raw_index(th["inverse"], keep, th["xyz"], RADIUS)
    for key, want in (("kept_xyz", th["xyz"][keep]), ("kept_rgb", th["rgb"][keep]), ("count", th["count"][keep]),
                      ("raw_index", raw)):
        want = want.cpu().numpy()
        assert d[key].dtype == want.dtype and d[key].shape == want.shape and d[key].tobytes() == want.tobytes(), key
    m, big_m = d["kept_xyz"].shape[0], int(th["xyz"].shape[0])
    far = xyz.min(1) > 9.0                                   # the planted far points: 10 to 30 m away, the room ends at 4 m
    assert far.sum() == int(0.01 * 18000) and 3000 < m <= big_m - far.sum()
    assert np.all(d["raw_index"][far] == -1)                 # alone within the radius: dropped, and nobody speaks for them
    assert (d["raw_index"][~far] >= 0).mean() > 0.95 and d["raw_index"].max() == m - 1
    # a raw point whose cell was dropped in the room is spoken for by a kept neighbour
    dropped_in_room = ~keep.cpu().numpy()[th["inverse"].cpu().numpy()] & ~far
    assert dropped_in_room.any() and (d["raw_index"][dropped_in_room] >= 0).any()


def test_no_graph_over_the_unfiltered_points(scan):
    _, d, new_calls, old, old_calls = scan
    m = d["kept_xyz"].shape[0]
    assert new_calls == [m]                                  # the one graph decode_points builds over the points it keeps
    assert len(old_calls) == 2 and old_calls[1] == old["xyz"].shape[0] and old_calls[0] > old_calls[1]


def test_kept_points_decode_to_the_same_bytes(scan):
    _, d, _, _, _ = scan
    plain = _host(mesh.decode_points((d["kept_xyz"], d["kept_rgb"]), device=DEV, k=K))
    assert sorted(plain) == ["nl", "rgb", "sup", "xyz"]
    for k in plain:
        assert d[k].dtype == plain[k].dtype and d[k].shape == plain[k].shape and d[k].tobytes() == plain[k].tobytes(), k


def test_labels_vote_and_carry_over_the_new_raw_index(scan):
    (_, _, sem, ins), d, _, _, _ = scan
    m = d["xyz"].shape[0]
    want = vote_ref.vote(d["raw_index"], sem, ins, m)
    got = _host(mesh.vote_labels(_to(d["raw_index"]), _to(sem), _to(ins), m=m))
    for k in VOTED:
        src = "old_id" if k == "ins_old_id" else k
        assert d[k].dtype == want[src].dtype and np.array_equal(d[k], want[src]) and np.array_equal(got[src], want[src]), k
    assert np.array_equal(d["members"], np.bincount(d["raw_index"][d["raw_index"] >= 0], minlength=m))
    assert d["ins_old_id"].tolist() == [0, 1, 7]
    raw = d["raw_index"]
    back = mesh.carry_labels(_to(d["sem_label"]), _to(raw)).cpu().numpy()
    assert np.array_equal(back[raw >= 0], d["sem_label"][raw[raw >= 0]]) and np.all(back[raw < 0] == -1)
    sure = (raw >= 0) & (d["votes"] == d["members"])[np.maximum(raw, 0)]
    assert sure.mean() > 0.5 and np.array_equal(back[sure], np.where(sem < 0, -100, sem)[sure])


def test_without_the_new_keywords_the_decode_is_todays(scan):
    (xyz, colours, _, _), _, _, old, _ = scan
    assert sorted(old) == ["count", "nl", "raw_index", "rgb", "sup", "xyz"]
    th = mesh.thin_points(_to(xyz), _to(colours.astype(np.float32)), PITCH)
    idx, d2 = mesh.knn_graph(th["xyz"], k=K)
    keep, _ = mesh.outlier_mask(d2, RATIO)
    assert np.array_equal(old["raw_index"], mesh.raw_index(th["inverse"], keep, idx).cpu().numpy())
    assert np.array_equal(old["count"], th["count"][keep].cpu().numpy())
    plain = _host(mesh.decode_points((th["xyz"][keep].cpu().numpy(), th["rgb"][keep].cpu().numpy()), device=DEV, k=K))
    for k in plain:
        assert old[k].dtype == plain[k].dtype and old[k].tobytes() == plain[k].tobytes(), k
    thinned_only = mesh.decode_points((xyz, colours), device=DEV, k=K, pitch=PITCH)
    assert sorted(thinned_only) == ["count", "nl", "raw_index", "rgb", "sup", "xyz"]
    assert torch.equal(thinned_only["raw_index"], th["inverse"])


def test_the_keywords_are_refused_in_part_or_with_the_ratio(scan):
    (xyz, colours, _, _), _, _, _, _ = scan
    with pytest.raises(ValueError):
        mesh.decode_points((xyz, colours), device=DEV, pitch=PITCH, outlier_radius=RADIUS)
    with pytest.raises(ValueError):
        mesh.decode_points((xyz, colours), device=DEV, pitch=PITCH, outlier_min_pts=MIN_PTS)
    with pytest.raises(ValueError):
        mesh.decode_points((xyz, colours), device=DEV, pitch=PITCH, outlier_radius=RADIUS, outlier_min_pts=MIN_PTS,
                           outlier_ratio=RATIO)


def test_radius_filter_without_thinning(scan):
    (xyz, colours, _, _), _, _, _, _ = scan
    d = _host(mesh.decode_points((xyz[:6000], colours[:6000]), device=DEV, k=K, outlier_radius=RADIUS, outlier_min_pts=2))
    x = _to(xyz[:6000])
    keep = mesh.radius_outlier_mask(x, RADIUS, 2)
    want = mesh.radius_raw_index(torch.arange(6000, dtype=torch.int32, device=DEV), keep, x, RADIUS).cpu().numpy()
    assert np.array_equal(d["raw_index"], want) and d["count"].tolist() == [1] * int(keep.sum().item())
    assert 0 < (want < 0).sum() < 600


def test_scene_cache_and_device_merge_take_the_result(scan):
    _, d, _, _, _ = scan
    m = d["xyz"].shape[0]
    sem, ins = _labels(m)
    scene = {k: v for k, v in d.items() if k not in VOTED}
    batch, (c, s, i, dbg) = _run(dict(scene, sem_label=sem, ins_label=ins))      # SceneCache takes the dict with its extra keys
    assert batch["xyz_original"].shape[0] > 0 and c.shape[0] > 0
    assert torch.isfinite(batch["xyz_original"]).all()
