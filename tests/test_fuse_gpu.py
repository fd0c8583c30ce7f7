"""On the GPU: every designed case of tests/fuse_cases.py through the C ABI, stage by stage, is bit for bit tests/fuse_ref.py:
block keys and origin (pbn_fuse_blocks, pbn_fuse_block_keys), the volume (pbn_fuse_integrate) and the surface rows
(pbn_fuse_extract_count, pbn_fuse_extract_write); the hand-built volumes through the extraction alone; two runs and the
_timed entries give the same bytes; fuse_frames wraps the same calls."""
import ctypes

import numpy as np
import pytest
import torch

import frames_ref as R
import fuse_cases as C
import fuse_ref as FR
from pbnet_amd import _native as N, frames

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
DP = ctypes.POINTER(ctypes.c_double)
_REFS = {}


def _want(name):
    if name not in _REFS:
        depth, pose, intr, colour, kw = C.arguments(C.CASES[name])
        _REFS[name] = FR.fuse_ref(depth, pose, intr, colour, **kw)
    return _REFS[name]


def _call(entry, args, timed, n_times, extra=()):
    lib = N.lib()
    if not timed:
        N.check(getattr(lib, entry)(*args), entry)
        return []
    t = (ctypes.c_float * n_times)()
    N.check(getattr(lib, entry + "_timed")(*args, t, *extra), entry + "_timed")
    return [float(v) for v in t]


def _extract(tsdf, weight, rgb, key, origin, voxel, min_weight, timed=False):
    lib, stream, m = N.lib(), N.current_stream(), int(key.shape[0])
    origin = np.ascontiguousarray(origin, np.float64)
    ws = torch.empty(lib.pbn_fuse_extract_workspace_bytes(m), dtype=torch.uint8, device=DEV)
    result = torch.full((2,), -7, dtype=torch.int32, device=DEV)
    times = _call("pbn_fuse_extract_count", (N.ptr(tsdf), N.ptr(weight), N.ptr(key), m, min_weight, N.ptr(result), N.ptr(ws),
                                             ws.numel(), stream), timed, 1)
    status, n = result.tolist()
    assert status == 0
    xyz, nl = (torch.full((n, 3), np.nan, dtype=torch.float32, device=DEV) for _ in range(2))
    out_rgb = None if rgb is None else torch.full((n, 3), np.nan, dtype=torch.float32, device=DEV)
    w = torch.full((n,), -7, dtype=torch.int32, device=DEV)
    vid = torch.full((n,), -7, dtype=torch.int64, device=DEV)
    times += _call("pbn_fuse_extract_write", (N.ptr(tsdf), N.ptr(weight), N.ptr(rgb), N.ptr(key), m, min_weight, float(voxel),
                                              origin.ctypes.data_as(DP), n, N.ptr(xyz), N.ptr(out_rgb), N.ptr(nl), N.ptr(w), N.ptr(vid),
                                              N.ptr(result), N.ptr(ws), ws.numel(), stream), timed, 1)
    assert result.tolist() == [0, n]
    out = {"xyz": xyz.cpu().numpy(), "nl": nl.cpu().numpy(), "weight": w.cpu().numpy(), "voxel_id": vid.cpu().numpy(), "n": n}
    if out_rgb is not None:
        out["rgb"] = out_rgb.cpu().numpy()
    return out, times


def _abi(case, timed=False):
    """The three stages behind pbn_frames_*'s cloud, as fuse_ref's dict."""
    depth, pose, intr, colour, kw = C.arguments(case)
    lib, stream = N.lib(), N.current_stream()
    n_f, h, w = depth.shape
    voxel = float(kw["voxel"])
    trunc = float(kw.get("trunc") or 4.0 * voxel)
    d = torch.from_numpy(depth).to(DEV)
    c = None if colour is None else torch.from_numpy(colour).to(DEV)
    cloud = frames.frames_to_points(d, pose, intr, None, kw.get("depth_scale", 1000.0), kw.get("depth_min", 0.0),
                                    kw.get("depth_max", np.inf), 1, kw.get("edge"))
    xyz, n = cloud["xyz"], int(cloud["xyz"].shape[0])
    ws = torch.empty(lib.pbn_fuse_blocks_workspace_bytes(n), dtype=torch.uint8, device=DEV)
    result = torch.full((8,), -7, dtype=torch.int32, device=DEV)
    times = _call("pbn_fuse_blocks", (N.ptr(xyz), n, voxel, N.ptr(result), N.ptr(ws), ws.numel(), stream), timed, 3)
    head = result.tolist()
    assert head[0] == 0
    m = head[1]
    origin = np.array(head[2:5], np.int32).view(np.float32).astype(np.float64) - 8.0 * voxel if n else np.zeros(3)
    key = torch.full((m,), -7, dtype=torch.int64, device=DEV)
    N.check(lib.pbn_fuse_block_keys(n, m, N.ptr(key), N.ptr(result), N.ptr(ws), ws.numel(), stream), "pbn_fuse_block_keys")
    assert result.tolist()[:2] == [0, m]
    out = {"status": 0, "n_raw": n, "origin": origin, "block_key": key.cpu().numpy()}
    tsdf = torch.full((m, 512), np.nan, dtype=torch.float32, device=DEV)
    weight = torch.full((m, 512), -7, dtype=torch.int32, device=DEV)
    rgb = None if c is None else torch.full((m, 512, 3), np.nan, dtype=torch.float32, device=DEV)
    pose16 = np.ascontiguousarray(np.asarray(pose, np.float64).reshape(n_f, 16))
    intr4 = np.ascontiguousarray(np.broadcast_to(np.asarray(intr, np.float64), (n_f, 4)))
    origin_c = np.ascontiguousarray(origin, np.float64)
    edge = kw.get("edge")
    ws = torch.empty(lib.pbn_fuse_integrate_workspace_bytes(n_f), dtype=torch.uint8, device=DEV)
    stats = (ctypes.c_uint64 * 2)()
    times += _call("pbn_fuse_integrate", (N.ptr(d), int(depth.dtype == np.float32), N.ptr(c), pose16.ctypes.data_as(DP),
                                          intr4.ctypes.data_as(DP), n_f, h, w, float(kw.get("depth_scale", 1000.0)),
                                          float(kw.get("depth_min", 0.0)), float(kw.get("depth_max", np.inf)),
                                          0.0 if edge is None else float(edge), voxel, trunc, origin_c.ctypes.data_as(DP), N.ptr(key), m,
                                          N.ptr(tsdf), N.ptr(weight), N.ptr(rgb), N.ptr(ws), ws.numel(), stream), timed, 1, (stats,))
    out.update(tsdf=tsdf.cpu().numpy(), vol_weight=weight.cpu().numpy(), vol_rgb=None if rgb is None else rgb.cpu().numpy())
    rows, t = _extract(tsdf, weight, rgb, key, origin, voxel, int(kw.get("min_weight", 1)), timed)
    out.update(rows)
    return out, times + t, (int(stats[0]), int(stats[1]))


def _same(got, want):
    assert sorted(got) == sorted(want)
    for k in want:
        if want[k] is None:
            assert got[k] is None, k
            continue
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.dtype == w.dtype and g.shape == w.shape, (k, g.dtype, w.dtype, g.shape, w.shape)
        if g.tobytes() != w.tobytes():
            bad = np.flatnonzero(g.reshape(-1) != w.reshape(-1))
            raise AssertionError("%s differs at %d of %d entries, first %s: %r != %r" %
                                 (k, bad.size, g.size, bad[:1], g.reshape(-1)[bad[:1]], w.reshape(-1)[bad[:1]]))


@pytest.mark.parametrize("name", list(C.CASES))
def test_case_is_the_restatement_stage_by_stage(name):
    _same(_abi(C.CASES[name])[0], _want(name))


@pytest.mark.parametrize("name", list(C.VOLUMES))
def test_volume_is_the_restatement(name):
    v = C.VOLUMES[name]
    dev = [None if v[k] is None else torch.from_numpy(v[k]).to(DEV) for k in ("tsdf", "weight", "rgb", "block_key")]
    got, _ = _extract(dev[0], dev[1], dev[2], dev[3], v["origin"], v["voxel"], v["min_weight"])
    _same(got, FR.extract_ref(v["tsdf"], v["weight"], v["rgb"], v["block_key"], v["origin"], v["voxel"], v["min_weight"]))


@pytest.mark.parametrize("name", ["room", "wall_y"])
def test_two_runs_and_the_timed_entries_give_the_same_bytes(name):
    first, _, _ = _abi(C.CASES[name])
    second, _, _ = _abi(C.CASES[name])
    timed, times, stats = _abi(C.CASES[name], timed=True)
    _same(second, first)
    _same(timed, first)
    assert len(times) == 6 and all(t >= 0.0 for t in times) and sum(times) > 0.0
    depth = C.CASES[name]["depth"]
    live = int(np.isfinite(C.CASES[name]["pose"][:, :3, :]).all(axis=(1, 2)).sum())
    m = first["block_key"].shape[0]
    assert 0 < stats[0] <= m * live and first["vol_weight"].sum() <= stats[1] <= stats[0] * 512
    assert depth.shape[0] >= live


@pytest.mark.parametrize("name", ["room", "all_lost", "weights_colour", "wall_f32"])
def test_fuse_frames_wraps_the_same_calls(name):
    depth, pose, intr, colour, kw = C.arguments(C.CASES[name])
    want = _want(name)
    times = {}
    for t in (None, times):
        out = frames.fuse_frames(torch.from_numpy(depth).to(DEV), pose, intr, None if colour is None else torch.from_numpy(colour).to(DEV),
                                 return_volume=True, times=t, **kw)
        assert out["shape"] == depth.shape and out["n_blocks"] == want["block_key"].shape[0]
        assert out["origin"].tobytes() == np.asarray(want["origin"], np.float64).tobytes()
        for k in ("xyz", "nl", "weight", "voxel_id", "block_key", "tsdf", "vol_weight") + (("rgb", "vol_rgb") if colour is not None else ()):
            assert out[k].is_cuda and out[k].cpu().numpy().tobytes() == want[k].tobytes(), k
        assert ("rgb" in out) == (colour is not None) and (out["vol_rgb"] is None) == (colour is None)
        centres, skipped = R.centres_ref(pose)
        assert out["centres"].cpu().numpy().tobytes() == centres.tobytes() and out["skipped"].cpu().numpy().tobytes() == skipped.tobytes()
    assert set(frames.FUSE_STAGES) | set(frames.FRAMES_STAGES) | {"stats"} == set(times)


def test_write_refuses_to_pass_its_rows():
    """The write pass with fewer rows than the count found writes none beyond them and says so in the status word; the key
    copy refuses a block count that is not the one it found."""
    v = C.VOLUMES["random"]
    lib, stream = N.lib(), N.current_stream()
    tsdf, weight, key = (torch.from_numpy(v[k]).to(DEV) for k in ("tsdf", "weight", "block_key"))
    m = int(key.shape[0])
    origin = np.ascontiguousarray(v["origin"], np.float64)
    ws = torch.empty(lib.pbn_fuse_extract_workspace_bytes(m), dtype=torch.uint8, device=DEV)
    result = torch.empty(2, dtype=torch.int32, device=DEV)
    N.check(lib.pbn_fuse_extract_count(N.ptr(tsdf), N.ptr(weight), N.ptr(key), m, 1, N.ptr(result), N.ptr(ws), ws.numel(), stream), "count")
    n = result.tolist()[1]
    short = 100
    assert n > short
    xyz, nl = (torch.full((n, 3), 7.0, dtype=torch.float32, device=DEV) for _ in range(2))
    w = torch.full((n,), -7, dtype=torch.int32, device=DEV)
    vid = torch.full((n,), -7, dtype=torch.int64, device=DEV)
    N.check(lib.pbn_fuse_extract_write(N.ptr(tsdf), N.ptr(weight), None, N.ptr(key), m, 1, v["voxel"], origin.ctypes.data_as(DP), short,
                                       N.ptr(xyz), None, N.ptr(nl), N.ptr(w), N.ptr(vid), N.ptr(result), N.ptr(ws), ws.numel(), stream),
            "write")
    assert result.tolist() == [frames.FUSE_ROWS, n]
    assert bool((vid[short:] == -7).all()) and bool((xyz[short:] == 7.0).all()) and bool((vid[:short] >= 0).all())
    with pytest.raises(RuntimeError, match="inputs changed between the two"):
        frames._fuse_status("fuse_frames", frames.FUSE_ROWS, 0.02)
    # the key copy
    pts = torch.tensor([[0.0, 0.0, 1.0]], device=DEV)
    ws = torch.empty(lib.pbn_fuse_blocks_workspace_bytes(1), dtype=torch.uint8, device=DEV)
    res8 = torch.empty(8, dtype=torch.int32, device=DEV)
    N.check(lib.pbn_fuse_blocks(N.ptr(pts), 1, 0.05, N.ptr(res8), N.ptr(ws), ws.numel(), stream), "blocks")
    assert res8.tolist()[:2] == [0, 27]
    out = torch.full((27,), -7, dtype=torch.int64, device=DEV)
    N.check(lib.pbn_fuse_block_keys(1, 26, N.ptr(out), N.ptr(res8), N.ptr(ws), ws.numel(), stream), "keys")
    assert res8.tolist()[0] == frames.FUSE_ROWS and bool((out == -7).all())


def test_status_bits_of_the_allocation():
    lib, stream = N.lib(), N.current_stream()
    # B = 1: the second point's block is its x + 1; block 2^21 - 3 is the last whose upper neighbour stays below 2^21 - 1
    for pts, voxel, bit in (([[0.0, 0.0, 1.0], [np.nan, 0.0, 0.0]], 0.05, 1), ([[0.0, 0.0, 0.0], [1.0e6, 0.0, 0.0]], 0.05, 2),
                            ([[0.0, 0.0, 0.0], [2097149.0, 0.0, 0.0]], 0.125, 2), ([[0.0, 0.0, 0.0], [2097148.0, 0.0, 0.0]], 0.125, 0)):
        xyz = torch.tensor(pts, dtype=torch.float32, device=DEV)
        ws = torch.empty(lib.pbn_fuse_blocks_workspace_bytes(2), dtype=torch.uint8, device=DEV)
        res8 = torch.empty(8, dtype=torch.int32, device=DEV)
        N.check(lib.pbn_fuse_blocks(N.ptr(xyz), 2, voxel, N.ptr(res8), N.ptr(ws), ws.numel(), stream), "blocks")
        assert res8.tolist()[0] == bit
        want = FR.blocks_ref(np.asarray(pts, np.float32), voxel)
        assert want[0] == bit
        if bit:
            with pytest.raises(ValueError):
                frames._fuse_status("fuse_frames", bit, voxel)
        else:
            assert res8.tolist()[1] == want[2].shape[0] == 54 and FR.unpack(want[2]).max() == (1 << 21) - 2
