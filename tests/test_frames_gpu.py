"""On the GPU: every designed case of tests/frames_cases.py through the C ABI (pbn_frames_count, one read-back,
pbn_frames_write) is bit for bit tests/frames_ref.py in xyz, rgb, pixel, frame_start, N and status, in both depth forms;
two runs give equal bytes; the _timed entries return the same arrays; frames_to_points wraps the same calls."""
import ctypes

import numpy as np
import pytest
import torch

import frames_cases as C
import frames_ref as R
from pbnet_amd import _native as N, frames

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
DP = ctypes.POINTER(ctypes.c_double)


def _abi(case, timed=False):
    depth, pose, intr, colour, kw = C.arguments(case)
    lib = N.lib()
    n_f, h, w = depth.shape
    d = torch.from_numpy(depth).to(DEV)
    c = None if colour is None else torch.from_numpy(colour).to(DEV)
    pose = np.ascontiguousarray(np.asarray(pose, np.float64).reshape(n_f, 16))
    intr = np.ascontiguousarray(np.broadcast_to(np.asarray(intr, np.float64), (n_f, 4)))
    edge = kw.get("edge")
    stride = kw.get("stride", 1)
    head = (N.ptr(d), int(depth.dtype == np.float32), N.ptr(c), pose.ctypes.data_as(DP), intr.ctypes.data_as(DP), n_f, h, w,
            float(kw.get("depth_scale", 1000.0)), float(kw.get("depth_min", 0.0)), float(kw.get("depth_max", np.inf)), stride,
            0.0 if edge is None else float(edge))
    nbytes = lib.pbn_frames_workspace_bytes(n_f, h, w, stride)
    assert nbytes > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    frame_start = torch.full((n_f + 1,), -7, dtype=torch.int32, device=DEV)
    result = torch.full((2,), -7, dtype=torch.int32, device=DEV)
    tail = (N.ptr(result), N.ptr(ws), ws.numel(), N.current_stream())
    times = (ctypes.c_float * 2)(), (ctypes.c_float * 1)()
    if timed:
        N.check(lib.pbn_frames_count_timed(*head, N.ptr(frame_start), *tail, times[0]), "pbn_frames_count_timed")
    else:
        N.check(lib.pbn_frames_count(*head, N.ptr(frame_start), *tail), "pbn_frames_count")
    status, n = result.tolist()
    xyz = torch.full((n, 3), np.nan, dtype=torch.float32, device=DEV)
    rgb = None if c is None else torch.full((n, 3), np.nan, dtype=torch.float32, device=DEV)
    pixel = torch.full((n,), -7, dtype=torch.int32, device=DEV)
    if timed:
        N.check(lib.pbn_frames_write_timed(*head, n, N.ptr(xyz), N.ptr(rgb), N.ptr(pixel), *tail, times[1]), "pbn_frames_write_timed")
    else:
        N.check(lib.pbn_frames_write(*head, n, N.ptr(xyz), N.ptr(rgb), N.ptr(pixel), *tail), "pbn_frames_write")
    out = {"xyz": xyz.cpu().numpy(), "pixel": pixel.cpu().numpy(), "n": n, "frame_start": frame_start.cpu().numpy()}
    if rgb is not None:
        out["rgb"] = rgb.cpu().numpy()
    assert result.tolist() == [0, n] and status == 0
    return out, [float(v) for t in times for v in t]


def _same(got, want):
    assert sorted(got) == sorted(want)
    for k in want:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.dtype == w.dtype and g.shape == w.shape, k
        assert g.tobytes() == w.tobytes(), k


def _want(case):
    depth, pose, intr, colour, kw = C.arguments(case)
    return R.frames_ref(depth, pose, intr, colour, **kw)


def test_the_workgroup_covers_what_the_cases_assume():
    assert N.lib().pbn_frames_block_pixels() == C.BLOCK_PIXELS


@pytest.mark.parametrize("name", list(C.CASES))
def test_case_is_the_restatement_bit_for_bit(name):
    _same(_abi(C.CASES[name])[0], _want(C.CASES[name]))


@pytest.mark.parametrize("name", ["f3h5w7", "block_plus_1", "edge_borders", "stride3", "max_inclusive", "big"])
def test_float32_metres_on_the_same_cases(name):
    """z = d / 1000 is not a float32, so the float32 image is a scene of its own: restated, not compared with uint16."""
    case = C._float_twin(C.CASES[name])
    _same(_abi(case)[0], _want(case))


@pytest.mark.parametrize("name", ["big", "f32_specials"])
def test_two_runs_and_the_timed_entries_give_the_same_bytes(name):
    first, _ = _abi(C.CASES[name])
    second, _ = _abi(C.CASES[name])
    timed, times = _abi(C.CASES[name], timed=True)
    _same(second, first)
    _same(timed, first)
    assert len(times) == 3 and all(t >= 0.0 for t in times) and sum(times) > 0.0


@pytest.mark.parametrize("name", ["big", "skip_middle", "none_valid", "no_colour"])
def test_frames_to_points_wraps_the_same_calls(name):
    depth, pose, intr, colour, kw = C.arguments(C.CASES[name])
    times = {}
    outs = [frames.frames_to_points(torch.from_numpy(depth).to(DEV), pose, intr, None if colour is None else
                                    torch.from_numpy(colour).to(DEV), times=t, **kw) for t in (None, times)]
    want = _want(C.CASES[name])
    centres, skipped = R.centres_ref(pose)
    for out in outs:
        assert out["shape"] == depth.shape and all(torch.is_tensor(v) and v.is_cuda for k, v in out.items() if k != "shape")
        got = {k: out[k].cpu().numpy() for k in want if k != "n"}
        _same(dict(got, n=int(out["xyz"].shape[0])), want)
        assert out["centres"].cpu().numpy().tobytes() == centres.tobytes()
        assert out["skipped"].cpu().numpy().tobytes() == skipped.tobytes() and out["skipped"].dtype == torch.bool
    assert sorted(times) == sorted(frames.FRAMES_STAGES)


def test_empty_sequences():
    for shape in ((0, 4, 5), (2, 0, 5), (2, 4, 0)):
        out = frames.frames_to_points(torch.zeros(shape, dtype=torch.uint16, device=DEV), np.tile(np.eye(4), (shape[0], 1, 1)),
                                      C.INTR)
        assert out["xyz"].shape == (0, 3) and out["pixel"].shape == (0,)
        assert out["frame_start"].tolist() == [0] * (shape[0] + 1)


def test_write_refuses_to_pass_its_rows():
    """The write pass with fewer rows than the count found writes none beyond them and says so in the status word."""
    case = C.CASES["all_valid"]
    depth, pose, intr, colour, kw = C.arguments(case)
    lib, (n_f, h, w) = N.lib(), depth.shape
    d = torch.from_numpy(depth).to(DEV)
    pose = np.ascontiguousarray(pose.reshape(n_f, 16))
    intr = np.ascontiguousarray(np.broadcast_to(np.asarray(intr, np.float64), (n_f, 4)))
    head = (N.ptr(d), 0, None, pose.ctypes.data_as(DP), intr.ctypes.data_as(DP), n_f, h, w, 1000.0, 0.0, float("inf"), 1, 0.0)
    ws = torch.empty(lib.pbn_frames_workspace_bytes(n_f, h, w, 1), dtype=torch.uint8, device=DEV)
    frame_start = torch.empty(n_f + 1, dtype=torch.int32, device=DEV)
    result = torch.empty(2, dtype=torch.int32, device=DEV)
    tail = (N.ptr(result), N.ptr(ws), ws.numel(), N.current_stream())
    N.check(lib.pbn_frames_count(*head, N.ptr(frame_start), *tail), "pbn_frames_count")
    n = result.tolist()[1]
    assert n == depth.size
    short = 100
    xyz = torch.full((n, 3), 7.0, dtype=torch.float32, device=DEV)
    pixel = torch.full((n,), -7, dtype=torch.int32, device=DEV)
    N.check(lib.pbn_frames_write(*head, short, N.ptr(xyz), None, N.ptr(pixel), *tail), "pbn_frames_write")
    assert result.tolist() == [1, n]
    assert bool((pixel[short:] == -7).all()) and bool((xyz[short:] == 7.0).all())
    assert pixel[:short].tolist() == list(range(short))
    with pytest.raises(RuntimeError, match="frames changed between the two"):
        frames._scan_status("frames_to_points", 1)
