"""Designed cases for the posed-depth-frames front end (csrc/frames.hip), each with one line saying which branch it exists
for.  A case is a dict: depth (uint16 or float32 [F, H, W]), pose (f64 [F, 4, 4]), intr ([4] or [F, 4]), colour (uint8
[F, H, W, 3] or absent) and kw (frames_to_points' keyword arguments).  tests/test_frames_cases_cpu.py holds the kill matrix
against tests/frames_mutants.py; tests/test_frames_gpu.py runs every case through the C ABI."""
import numpy as np

BLOCK_PIXELS = 1024                       # pbn_frames_block_pixels(): asserted where the library is at hand
INTR = (57.5, 58.25, 31.25, 23.5)


def _rotation(rng):
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q


def _poses(rng, n, spread=2.0):
    pose = np.tile(np.eye(4), (n, 1, 1))
    for f in range(n):
        pose[f, :3, :3] = _rotation(rng)
        pose[f, :3, 3] = rng.uniform(-spread, spread, 3)
    return pose


def _depth(rng, shape, holes=0.0, lo=400, hi=6000):
    d = rng.integers(lo, hi, shape).astype(np.uint16)
    d[rng.random(shape) < holes] = 0
    return d


def _colour(rng, shape):
    return rng.integers(0, 256, tuple(shape) + (3,)).astype(np.uint8)


def _random(seed, shape, holes=0.2, colour=True, per_frame_intr=False, **kw):
    rng = np.random.default_rng(seed)
    intr = np.asarray(INTR, np.float64)
    if per_frame_intr:
        intr = intr[None] * rng.uniform(0.8, 1.25, (shape[0], 4))
    case = {"depth": _depth(rng, shape, holes), "pose": _poses(rng, shape[0]), "intr": intr, "kw": kw}
    if colour:
        case["colour"] = _colour(rng, shape)
    return case


def _with(case, **changes):
    out = dict(case)
    out.update(changes)
    return out


def _skip(seed, which):
    case = _random(seed, (4, 5, 9), holes=0.1)
    pose = case["pose"].copy()
    for i, f in enumerate(which):
        pose[f, i % 3, (i + f) % 4] = (-np.inf, np.nan, np.inf)[i % 3]         # ScanNet's lost frames are all -inf
    if len(which) == 1:
        pose[which[0], :, :] = -np.inf
    return _with(case, pose=pose)


def _stride(seed, stride):
    """H and W no multiples of the stride; one full-resolution column jumps, which only a stride-1 neighbour test sees."""
    case = _random(seed, (2, 7, 11), holes=0.0, stride=stride, edge=0.1)
    depth = np.full((2, 7, 11), 1000, np.uint16)
    depth[:, :, stride + 1] = 2000                                               # a neighbour of the sampled column `stride`
    depth[1, 2 * stride - 1, :] = 2000                                           # and a row, above a sampled row
    return _with(case, depth=depth)


def _edge_borders():
    """A smooth image whose corners and border mid-points jump: a border pixel is an edge by its inside neighbours only."""
    case = _random(21, (1, 8, 8), holes=0.0, edge=0.05)
    depth = np.full((1, 8, 8), 1500, np.uint16)
    for v, u in ((0, 0), (0, 7), (7, 0), (7, 7), (0, 4), (7, 3), (3, 0), (4, 7)):
        depth[0, v, u] = 1700
    return _with(case, depth=depth)


def _edge_ratio():
    """|zn - z| = 0.06 lies between edge * z = 0.058 and edge * zn = 0.0615: the nearer pixel is an edge, the farther is not."""
    case = _random(22, (1, 3, 6), holes=0.0, edge=0.058)
    depth = np.full((1, 3, 6), 1000, np.uint16)
    depth[0, :, 3:] = 1060
    return _with(case, depth=depth)


def _max_depth(depth_max):
    case = _random(23, (1, 4, 5), holes=0.0, depth_max=depth_max)
    depth = case["depth"].copy()
    depth[0, 1, 2] = depth[0, 3, 4] = 65535
    return _with(case, depth=depth)


def _f32_specials():
    case = _random(24, (2, 4, 6), holes=0.0, colour=False)
    depth = np.random.default_rng(24).uniform(0.4, 5.0, (2, 4, 6)).astype(np.float32)
    depth[0, 0, :5] = (np.nan, np.inf, -0.0, -1.5, 0.0)
    depth[1, 3, 2:6] = (-np.inf, np.float32(1e-45), np.float32(3.0e38), 2.5)
    return _with(case, depth=depth)


def _translated(seed, t, frames=(0,)):
    case = _random(seed, (2, 5, 7), holes=0.1)
    pose = case["pose"].copy()
    for f in frames:
        pose[f, :3, 3] = t
    return _with(case, pose=pose)


def _bottom_row():
    case = _random(27, (2, 4, 5), holes=0.1)
    pose = case["pose"].copy()
    pose[0, 3, :] = (np.nan, np.inf, -np.inf, np.nan)
    return _with(case, pose=pose)


def _quotient_order():
    """((u - cx) * z) / fx and (u - cx) * (z / fx) differ in the last bit of a float64, which the float32 store hides -- unless
    the translation cancels the sum: identity rotation and t0 = -xc make X exactly 0 for the contract and 1e-16 for the other."""
    fx, fy, cx, cy = INTR
    depth = np.zeros((1, 1, 8), np.uint16)
    u = 7
    d = next(d for d in range(1000, 4000) if ((u - cx) * (d / 1000.0)) / fx != (u - cx) * ((d / 1000.0) / fx))
    depth[0, 0, u] = d
    pose = np.eye(4)[None].copy()
    pose[0, 0, 3] = -(((u - cx) * (d / 1000.0)) / fx)
    return {"depth": depth, "pose": pose, "intr": np.asarray(INTR, np.float64), "kw": {}}


def _only(case, keep):
    depth = np.zeros_like(case["depth"])
    for i in keep:
        depth.reshape(-1)[i] = 1234
    return _with(case, depth=depth)


def _float_twin(case):
    """The same scene as float32 metres: the other depth form on the same branches."""
    return _with(case, depth=(case["depth"].astype(np.float64) / 1000.0).astype(np.float32))


CASES = {}


def _add(name, why, case):
    CASES[name] = dict(case, why=why)


_add("one", "F, H, W of 1: one workgroup, one lane", _random(1, (1, 1, 1), holes=0.0))
_add("f3h5w7", "3 x 5 x 7 with per-frame intrinsics: odd sizes, a short last workgroup per frame", _random(2, (3, 5, 7), per_frame_intr=True))
_add("w63", "W = 63: one lane short of a ballot", _random(3, (2, 3, 63)))
_add("w64", "W = 64: a row is exactly one ballot", _random(4, (2, 3, 64)))
_add("w65", "W = 65: a row spills one lane into the next ballot", _random(5, (2, 3, 65)))
_add("block_minus_1", "H * W one below the workgroup's pixels", _random(6, (2, 33, 31)))
_add("block", "H * W exactly the workgroup's pixels: no short chunk", _random(7, (2, 32, 32)))
_add("block_plus_1", "H * W one above: a second workgroup of one pixel in every frame", _random(8, (2, 25, 41)))
_add("all_valid", "every pixel valid: every ballot full", _random(9, (2, 9, 70), holes=0.0))
_add("none_valid", "no measurement anywhere: N = 0", _only(_random(10, (2, 5, 9)), ()))
_add("last_only", "only the very last pixel valid: every offset but one is zero", _only(_random(11, (2, 5, 67)), (2 * 5 * 67 - 1,)))
_add("skip_first", "the first frame lost (-inf pose)", _skip(12, (0,)))
_add("skip_last", "the last frame lost", _skip(13, (3,)))
_add("skip_middle", "a middle frame lost", _skip(14, (2,)))
_add("skip_every", "every frame lost, each by one non-finite number in another row", _skip(15, (0, 1, 2, 3)))
_add("bottom_row", "a non-finite bottom row is not read: the frame stays", _bottom_row())
_add("stride2", "stride 2, H and W odd; the neighbour test stays at full resolution", _stride(16, 2))
_add("stride3", "stride 3, H and W no multiples of 3", _stride(17, 3))
_add("stride_plain", "stride 2 without an edge test on random depth", _random(18, (2, 7, 11), stride=2))
_add("edge_borders", "an edge pixel on every image border and corner; outside neighbours make no edge", _edge_borders())
_add("edge_holes", "holes next to valid pixels with the edge test on: a hole makes no edge",
     _with(_random(19, (2, 6, 9), holes=0.3, edge=10.0), depth=_depth(np.random.default_rng(19), (2, 6, 9), 0.3, 1000, 1100)))
_add("edge_ratio", "the edge bound is edge * z of the pixel, not of the neighbour", _edge_ratio())
_add("max_cut", "d = 65535 cut by depth_max", _max_depth(10.0))
_add("max_inclusive", "z equal to depth_max stays: the bound is inclusive", _max_depth(65.535))
def _min_depth():
    case = _random(20, (1, 5, 8), holes=0.0, depth_min=3.0, depth_scale=500.0)
    depth = case["depth"].copy()
    depth[0, 2, 3], depth[0, 2, 4] = 1500, 1499                                  # z = 3.0 exactly, and just below
    return _with(case, depth=depth)


_add("min_cut", "depth_min cuts the near pixels, and equal stays", _min_depth())
_add("f32_specials", "float32 depth holding NaN, +-inf, -0.0, 0, negatives, a denormal and a huge value", _f32_specials())
_add("far_translation", "a translation of 1e4 m: the float32 store rounds", _translated(25, (1.0e4, -1.0e4, 12345.678)))
_add("overflow", "a translation past float32: rule (d) drops the frame's points, the other frame stays", _translated(26, (1.0e39, 0.0, 0.0)))
_add("quotient_order", "the product is divided, not the depth: a cancelling translation shows the last float64 bit", _quotient_order())
_add("shared_intr", "one [4] intrinsics for all frames", _random(28, (3, 4, 6)))
_add("per_frame_intr", "the same frames with [F, 4] intrinsics that differ", _random(28, (3, 4, 6), per_frame_intr=True))
_add("no_colour", "no colour image: rgb is absent", _random(29, (2, 5, 9), colour=False))
_add("f32_twin", "float32 metres on a random scene with the edge test", _float_twin(_random(30, (2, 9, 33), edge=0.3)))
_add("big", "4 x 96 x 128 with 30 % holes and the edge test: several workgroups per frame cross the scan",
     _random(31, (4, 96, 128), holes=0.3, edge=0.8))


def arguments(case):
    """frames_ref's and frames_to_points' arguments of a case: (depth, pose, intr, colour, kw)."""
    return case["depth"], case["pose"], case["intr"], case.get("colour"), dict(case.get("kw", {}))
