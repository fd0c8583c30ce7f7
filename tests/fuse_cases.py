"""Designed cases for depth-frame fusion (csrc/tsdf.hip), each with one line saying which branch it exists for.  A case is a
dict: depth (uint16 or float32 [F, H, W]), pose (f64 [F, 4, 4]), intr ([4] or [F, 4]), colour (uint8 [F, H, W, 3] or absent)
and kw (fuse_ref's keyword arguments).  VOLUMES are hand-built volumes for the extraction alone: block_key, tsdf, weight,
rgb (or None), origin, voxel, min_weight.  tests/test_fuse_cases_cpu.py holds the kill matrix against tests/fuse_mutants.py;
tests/test_fuse_gpu.py runs every case and volume through the C ABI.

The exact cases share one construction: voxel = 1/16, so B = 1/2, and a cloud whose minimum is (0, 0, 1) puts the origin at
(-1/2, -1/2, 1/2) and every voxel centre on an odd multiple of 1/32.  With fx = 16.5, an identity pose and zc = 33/32 (the
first layer behind z = 1) uf = n - 7.5 + cx exactly, n the voxel's index along x: every such voxel projects onto a tie."""
import numpy as np

import frames_ref as R

VOXEL = 0.0625
TIE_INTR = (16.5, 16.5, 8.0, 8.0)


def _eye(n):
    return np.tile(np.eye(4), (n, 1, 1))


def _single(cx=8.0, cy=8.0, w=9, h=9, d=1000, frames=1, **kw):
    """One measured pixel at (cx, cy) with z = 1: the cloud is the one point (0, 0, 1)."""
    depth = np.zeros((frames, h, w), np.uint16)
    depth[:, int(cy), int(cx)] = d
    kw.setdefault("voxel", VOXEL)
    return {"depth": depth, "pose": _eye(frames), "intr": np.array((16.5, 16.5, cx, cy)), "kw": kw}


def _with(case, **changes):
    out = dict(case)
    out.update(changes)
    return out


def _colour(case, seed):
    return _with(case, colour=np.random.default_rng(seed).integers(0, 256, case["depth"].shape + (3,)).astype(np.uint8))


def _f32(case, scale=1000.0):
    return _with(case, depth=(case["depth"].astype(np.float64) / scale).astype(np.float32))


def _wall(axis, seed=0, h=6, w=8, frames=1, **kw):
    """A wall one metre in front of a camera that looks along +`axis`; every pixel measured, with a little relief."""
    rng = np.random.default_rng(seed)
    depth = (1000 + rng.integers(0, 40, (frames, h, w))).astype(np.uint16)
    pose = _eye(frames)
    rot = {0: [[0, 0, 1], [1, 0, 0], [0, 1, 0]], 1: [[1, 0, 0], [0, 0, 1], [0, -1, 0]], 2: np.eye(3)}[axis]
    pose[:, :3, :3] = np.asarray(rot, np.float64)
    for f in range(frames):
        pose[f, :3, 3] = rng.uniform(-0.05, 0.05, 3)
    kw.setdefault("voxel", 0.04)
    return {"depth": depth, "pose": pose, "intr": np.array((7.5, 7.25, 3.5, 2.5)), "kw": kw}


def _two_adjacent():
    """Two pixels whose points are exactly B = 1/2 apart along x: blocks 1 and 2, 27 + 9 allocated."""
    depth = np.full((1, 1, 2), 1000, np.uint16)
    return {"depth": depth, "pose": _eye(1), "intr": np.array((2.0, 2.0, 0.0, 0.0)), "kw": {"voxel": VOXEL}}


def _lost(case):
    pose = case["pose"].copy()
    pose[:] = -np.inf
    return _with(case, pose=pose)


def _nan_cx():
    case = _single(frames=2)
    intr = np.tile(case["intr"], (2, 1))
    intr[1, 2] = np.nan
    return _with(case, intr=intr)


def _inside():
    """A second camera inside the blocks: zc = 0 exactly on the layer of centres at 33/32, negative below it."""
    case = _f32(_single(frames=2, w=5, h=5, cx=2.0, cy=2.0))
    depth = case["depth"].copy()
    depth[1] = np.float32(0.25)
    pose = case["pose"].copy()
    pose[1, 2, 3] = 1.03125
    return _with(case, depth=depth, pose=pose)


def _weights():
    """Four frames of one pixel whose depth steps back by one voxel: layers of voxels seen by 4, 3, 2 and 1 frames; min_weight = 3."""
    case = _f32(_single(frames=4, min_weight=3))
    depth = case["depth"].copy()
    for f in range(4):
        depth[f, 8, 8] = 1.0 + f * VOXEL
    return _with(case, depth=depth)


def _many(n, seen):
    """n frames of one pixel; only `seen` face the point, the others look the other way and measure nothing."""
    case = _single(frames=n, w=1, h=1, cx=0.0, cy=0.0)
    depth, pose = case["depth"].copy(), case["pose"].copy()
    for f in range(n):
        if f not in seen:
            depth[f] = 0
            pose[f, :3, :3] = np.diag([-1.0, 1.0, -1.0])
        else:
            pose[f, 0, 3] = (f % 3) * VOXEL
    return _with(case, depth=depth, pose=pose)


def _zero_d():
    """Float32 depth 1 and 33/32 side by side: the second pixel's surface lies exactly on a voxel centre, D = 0."""
    depth = np.array([[[1.0, 1.03125]]], np.float32)
    return {"depth": depth, "pose": _eye(1), "intr": np.array((16.5, 16.5, 0.25, 0.0)), "kw": {"voxel": VOXEL}}


def _room(frames=6, h=60, w=80, lost=2):
    """The largest case: a ray-cast box room with a box in it, six 60 x 80 frames at 4 cm voxels, one lost."""
    planes = [(0, -1.5, (200, 60, 60)), (0, 1.5, (60, 200, 60)), (1, -1.2, (60, 60, 200)), (1, 1.2, (200, 200, 60)),
              (2, 0.0, (120, 120, 120)), (2, 2.4, (240, 240, 240))]
    box = ((-0.4, -0.3, 0.0), (0.3, 0.4, 0.7), (250, 120, 10))
    intr = (70.0, 70.0, 39.5, 29.5)
    depth, colour, pose = [], [], []
    for f in range(frames):
        a = 2.0 * np.pi * f / frames
        p = R.look_at((0.8 * np.cos(a), 0.6 * np.sin(a), 1.3), (-0.9 * np.cos(a), -0.8 * np.sin(a), 0.6))
        img = R.render(p, intr, h, w, planes=planes, box=box)
        depth.append(img["u16"]); colour.append(img["colour"]); pose.append(p)
    pose = np.stack(pose)
    if lost is not None:
        pose[lost] = -np.inf
    return {"depth": np.stack(depth), "colour": np.stack(colour), "pose": pose, "intr": np.array(intr),
            "kw": {"voxel": 0.04, "edge": 0.05, "depth_max": 4.0}}


CASES = {}


def _add(name, why, case):
    CASES[name] = dict(case, why=why)


_add("one", "F = H = W = 1: one point, exactly 27 blocks", _single(cx=0.0, cy=0.0, w=1, h=1))
_add("min_rounding", "(min - (min - B)) / B rounds a last bit below 1 on z (z = 2, voxel 0.05): the point still lies in block 1",
     _f32(_single(cx=0.0, cy=0.0, w=1, h=1, d=2000, voxel=0.05)))
_add("all_lost", "every frame lost: an empty cloud, M_b = 0, nothing launched behind it", _lost(_single(frames=2)))
_add("none_measured", "no measurement anywhere: an empty cloud", _with(_single(), depth=np.zeros((1, 9, 9), np.uint16)))
_add("two_adjacent", "two points in adjacent blocks: the dilations overlap, 36 blocks", _two_adjacent())
_add("tie", "uf and vf exactly x.5 for even and odd x around the one measured pixel; W - 0.5 stays inside", _single())
_add("tie_low", "ur = -0.5 rounds to -0 and stays inside; -1.5 is outside", _single(cx=0.0, cy=0.0))
_add("tie_colour", "the tie case with colour", _colour(_single(), 3))
_add("tie_f32", "the tie case as float32 metres with colour", _colour(_f32(_single()), 4))
_add("nan_cx", "a frame whose cx is NaN: uf is NaN, every comparison false, the frame adds nothing", _nan_cx())
_add("inside", "a camera inside the blocks: zc = 0 and negative for part of a block, the block straddles zc = 0", _inside())
_add("trunc_exact", "s exactly -trunc is kept", _single(trunc=0.21875))
_add("trunc_ulp", "s one ulp below -trunc is skipped", _single(trunc=float(np.nextafter(0.21875, 0.0))))
_add("trunc_max", "trunc = 8 * voxel", _single(trunc=8 * VOXEL))
_add("trunc_small", "a truncation below one voxel: s >= trunc, every voxel in front clamps to 1", _wall(2, 11, trunc=0.03))
_add("weights", "voxels seen by 1, 2, min_weight - 1 = 2, 3 and 4 frames with min_weight = 3", _weights())
_add("weights_colour", "the same with colour: C accumulates over the frames", _colour(_weights(), 5))
for _n, _seen in ((63, (0, 31, 62)), (64, (5, 63)), (65, (0, 63, 64)), (130, (1, 64, 127, 128, 129))):
    _add("frames%d" % _n, "%d one-pixel frames of which %d see the block: the ballot walk" % (_n, len(_seen)), _many(_n, _seen))
_add("zero_d", "D(q) = 0 exactly next to negative and positive neighbours", _zero_d())
_add("wall_z", "a wall seen along +z: crossings into the next block along z, blocks straddling the image border", _wall(2, 6))
_add("wall_x", "the same along +x through a rotated pose: Rt is not R", _wall(0, 7))
_add("wall_y", "the same along +y, with colour and the edge test", _colour(_wall(1, 8, edge=0.02), 9))
_add("wall_f32", "three offset frames of float32 metres averaging one wall", _f32(_wall(2, 10, frames=3, min_weight=2)))
_add("room", "6 frames of 60 x 80 at 4 cm voxels, one lost: several hundred blocks", _room())


def arguments(case):
    """fuse_ref's arguments of a case: (depth, pose, intr, colour, kw)."""
    return case["depth"], case["pose"], case["intr"], case.get("colour"), dict(case.get("kw", {}))


# ---------------------------------------------------------------------------------------------------------------- volumes
def _key(b):
    return (int(b[2]) << 42) | (int(b[1]) << 21) | int(b[0])


def _random_volume(seed, colour, min_weight):
    """Blocks of a 3 x 3 x 2 region with gaps (neighbours that are not allocated), random distances that hold exact 0 and
    -0, weights 0..3: every branch of the crossing test and of the gradient, across block borders on every axis."""
    rng = np.random.default_rng(seed)
    blocks = [(x, y, z) for z in (1, 2) for y in (1, 2, 3) for x in (1, 2, 3) if rng.random() < 0.7]
    key = np.sort(np.array([_key(b) for b in blocks], np.int64))
    m = len(key)
    tsdf = rng.choice(np.array([-1.0, -0.5, -0.25, -0.0, 0.0, 0.125, 0.5, 1.0], np.float32), (m, 512))
    tsdf = (tsdf * rng.choice(np.array([1.0, 0.75], np.float32), (m, 512))).astype(np.float32)
    weight = rng.integers(0, 4, (m, 512)).astype(np.int32)
    tsdf[weight == 0] = 0.0
    rgb = rng.uniform(0, 255, (m, 512, 3)).astype(np.float32) if colour else None
    return {"block_key": key, "tsdf": tsdf, "weight": weight, "rgb": rgb, "origin": np.array([-0.3, 0.2, 1.1]), "voxel": 0.05,
            "min_weight": min_weight}


def _zero_gradient():
    """Four voxels in a row, -1/2, 1/2, -1/2, 1/2, alone in a block: the middle crossing has G(q) = G(n) = 0, a zero normal."""
    tsdf = np.zeros((1, 512), np.float32)
    weight = np.zeros((1, 512), np.int32)
    for i, d in enumerate((-0.5, 0.5, -0.5, 0.5)):
        tsdf[0, (3 * 8 + 3) * 8 + 2 + i] = d
        weight[0, (3 * 8 + 3) * 8 + 2 + i] = 1
    return {"block_key": np.array([_key((1, 1, 1))], np.int64), "tsdf": tsdf, "weight": weight, "rgb": None,
            "origin": np.zeros(3), "voxel": 0.02, "min_weight": 1}


VOLUMES = {
    "random": dict(_random_volume(1, False, 1), why="every crossing and gradient branch, block borders, gaps"),
    "random_colour_w2": dict(_random_volume(2, True, 2), why="the same with colour and min_weight = 2"),
    "random_w3": dict(_random_volume(3, False, 3), why="min_weight = 3: weight equal to min_weight is observed"),
    "zero_gradient": dict(_zero_gradient(), why="len = 0: the zero normal"),
}
