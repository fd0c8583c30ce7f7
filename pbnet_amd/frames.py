"""Posed depth frames to a raw scan on the device (csrc/frames.hip): what a depth camera hands over -- depth images, colour
images, one pose per frame, the intrinsics -- back-projected into the cloud pbnet_amd.mesh.decode_points' chain takes.
include/pbnet_hip.h ("Posed depth frames") states every operation; tests/frames_ref.py restates it in numpy.

The images are device tensors.  The poses and the intrinsics are a few numbers per frame that every tracker produces on the
host: they are host arrays here, which is what lets their values be checked before anything is launched and lets the
sensor positions reach decode_frames without a read-back.  As everywhere in the scan chain the checks come in one order:
values, dtypes and shapes on the host, then the tensors' device, then the library.  There is no CPU path."""
import ctypes
import math

import numpy as np
import torch

from . import _native as N
from .cloud import _device, _got, _int_in, _real, _scan_status, _scan_workspace

FRAMES_STAGES = ("count", "scan + starts", "write")
FUSE_STAGES = ("box + keys", "point blocks", "dilation + blocks", "integrate", "extract count", "extract write")
FUSE_TOO_MANY, FUSE_ROWS, FUSE_MAX_BLOCKS, FUSE_MAX_EXTRACT_BLOCKS = 4, 32, 1 << 21, 1398101     # csrc/tsdf.hip
FRAMES_MAX_PIXELS, FRAMES_MAX_SAMPLED = (1 << 31) - 1, 1 << 28      # F * H * W; csrc/scan_dev.h's SCAN_MAX_POINTS
_DOUBLE_P = ctypes.POINTER(ctypes.c_double)


def _host_f64(what, name, v, shapes, shown):
    """A small host array of real numbers as contiguous float64; its shape is one of `shapes`."""
    if torch.is_tensor(v):
        if v.device.type != "cpu":
            raise TypeError("%s: %s must be a host array (numpy or a CPU tensor), got a %s tensor" % (what, name, v.device))
        v = v.detach().numpy()
    try:
        a = np.asarray(v)
    except (TypeError, ValueError):
        raise TypeError("%s: %s must be a float array of shape %s, got %s" % (what, name, shown, type(v).__name__)) from None
    if a.dtype.kind != "f":
        raise TypeError("%s: %s must be a float array of shape %s, got dtype %s" % (what, name, shown, a.dtype))
    if tuple(a.shape) not in shapes:
        raise ValueError("%s: %s must have shape %s, got %s" % (what, name, shown, tuple(a.shape)))
    return np.ascontiguousarray(a, np.float64)


def _frames_args(what, depth, poses, intrinsics, colour, depth_scale, depth_min, depth_max, stride, edge):
    """Every host-side check, before a device or the library is asked: (F, H, W), pose f64 [F, 16], intr f64 [F, 4] and the
    scalars as the library takes them."""
    if not torch.is_tensor(depth) or depth.dtype not in (torch.uint16, torch.float32) or depth.dim() != 3:
        raise TypeError("%s: depth must be a uint16 or float32 [F, H, W] tensor, got %s" % (what, _got(depth)))
    f, h, w = (int(s) for s in depth.shape)
    if colour is not None and (not torch.is_tensor(colour) or colour.dtype != torch.uint8 or tuple(colour.shape) != (f, h, w, 3)):
        raise TypeError("%s: colour must be a uint8 [%d, %d, %d, 3] tensor on the depth grid, got %s" % (what, f, h, w, _got(colour)))
    pose = _host_f64(what, "poses", poses, ((f, 4, 4),), "[%d, 4, 4]" % f).reshape(f, 16)
    intr = _host_f64(what, "intrinsics", intrinsics, ((4,), (f, 4)), "[4] or [%d, 4]" % f)
    intr = np.ascontiguousarray(np.broadcast_to(intr, (f, 4)))
    scale = float(_real(what, "depth_scale", depth_scale))
    z_min, z_max = float(_real(what, "depth_min", depth_min)), float(_real(what, "depth_max", depth_max))
    stride = _int_in(what, "stride", stride, 1, (1 << 31) - 1, "1..2^31 - 1")
    edge = 0.0 if edge is None else float(_real(what, "edge", edge, "a number or None"))
    if not (scale > 0.0 and math.isfinite(scale)):
        raise ValueError("%s: depth_scale must be positive and finite, got %r" % (what, depth_scale))
    if not z_min <= z_max:
        raise ValueError("%s: depth_min must not exceed depth_max, got %r and %r" % (what, depth_min, depth_max))
    if not np.all(np.isfinite(intr[:, :2]) & (intr[:, :2] > 0.0)):
        raise ValueError("%s: fx and fy must be positive and finite in every frame" % what)
    if f * h * w > FRAMES_MAX_PIXELS:
        raise ValueError("%s: %d x %d x %d pixels exceed 2^31 - 1" % (what, f, h, w))
    sampled = f * -(-h // stride) * -(-w // stride)
    if sampled > FRAMES_MAX_SAMPLED:
        raise ValueError("%s: %d sampled pixels (stride %d) exceed 2^28" % (what, sampled, stride))
    return (f, h, w), pose, intr, (scale, z_min, z_max, stride, edge)


def host_centres(pose):
    """From pose f64 [F, 16]: centres f32 [F, 3] (the float32 of each translation, NaN rows for skipped frames) and skipped
    bool [F] (a top-three-rows entry is not finite), as host arrays."""
    skipped = ~np.isfinite(pose[:, :12]).all(axis=1)
    with np.errstate(over="ignore"):
        centres = pose[:, (3, 7, 11)].astype(np.float32)
    centres[skipped] = np.nan
    return centres, skipped


def frames_to_points(depth, poses, intrinsics, colour=None, depth_scale=1000.0, depth_min=0.0, depth_max=math.inf, stride=1,
                     edge=None, times=None):
    """An RGB-D sequence as one raw cloud (csrc/frames.hip).  `depth` is a device tensor [F, H, W]: uint16 with
    z = d / depth_scale and 0 = no measurement (ScanNet, RealSense, Kinect), or float32 metres.  `colour` (uint8
    [F, H, W, 3] on the depth grid, device) is optional.  `poses` (float [F, 4, 4], camera to world) and `intrinsics`
    (fx, fy, cx, cy: [4] for all frames or [F, 4]) are host arrays.  Pixel (u = column, v = row) is the pixel's centre; with
    `stride` only the pixels with u % stride == 0 and v % stride == 0 are taken.  A pixel gives a point when its frame's
    pose is finite in its top three rows (ScanNet writes -inf for lost tracking), when z is finite, positive and within
    [depth_min, depth_max], when -- with `edge`, a ratio -- no measured 4-neighbour at full resolution differs from it by
    more than edge * z (the depth-discontinuity test for flying pixels), and when its world point is finite in float32.
    x = (u - cx) * z / fx, y = (v - cy) * z / fy, world = R . (x, y, z) + t, in float64, rounded once.

    Returns a dict on the device: xyz f32 [N, 3], rgb f32 [N, 3] (the bytes as 0..255 floats; with `colour`), pixel int32
    [N] = (f * H + v) * W + u, ascending -- so a point's frame is pixel // (H * W) and label images gather through it --,
    frame_start int32 [F + 1] (frame f owns rows frame_start[f]:frame_start[f + 1], a skipped frame none), centres f32
    [F, 3] (the float32 of each pose's translation, NaN rows for skipped frames), skipped bool [F], and shape = (F, H, W).
    One read-back (status and N) between the count pass and the write pass; no atomics order the rows, so two runs give the
    same bytes.  `times` (a dict) takes the stage times of the measurement entries, which synchronise."""
    what = "frames_to_points"
    (f, h, w), pose, intr, (scale, z_min, z_max, stride, edge) = _frames_args(what, depth, poses, intrinsics, colour, depth_scale,
                                                                            depth_min, depth_max, stride, edge)
    depth, colour = _device(depth, colour)
    dev, lib = depth.device, N.lib()
    ws = _scan_workspace(lib.pbn_frames_workspace_bytes(f, h, w, stride), dev, "%d frames of %d x %d" % (f, h, w), "sequence")
    frame_start = torch.empty(f + 1, dtype=torch.int32, device=dev)
    result = torch.empty(2, dtype=torch.int32, device=dev)
    head = (N.ptr(depth), int(depth.dtype == torch.float32), N.ptr(colour), pose.ctypes.data_as(_DOUBLE_P),
            intr.ctypes.data_as(_DOUBLE_P), f, h, w, scale, z_min, z_max, stride, edge)
    tail = (N.ptr(result), N.ptr(ws), ws.numel(), N.current_stream())
    t = None if times is None else ((ctypes.c_float * 2)(), (ctypes.c_float * 1)())
    if t is None:
        N.check(lib.pbn_frames_count(*head, N.ptr(frame_start), *tail), "pbn_frames_count")
    else:
        N.check(lib.pbn_frames_count_timed(*head, N.ptr(frame_start), *tail, t[0]), "pbn_frames_count_timed")
    st, n = (int(v) for v in result.tolist())                # the one read-back
    _scan_status(what, st)
    xyz = torch.empty(n, 3, dtype=torch.float32, device=dev)
    rgb = torch.empty(n, 3, dtype=torch.float32, device=dev) if colour is not None else None
    pixel = torch.empty(n, dtype=torch.int32, device=dev)
    if t is None:                                            # its status bit needs the frames to change under the two passes
        N.check(lib.pbn_frames_write(*head, n, N.ptr(xyz), N.ptr(rgb), N.ptr(pixel), *tail), "pbn_frames_write")
    else:
        N.check(lib.pbn_frames_write_timed(*head, n, N.ptr(xyz), N.ptr(rgb), N.ptr(pixel), *tail, t[1]), "pbn_frames_write_timed")
        _scan_status(what, int(result[0].item()))            # the measurement entry has synchronised already
        times.update(zip(FRAMES_STAGES, (float(t[0][0]), float(t[0][1]), float(t[1][0]))))
    centres, skipped = host_centres(pose)
    out = {"xyz": xyz, "pixel": pixel, "frame_start": frame_start, "centres": torch.from_numpy(centres).to(dev),
           "skipped": torch.from_numpy(skipped).to(dev), "shape": (f, h, w)}
    if rgb is not None:
        out["rgb"] = rgb
    return out


def _fuse_args(what, voxel, trunc, min_weight):
    """fuse_frames' own scalars, checked on the host: (voxel, trunc, min_weight) as the library takes them."""
    voxel = float(_real(what, "voxel", voxel))
    if not (voxel > 0.0 and math.isfinite(voxel) and math.isfinite(8.0 * voxel)):
        raise ValueError("%s: voxel must be positive and finite, got %r" % (what, voxel))
    trunc = 4.0 * voxel if trunc is None else float(_real(what, "trunc", trunc, "a number or None"))
    if not (math.isfinite(trunc) and 0.0 < trunc <= 8.0 * voxel):
        raise ValueError("%s: trunc must be finite with 0 < trunc <= 8 * voxel = %r, got %r" % (what, 8.0 * voxel, trunc))
    min_weight = _int_in(what, "min_weight", min_weight, 1, (1 << 31) - 1, "1..2^31 - 1")
    return voxel, trunc, min_weight


def _fuse_status(what, status, voxel):
    """A fusion stage's status word: the chain's bits, then the stage's own."""
    if status & FUSE_TOO_MANY:
        raise ValueError("%s: more than 2^21 blocks of 8 voxels of %r: the voxel is too small for the scene" % (what, voxel))
    if status & 2:
        raise ValueError("%s: the cloud spans 2^21 blocks or more of 8 voxels of %r on an axis" % (what, voxel))
    if status & 1:
        raise ValueError("%s: a coordinate is NaN or infinite" % what)
    if status & FUSE_ROWS:
        raise RuntimeError("%s: a pass met more rows than its count pass: the inputs changed between the two (status %d)"
                           % (what, status))
    if status:
        raise RuntimeError("%s: the device sort gave up (status %d)" % (what, status))


def fuse_frames(depth, poses, intrinsics, colour=None, voxel=0.02, trunc=None, depth_scale=1000.0, depth_min=0.0,
                depth_max=math.inf, edge=None, min_weight=1, return_volume=False, times=None):
    """An RGB-D sequence fused into a truncated signed distance volume and its surface points (csrc/tsdf.hip; the contract
    is include/pbnet_hip.h's "Depth-frame fusion", tests/fuse_ref.py restates it).  The arguments are frames_to_points'
    without `stride`, plus `voxel` (metres), `trunc` (the truncation distance, None = 4 * voxel, at most 8 * voxel) and
    `min_weight` (a voxel counts as observed when that many frames saw it).

    Blocks of 8^3 voxels are allocated around the raw cloud (frames_to_points at stride 1, never read back); every voxel
    of every block then meets every frame in ascending order -- projective distance, truncated, averaged with weight 1 --
    with its sums in one lane's registers; the zero crossings between observed neighbours along x, y and z come back as
    points with interpolated colour and the normalised gradient of the distance field, which points towards the sensors.

    Returns a dict on the device: xyz, nl f32 [N, 3], rgb f32 [N, 3] (with `colour`), weight int32 [N] (the lesser
    of the crossing's two voxels), voxel_id int64 [N] = (block rank * 512 + in-block index) * 3 + axis, ascending; origin
    (f64 [3], host: the corner of block (0, 0, 0)), n_blocks, centres, skipped and shape as frames_to_points gives them; with
    return_volume also block_key int64 [M_b], tsdf f32 [M_b, 512], vol_weight int32 [M_b, 512] and vol_rgb f32
    [M_b, 512, 3].  More than 1 398 101 blocks raise ValueError (the allocation takes 2^21, the extraction's int32 row
    count does not).  Three read-backs, each a status and a count: the raw points, the blocks, the surface rows.  `times` (a
    dict) takes the stage times of the measurement entries, which synchronise, and "stats": the block-frame pairs the cull
    left and the depth samples gathered."""
    what = "fuse_frames"
    (f, h, w), pose, intr, (scale, z_min, z_max, _, edge) = _frames_args(what, depth, poses, intrinsics, colour, depth_scale,
                                                                         depth_min, depth_max, 1, edge)
    voxel, trunc, min_weight = _fuse_args(what, voxel, trunc, min_weight)
    depth, colour = _device(depth, colour)
    dev, lib = depth.device, N.lib()
    cloud = frames_to_points(depth, pose.reshape(f, 4, 4), intr, None, scale, z_min, z_max, 1, edge, times=times)
    xyz, n = cloud["xyz"], int(cloud["xyz"].shape[0])
    stream = N.current_stream()
    t = None if times is None else [(ctypes.c_float * k)() for k in (3, 1, 1, 1)]
    stats = (ctypes.c_uint64 * 2)()

    def call(entry, args, slot):
        if t is None:
            N.check(getattr(lib, entry)(*args), entry)
        else:
            extra = (t[slot], stats) if entry == "pbn_fuse_integrate" else (t[slot],)
            N.check(getattr(lib, entry + "_timed")(*args, *extra), entry + "_timed")

    ws = _scan_workspace(lib.pbn_fuse_blocks_workspace_bytes(n), dev, "%d raw points" % n)
    result = torch.empty(8, dtype=torch.int32, device=dev)
    call("pbn_fuse_blocks", (N.ptr(xyz), n, voxel, N.ptr(result), N.ptr(ws), ws.numel(), stream), 0)
    head = result.tolist()                                   # the second read-back: status, M_b and the minimum's bits
    _fuse_status(what, head[0], voxel)
    m_b = head[1]
    origin = np.array(head[2:5], np.int32).view(np.float32).astype(np.float64) - 8.0 * voxel if n else np.zeros(3)
    origin = np.ascontiguousarray(origin, np.float64)
    block_key = torch.empty(m_b, dtype=torch.int64, device=dev)
    if m_b:
        N.check(lib.pbn_fuse_block_keys(n, m_b, N.ptr(block_key), N.ptr(result), N.ptr(ws), ws.numel(), stream), "pbn_fuse_block_keys")
    del ws, xyz, cloud["xyz"]
    if m_b > FUSE_MAX_EXTRACT_BLOCKS:
        raise ValueError("%s: %d blocks exceed the %d whose surface rows fit an int32: the voxel is too small for the scene"
                         % (what, m_b, FUSE_MAX_EXTRACT_BLOCKS))
    tsdf = torch.empty(m_b, 512, dtype=torch.float32, device=dev)
    vol_weight = torch.empty(m_b, 512, dtype=torch.int32, device=dev)
    vol_rgb = torch.empty(m_b, 512, 3, dtype=torch.float32, device=dev) if colour is not None else None
    n_rows = 0
    if m_b:                                                  # an empty cloud: every later stage returns empty without a launch
        ws = torch.empty(lib.pbn_fuse_integrate_workspace_bytes(f), dtype=torch.uint8, device=dev)
        call("pbn_fuse_integrate", (N.ptr(depth), int(depth.dtype == torch.float32), N.ptr(colour), pose.ctypes.data_as(_DOUBLE_P),
                                    intr.ctypes.data_as(_DOUBLE_P), f, h, w, scale, z_min, z_max, edge, voxel, trunc,
                                    origin.ctypes.data_as(_DOUBLE_P), N.ptr(block_key), m_b, N.ptr(tsdf), N.ptr(vol_weight),
                                    N.ptr(vol_rgb), N.ptr(ws), ws.numel(), stream), 1)
        ws = torch.empty(lib.pbn_fuse_extract_workspace_bytes(m_b), dtype=torch.uint8, device=dev)
        res2 = torch.empty(2, dtype=torch.int32, device=dev)
        call("pbn_fuse_extract_count", (N.ptr(tsdf), N.ptr(vol_weight), N.ptr(block_key), m_b, min_weight, N.ptr(res2), N.ptr(ws),
                                        ws.numel(), stream), 2)
        st, n_rows = res2.tolist()                           # the third read-back
        _fuse_status(what, st, voxel)
    out_xyz = torch.empty(n_rows, 3, dtype=torch.float32, device=dev)
    out_nl = torch.empty(n_rows, 3, dtype=torch.float32, device=dev)
    out_rgb = torch.empty(n_rows, 3, dtype=torch.float32, device=dev) if colour is not None else None
    out_weight = torch.empty(n_rows, dtype=torch.int32, device=dev)
    voxel_id = torch.empty(n_rows, dtype=torch.int64, device=dev)
    if m_b:
        call("pbn_fuse_extract_write", (N.ptr(tsdf), N.ptr(vol_weight), N.ptr(vol_rgb), N.ptr(block_key), m_b, min_weight, voxel,
                                        origin.ctypes.data_as(_DOUBLE_P), n_rows, N.ptr(out_xyz), N.ptr(out_rgb), N.ptr(out_nl),
                                        N.ptr(out_weight), N.ptr(voxel_id), N.ptr(res2), N.ptr(ws), ws.numel(), stream), 3)
        if t is not None:
            _fuse_status(what, int(res2[0].item()), voxel)   # the measurement entry has synchronised already
    if t is not None:
        flat = [float(v) for a in t for v in a] if m_b else [float(v) for v in t[0]] + [0.0, 0.0, 0.0]
        times.update(zip(FUSE_STAGES, flat))
        times["stats"] = {"block_frame_pairs": int(stats[0]), "depth_samples": int(stats[1])}
    out = {"xyz": out_xyz, "nl": out_nl, "weight": out_weight, "voxel_id": voxel_id, "origin": origin, "n_blocks": m_b,
           "centres": cloud["centres"], "skipped": cloud["skipped"], "shape": (f, h, w)}
    if out_rgb is not None:
        out["rgb"] = out_rgb
    if return_volume:
        out.update(block_key=block_key, tsdf=tsdf, vol_weight=vol_weight, vol_rgb=vol_rgb)
    return out
