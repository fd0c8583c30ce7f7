"""The numpy restatement of the posed-depth-frames front end (include/pbnet_hip.h "Posed depth frames", csrc/frames.hip) and of
pbn_cloud_normals_views, operation by operation in float64 (numpy array operations and Python floats round once per
operation; nothing is fused), and a small analytic ray-caster that renders the depth and colour images the tests feed it."""
import math

import numpy as np

import upright_ref

F32, F64 = np.float32, np.float64


# ------------------------------------------------------------------------------------------------------ back-projection
def depth_z(depth, depth_scale):
    """z in float64: a uint16 image is divided by depth_scale, a float32 image is metres already."""
    d = np.asarray(depth)
    assert d.dtype in (np.uint16, np.float32) and d.ndim == 3
    return d.astype(F64) / F64(depth_scale) if d.dtype == np.uint16 else d.astype(F64)


def measured(z, depth_min, depth_max):
    """Rule (b): finite, positive, inside [depth_min, depth_max]; a uint16 0 is z = 0 and fails z > 0."""
    with np.errstate(invalid="ignore"):
        return np.isfinite(z) & (z > 0.0) & (z >= depth_min) & (z <= depth_max)


def edge_mask(z, ok, edge):
    """Rule (c) at full resolution: True where a 4-neighbour inside the image that is itself measured differs by more than
    edge * z.  A neighbour outside the image or without a measurement makes no edge."""
    out = np.zeros(z.shape, bool)
    if not edge > 0.0:
        return out
    with np.errstate(invalid="ignore", over="ignore"):
        lim = F64(edge) * z
        for axis, step in ((2, -1), (2, 1), (1, -1), (1, 1)):
            zn = np.full(z.shape, np.nan)
            okn = np.zeros(z.shape, bool)
            src = [slice(None)] * 3
            dst = [slice(None)] * 3
            src[axis] = slice(1, None) if step > 0 else slice(None, -1)
            dst[axis] = slice(None, -1) if step > 0 else slice(1, None)
            zn[tuple(dst)] = z[tuple(src)]
            okn[tuple(dst)] = ok[tuple(src)]
            out |= okn & (np.abs(zn - z) > lim)
    return out


def frames_ref(depth, pose, intr, colour=None, depth_scale=1000.0, depth_min=0.0, depth_max=math.inf, stride=1, edge=None):
    """The contract of pbn_frames_count + pbn_frames_write as a dict of numpy arrays: xyz f32 [N, 3], rgb f32 [N, 3] (with
    colour), pixel int32 [N], frame_start int32 [F + 1], n."""
    depth = np.asarray(depth)
    n_f, h, w = depth.shape
    pose = np.asarray(pose, F64).reshape(n_f, 4, 4)
    intr = np.broadcast_to(np.asarray(intr, F64), (n_f, 4))
    edge = 0.0 if edge is None else float(edge)
    z = depth_z(depth, depth_scale)
    ok_b = measured(z, depth_min, depth_max)
    pose_ok = np.isfinite(pose[:, :3, :]).all(axis=(1, 2))                    # rule (a): the top three rows
    v, u = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    sampled = (v % stride == 0) & (u % stride == 0)
    ok = ok_b & pose_ok[:, None, None] & sampled[None] & ~edge_mask(z, ok_b, edge)
    fx, fy, cx, cy = (intr[:, i][:, None, None] for i in range(4))
    uu, vv = u.astype(F64)[None], v.astype(F64)[None]
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        xc = ((uu - cx) * z) / fx
        yc = ((vv - cy) * z) / fy
        world = []
        for r in range(3):
            r0, r1, r2, t = (pose[:, r, c][:, None, None] for c in range(4))
            world.append((((r0 * xc + r1 * yc) + r2 * z) + t).astype(F32))     # rounded once, on the store
    xyz = np.stack(world, axis=-1)
    ok &= np.isfinite(xyz).all(axis=-1)                                       # rule (d)
    pixel = np.flatnonzero(ok.reshape(-1)).astype(np.int32)                   # ascending (f * H + v) * W + u
    counts = ok.reshape(n_f, -1).sum(axis=1)
    out = {"xyz": np.ascontiguousarray(xyz.reshape(-1, 3)[pixel]), "pixel": pixel, "n": int(pixel.shape[0]),
           "frame_start": np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)}
    if colour is not None:
        out["rgb"] = np.ascontiguousarray(np.asarray(colour, np.uint8).reshape(-1, 3)[pixel].astype(F32))
    return out


def centres_ref(pose):
    """frames_to_points' centres f32 [F, 3] (NaN rows for skipped frames) and skipped bool [F]."""
    pose = np.asarray(pose, F64).reshape(-1, 4, 4)
    skipped = ~np.isfinite(pose[:, :3, :]).all(axis=(1, 2))
    with np.errstate(over="ignore"):
        c = pose[:, :3, 3].astype(F32)
    c[skipped] = np.nan
    return c, skipped


# ------------------------------------------------------------------------------------------------- normals towards views
def normals_views_ref(xyz, idx, views, view_of):
    """pbn_cloud_normals_views in Python floats: pbn_cloud_normals' mean, covariance and Jacobi eigenvector, flipped when
    (nx * (vx - px) + ny * (vy - py)) + nz * (vz - pz) < 0 with v = views[view_of[i]]; a view_of outside [0, V) flips
    nothing; fewer than three points give the zero vector.  f32 [N, 3]."""
    p = np.asarray(xyz, F32).astype(F64).tolist()
    vw = np.asarray(views, F32).astype(F64).reshape(-1, 3).tolist()
    idx = np.asarray(idx)
    n, k = idx.shape
    out = np.zeros((n, 3), F32)
    for i in range(n):
        px, py, pz = p[i]
        nb = [int(j) for j in idx[i] if 0 <= j < n]
        if len(nb) + 1 < 3:
            continue
        sx, sy, sz = px, py, pz
        for j in nb:
            sx, sy, sz = sx + p[j][0], sy + p[j][1], sz + p[j][2]
        m = float(len(nb) + 1)
        mx, my, mz = sx / m, sy / m, sz / m
        dx, dy, dz = px - mx, py - my, pz - mz
        a = [dx * dx, dx * dy, dx * dz, dy * dy, dy * dz, dz * dz]
        for j in nb:
            dx, dy, dz = p[j][0] - mx, p[j][1] - my, p[j][2] - mz
            a = [a[0] + dx * dx, a[1] + dx * dy, a[2] + dx * dz, a[3] + dy * dy, a[4] + dy * dz, a[5] + dz * dz]
        nx, ny, nz = upright_ref.jacobi_smallest(a)
        w = int(view_of[i])
        if 0 <= w < len(vw):
            dot = (nx * (vw[w][0] - px) + ny * (vw[w][1] - py)) + nz * (vw[w][2] - pz)
            if dot < 0.0:
                nx, ny, nz = -nx, -ny, -nz
        out[i] = (nx, ny, nz)
    return out


# ------------------------------------------------------------------------------------------------------------ ray-caster
def look_at(eye, target, up=(0.0, 0.0, 1.0)):
    """A camera-to-world pose f64 [4, 4]: +z looks from eye to target, +x is right, +y is down (the depth-camera frame)."""
    eye, target, up = (np.asarray(a, F64) for a in (eye, target, up))
    fwd = target - eye
    fwd = fwd / np.linalg.norm(fwd)
    right = np.cross(fwd, up)
    right = right / np.linalg.norm(right)
    down = np.cross(fwd, right)
    pose = np.eye(4)
    pose[:3, 0], pose[:3, 1], pose[:3, 2], pose[:3, 3] = right, down, fwd, eye
    return pose


def _slab_hit(o, d, lo, hi):
    """Ray o + t d against the axis-aligned box [lo, hi]: (t of entry, the entered axis), t = inf where it misses."""
    with np.errstate(divide="ignore", invalid="ignore"):
        t0 = (lo - o) / d
        t1 = (hi - o) / d
    near, far = np.minimum(t0, t1), np.maximum(t0, t1)
    near = np.where(np.isnan(near), -np.inf, near)
    far = np.where(np.isnan(far), np.inf, far)
    t_in, t_out = near.max(axis=-1), far.min(axis=-1)
    hit = (t_in <= t_out) & (t_in > 1e-9)
    return np.where(hit, t_in, np.inf), near.argmax(axis=-1)


def render(pose, intr, h, w, planes=(), box=None, depth_scale=1000.0):
    """Depth and colour of axis-aligned planes and one box seen from `pose` (camera to world) with intrinsics (fx, fy, cx, cy),
    pixel centres at the integers.  planes: (axis, offset, colour) = the plane x[axis] = offset; box: (lo, hi, colour).
    Returns z f64 [h, w] (the exact camera-frame depth, inf = nothing hit), depth uint16 (rint(z * depth_scale), 0 = no
    hit or out of range), depth f32 metres (0 = no hit), colour uint8 [h, w, 3], surface int [h, w] (the index of the plane
    hit, len(planes) for the box, -1 for none) and ray f64 [h, w] = |ray| / z of each pixel."""
    pose = np.asarray(pose, F64)
    fx, fy, cx, cy = (float(a) for a in intr)
    v, u = np.meshgrid(np.arange(h, dtype=F64), np.arange(w, dtype=F64), indexing="ij")
    d_cam = np.stack([(u - cx) / fx, (v - cy) / fy, np.ones_like(u)], axis=-1)          # z component 1: t IS the depth
    d = d_cam @ pose[:3, :3].T
    o = pose[:3, 3]
    best = np.full((h, w), np.inf)
    surface = np.full((h, w), -1)
    colour = np.zeros((h, w, 3), np.uint8)
    for i, (axis, offset, col) in enumerate(planes):
        with np.errstate(divide="ignore", invalid="ignore"):
            t = (offset - o[axis]) / d[..., axis]
        t = np.where(np.isfinite(t) & (t > 1e-9), t, np.inf)
        closer = t < best
        best, surface = np.where(closer, t, best), np.where(closer, i, surface)
        colour[closer] = col
    if box is not None:
        t, _ = _slab_hit(o, d, np.asarray(box[0], F64), np.asarray(box[1], F64))
        closer = t < best
        best, surface = np.where(closer, t, best), np.where(closer, len(planes), surface)
        colour[closer] = box[2]
    hit = np.isfinite(best)
    q = np.where(hit, np.rint(best * depth_scale), 0.0)
    d16 = np.where((q >= 1) & (q <= 65535), q, 0.0).astype(np.uint16)
    d32 = np.where(hit, best, 0.0).astype(F32)
    return {"z": best, "u16": d16, "f32": d32, "colour": colour, "surface": surface, "ray": np.linalg.norm(d_cam, axis=-1)}
