"""The numpy restatement of depth-frame fusion (include/pbnet_hip.h "Depth-frame fusion", csrc/tsdf.hip), stage by stage:
blocks_ref (allocation), integrate_ref (the volume) and extract_ref (the surface rows), and fuse_ref, which chains them
behind frames_ref's raw cloud.  Float64 numpy array operations round once per operation and nothing is fused; results are
rounded to float32 once.  There is no cull here: every voxel meets every frame."""
import math

import numpy as np

import frames_ref as R

F32, F64, I64 = np.float32, np.float64, np.int64
SIDE, VOXELS, BITS = 8, 512, 21
MAX_BLOCKS = 1 << 21
NONFINITE, EXTENT, TOO_MANY = 1, 2, 4
_OFF = np.array([(dx, dy, dz) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1)], I64)


def pack(b):
    """key = bz << 42 | by << 21 | bx of int64 block coordinates [..., 3]."""
    b = np.asarray(b, I64)
    return (b[..., 2] << (2 * BITS)) | (b[..., 1] << BITS) | b[..., 0]


def unpack(key):
    key = np.asarray(key, I64)
    m = (1 << BITS) - 1
    return np.stack([key & m, (key >> BITS) & m, (key >> (2 * BITS)) & m], axis=-1)


def blocks_ref(xyz, voxel, neighbours=_OFF):
    """Stage 1: (status, origin f64 [3], block_key int64 [M_b]) of a raw float32 cloud [n, 3]."""
    xyz = np.asarray(xyz, F32).reshape(-1, 3)
    if xyz.shape[0] == 0:
        return 0, np.zeros(3, F64), np.zeros(0, I64)
    if not np.all(np.isfinite(xyz)):
        return NONFINITE, np.zeros(3, F64), np.zeros(0, I64)
    B = F64(8.0) * F64(voxel)
    g = xyz.min(axis=0).astype(F64) - B
    with np.errstate(over="ignore"):
        q = np.maximum(np.floor((xyz.astype(F64) - g[None]) / B), 1.0)       # a point on the minimum: 1 up to the rounding
    if not np.all(q + 1.0 < 2.0 ** BITS - 1.0):                              # coordinate 2^21 - 1 stays free (key borrows)
        return EXTENT, g, np.zeros(0, I64)
    occupied = np.unique(pack(q.astype(I64)))
    keys = np.unique((unpack(occupied)[:, None, :] + np.asarray(neighbours, I64)[None]).reshape(-1, 3), axis=0)
    keys = np.sort(pack(keys))
    if keys.shape[0] > MAX_BLOCKS:
        return TOO_MANY, g, np.zeros(0, I64)
    return 0, g, keys


def world_to_camera(pose):
    """Rt [F, 3, 3] and tc [F, 3] of camera-to-world poses [F, 4, 4], by the contract's expressions."""
    pose = np.asarray(pose, F64).reshape(-1, 4, 4)
    with np.errstate(invalid="ignore", over="ignore"):
        Rt = np.transpose(pose[:, :3, :3], (0, 2, 1)).copy()
        t = pose[:, :3, 3]
        tc = np.stack([-((Rt[:, r, 0] * t[:, 0] + Rt[:, r, 1] * t[:, 1]) + Rt[:, r, 2] * t[:, 2]) for r in range(3)], axis=1)
    return Rt, tc


def centres(g, block_key, voxel):
    """Voxel centres f64 [M_b, 512, 3]: p[a] = g[a] + (double(8 * b[a] + i[a]) + 0.5) * voxel."""
    b = unpack(block_key)
    idx = np.arange(VOXELS)
    i = np.stack([idx & 7, (idx >> 3) & 7, idx >> 6], axis=-1)
    n = (SIDE * b[:, None, :] + i[None]).astype(F64)
    return np.asarray(g, F64)[None, None, :] + (n + 0.5) * F64(voxel)


def valid_depth(depth, depth_scale, depth_min, depth_max, edge):
    """z f64 [F, H, W] and the mask of rules (b) and (c)."""
    z = R.depth_z(depth, depth_scale)
    ok = R.measured(z, depth_min, depth_max)
    return z, ok & ~R.edge_mask(z, ok, 0.0 if edge is None else float(edge))


def integrate_ref(depth, pose, intr, colour, g, block_key, voxel, trunc, depth_scale=1000.0, depth_min=0.0, depth_max=math.inf,
                  edge=None):
    """Stage 2: tsdf f32 [M_b, 512], weight int32 [M_b, 512], rgb f32 [M_b, 512, 3] or None."""
    depth = np.asarray(depth)
    n_f, h, w = depth.shape
    pose = np.asarray(pose, F64).reshape(n_f, 4, 4)
    intr = np.broadcast_to(np.asarray(intr, F64), (n_f, 4))
    m = int(np.asarray(block_key).shape[0])
    p = centres(g, block_key, voxel).reshape(-1, 3)
    S = np.zeros(m * VOXELS, F64)
    Wt = np.zeros(m * VOXELS, np.int32)
    C = np.zeros((m * VOXELS, 3), F64) if colour is not None else None
    z_all, ok_all = valid_depth(depth, depth_scale, depth_min, depth_max, edge)
    Rt, tc = world_to_camera(pose)
    trunc = F64(trunc)
    live = np.isfinite(pose[:, :3, :]).all(axis=(1, 2))
    for f in range(n_f if h * w and m else 0):
        if not live[f]:
            continue
        fx, fy, cx, cy = intr[f]
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            pc = [((Rt[f, r, 0] * p[:, 0] + Rt[f, r, 1] * p[:, 1]) + Rt[f, r, 2] * p[:, 2]) + tc[f, r] for r in range(3)]
            zc = pc[2]
            ok = zc > 0.0
            uf = (fx * pc[0]) / zc + cx
            vf = (fy * pc[1]) / zc + cy
            ur, vr = np.rint(uf), np.rint(vf)
            ok &= (ur >= 0.0) & (ur <= F64(w - 1)) & (vr >= 0.0) & (vr <= F64(h - 1))
            u = np.where(ok, ur, 0.0).astype(I64)
            v = np.where(ok, vr, 0.0).astype(I64)
            ok &= ok_all[f, v, u]
            s = z_all[f, v, u] - zc
            ok &= ~(s < -trunc)
            d = np.minimum(1.0, s / trunc)
            S = np.where(ok, S + d, S)
        Wt = Wt + ok.astype(np.int32)
        if C is not None:
            byte = np.asarray(colour, np.uint8)[f, v, u].astype(F64)
            C = np.where(ok[:, None], C + byte, C)
    seen = Wt > 0
    with np.errstate(invalid="ignore", divide="ignore"):
        tsdf = np.where(seen, S / Wt.astype(F64), 0.0).astype(F32)
        rgb = None if C is None else np.where(seen[:, None], C / Wt.astype(F64)[:, None], 0.0).astype(F32).reshape(m, VOXELS, 3)
    return tsdf.reshape(m, VOXELS), Wt.reshape(m, VOXELS), rgb


class _Volume:
    """Lookups of voxels by (block rank, x, y, z) with x, y, z in -8 .. 15 relative to the block."""

    def __init__(self, tsdf, weight, block_key, min_weight):
        self.key = np.asarray(block_key, I64)
        self.D = np.asarray(tsdf, F32).astype(F64).reshape(-1)
        self.w = np.asarray(weight, np.int32).reshape(-1)
        self.min_weight = int(min_weight)

    def at(self, rank, x, y, z):
        """(allocated and observed, flat voxel index -- 0 where the block is not allocated)."""
        key = self.key[rank] + ((x + 8) // 8 - 1) + (((y + 8) // 8 - 1) << BITS) + (((z + 8) // 8 - 1) << (2 * BITS))
        pos = np.searchsorted(self.key, key)
        pos = np.minimum(pos, len(self.key) - 1)
        found = self.key[pos] == key
        flat = np.where(found, pos * VOXELS + ((z & 7) * 8 + (y & 7)) * 8 + (x & 7), 0)
        return found & (self.w[flat] >= self.min_weight), flat

    def gradient(self, rank, x, y, z, Dx):
        G = []
        for b in range(3):
            e = [int(b == 0), int(b == 1), int(b == 2)]
            op, fp = self.at(rank, x + e[0], y + e[1], z + e[2])
            om, fm = self.at(rank, x - e[0], y - e[1], z - e[2])
            G.append(np.where(op, self.D[fp], Dx) - np.where(om, self.D[fm], Dx))
        return G


def extract_ref(tsdf, weight, rgb, block_key, g, voxel, min_weight=1):
    """Stage 3: dict of xyz, nl f32 [N, 3], rgb (with a colour volume), weight int32 [N], voxel_id int64 [N], n."""
    m = int(np.asarray(block_key).shape[0])
    out = {"xyz": np.zeros((0, 3), F32), "nl": np.zeros((0, 3), F32), "weight": np.zeros(0, np.int32),
           "voxel_id": np.zeros(0, I64), "n": 0}
    if rgb is not None:
        out["rgb"] = np.zeros((0, 3), F32)
    if m == 0:
        return out
    vol = _Volume(tsdf, weight, block_key, min_weight)
    rank = np.repeat(np.arange(m), VOXELS)
    idx = np.tile(np.arange(VOXELS), m)
    x, y, z = idx & 7, (idx >> 3) & 7, idx >> 6
    obs_q, flat_q = vol.at(rank, x, y, z)
    ids, rows = [], {}
    for a in range(3):
        e = [int(a == 0), int(a == 1), int(a == 2)]
        obs_n, flat_n = vol.at(rank, x + e[0], y + e[1], z + e[2])
        Dq, Dn = vol.D[flat_q], vol.D[flat_n]
        hit = np.flatnonzero(obs_q & obs_n & ((Dq < 0.0) != (Dn < 0.0)))
        ids.append((rank[hit] * VOXELS + idx[hit]) * 3 + a)
        rows[a] = (hit, flat_n[hit])
    order = np.argsort(np.concatenate(ids), kind="stable")
    p_all = centres(g, block_key, voxel).reshape(-1, 3)
    parts = {k: [] for k in ("xyz", "nl", "rgb", "weight")}
    for a in range(3):
        hit, fn = rows[a]
        fq = flat_q[hit]
        e = [int(a == 0), int(a == 1), int(a == 2)]
        Dq, Dn = vol.D[fq], vol.D[fn]
        with np.errstate(invalid="ignore", divide="ignore"):
            r = Dq / (Dq - Dn)
            p = p_all[fq].copy()
            p[:, a] = p[:, a] + r * F64(voxel)
            Gq = vol.gradient(rank[hit], x[hit], y[hit], z[hit], Dq)
            Gn = vol.gradient(rank[hit], x[hit] + e[0], y[hit] + e[1], z[hit] + e[2], Dn)
            gv = [Gq[b] + r * (Gn[b] - Gq[b]) for b in range(3)]
            length = np.sqrt((gv[0] * gv[0] + gv[1] * gv[1]) + gv[2] * gv[2])
            unit = (length > 0.0) & np.isfinite(length)
            nl = np.stack([np.where(unit, gv[b] / length, 0.0) for b in range(3)], axis=1)
        parts["xyz"].append(p.astype(F32))
        parts["nl"].append(nl.astype(F32))
        parts["weight"].append(np.minimum(vol.w[fq], vol.w[fn]).astype(np.int32))
        if rgb is not None:
            c = np.asarray(rgb, F32).astype(F64).reshape(-1, 3)
            parts["rgb"].append((c[fq] + r[:, None] * (c[fn] - c[fq])).astype(F32))
    out["voxel_id"] = np.concatenate(ids)[order].astype(I64)
    out["n"] = int(order.shape[0])
    for k in ("xyz", "nl", "weight") + (("rgb",) if rgb is not None else ()):
        out[k] = np.ascontiguousarray(np.concatenate(parts[k])[order])
    return out


def fuse_ref(depth, pose, intr, colour=None, voxel=0.02, trunc=None, depth_scale=1000.0, depth_min=0.0, depth_max=math.inf,
             edge=None, min_weight=1):
    """The three stages behind frames_ref's raw cloud: a dict with status, origin, block_key, tsdf, vol_weight, vol_rgb and
    extract_ref's rows.  With a status nothing follows it."""
    trunc = 4.0 * voxel if trunc is None else trunc
    cloud = R.frames_ref(depth, pose, intr, None, depth_scale, depth_min, depth_max, 1, edge)
    status, g, key = blocks_ref(cloud["xyz"], voxel)
    out = {"status": status, "n_raw": cloud["n"], "origin": g, "block_key": key}
    if status:
        return out
    tsdf, weight, rgb = integrate_ref(depth, pose, intr, colour, g, key, voxel, trunc, depth_scale, depth_min, depth_max, edge)
    out.update(tsdf=tsdf, vol_weight=weight, vol_rgb=rgb)
    out.update(extract_ref(tsdf, weight, rgb, key, g, voxel, min_weight))
    return out
