"""A second statement of depth-frame fusion, block by block and voxel by voxel in Python, with switches: every switch is a
plausible wrong reading of the contract in include/pbnet_hip.h ("Depth-frame fusion").  With no switch it must agree with
tests/fuse_ref.py bit for bit; with one it must disagree on at least one designed case (tests/test_fuse_cases_cpu.py holds
the kill matrix)."""
import math

import numpy as np

import frames_ref as R
import fuse_ref as FR

F32, F64 = np.float32, np.float64

MUTANTS = ("centre_no_half", "floor", "half_up", "r_not_rt", "skip_equal_trunc", "no_clamp", "euclidean", "cross_product",
           "r_from_n", "unobserved_zero", "weight_strict", "axis_reversed", "dilate6")
EXTRACT_MUTANTS = ("cross_product", "r_from_n", "unobserved_zero", "weight_strict", "axis_reversed")
_SIX = [(0, 0, 0), (1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]


def _key(b):
    return (int(b[2]) << 42) | (int(b[1]) << 21) | int(b[0])


def _unkey(k):
    m = (1 << 21) - 1
    return int(k) & m, (int(k) >> 21) & m, (int(k) >> 42) & m


def blocks(xyz, voxel, mutant=None):
    """Allocation with Python sets: (origin, sorted keys)."""
    xyz = np.asarray(xyz, F32).reshape(-1, 3)
    if xyz.shape[0] == 0:
        return np.zeros(3, F64), np.zeros(0, np.int64)
    B = 8.0 * float(voxel)
    g = [float(xyz[:, a].min()) - B for a in range(3)]
    near = _SIX if mutant == "dilate6" else [(x, y, z) for z in (-1, 0, 1) for y in (-1, 0, 1) for x in (-1, 0, 1)]
    keys = set()
    for b in {tuple(max(int(math.floor((float(p[a]) - g[a]) / B)), 1) for a in range(3)) for p in xyz}:
        for d in near:
            keys.add(_key((b[0] + d[0], b[1] + d[1], b[2] + d[2])))
    return np.array(g, F64), np.array(sorted(keys), np.int64)


def integrate(depth, pose, intr, colour, g, keys, voxel, trunc, depth_scale, depth_min, depth_max, edge, mutant=None):
    """One block at a time: a [512] vector of voxels against the frames in ascending order."""
    depth = np.asarray(depth)
    n_f, h, w = depth.shape
    pose = np.asarray(pose, F64).reshape(n_f, 4, 4)
    intr = np.broadcast_to(np.asarray(intr, F64), (n_f, 4))
    z_all, ok_all = FR.valid_depth(depth, depth_scale, depth_min, depth_max, edge)
    m = len(keys)
    tsdf, weight = np.zeros((m, 512), F32), np.zeros((m, 512), np.int32)
    rgb = np.zeros((m, 512, 3), F32) if colour is not None else None
    idx = np.arange(512)
    local = [idx & 7, (idx >> 3) & 7, idx >> 6]
    half = 0.0 if mutant == "centre_no_half" else 0.5
    live = [f for f in range(n_f) if np.isfinite(pose[f, :3, :]).all() and h * w]
    for t, key in enumerate(keys):
        b = _unkey(key)
        p = [g[a] + ((8 * b[a] + local[a]).astype(F64) + half) * float(voxel) for a in range(3)]
        S, Wt, C = np.zeros(512), np.zeros(512, np.int64), np.zeros((512, 3))
        for f in live:
            Rm, tr = pose[f, :3, :3], pose[f, :3, 3]
            Rt = Rm if mutant == "r_not_rt" else Rm.T
            fx, fy, cx, cy = (float(v) for v in intr[f])
            with np.errstate(all="ignore"):
                tc = [-((Rt[r, 0] * tr[0] + Rt[r, 1] * tr[1]) + Rt[r, 2] * tr[2]) for r in range(3)]
                pc = [((Rt[r, 0] * p[0] + Rt[r, 1] * p[1]) + Rt[r, 2] * p[2]) + tc[r] for r in range(3)]
                zc = pc[2]
                uf, vf = (fx * pc[0]) / zc + cx, (fy * pc[1]) / zc + cy
                if mutant == "floor":
                    ur, vr = np.floor(uf), np.floor(vf)
                elif mutant == "half_up":
                    ur, vr = np.floor(uf + 0.5), np.floor(vf + 0.5)
                else:
                    ur, vr = np.rint(uf), np.rint(vf)
                for i in np.flatnonzero((zc > 0.0) & (ur >= 0.0) & (ur <= w - 1.0) & (vr >= 0.0) & (vr <= h - 1.0)):
                    u, v = int(ur[i]), int(vr[i])
                    if not ok_all[f, v, u]:
                        continue
                    s = float(z_all[f, v, u]) - float(zc[i])
                    if mutant == "euclidean":
                        s = s * (math.sqrt(float(pc[0][i]) ** 2 + float(pc[1][i]) ** 2 + float(zc[i]) ** 2) / float(zc[i]))
                    if s < -trunc or (mutant == "skip_equal_trunc" and s <= -trunc):
                        continue
                    d = s / trunc if mutant == "no_clamp" else min(1.0, s / trunc)
                    S[i] = S[i] + d
                    Wt[i] += 1
                    if colour is not None:
                        C[i] = C[i] + colour[f, v, u].astype(F64)
        seen = Wt > 0
        with np.errstate(all="ignore"):
            tsdf[t] = np.where(seen, S / Wt, 0.0).astype(F32)
            if rgb is not None:
                rgb[t] = np.where(seen[:, None], C / Wt[:, None], 0.0).astype(F32)
        weight[t] = Wt
    return tsdf, weight, rgb


def extract(tsdf, weight, rgb, keys, g, voxel, min_weight, mutant=None):
    """Voxel by voxel in Python floats, neighbours through a dict of block coordinates."""
    rank = {_unkey(k): t for t, k in enumerate(keys)}
    D = np.asarray(tsdf, F32).astype(F64)
    W = np.asarray(weight)
    voxel = float(voxel)

    def at(b, x, y, z):
        """(observed, block rank, in-block index) of voxel (x, y, z) relative to block b."""
        nb = (b[0] + x // 8, b[1] + y // 8, b[2] + z // 8)
        t = rank.get(nb)
        if t is None:
            return False, 0, 0
        i = ((z % 8) * 8 + (y % 8)) * 8 + (x % 8)
        w = int(W[t, i])
        return (w > min_weight if mutant == "weight_strict" else w >= min_weight), t, i

    def grad(b, x, y, z, Dx):
        G = []
        for e in ((1, 0, 0), (0, 1, 0), (0, 0, 1)):
            op, tp, ip = at(b, x + e[0], y + e[1], z + e[2])
            om, tm, im = at(b, x - e[0], y - e[1], z - e[2])
            miss = 0.0 if mutant == "unobserved_zero" else Dx
            G.append((float(D[tp, ip]) if op else miss) - (float(D[tm, im]) if om else miss))
        return G

    rows = {k: [] for k in ("xyz", "nl", "rgb", "weight", "voxel_id")}
    axes = (2, 1, 0) if mutant == "axis_reversed" else (0, 1, 2)
    for t, key in enumerate(keys):
        b = _unkey(key)
        for i in np.flatnonzero(W[t] >= 1):
            i = int(i)
            x, y, z = i & 7, (i >> 3) & 7, i >> 6
            if not at(b, x, y, z)[0]:
                continue
            Dq = float(D[t, i])
            for a in axes:
                e = (int(a == 0), int(a == 1), int(a == 2))
                on, tn, i_n = at(b, x + e[0], y + e[1], z + e[2])
                if not on:
                    continue
                Dn = float(D[tn, i_n])
                if (Dq * Dn < 0.0) if mutant == "cross_product" else ((Dq < 0.0) != (Dn < 0.0)):
                    r = (Dn if mutant == "r_from_n" else Dq) / (Dq - Dn)
                    p = [float(g[c]) + (float(8 * b[c] + (x, y, z)[c]) + 0.5) * voxel for c in range(3)]
                    p[a] = p[a] + r * voxel
                    Gq, Gn = grad(b, x, y, z, Dq), grad(b, x + e[0], y + e[1], z + e[2], Dn)
                    gv = [Gq[c] + r * (Gn[c] - Gq[c]) for c in range(3)]
                    ln = math.sqrt((gv[0] * gv[0] + gv[1] * gv[1]) + gv[2] * gv[2])
                    rows["xyz"].append(p)
                    rows["nl"].append([c / ln for c in gv] if ln > 0.0 and math.isfinite(ln) else [0.0, 0.0, 0.0])
                    rows["weight"].append(min(int(W[t, i]), int(W[tn, i_n])))
                    rows["voxel_id"].append((t * 512 + i) * 3 + a)
                    if rgb is not None:
                        cq, cn = rgb[t, i].astype(F64), rgb[tn, i_n].astype(F64)
                        rows["rgb"].append(cq + r * (cn - cq))
    out = {"xyz": np.array(rows["xyz"], F64).reshape(-1, 3).astype(F32), "nl": np.array(rows["nl"], F64).reshape(-1, 3).astype(F32),
           "weight": np.array(rows["weight"], np.int32), "voxel_id": np.array(rows["voxel_id"], np.int64), "n": len(rows["weight"])}
    if rgb is not None:
        out["rgb"] = np.array(rows["rgb"], F64).reshape(-1, 3).astype(F32)
    return out


def fuse(case, mutant=None):
    """fuse_ref's dict of a case by this statement (no status: the designed cases have none)."""
    depth, pose, intr, colour = case["depth"], case["pose"], case["intr"], case.get("colour")
    kw = dict(voxel=0.02, trunc=None, depth_scale=1000.0, depth_min=0.0, depth_max=math.inf, edge=None, min_weight=1)
    kw.update(case.get("kw", {}))
    trunc = 4.0 * kw["voxel"] if kw["trunc"] is None else kw["trunc"]
    cloud = R.frames_ref(depth, pose, intr, None, kw["depth_scale"], kw["depth_min"], kw["depth_max"], 1, kw["edge"])
    g, keys = blocks(cloud["xyz"], kw["voxel"], mutant)
    tsdf, weight, rgb = integrate(depth, pose, intr, colour, g, keys, kw["voxel"], trunc, kw["depth_scale"], kw["depth_min"],
                                  kw["depth_max"], kw["edge"], mutant)
    out = {"status": 0, "n_raw": cloud["n"], "origin": g, "block_key": keys, "tsdf": tsdf, "vol_weight": weight, "vol_rgb": rgb}
    out.update(extract(tsdf, weight, rgb, keys, g, kw["voxel"], kw["min_weight"], mutant))
    return out


def same(a, b):
    if sorted(a) != sorted(b):
        return False
    for k in a:
        if a[k] is None or b[k] is None:
            if a[k] is not b[k]:
                return False
            continue
        x, y = np.asarray(a[k]), np.asarray(b[k])
        if x.dtype != y.dtype or x.shape != y.shape or x.tobytes() != y.tobytes():
            return False
    return True
