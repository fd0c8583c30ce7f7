"""numpy restatement of csrc/thin.hip: grid thinning, statistical outlier removal and the raw index, operation by operation
in the order the contract fixes (include/pbnet_hip.h).  Every function takes a `wrong` keyword naming ONE deliberate
mistake; tests/test_thin_ref_cpu.py shows which designed case tells each mistake from the contract."""
import math

import numpy as np

F32, F64 = np.float32, np.float64
AXIS_CELLS = 1 << 21
THIN_WRONG = ("reversed", "float32", "trunc", "xmajor", "ties", "low_word")
OUTLIER_WRONG = ("sample", "lt")
RAW_WRONG = ("by_index",)


def cells(xyz, pitch, wrong=None):
    """int64 [N, 3] cells: floor((double(p) - double(min)) / pitch).  Raises ValueError as mesh.thin_points does."""
    pitch = float(pitch)
    if not (pitch > 0.0 and math.isfinite(pitch)):
        raise ValueError("pitch must be positive and finite")
    xyz = np.asarray(xyz, F32).reshape(-1, 3)
    if not np.isfinite(xyz).all():
        raise ValueError("a coordinate is NaN or infinite")
    if xyz.shape[0] == 0:
        return np.zeros((0, 3), np.int64)
    with np.errstate(over="ignore"):
        q = (xyz.astype(F64) - xyz.min(0).astype(F64)) / F64(pitch)
    if (q >= AXIS_CELLS).any():
        raise ValueError("an axis spans 2^21 cells or more")
    return (np.trunc(q) if wrong == "trunc" else np.floor(q)).astype(np.int64)


def keys(c, wrong=None):
    c = c.astype(np.uint64)
    if wrong == "xmajor":
        return (c[:, 0] << np.uint64(42)) | (c[:, 1] << np.uint64(21)) | c[:, 2]
    return (c[:, 2] << np.uint64(42)) | (c[:, 1] << np.uint64(21)) | c[:, 0]


def _run_sums(vals, start, count, wrong):
    """Per run the sum of its members in sorted order from 0.0 (float64), one member per round over all runs at once."""
    acc = np.zeros((start.shape[0], vals.shape[1]), F32 if wrong == "float32" else F64)
    for r in range(int(count.max()) if count.size else 0):
        sel = count > r
        at = start[sel] + (count[sel] - 1 - r if wrong == "reversed" else r)
        acc[sel] = acc[sel] + vals[at].astype(acc.dtype)
    return (acc / count[:, None].astype(acc.dtype)).astype(F32)


def thin(xyz, rgb=None, pitch=0.02, wrong=None):
    """mesh.thin_points on the host: dict of xyz, (rgb), count, first, inverse."""
    xyz = np.asarray(xyz, F32).reshape(-1, 3)
    n = xyz.shape[0]
    key = keys(cells(xyz, pitch, wrong), wrong)
    if wrong == "low_word":                                  # only the first of the two sorts
        order = np.argsort(key & np.uint64(0xffffffff), kind="stable")
    elif wrong == "ties":                                    # equal keys in descending index order
        order = np.lexsort((-np.arange(n), key))
    else:
        order = np.argsort(key, kind="stable")               # (key, index)
    ks = key[order]
    head = np.ones(n, bool)
    head[1:] = ks[1:] != ks[:-1]
    start = np.flatnonzero(head)
    count = np.diff(np.append(start, n)).astype(np.int32)
    inverse = np.zeros(n, np.int32)
    inverse[order] = (np.cumsum(head) - 1).astype(np.int32)
    out = {"xyz": _run_sums(xyz[order], start, count, wrong), "count": count, "first": order[start].astype(np.int32),
           "inverse": inverse}
    if rgb is not None:
        out["rgb"] = _run_sums(np.asarray(rgb, F32).reshape(-1, 3)[order], start, count, wrong)
    return out


def thin_loop(xyz, rgb=None, pitch=0.02):
    """The same by a plain Python dict of cells (Python floats are float64; math.floor; sums in index order)."""
    xyz = np.asarray(xyz, F32).reshape(-1, 3)
    n = xyz.shape[0]
    o = [float(v) for v in xyz.min(0)] if n else [0.0] * 3
    members = {}
    for i in range(n):
        c = [math.floor((float(xyz[i, a]) - o[a]) / float(pitch)) for a in range(3)]
        members.setdefault((c[2], c[1], c[0]), []).append(i)
    rows = sorted(members)
    out = {"xyz": np.zeros((len(rows), 3), F32), "count": np.zeros(len(rows), np.int32), "first": np.zeros(len(rows), np.int32),
           "inverse": np.zeros(n, np.int32)}
    if rgb is not None:
        rgb = np.asarray(rgb, F32).reshape(-1, 3)
        out["rgb"] = np.zeros((len(rows), 3), F32)
    for t, c in enumerate(rows):
        for name, src in (("xyz", xyz), ("rgb", rgb)):
            if src is None:
                continue
            for a in range(3):
                s = 0.0
                for i in members[c]:
                    s = s + float(src[i, a])
                out[name][t, a] = F32(s / float(len(members[c])))
        out["count"][t], out["first"][t] = len(members[c]), members[c][0]
        out["inverse"][members[c]] = t
    return out


# ------------------------------------------------------------------------------------------------------------ outliers
def block_sum(v):
    """The contract's sum over points: blocks of 256 consecutive entries, the tree v[j] += v[j + s] for s = 128 .. 1 inside
    a block, the block partials added in block order from 0.0."""
    v = np.asarray(v, F64)
    nb = -(-v.shape[0] // 256)
    w = np.zeros(nb * 256, F64)
    w[:v.shape[0]] = v
    w = w.reshape(nb, 256)
    s = 128
    while s >= 1:
        w[:, :s] = w[:, :s] + w[:, s:2 * s]
        s //= 2
    total = F64(0.0)
    for b in range(nb):
        total = total + w[b, 0]
    return total


def outlier(d2, ratio=2.0, wrong=None):
    """mesh.outlier_mask on the host: keep bool [N], stats float64 [3] = mu, sigma, n_valid."""
    ratio = float(ratio)
    if not (ratio >= 0.0 and math.isfinite(ratio)):
        raise ValueError("ratio must be finite and >= 0")
    d2 = np.asarray(d2, F32)
    n, k = d2.shape
    if n == 0:
        return np.zeros(0, bool), np.zeros(3, F64)
    fin = np.isfinite(d2)
    s = np.zeros(n, F64)
    with np.errstate(invalid="ignore", divide="ignore"):
        for r in range(k):
            s = np.where(fin[:, r], s + np.sqrt(d2[:, r].astype(F64)), s)
        cnt = fin.sum(1)
        valid = cnt > 0
        m = np.where(valid, s / cnt.astype(F64), 0.0)
        n_valid = F64(valid.sum())
        mu = block_sum(m) / n_valid
        d = m - mu
        var = block_sum(np.where(valid, d * d, 0.0)) / (n_valid - 1.0 if wrong == "sample" else n_valid)
        sigma = np.sqrt(var)
        thr = mu + F64(ratio) * sigma
        keep = valid & ((m < thr) if wrong == "lt" else (m <= thr))
    return keep, np.array([mu, sigma, n_valid], F64)


def outlier_loop(d2, ratio=2.0):
    """The same with Python floats and explicit loops (the tree included)."""
    d2 = np.asarray(d2, F32)
    n, k = d2.shape
    m, valid = [0.0] * n, [False] * n
    for i in range(n):
        s, c = 0.0, 0
        for r in range(k):
            if math.isfinite(float(d2[i, r])):
                s, c = s + math.sqrt(float(d2[i, r])), c + 1
        if c:
            m[i], valid[i] = s / c, True

    def total(vals):
        tot = 0.0
        for b in range(0, n, 256):
            v = [vals[b + j] if b + j < n else 0.0 for j in range(256)]
            s = 128
            while s >= 1:
                for j in range(s):
                    v[j] = v[j] + v[j + s]
                s //= 2
            tot = tot + v[0]
        return tot

    nv = sum(valid)
    if n == 0:
        return np.zeros(0, bool), np.zeros(3, F64)
    mu = total(m) / nv if nv else float("nan")
    sq = total([(m[i] - mu) * (m[i] - mu) if valid[i] else 0.0 for i in range(n)])
    sigma = math.sqrt(sq / nv) if nv else float("nan")
    thr = mu + float(ratio) * sigma
    return np.array([valid[i] and m[i] <= thr for i in range(n)], bool), np.array([mu, sigma, nv], F64)


# ----------------------------------------------------------------------------------------------------------- raw index
def raw_index(inverse, keep, idx, wrong=None):
    """mesh.raw_index on the host: int32 [N_raw]."""
    inverse, keep, idx = np.asarray(inverse, np.int64), np.asarray(keep, bool), np.asarray(idx, np.int64)
    m = keep.shape[0]
    before = np.cumsum(keep) - keep
    row = np.full(m, -1, np.int64)
    for t in range(m):
        if keep[t]:
            row[t] = before[t]
            continue
        kept = [int(j) for j in idx[t] if 0 <= j < m and keep[j]]
        if kept:
            row[t] = before[min(kept) if wrong == "by_index" else kept[0]]
    out = np.full(inverse.shape[0], -1, np.int32)
    ok = (inverse >= 0) & (inverse < m)
    out[ok] = row[inverse[ok]]
    return out


def carry(labels, raw, fill=-1):
    labels, raw = np.asarray(labels), np.asarray(raw, np.int64)
    out = np.full((raw.shape[0],) + labels.shape[1:], fill, labels.dtype)
    out[raw >= 0] = labels[raw[raw >= 0]]
    return out
