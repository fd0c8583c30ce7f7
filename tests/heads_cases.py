"""Inputs shared by tests/test_heads_ref_cpu.py (which shows that they separate an honest fp32 kernel from a subtly wrong one) and
tests/test_heads_pool_iou_gpu.py (which runs the kernels on them).  Numpy only, fixed seeds.  16-bit inputs are float32 arrays whose
values are already representable in the type, so the conversion on the device is exact."""
import functools

import numpy as np

import heads_ref as R

DTYPES = ("fp32", "bf16", "fp16")


def _as(v, dtype):
    return R.round_to(np.asarray(v, np.float64), dtype).astype(np.float32)


# ---- heads --------------------------------------------------------------------------------------------------------------
HEAD_ROWS = 16005                    # 1001 blocks of 16 rows, the last one of 5: 63 workgroups, about 4 blocks per wave
HEAD_N = (1, 15, 16, 17, HEAD_ROWS)
HEAD_HIDDEN = (16, 32)
HEAD_OUT_MFMA = (1, 3, 15, 16, 17, 20, 31, 32)
HEAD_OUT_SCALAR = (33, 40)
HEAD_FORMS = ("none", "a", "ab")
BN_EPS = 1e-5
CAP_ROWS, CAP_SLAB = 2097152 + 21, 4096      # 8192 workgroups x 4 waves x 4 blocks x 16 rows = 2 097 152: beyond the cap


@functools.lru_cache(maxsize=None)
def head_params(hidden, n_out):
    """fp32 parameters of Linear(32, hidden, no bias) -> BatchNorm(eval) -> PReLU(hidden slopes) -> Linear(hidden, n_out)."""
    rng = np.random.default_rng(1000 * hidden + n_out)
    f4 = np.float32
    var = rng.uniform(0.3, 2.0, hidden)
    var[rng.permutation(hidden)[:3]] = (1e-3, 3e-3, 2e-2)
    slope = rng.permutation(np.linspace(0.05, 0.9, hidden))          # distinct
    slope[rng.integers(hidden)] = -0.3                               # one negative
    w2 = rng.normal(0, 1, (n_out, hidden)) / np.sqrt(hidden) * np.minimum(1.0, np.sqrt(var))   # keeps the outputs near +-2
    p = dict(w1=rng.normal(0, 1, (hidden, 32)) / np.sqrt(32), bn_weight=rng.uniform(0.5, 1.5, hidden),
             bn_bias=rng.normal(0, 0.2, hidden), mean=rng.normal(0, 0.3, hidden), var=var, slope=slope, w2=w2,
             b2=rng.normal(0, 0.5, n_out))
    return {k: np.ascontiguousarray(v, f4) for k, v in p.items()}


def fold_bn(p, eps=BN_EPS):
    """float64 (scale, shift) of the eval-mode BatchNorm."""
    f8 = np.float64
    scale = p["bn_weight"].astype(f8) / np.sqrt(p["var"].astype(f8) + eps)
    return scale, p["bn_bias"].astype(f8) - p["mean"].astype(f8) * scale


def fold_bn_bounds(p, eps=BN_EPS):
    """How far fp32 (scale, shift) computed as w / sqrt(var + eps) and b - mean * scale may lie from fold_bn: one rounding each for the
    add, the square root and the divide; one each for the product and the subtraction."""
    scale, shift = fold_bn(p, eps)
    e_scale = R.gamma(3) * np.abs(scale)
    m = np.abs(p["mean"].astype(np.float64))
    e_shift = m * e_scale + R.U * m * (np.abs(scale) + e_scale) + R.U * (np.abs(shift) + 2 * m * e_scale)
    return e_scale, e_shift


@functools.lru_cache(maxsize=None)
def head_x(dtype, rows=HEAD_ROWS):
    x = np.random.default_rng(7).normal(0, 1, (rows, 32))
    x[::97] *= 8.0                                                    # a few large rows
    return _as(x, dtype)


@functools.lru_cache(maxsize=None)
def head_index(form, n):
    """(idx_a, idx_b, rows of the slab that are read): a few entries of either level are -1 (the row reads as zeros)."""
    rng = np.random.default_rng(31 * n + len(form))
    if form == "none":
        return None, None
    if form == "a":
        a = rng.integers(0, HEAD_ROWS, n)
        if n >= 15:
            a[rng.permutation(n)[:max(n // 50, 1)]] = -1
        return a.astype(np.int64), None
    b = rng.integers(0, HEAD_ROWS, 3000)
    b[::41] = -1
    a = rng.integers(0, 3000, n)
    if n >= 15:
        a[rng.permutation(n)[:max(n // 50, 1)]] = -1
    return a.astype(np.int64), b.astype(np.int64)


def head_cases():
    """(n, sigmoid, form) of every launch of one (dtype, hidden, n_out) head."""
    return [(n, s, f) for n in HEAD_N for s in (False, True) for f in HEAD_FORMS]


@functools.lru_cache(maxsize=None)
def cap_index():
    return np.random.default_rng(5).integers(0, CAP_SLAB, CAP_ROWS).astype(np.int64)


# ---- class scores -------------------------------------------------------------------------------------------------------
SEM_N = (1, 1023, 1025, 2049)
SEM_CLS = (2, 20, 32)
MAX_SCENES = 8                       # include/pbnet_hip.h PBN_MAX_SCENES (tests/test_abi.py pins the header)


@functools.lru_cache(maxsize=None)
def sem_scores(dtype, n, n_cls, nb):
    """(score float32 [n, n_cls] representable in dtype, batch int32 [n]).  Row i is of kind (i + n_cls) % 16:
    0 / 1 / 2 the maximum tied at the first / a middle / the last position and one more; 3 all equal; 4 -inf in every entry but
    two; 5 +-80 (fp32 only); 6 +-100; 7 +-100 with the maximum tied; the rest random."""
    rng = np.random.default_rng(100 * n + n_cls + nb)
    s = rng.normal(0, 3, (n, n_cls))
    s = R.round_to(s, dtype)
    for i in range(n):
        kind = (i + n_cls) % 16
        top = np.ceil(s[i].max()) + 1.0
        other = int(rng.integers(n_cls))
        if kind == 0:
            s[i, 0] = s[i, other] = top
        elif kind == 1:
            s[i, n_cls // 2] = s[i, other] = top
        elif kind == 2:
            s[i, n_cls - 1] = s[i, other] = top
        elif kind == 3:
            s[i, :] = s[i, 0]
        elif kind == 4:
            keep = s[i, [other, (other + 1) % n_cls]].copy()
            s[i, :] = -np.inf
            s[i, [other, (other + 1) % n_cls]] = keep
        elif kind in (5, 6, 7) and not (kind == 5 and dtype != "fp32"):
            big = 80.0 if kind == 5 else 100.0
            s[i, :] = -big
            s[i, other] = big
            if kind == 7:
                s[i, (other + 1) % n_cls] = big
    return s.astype(np.float32), rng.integers(0, nb, n).astype(np.int32)


# ---- segment pooling ----------------------------------------------------------------------------------------------------
POOL_CHANNELS = (4, 16, 20, 32, 48, 96)
POOL_SEGS = (1, 7, 17, 1024, 1500)
POOL_LONG = 20011


def pool_split(n_seg):
    return min(max(1024 // n_seg, 1), 64)


def pool_rps(n_seg, channels, dtype):
    """Rows per sweep of the two-pass kernel: 256 threads / (16-byte vectors per row); 8 row groups in the single-pass kernel
    (one slice, or a row that is no whole number of vectors)."""
    row_bytes = channels * (4 if dtype == "fp32" else 2)
    return 256 // (row_bytes // 16) if row_bytes % 16 == 0 and pool_split(n_seg) > 1 else 8


def pool_lens(n_seg, channels, dtype):
    split, rps = pool_split(n_seg), pool_rps(n_seg, channels, dtype)
    edges = [0, 1, split - 1, split, split + 1, 4 * rps - 1, 4 * rps, 4 * rps + 1, 8 * rps - 1, 8 * rps + 1, 3, 130, 2]
    if split > 1:
        edges += [split * 4 * rps - 1, split * 4 * rps + 1]          # every slice one row short of / past 4 sweeps
    if n_seg == 1:
        return [POOL_LONG]
    if n_seg == 7:
        return [POOL_LONG, 0, 1, split - 1, split + 1, 4 * rps + 1, 8 * rps - 1]
    if n_seg == 17:
        return ([POOL_LONG] + edges + [777])[:17]
    rng = np.random.default_rng(n_seg)
    return edges + [int(v) for v in rng.integers(0, 40, n_seg - len(edges))]


@functools.lru_cache(maxsize=None)
def pool_feats(family, dtype, rows, cols):
    rng = np.random.default_rng(rows + cols)
    if family == "exact":
        return (rng.integers(-64, 65, (rows, cols)) / 8.0).astype(np.float32)    # exact in all three types
    return _as(rng.normal(0, 1, (rows, cols)), dtype)


# ---- IoU targets --------------------------------------------------------------------------------------------------------
IOU_CASES = [(1, 1), (1, 64), (37, 1), (37, 64), (257, 1), (257, 64), (20000, 5), (3, 32768 + 5)]     # (n_inst, n_prop)


@functools.lru_cache(maxsize=None)
def iou_case(n_inst, n_prop):
    """dict(idx i32, off i32, labels i64, pointnum i32, scores f32 [len(idx), 1], planted).  Labels hold -100 and values >= n_inst
    (ignored); pointnum holds entries above 2^24; scores hold exactly 0.5 (excluded) and the next float above it.  With 64 proposals
    the first three are planted: best IoU on the 0.5 side (inter = uni / 2: the 1e-5 keeps it below), one above, one with two
    instances tied above 0.5."""
    rng = np.random.default_rng(1000 * n_inst + n_prop)
    n_pts = 6000
    labels = rng.integers(-1, n_inst + 2, n_pts).astype(np.int64)
    labels[labels < 0] = -100
    pointnum = np.array([np.count_nonzero(labels == i) for i in range(n_inst)] if n_inst <= 300
                        else np.bincount(labels[(labels >= 0) & (labels < n_inst)], minlength=n_inst), np.int64)
    if n_prop > 30000:
        lens = rng.integers(1, 3, n_prop)
    else:
        lens = rng.integers(0, 300, n_prop)
        if n_prop > 4:
            lens[4] = 0
    planted = n_prop == 64
    groups = []
    if planted:
        L = 10
        if n_inst == 1:
            spec = [[(0, L)], [(0, 19)]]                          # uni = 20 either way: 10 / 20 and 19 / 20
            pointnum[0] = 2 * L
        else:
            k = [0, 1, 2, 3] if n_inst >= 4 else [0, 1, 0, 1]
            spec = [[(k[0], L)], [(k[1], L)]]
            pointnum[k[0]], pointnum[k[1]] = 2 * L, L + 1
            if n_inst >= 4:
                spec.append([(k[3], L), (k[2], L)])               # the later instance's points come first in the proposal
                pointnum[k[2]] = pointnum[k[3]] = 1               # uni = 20 + 1 - 10: 10 / 11 for both
        for g in spec:
            pts = []
            for lab, cnt in g:
                pts += list(range(len(labels), len(labels) + cnt))
                labels = np.concatenate([labels, np.full(cnt, lab, np.int64)])
            groups.append(np.array(pts, np.int64))
            lens[len(groups) - 1] = len(pts)
    for j, big in enumerate((2 ** 24 + 1, 2 ** 25 + 3, 2 ** 26 + 5, 2 ** 24 + 3)):
        if n_inst > 5 + 6 * j:
            pointnum[5 + 6 * j] = big
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    idx = rng.integers(0, n_pts, int(off[-1])).astype(np.int32)
    scores = rng.uniform(0, 1, int(off[-1])).astype(np.float32)
    scores[::7] = 0.5
    scores[3::7] = np.nextafter(np.float32(0.5), np.float32(1))
    for j, pts in enumerate(groups):
        idx[off[j]:off[j + 1]] = pts
        scores[off[j]:off[j + 1]] = 0.9
    return dict(idx=idx, off=off, labels=labels, pointnum=pointnum.astype(np.int32), scores=scores.reshape(-1, 1),
                planted=len(groups))
