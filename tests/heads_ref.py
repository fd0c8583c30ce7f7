"""Plain numpy float64 restatements of the ops between the backbone and the losses / the post-processing, each with the
error bound an honest fp32 kernel must meet:

  mlp_rows      the two-layer heads (csrc/heads.hip k_mlp_rows / k_mlp_rows_mfma)
  sem_argmax    arg-max class, own-class softmax score, [class, batch] table, per-block class histogram (k_sem_argmax_table)
  segment_pool  per-segment maximum and mean (csrc/pool.hip)
  iou / mask_label   proposal x instance IoU and the mask targets (csrc/iou.hip), bit-exact

Bounds: u = 2^-24 is the unit roundoff of fp32 and gamma(k) = k u / (1 - k u) bounds a sum of k products (or k + 1 addends)
accumulated in fp32 in ANY order, fused or not.  Nothing here is fitted to a kernel's output except EXP_DIV_ULPS, whose
source is written next to it.  No torch: every input is a numpy array; 16-bit values arrive widened (widen_bf16 for raw
bfloat16 bit patterns, astype for float16), which is exact."""
import numpy as np

U = 2.0 ** -24

# Allowance, in fp32 ulps of the result, for expf followed by one add and one divide: the sigmoid 1 / (1 + expf(-a)) of the heads,
# and expf and the divide in 1 / sum expf(v - best) of the class scores (the summation itself is in gamma(n_cls)).  The ROCm
# installation documents no ulp figure for expf, so it was measured once on an MI355X (tests/test_heads_pool_iou_gpu.py
# test_class_scores prints it): with n_cls = 2 the kernel computes 1 / (expf(0) + expf(-t)), exactly the heads' sigmoid expression and
# nothing else, and over every fp32 two-class input set of tests/heads_cases.py (t from 0 to 200) its largest deviation from this
# file's float64 value was 1.474 ulps.  Twice that is allowed.  (At n_cls = 20 / 32, where the deviation includes the summation that
# gamma(n_cls) already covers, 6.62 / 8.14 ulps were measured.)
MEASURED_EXP_DIV_ULPS = 1.474
EXP_DIV_ULPS = 2.0 * MEASURED_EXP_DIV_ULPS

# (significand bits, minimum normal exponent, maximum exponent)
FORMATS = {"fp32": (24, -126, 127), "bf16": (8, -126, 127), "fp16": (11, -14, 15)}


def gamma(k):
    k = np.asarray(k, np.float64)
    return k * U / (1.0 - k * U)


def round_to(v, fmt):
    """Round float64 to the nearest value of the format, ties to even, ONE rounding (no detour through fp32); the result is
    returned as float64.  Subnormals are kept; beyond the largest finite value + half a step the result is infinite."""
    p, emin, emax = FORMATS[fmt]
    v = np.asarray(v, np.float64)
    out = v.copy()
    fin = np.isfinite(v) & (v != 0)
    m, e = np.frexp(np.where(fin, v, 1.0))               # |v| = m 2^e, m in [0.5, 1): exponent of the leading bit is e - 1
    q = np.ldexp(1.0, np.maximum(e - 1, emin) - (p - 1))  # spacing of the format at v
    r = np.rint(v / q) * q                               # division by a power of two is exact; rint rounds ties to even
    big = np.ldexp(2.0 - np.ldexp(1.0, 1 - p), emax)
    r = np.where(np.abs(r) > big, np.copysign(np.inf, r), r)
    return np.where(fin, r, out)


def ulp32(v):
    """Spacing of fp32 at |v| (2^-149 in the subnormal range)."""
    v = np.abs(np.asarray(v, np.float64))
    _, e = np.frexp(np.where((v > 0) & np.isfinite(v), v, 1.0))
    return np.where(v > 0, np.ldexp(1.0, np.maximum(e - 1, -126) - 23), 2.0 ** -149)


def widen_bf16(bits):
    """uint16 bfloat16 bit patterns -> float64, exactly."""
    return (np.asarray(bits, np.uint16).astype(np.uint32) << 16).view(np.float32).astype(np.float64)


def accept(got, value, bound, dtype):
    """Boolean array: which elements of `got` (widened to float64) an honest kernel could have produced.
    fp32: |got - value| <= bound.  bf16 / fp16: got lies in [round(value - bound), round(value + bound)] -- rounding to nearest
    even is monotone, so this admits the ONE final rounding and nothing more.  An infinite value must be met exactly and a NaN
    value (the mean of an empty segment) by a NaN."""
    got = np.asarray(got, np.float64)
    value = np.asarray(value, np.float64)
    bound = np.broadcast_to(np.asarray(bound, np.float64), value.shape)
    assert got.shape == value.shape
    with np.errstate(invalid="ignore"):
        if dtype == "fp32":
            ok = np.abs(got - value) <= bound
        else:
            ok = (got >= round_to(value - bound, dtype)) & (got <= round_to(value + bound, dtype))
        ok = np.where(np.isinf(value), got == value, ok)
    return np.where(np.isnan(value), np.isnan(got), ok)


# ---- two-layer head -----------------------------------------------------------------------------------------------------

def resolve_rows(n_x, idx_a, idx_b, in_rows):
    """Input row of every output row, -1 where it reads as zeros (an index < 0 at either level, or a row >= in_rows)."""
    row = np.arange(n_x, dtype=np.int64) if idx_a is None else np.asarray(idx_a, np.int64).copy()
    if idx_b is not None:
        ib = np.asarray(idx_b, np.int64)
        row = np.where(row >= 0, ib[np.clip(row, 0, len(ib) - 1)], row)
    return np.where((row >= 0) & (row < in_rows), row, -1)


def mlp_rows(x, idx_a, idx_b, in_rows, w1, scale, shift, slope, w2, b2, sigmoid):
    """out[i] = act(W2 . prelu(scale * (W1 . x[row_i]) + shift) + b2), row_i = idx_b[idx_a[i]] (either None = identity); returns
    (value, bound), both [n, n_out] float64.  bound holds for every evaluation that keeps the operands in fp32, accumulates
    each dot product in fp32 in any order and rounds once per operation."""
    f8 = np.float64
    x = np.asarray(x, f8)
    in_rows = x.shape[0] if in_rows is None else int(in_rows)
    w1, scale, shift, slope, w2 = (np.asarray(a, f8) for a in (w1, scale, shift, slope, w2))
    hid, n_out = w1.shape[0], w2.shape[0]
    b2 = np.zeros(n_out, f8) if b2 is None else np.asarray(b2, f8)
    xs = np.concatenate([x[:in_rows], np.zeros((1, x.shape[1]), f8)])           # last row: what a row outside the slab reads
    # layer 1: a = W1 x, |a^ - a| <= gamma(33) sum |w1| |x|
    a = xs @ w1.T
    e_a = gamma(33) * (np.abs(xs) @ np.abs(w1).T)
    # t = a * scale + shift in one fused step: the exact step on a^ is off by |scale| e_a, then one rounding
    t = a * scale + shift
    e_t = np.abs(scale) * e_a
    e_t = e_t + U * (np.abs(t) + e_t)
    # PReLU: factor 1 on the positive side, |slope| on the negative side (one more rounding there); where the sign of t is not
    # determined (|t| <= e_t) both results are bounded by max(1, |slope|) (|t| + e_t) in magnitude
    asl = np.abs(slope)
    h = np.where(t >= 0, t, t * slope)
    e_pos = e_t
    e_neg = asl * e_t + U * asl * (np.abs(t) + e_t)
    e_mix = np.maximum(1.0, asl) * (2.0 * np.abs(t) + e_t) * (1.0 + U)
    e_h = np.where(np.abs(t) > e_t, np.where(t >= 0, e_pos, e_neg), e_mix)
    # layer 2: bias + hid products, gamma(hid + 1) on the magnitudes actually summed, plus the propagated e_h
    o = h @ w2.T + b2
    e_o = gamma(hid + 1) * (np.abs(b2) + (np.abs(h) + e_h) @ np.abs(w2).T) + e_h @ np.abs(w2).T
    if sigmoid:
        with np.errstate(over="ignore"):
            s = 1.0 / (1.0 + np.exp(-o))
        e_o = 0.25 * e_o + EXP_DIV_ULPS * ulp32(s)       # |sigmoid'| <= 1/4
        o = s
    n = x.shape[0] if idx_a is None else len(idx_a)
    row = resolve_rows(n, idx_a, idx_b, in_rows)
    row = np.where(row < 0, in_rows, row)
    return o[row], e_o[row]


# ---- class scores -------------------------------------------------------------------------------------------------------

SEL_BLOCK = 1024


def sem_argmax(score, batch, nb):
    """score [n, n_cls] (widened, no NaN), batch int [n] or None.  Returns (arg i64[n] -- FIRST maximum, prob f64[n] =
    1 / sum exp(v - best), prob_bound f64[n], table i64[n_cls, nb], block_hist i64[ceil(n / 1024), n_cls])."""
    s = np.asarray(score, np.float64)
    n, n_cls = s.shape
    arg = np.argmax(s, 1)                                 # numpy documents: the first occurrence of the maximum
    best = s[np.arange(n), arg]
    with np.errstate(invalid="ignore"):
        d = s - best[:, None]                             # <= 0; -inf where the entry is -inf (best is finite or all are equal)
    d = np.where(np.isnan(d), 0.0, d)                     # -inf - -inf: an all -inf row is "all equal"; not generated
    e = np.exp(d)
    tot = e.sum(1)
    prob = 1.0 / tot
    # fp32: d^ = d (1 + u) -> exp(d^) = exp(d) (1 + u |d|); each expf and the final divide are in EXP_DIV_ULPS; the sum of
    # n_cls terms in any order gamma(n_cls)
    with np.errstate(invalid="ignore"):
        de = np.where(np.isfinite(d), np.abs(d) * e, 0.0)
    rel = gamma(n_cls) + U * de.sum(1) / tot
    bound = prob * rel + EXP_DIV_ULPS * ulp32(prob)
    b = np.zeros(n, np.int64) if batch is None else np.asarray(batch, np.int64)
    keep = (b >= 0) & (b < nb)
    table = np.bincount(arg[keep] * nb + b[keep], minlength=n_cls * nb).reshape(n_cls, nb)
    n_blk = max((n + SEL_BLOCK - 1) // SEL_BLOCK, 1)
    hist = np.bincount((np.arange(n) // SEL_BLOCK) * n_cls + arg, minlength=n_blk * n_cls).reshape(n_blk, n_cls)
    return arg.astype(np.int64), prob, bound, table, hist


# ---- segment pooling ----------------------------------------------------------------------------------------------------

def segment_pool(feats, seg_start):
    """feats [n, C] widened, seg_start int [S + 1].  Returns (max [S, C] exact, mean [S, C] float64, bound [S, C]): an fp32 sum in
    any order (len - 1 additions) and one division give |avg - mean| <= gamma(len - 1) sum |v| / len + u |mean|.  An empty
    segment: max -inf, mean NaN."""
    f = np.asarray(feats, np.float64)
    ss = np.asarray(seg_start, np.int64)
    n_seg, c = len(ss) - 1, f.shape[1]
    mx = np.full((n_seg, c), -np.inf)
    mean = np.full((n_seg, c), np.nan)
    bound = np.zeros((n_seg, c))
    for b in range(n_seg):
        seg = f[ss[b]:ss[b + 1]]
        ln = len(seg)
        if ln == 0:
            continue
        mx[b] = seg.max(0)
        mean[b] = seg.sum(0) / ln
        bound[b] = gamma(ln - 1) * np.abs(seg).sum(0) / ln + U * np.abs(mean[b])
    return mx, mean, bound


def segment_sums(feats, seg_start):
    """The float64 sums (exact for the k / 8 family: every partial sum is an integer multiple of 1/8 below 2^24 / 8)."""
    f = np.asarray(feats, np.float64)
    ss = np.asarray(seg_start, np.int64)
    return np.stack([f[ss[b]:ss[b + 1]].sum(0) for b in range(len(ss) - 1)])


# ---- IoU targets --------------------------------------------------------------------------------------------------------

def _counts(idx, off, labels, n_inst, mask_scores, mode, p):
    pts = np.asarray(idx[off[p]:off[p + 1]], np.int64)
    if mode == 1:
        pts = pts[np.asarray(mask_scores, np.float32).reshape(-1)[off[p]:off[p + 1]] > np.float32(0.5)]
    lab = np.asarray(labels, np.int64)[pts].astype(np.int32)          # the (int) cast of the original
    lab = lab[(lab >= 0) & (lab < n_inst)]
    total = len(pts) if mode == 1 else int(off[p + 1] - off[p])
    return np.bincount(lab, minlength=n_inst).astype(np.int64), total


def iou(idx, off, labels, pointnum, mask_scores=None, mode=-1):
    """proposals_iou [P, I] float32.  mode -1: get_iou; 0: the same through cal_iou_and_masklabel; 1: only the points whose mask score
    is > 0.5 count, in the intersection AND in the proposal's size.  inter and uni are rounded to fp32 first, the 1e-5 and the
    quotient are double, the result is rounded to fp32 once."""
    pn = np.asarray(pointnum, np.int32).astype(np.int64)
    n_prop, n_inst = len(off) - 1, len(pn)
    out = np.zeros((n_prop, n_inst), np.float32)
    for p in range(n_prop):
        inter, total = _counts(idx, off, labels, n_inst, mask_scores, mode, p)
        uni = (total + pn - inter).astype(np.int32)
        out[p] = (inter.astype(np.float32).astype(np.float64) / (uni.astype(np.float32).astype(np.float64) + 1e-5)).astype(np.float32)
    return out


def mask_label(idx, off, labels, iou_pi):
    """float32 [len(idx)]: -1 where the proposal's best IoU is not > 0.5; else 1 for the points of the best instance (the FIRST
    of equal maxima) and 0 for the rest.  The mask scores play no part here, in either mode."""
    out = np.full(len(idx), -1.0, np.float32)
    lab = np.asarray(labels, np.int64)
    for p in range(len(off) - 1):
        row = iou_pi[p]
        best, ind = np.float32(0.0), 0
        if row.size and row.max() > 0:
            ind = int(np.argmax(row))                     # first occurrence of the maximum
            best = row[ind]
        if best > np.float32(0.5):
            pts = np.asarray(idx[off[p]:off[p + 1]], np.int64)
            out[off[p]:off[p + 1]] = (lab[pts].astype(np.int32) == ind).astype(np.float32)
    return out
