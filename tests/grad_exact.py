"""float64 references and per-element checkers for the training side of the sparse backbone: the weight gradient
(pbn_spconv_wgrad), the input and bias gradients of a convolution (_ConvFn.backward), and train-mode batch norm with its
fused tail (pbn_bn_act_train_forward / _backward).  The counterpart of tests/conv_exact.py, whose ulp / RNE / sentinel
helpers it reuses.

Gradients of a convolution  out[o] = sum_k x[nbr[o, k]] @ W[k]  (pairs (i, o) of offset k: i = nbr[o, k] >= 0):
    dW[k]     = sum over the pairs of offset k  x[i]^T g[o]                        (S = the same sum of |x| |g|)
    gx[i]    += g[o] @ W[k]^T  for every pair                                       (S = the same sum of |g| |W|)
    dbias     = sum_o g[o]
The input gradient is stated on the FORWARD map, scattered with index_add: it does not know how the layer mirrors the
offsets (flip) or swaps the down / up tables (transpose) to run the same thing as a gather -- that is what it checks.

Exact mode: integer-valued operands (x, g in -3..3, W in (-2..2) 2^-e) with S < 2^24 units.  Every product and every
partial sum is an fp32 integer multiple of one unit, whatever the order or the split of the reduction: the fp32 dW must
EQUAL the float64 value, gx must equal RNE_T(reference) bit for bit.

Bounded mode: Gaussian operands, |got - ref| <= ulp_T(ref) + C S per element, C = conv_exact.BOUND_C = 2^-20 (one
rounding to T plus an fp32 reduction, whose random-walk error is ~2^-24 S).

Batch norm (train mode, x [n, c], per channel; u = 2^-24 the fp32 unit roundoff):
    mean = sum x / n, var = sum (x - mean)^2 / n (biased: normalisation), invstd = 1 / sqrt(var + eps)
    y = act((x - mean) invstd w + b [+ res]);  running_mean += m (mean - running_mean),
    running_var += m (var n / (n - 1) - running_var)  (unbiased; n = 1: var itself)
    g = dy masked by (y > 0) when the ReLU is fused (the KERNEL's y decides: outputs within an ulp of zero are its call),
    dres = g, dbias = sum g, dweight = sum g xhat, dx = w invstd (g - mean(g) - xhat mean(g xhat)).
The kernel takes its forward sums about the slab's FIRST row x0 (d = x - x0; s1 = sum d, s2 = sum d^2 in fp32 chains of
L terms, merged across blocks in double), then mean = x0 + s1 / n, var = s2 / n - (s1 / n)^2 in double, rounded to fp32.
With M1 = mean |d|, M2 = mean d^2 = var + (mean - x0)^2 and sh = |mean - x0|:
    |d mean|   <= u |mean| + C M1
    |d var|    <= C (M2 + 2 sh M1)                       (s2 / n, and the cancellation of (s1 / n)^2)
    |d invstd| <= invstd (u + (|d var| / 2) / (var + eps))
The term sh is the cost of the shift: a first row far from the mean (sh = 100 std) makes M2 = 10^4 var, and the fp32 sums
of d^2 lose that factor of relative accuracy in the variance -- the kernel guarantees no better, and the bound says so.
A constant channel has d = 0 exactly: var = 0 and invstd = 1 / sqrt(eps) with no error.
The apply pass y = fma(x - mean_f, invstd_f w, b) [+ res] adds, per element (a = |x - mean| |w| invstd):
    |d y| <= |w| invstd |d mean| + a (|d invstd| / invstd + 3 u) + 2 u (|b| + |res| + |z|)
Backward, given the fp32 statistics mean_f / invstd_f it is handed (deviations dm = |mean_f - mean|, di = |invstd_f -
invstd| from the exact ones), Sg = sum |g|, Sga = sum |g| |x - mean|:
    |d s2|      <= C (Sga + dm Sg) + dm Sg + u Sga        (s2 = sum g (x - mean_f))
    dbias       <= C Sg + u |dbias|;   dweight <= invstd |d s2| + |s2| di + 2 u |dweight|
    coef0 = s1 / n:  C Sg / n + u |coef0|;   coef1 = s2 invstd^2 / n:  (invstd^2 |d s2| + 2 invstd di |s2|) / n + 3 u |coef1|
    |d dx| <= |w| invstd (|d coef0| + a' |d coef1| + (dm + u a') |coef1| + 3 u T) + T |w| (di + u invstd),
              T = |g| + |coef0| + a' |coef1|, a' = |x - mean|
C for batch norm is BOUND_C, raised to 4 u sqrt(L) when the fp32 chains are longer than ~16 terms (L = rows per thread
+ row slots merged in fp32; bn_chain()): a random walk of L roundings, each at most u of a partial sum <= S.
dres is the masked dy itself: bit for bit."""
import math

import torch

import conv_exact as X
from conv_exact import BOUND_C, ulp, check_exact, expected_bits, SentinelOut   # noqa: F401  (re-exported)

U = 2.0 ** -24


# ---- convolution gradients ----------------------------------------------------------------------------------------------

def pairs_of(nbr, n_in=None):
    """nbr [n_out, K] (entries < 0, or >= n_in when given: no pair) -> per offset (in_rows, out_rows) int64, on nbr's device."""
    nb = nbr.long()
    out = []
    for k in range(nb.shape[1]):
        ok = nb[:, k] >= 0
        if n_in is not None:
            ok &= nb[:, k] < n_in
        o = torch.nonzero(ok).flatten()
        out.append((nb[o, k], o))
    return out


def wgrad_reference(x, g, pairs=None, nbr=None, n_pairs=None):
    """dW float64 [K, cin, cout] and S = the same contraction of |x| |g|, on x's device.  pairs: per offset (in_rows,
    out_rows); nbr: a map [n_out, K] instead; neither: identity pairs (row p with row p, p < n_pairs or every row of x)."""
    x, g = x.double(), g.double().to(x.device)
    if pairs is None and nbr is not None:
        pairs = pairs_of(nbr.to(x.device), x.shape[0])
    if pairs is None:
        n = x.shape[0] if n_pairs is None else n_pairs
        return (x[:n].t() @ g[:n])[None], (x[:n].abs().t() @ g[:n].abs())[None]
    K = len(pairs)
    dw = x.new_zeros(K, x.shape[1], g.shape[1])
    S = x.new_zeros(K, x.shape[1], g.shape[1])
    for k, (i, o) in enumerate(pairs):
        if len(i):
            xi, go = x.index_select(0, i.to(x.device).long()), g.index_select(0, o.to(x.device).long())
            dw[k] = xi.t() @ go
            S[k] = xi.abs().t() @ go.abs()
    return dw, S


def dgrad_reference(g, w, nbr, n_in):
    """Input gradient of  out[o] = sum_k x[nbr[o, k]] @ w[k]  (the forward map): gx float64 [n_in, cin] and S, scattered
    pair by pair with index_add (no mirrored offsets, no transposed tables).  w [K, cin, cout]; nbr None: a 1x1 (w [1, ...])."""
    g, w = g.double(), w.double().to(g.device)
    cin = w.shape[1]
    gx = g.new_zeros(n_in, cin)
    S = g.new_zeros(n_in, cin)
    if nbr is None:
        return g[:n_in] @ w[0].t(), g[:n_in].abs() @ w[0].abs().t()
    for k, (i, o) in enumerate(pairs_of(nbr.to(g.device), n_in)):
        if len(i):
            go = g.index_select(0, o)
            gx.index_add_(0, i, go @ w[k].t())
            S.index_add_(0, i, go.abs() @ w[k].abs().t())
    return gx, S


def dgrad_via_table(g, wd, dgrad_nbr, n_in):
    """The input gradient the way the layer computes it: a forward convolution of g over the dgrad table with the packed
    input-gradient weights wd [K, cout, cin] (w mirrored / transposed by the layer's convention).  For planted faults."""
    g, wd = g.double(), wd.double().to(g.device)
    n_g = g.shape[0]
    gz = torch.cat([g, g.new_zeros(1, g.shape[1])], 0)
    idx = dgrad_nbr.to(g.device).long()
    idx = torch.where((idx < 0) | (idx >= n_g), torch.full_like(idx, n_g), idx)
    out = g.new_zeros(n_in, wd.shape[2])
    for k in range(idx.shape[1]):
        out += gz.index_select(0, idx[:n_in, k]) @ wd[k]
    return out


def bias_grad_reference(g):
    return g.double().sum(0)


def check_wgrad_exact(got, ref, what):
    """fp32 dW against the float64 value: equal (exact mode makes every fp32 partial sum exact)."""
    assert got.dtype == torch.float32
    assert bool(torch.equal(ref.float().double(), ref.to(got.device))), "%s: reference not exact in fp32" % what
    bad = got.double() != ref.to(got.device)
    n_bad = int(bad.sum())
    if n_bad:
        k, ci, co = [int(v) for v in torch.nonzero(bad)[0]]
        ks = torch.unique(torch.nonzero(bad)[:, 0]).tolist()
        raise AssertionError("%s: %d of %d dW elements differ (offsets %s; first [%d, %d, %d]: got %r want %r)" % (
            what, n_bad, bad.numel(), ks[:8], k, ci, co, float(got[k, ci, co]), float(ref[k, ci, co])))
    return 0


def check_wgrad_bounded(got, ref, S, what, c=BOUND_C):
    """fp32 dW: |got - ref| <= ulp_f32(ref) + c S per element.  Returns the worst err / bound."""
    return X.check_bounded(got.reshape(-1, got.shape[-1]), ref.reshape(-1, ref.shape[-1]).to(got.device),
                           S.reshape(-1, S.shape[-1]).to(got.device), torch.float32, what, c)


def assert_grad_exact_premise(dtype, ref, S, unit):
    """Exact mode holds only while every fp32 intermediate is an integer multiple of `unit` below 2^24 units."""
    assert float(S.max()) < 2.0 ** 24 * unit, "S = %g >= 2^24 units of %g: fp32 sums not exact" % (float(S.max()), unit)
    assert bool(torch.equal(ref.float().double(), ref)), "reference not exact in fp32"
    if dtype == torch.float16:
        assert float(ref.abs().max()) < 2048, "fp16 exact mode keeps outputs below 2048"


def exact_ints(gen, *shape, lo=-3, hi=3):
    return torch.randint(lo, hi + 1, shape, generator=gen).float()


GRAD_W_EXP = {torch.float32: 5, torch.bfloat16: 14, torch.float16: 14}


def exact_weight(gen, shape, dtype, lo=-2, hi=2):
    """(lo..hi) 2^-e, inside (-2..2), with a per-type exponent fine enough that gx needs more bits than T holds (the final
    RNE is exercised; fp16's 2^-14 is its smallest normal).  Skewed ranges (g in -1..3, W in -1..2) keep the sums from
    cancelling to a few bits."""
    e = GRAD_W_EXP[dtype]
    return torch.randint(lo, hi + 1, shape, generator=gen).float() * 2.0 ** -e, 2.0 ** -e


# ---- batch norm ---------------------------------------------------------------------------------------------------------

def bn_chain(n, c, dtype, max_blocks=1024, tpb=256):
    """Length of the longest fp32 chain of csrc/bnorm.hip's partial sums: rows per thread + row slots merged in fp32."""
    W = 4 if dtype == torch.float32 else 8
    blocks = min(max(1, -(-n // 128)), max_blocks)
    per_block = -(-n // blocks)
    rpi = tpb // (c // W)
    return -(-per_block // rpi) + rpi


def bn_c(n, c, dtype):
    return max(BOUND_C, 4 * U * math.sqrt(bn_chain(n, c, dtype)))


def bn_reference(x, w, b, eps, momentum, running_mean, running_var, residual=None, relu=False):
    """Forward in float64.  -> dict(y, mean, var, invstd, running_mean, running_var, z) and error scales (E_*: allowed
    absolute error beyond one ulp of the output type).  x, residual: [n, c] values of the slab type (any float dtype)."""
    slab = x.dtype if x.dtype != torch.float64 else torch.float32
    x = x.double()
    n, c = x.shape
    w = torch.ones(c, dtype=torch.float64, device=x.device) if w is None else w.double().to(x.device)
    b = torch.zeros(c, dtype=torch.float64, device=x.device) if b is None else b.double().to(x.device)
    mean = x.mean(0)
    var = ((x - mean) ** 2).mean(0)
    invstd = 1.0 / torch.sqrt(var + eps)
    xc = x - mean
    z = xc * (invstd * w) + b
    res = None if residual is None else residual.double().to(x.device)
    if res is not None:
        z = z + res
    y = z.clamp_min(0.0) if relu else z
    rm, rv = running_mean.double().to(x.device), running_var.double().to(x.device)
    unb = var * n / (n - 1) if n > 1 else var
    out = dict(y=y, z=z, mean=mean, var=var, invstd=invstd,
               running_mean=(1 - momentum) * rm + momentum * mean, running_var=(1 - momentum) * rv + momentum * unb)
    # error scales (module docstring)
    C = bn_c(n, c, slab)
    d = x - x[0]
    M1, M2, sh = d.abs().mean(0), (d * d).mean(0), (mean - x[0]).abs()
    e_mean = U * mean.abs() + C * M1
    e_var = C * (M2 + 2 * sh * M1)
    e_is = invstd * (U + 0.5 * e_var / (var + eps))
    a = xc.abs() * w.abs() * invstd
    e_y = w.abs() * invstd * e_mean + a * (e_is / invstd + 3 * U) + 2 * U * (b.abs() + z.abs() + (0 if res is None else res.abs()))
    out.update(E_mean=e_mean, E_invstd=e_is, E_y=e_y,
               E_running_mean=momentum * e_mean + 2 * U * (out["running_mean"].abs() + rm.abs()),
               E_running_var=momentum * (n / (n - 1) if n > 1 else 1.0) * e_var + 2 * U * (out["running_var"].abs() + rv.abs()))
    return out


def bn_backward_reference(x, w, dy, mean, invstd, mean_f=None, invstd_f=None, y_got=None):
    """Backward in float64 from the EXACT statistics (mean, invstd: float64).  mean_f / invstd_f: the fp32 statistics the
    kernel is handed (their deviations enter the error scales); y_got: the kernel's forward output when the ReLU is fused
    -- its (y > 0) decides the mask.  -> dict(g, dx, dres, dweight, dbias) and E_dx, E_dweight, E_dbias."""
    slab = x.dtype if x.dtype != torch.float64 else torch.float32
    x, dy = x.double(), dy.double().to(x.device)
    n, c = x.shape
    mean, invstd = mean.double().to(x.device), invstd.double().to(x.device)
    w = torch.ones(c, dtype=torch.float64, device=x.device) if w is None else w.double().to(x.device)
    g = dy if y_got is None else torch.where(y_got.to(x.device).double() > 0, dy, torch.zeros_like(dy))
    xc = x - mean
    xhat = xc * invstd
    s1, sgx = g.sum(0), (g * xc).sum(0)
    dbias = s1
    dweight = sgx * invstd
    dx = w * invstd * (g - s1 / n - xhat * (sgx * invstd / n))
    out = dict(g=g, dres=g, dx=dx, dweight=dweight, dbias=dbias)
    C = bn_c(n, c, slab)
    dm = torch.zeros_like(mean) if mean_f is None else (mean_f.double().to(x.device) - mean).abs()
    di = torch.zeros_like(invstd) if invstd_f is None else (invstd_f.double().to(x.device) - invstd).abs()
    ap = xc.abs()
    Sg, Sga = g.abs().sum(0), (g.abs() * ap).sum(0)
    e_s2 = C * (Sga + dm * Sg) + dm * Sg + U * Sga
    c0, c1 = s1 / n, sgx * invstd * invstd / n
    e_c0 = C * Sg / n + U * c0.abs()
    e_c1 = (invstd * invstd * e_s2 + 2 * invstd * di * sgx.abs()) / n + 3 * U * c1.abs()
    T = g.abs() + c0.abs() + ap * c1.abs()
    out.update(E_dbias=C * Sg + U * dbias.abs(),
               E_dweight=invstd * e_s2 + sgx.abs() * di + 2 * U * dweight.abs(),
               E_dx=w.abs() * invstd * (e_c0 + ap * e_c1 + (dm + U * ap) * c1.abs() + 3 * U * T) + T * w.abs() * (di + U * invstd))
    return out


def check_bn(got, ref, E, dtype, what):
    """|got - ref| <= ulp_T(ref) + E per element (E: an error scale of bn_reference / bn_backward_reference).  Returns the
    worst err / bound (asserts it is <= 1)."""
    g = got.double().to(ref.device)
    err = (g - ref).abs()
    bound = ulp(ref, dtype) + E.to(ref.device)
    ok = err <= bound                                        # (NaN fails)
    ratio = err / bound
    worst = float(torch.nan_to_num(ratio, nan=float("inf")).max()) if ratio.numel() else 0.0
    if not bool(ok.all()):
        idx = tuple(int(v) for v in torch.nonzero(~ok)[0])
        raise AssertionError("%s: %d of %d elements outside ulp + E (worst err/bound %.3g; first %s: got %r ref %r E %r)" % (
            what, int((~ok).sum()), ok.numel(), worst, idx, float(g[idx]), float(ref[idx]), float(E.to(ref.device)[idx])))
    return worst


def check_bits(got, want, what):
    """Bit equality of two tensors of the same float dtype (dres: the masked dy itself)."""
    it = X._INT[got.dtype]
    bad = got.contiguous().view(it) != want.to(got.device).to(got.dtype).contiguous().view(it)
    n_bad = int(bad.sum())
    if n_bad:
        idx = tuple(int(v) for v in torch.nonzero(bad)[0])
        raise AssertionError("%s: %d of %d elements differ bit for bit (first %s: got %r want %r)" % (
            what, n_bad, bad.numel(), idx, float(got[idx]), float(want[idx])))


class SentinelSlab(object):
    """A [rows, cols] column view at column `col0` (16-byte aligned) of a wider slab [rows + extra_rows, ld], everything
    filled with conv_exact's sentinel bit pattern; check() asserts that nothing outside rows x [col0, col0 + cols) changed."""

    def __init__(self, rows, cols, dtype, device, col0=None, extra_cols=None, extra_rows=7):
        W = 4 if dtype == torch.float32 else 8
        self.col0 = W if col0 is None else col0
        self.ld = self.col0 + cols + (W if extra_cols is None else extra_cols)
        self.dtype, self.rows, self.cols = dtype, rows, cols
        self.buf = torch.empty(rows + extra_rows, self.ld, dtype=dtype, device=device)
        self.buf.view(X._INT[dtype]).fill_(X._SENT[dtype])
        self.view = self.buf[:rows, self.col0:self.col0 + cols]

    def fill(self, values):
        self.view.copy_(values.to(self.dtype))
        return self

    def check(self, what, written=True):
        bits = self.buf.view(X._INT[self.dtype])
        m = torch.ones(self.buf.shape, dtype=torch.bool, device=self.buf.device)
        if written:
            m[:self.rows, self.col0:self.col0 + self.cols] = False
        bad = (bits != X._SENT[self.dtype]) & m
        n_bad = int(bad.sum())
        if n_bad:
            r, c = [int(v) for v in torch.nonzero(bad)[0]]
            raise AssertionError("%s: %d elements outside the written region changed (first buffer [%d, %d]; region rows < %d, "
                                 "columns [%d, %d))" % (what, n_bad, r, c, self.rows, self.col0, self.col0 + self.cols))
