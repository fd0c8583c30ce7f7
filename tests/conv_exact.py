"""A float64 reference and a two-mode checker for the sparse convolution forward (pbn_spconv_forward / _dual).

    out[o, c] = act( scale[c] * (sum_k x[nbr[o,k]] @ W[k] (+ x2[o] @ W2)) + shift[c] + res[o, c] )

The reference is one plain-torch statement in float64 (index_select + matmul per offset); it runs on whichever device its
operands live on, so the same statement serves a CPU self-test and bench-sized shapes on the GPU.  Next to the value it
returns S = |scale| * sum |x||w| + |shift| + |res| per element: the magnitude every fp32 error bound scales with.

Exact mode: integer-valued operands (x in -3..3, W in (-2..2) * 2^-e, scale a power of two, shift a multiple of 2^-4,
res an integer).  When S < 2^24 units every product and every partial sum is exact in fp32, whatever the summation order
or split of the reduction, and so is the epilogue: the only rounding left is the final one to the slab's type.  The kernel
must then equal RNE_T(reference) bit for bit, padding columns cout..cout_p included (they hold relu?(0) = +0).

Bounded mode: Gaussian operands.  Per element |got - ref| <= ulp_T(ref) + C * S, C = 2^-20 by default: one rounding to
T plus fp32 accumulation, whose random-walk error is ~2^-24 * S (each partial sum is ~sqrt(i) terms, its rounding error
2^-24 of that; n of them add up to ~n * 2^-24 * |term| ~ 2^-24 * S).  A per-element bound: a dropped tap or channel
shows in the elements it touches, not only against the largest output.

Sentinels: the output slab is a strided view into a larger buffer (rows past the count, columns before and after the
slab) filled with a bit pattern; everything outside the rows written x [col0, col0 + cout_p) must keep it."""
import numpy as np
import torch

BOUND_C = 2.0 ** -20
_MANT = {torch.float32: 23, torch.bfloat16: 7, torch.float16: 10}
_EMIN = {torch.float32: -126, torch.bfloat16: -126, torch.float16: -14}
_INT = {torch.float32: torch.int32, torch.bfloat16: torch.int16, torch.float16: torch.int16}
_SENT = {torch.float32: 0x5A5A5A5A, torch.bfloat16: 0x5A5A, torch.float16: 0x5A5A}
SHIFT_UNIT = 2.0 ** -4


def maps_to_nbr(maps, n_out):
    """oracle/sparse_ref.py's per-offset (in_rows, out_rows) maps -> an nbr table [n_out, K] (-1: no neighbour)."""
    nbr = np.full((n_out, len(maps)), -1, np.int64)
    for k, (i, o) in enumerate(maps):
        nbr[np.asarray(o, np.int64), k] = np.asarray(i, np.int64)
    return torch.from_numpy(nbr)


def nbr_to_maps(nbr):
    """nbr [n_out, K] -> the oracle's per-offset (in_rows, out_rows) maps (R.conv)."""
    nb = nbr.cpu().numpy()
    maps = []
    for k in range(nb.shape[1]):
        o = np.nonzero(nb[:, k] >= 0)[0]
        maps.append((nb[o, k].astype(np.int64), o.astype(np.int64)))
    return maps


def reference(x, w, nbr, scale=None, shift=None, res=None, relu=False, x2=None, w2=None):
    """float64 forward and its error scale S, both [n_out, cout], on x's device.  x [n_in, cin], w [K, cin, cout],
    nbr [n_out, K] (entries < 0 or >= n_in gather a zero row, as the kernels do), x2 [>= n_out, cin2] / w2 [cin2, cout]:
    the second source of the dual launch (row o pairs with output row o)."""
    x, w = x.double(), w.double()
    n_in, cin = x.shape
    n_out, K = nbr.shape
    cout = w.shape[2]
    assert w.shape[:2] == (K, cin)
    xz = torch.cat([x, x.new_zeros(1, cin)], 0)                     # row n_in: the zero row of a missing neighbour
    idx = nbr.to(x.device).long()
    idx = torch.where((idx < 0) | (idx >= n_in), torch.full_like(idx, n_in), idx)
    acc = x.new_zeros(n_out, cout)
    mag = x.new_zeros(n_out, cout)
    for k in range(K):
        g = xz.index_select(0, idx[:, k])
        acc += g @ w[k]
        mag += g.abs() @ w[k].abs()
    if x2 is not None:
        g = x2.double()[:n_out]
        acc += g @ w2.double()
        mag += g.abs() @ w2.double().abs()
    return _epilogue(acc, mag, scale, shift, res, relu)


def oracle_reference(x, w, maps, n_out, scale=None, shift=None, res=None, relu=False, x2=None, w2=None):
    """The same (value, S) pair from oracle/sparse_ref.py's R.conv on float64 tensors and the oracle's per-offset maps
    (maps None: a 2-D w, x @ w).  CPU; for the existing oracle-based tests."""
    from oracle import sparse_ref as R
    x, w = x.double(), w.double()
    acc = R.conv(x, w, maps, n_out)
    mag = R.conv(x.abs(), w.abs(), maps, n_out)
    if x2 is not None:
        acc = acc + x2.double()[:n_out] @ w2.double()
        mag = mag + x2.double()[:n_out].abs() @ w2.double().abs()
    return _epilogue(acc, mag, scale, shift, res, relu)


def _epilogue(acc, mag, scale, shift, res, relu):
    dev = acc.device
    if scale is not None:
        acc = acc * scale.double().to(dev)
        mag = mag * scale.double().to(dev).abs()
    if shift is not None:
        acc = acc + shift.double().to(dev)
        mag = mag + shift.double().to(dev).abs()
    if res is not None:
        acc = acc + res.double().to(dev)[:acc.shape[0]]
        mag = mag + res.double().to(dev)[:acc.shape[0]].abs()
    if relu:
        acc = acc.clamp_min(0.0)
    return acc, mag


def ulp(v, dtype):
    """Unit in the last place of T at |v| (float64 tensor; the smallest normal's ulp at 0 and below)."""
    v = v.double().abs()
    _, e = torch.frexp(v)
    e = torch.where(v == 0, torch.full_like(e, _EMIN[dtype]), (e - 1).clamp_min(_EMIN[dtype]))
    return torch.ldexp(torch.ones_like(v), e - _MANT[dtype])


def _integral(t):
    t = t.double()
    return bool(torch.equal(t, torch.round(t)))


def assert_exact_premise(dtype, x, w, w_unit, scale, shift, res, ref, S, x2=None, w2=None):
    """Refuse to trust exact mode unless every intermediate of the kernel's arithmetic is an fp32 integer multiple of one
    unit below 2^24 units: the products x * w, every partial sum, acc * scale, + shift, + res."""
    rep = lambda t: bool(torch.equal(t.to(dtype).double(), t.double()))
    for name, t in (("x", x), ("x2", x2)):
        if t is not None:
            assert _integral(t) and float(t.abs().max()) <= 3, "%s must hold integers in -3..3" % name
            assert rep(t), "%s not representable in %s" % (name, dtype)
    for name, t in (("w", w), ("w2", w2)):
        if t is not None:
            assert _integral(t / w_unit), "%s must be an integer multiple of %g" % (name, w_unit)
            assert rep(t), "%s not representable in %s" % (name, dtype)
    unit = w_unit
    if scale is not None:
        m, _ = torch.frexp(scale.double())
        assert bool((m == 0.5).all()), "scale must hold positive powers of two"
        unit = unit * float(scale.min())
    if shift is not None:
        assert _integral(shift.double() / SHIFT_UNIT), "shift must be a multiple of 2^-4"
        unit = min(unit, SHIFT_UNIT)
    if res is not None:
        assert _integral(res) and rep(res), "res must hold integers representable in %s" % dtype
        unit = min(unit, 1.0)
    assert float(S.max()) < 2.0 ** 24 * unit, "S = %g >= 2^24 units of %g: fp32 sums not exact" % (float(S.max()), unit)
    assert bool(torch.equal(ref.float().double(), ref)), "reference not exact in fp32"
    if dtype == torch.float16:
        assert float(ref.abs().max()) < 2048, "fp16 exact mode keeps outputs below 2048"


def expected_bits(ref, dtype, cout_p):
    """RNE_T(ref) widened to cout_p columns of +0 (padding: zero weights, scale 1, shift 0, residual 0)."""
    want = torch.zeros(ref.shape[0], cout_p, dtype=dtype, device=ref.device)
    want[:, :ref.shape[1]] = ref.float().to(dtype)          # ref is exact in fp32: one rounding, fp32 -> T (RNE)
    return want


def check_exact(got, ref, dtype, what, rows=None):
    """got [n, cout_p] of T against RNE_T(ref) [n, cout] bit for bit, padding columns included.  rows: the slab rows to
    compare (default all).  Returns the number of mismatching elements (asserts it is 0)."""
    cout_p = got.shape[1]
    want = expected_bits(ref.to(got.device), dtype, cout_p)
    if rows is not None:
        got, want = got[rows], want[rows]
    it = _INT[dtype]
    bad = got.contiguous().view(it) != want.contiguous().view(it)
    n_bad = int(bad.sum())
    if n_bad:
        r, c = [int(v) for v in torch.nonzero(bad)[0]]
        rs = torch.unique(torch.nonzero(bad)[:, 0])
        raise AssertionError("%s: %d of %d elements differ from RNE(ref64) in %d rows (first [%d, %d]: got %r want %r)" % (
            what, n_bad, bad.numel(), rs.numel(), r, c, float(got[r, c]), float(want[r, c])))
    return n_bad


def check_bounded(got, ref, S, dtype, what, c=BOUND_C):
    """|got - ref| <= ulp_T(ref) + c * S per element over the real columns; padding columns must be exactly +0.
    Returns the worst err / bound (asserts it is <= 1)."""
    cout = ref.shape[1]
    ref, S = ref.to(got.device), S.to(got.device)
    g = got[:, :cout].double()
    err = (g - ref).abs()
    bound = ulp(ref, dtype) + c * S
    ratio = err / bound
    ok = err <= bound                                       # (NaN fails)
    worst = float(torch.nan_to_num(ratio, nan=float("inf")).max()) if ratio.numel() else 0.0
    if not bool(ok.all()):
        r, cc = [int(v) for v in torch.nonzero(~ok)[0]]
        raise AssertionError("%s: %d of %d elements outside ulp + %g S (worst err/bound %.3g; first [%d, %d]: got %r ref %r S %r)" % (
            what, int((~ok).sum()), ok.numel(), c, worst, r, cc, float(g[r, cc]), float(ref[r, cc]), float(S[r, cc])))
    if got.shape[1] > cout:
        pad = got[:, cout:].contiguous().view(_INT[got.dtype])
        assert bool((pad == 0).all()), "%s: padding columns written with non-zero values" % what
    return worst


class SentinelOut(object):
    """An output slab [rows, cout_p] as a strided view (ld_out = cout_p + 2 * margin) into a buffer with `extra_rows` rows
    after it and `margin` columns on both sides, all filled with a sentinel bit pattern."""

    def __init__(self, rows, cout_p, dtype, device, extra_rows=33, margin=8):
        self.dtype, self.margin, self.cout_p = dtype, margin, cout_p
        self.ld = cout_p + 2 * margin
        self.buf = torch.empty(rows + extra_rows, self.ld, dtype=dtype, device=device)
        self.buf.view(_INT[dtype]).fill_(_SENT[dtype])
        self.view = self.buf[:, margin:margin + cout_p]

    def written_mask(self, rows):
        """rows: an int (rows [0, rows) written) or a 1-D index / bool tensor of the rows written."""
        m = torch.zeros(self.buf.shape, dtype=torch.bool, device=self.buf.device)
        if isinstance(rows, int):
            m[:rows, self.margin:self.margin + self.cout_p] = True
        else:
            sel = torch.zeros(self.buf.shape[0], dtype=torch.bool, device=self.buf.device)
            sel[rows.to(self.buf.device)] = True
            m[sel, self.margin:self.margin + self.cout_p] = True
        return m

    def check(self, rows, what):
        """Everything outside the written rows x slab columns is bit-unchanged."""
        bits = self.buf.view(_INT[self.dtype])
        bad = (bits != _SENT[self.dtype]) & ~self.written_mask(rows)
        n_bad = int(bad.sum())
        if n_bad:
            r, c = [int(v) for v in torch.nonzero(bad)[0]]
            raise AssertionError("%s: %d elements outside the slab written (first buffer [%d, %d], slab columns start at %d)" % (
                what, n_bad, r, c, self.margin))


# ---- operands -----------------------------------------------------------------------------------------------------------

W_EXP = {torch.float32: 5, torch.bfloat16: 6, torch.float16: 9}


def exact_operands(g, n_in, cin, K, cout, n_out, dtype, cin2=0, w_exp=None, span=8):
    """Integer-valued operands of exact mode (float32 tensors on the CPU): x, w, scale, shift, res (+ x2, w2).  The weight
    unit 2^-w_exp is chosen per type so that outputs of magnitude `span` (shift and residual) carry more significant bits
    than T holds: the final rounding, and a double rounding, are exercised, not only the sums."""
    e = W_EXP[dtype] if w_exp is None else w_exp
    ri = lambda lo, hi, *shape: torch.randint(lo, hi + 1, shape, generator=g).float()
    op = dict(x=ri(-3, 3, n_in, cin), w=ri(-2, 2, K, cin, cout) * 2.0 ** -e, w_unit=2.0 ** -e,
              scale=torch.ldexp(torch.ones(cout), torch.randint(-1, 2, (cout,), generator=g)),
              shift=ri(-16 * span, 16 * span, cout) * SHIFT_UNIT, res=ri(-span, span, n_out, cout))
    if cin2:
        op["x2"], op["w2"] = ri(-3, 3, n_out, cin2), ri(-2, 2, cin2, cout) * 2.0 ** -e
    return op


def gaussian_operands(g, n_in, cin, K, cout, n_out, dtype, cin2=0):
    """Gaussian operands of bounded mode, already rounded to the slab type where the kernel reads them in that type."""
    q = lambda t: t.to(dtype).float()
    op = dict(x=q(torch.randn(n_in, cin, generator=g)), w=q(torch.randn(K, cin, cout, generator=g) * (2.0 / (K * cin)) ** 0.5),
              scale=torch.rand(cout, generator=g) + 0.5, shift=torch.randn(cout, generator=g) * 0.1,
              res=q(torch.randn(n_out, cout, generator=g)), w_unit=None)
    if cin2:
        op["x2"] = q(torch.randn(n_out, cin2, generator=g))
        op["w2"] = q(torch.randn(cin2, cout, generator=g) * (1.0 / cin2) ** 0.5)
    return op
