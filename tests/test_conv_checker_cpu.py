"""CPU tier: the convolution checker of tests/conv_exact.py rejects subtly wrong outputs and accepts correct ones.

"Kernel outputs" are built on the CPU from the float64 reference: RNE_T(ref) and an fp32 sum in a shuffled order (what any
correct kernel produces) must pass; each perturbation below -- the faults a 6 %-of-max bound lets through -- must fail."""
import pytest
import torch

from oracle import sparse_ref as R
import conv_exact as X

N_IN, N_OUT, K, CIN, COUT, COUT_P = 190, 150, 27, 40, 20, 32


def _nbr(seed):
    g = torch.Generator().manual_seed(seed)
    nbr = torch.randint(0, N_IN, (N_OUT, K), generator=g)
    nbr[torch.rand(N_OUT, K, generator=g) < 0.4] = -1        # ~40 % empty taps, as on a surface scene
    nbr[:, K // 2] = torch.arange(N_OUT)                        # the centre tap: every row has itself
    return nbr


def _exact_case(dtype, relu=False, seed=0):
    g = torch.Generator().manual_seed(seed)
    nbr = _nbr(seed)
    op = X.exact_operands(g, N_IN, CIN, K, COUT, N_OUT, dtype)
    ref, S = X.reference(op["x"], op["w"], nbr, op["scale"], op["shift"], op["res"], relu)
    X.assert_exact_premise(dtype, op["x"], op["w"], op["w_unit"], op["scale"], op["shift"], op["res"], ref, S)
    return nbr, op, ref, S


def _bounded_case(dtype, seed=1):
    g = torch.Generator().manual_seed(seed)
    nbr = _nbr(seed)
    op = X.gaussian_operands(g, N_IN, CIN, K, COUT, N_OUT, dtype)
    ref, S = X.reference(op["x"], op["w"], nbr, op["scale"], op["shift"], op["res"], True)
    return nbr, op, ref, S


def _shuffled_fp32(nbr, op, dtype, relu, seed, split=1):
    """A correct kernel's output: fp32 sum of the exact products in a random order (optionally in `split` partial sums,
    combined in order, as split-K does), fp32 epilogue, one rounding to T."""
    x = torch.cat([op["x"], torch.zeros(1, CIN)], 0)
    idx = torch.where(nbr < 0, torch.full_like(nbr, N_IN), nbr)
    terms = (x[idx].unsqueeze(-1) * op["w"].unsqueeze(0)).reshape(N_OUT, K * CIN, COUT)    # exact in fp32 (16-bit operands)
    order = torch.randperm(K * CIN, generator=torch.Generator().manual_seed(seed))
    parts = []
    for chunk in order.chunk(split):
        acc = torch.zeros(N_OUT, COUT, dtype=torch.float32)
        for j in chunk.tolist():
            acc = acc + terms[:, j]
        parts.append(acc)
    acc = parts[0]
    for p in parts[1:]:
        acc = acc + p
    v = acc * op["scale"] + op["shift"] + op["res"]
    if relu:
        v = v.clamp_min(0.0)
    out = torch.zeros(N_OUT, COUT_P, dtype=dtype)
    out[:, :COUT] = v.to(dtype)
    return out


def test_reference_statement_equals_the_oracle():
    """The float64 statement of the checker against oracle/sparse_ref.py's R.conv (gather-mm-index_add) on float64."""
    g = torch.Generator().manual_seed(3)
    nbr = _nbr(3)
    x, w = torch.randn(N_IN, CIN, generator=g).double(), torch.randn(K, CIN, COUT, generator=g).double()
    ref, S = X.reference(x, w, nbr)
    want = R.conv(x, w, X.nbr_to_maps(nbr), N_OUT)
    assert torch.allclose(ref, want, rtol=0, atol=1e-12 * float(S.max()))
    assert torch.equal(X.maps_to_nbr(X.nbr_to_maps(nbr), N_OUT), torch.where(nbr < 0, -1, nbr))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32])
def test_exact_mode_accepts_rne_and_any_summation_order(dtype):
    nbr, op, ref, S = _exact_case(dtype)
    assert X.check_exact(X.expected_bits(ref, dtype, COUT_P), ref, dtype, "RNE(ref64)") == 0
    for split in (1, 3):        # exact operands: every order and every split of the reduction gives the same bits
        got = _shuffled_fp32(nbr, op, dtype, False, seed=split, split=split)
        assert X.check_exact(got, ref, dtype, "shuffled fp32 split %d" % split) == 0
    # ... and the outputs do need rounding (exact mode tests the final RNE, not only the sums)
    if dtype != torch.float32:
        assert int((ref[:, :COUT].float().to(dtype).double() != ref).sum()) > ref.numel() // 4


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_exact_mode_rejects_each_fault(dtype):
    nbr, op, ref, S = _exact_case(dtype)
    good = X.expected_bits(ref, dtype, COUT_P)

    def rejects(got, what):
        with pytest.raises(AssertionError):
            X.check_exact(got, ref, dtype, what)

    # one tap dropped in one row
    r, k = 17, 3
    assert nbr[r, k] >= 0
    nb = nbr.clone(); nb[r, k] = -1
    rejects(X.expected_bits(X.reference(op["x"], op["w"], nb, op["scale"], op["shift"], op["res"])[0], dtype, COUT_P), "tap dropped")
    # one input channel dropped (a lost tail step of the reduction)
    x = op["x"].clone(); x[:, CIN - 1] = 0
    rejects(X.expected_bits(X.reference(x, op["w"], nbr, op["scale"], op["shift"], op["res"])[0], dtype, COUT_P), "channel dropped")
    # the residual added after the rest was rounded to 16 bits (double rounding)
    pre, _ = X.reference(op["x"], op["w"], nbr, op["scale"], op["shift"], None)
    twice = pre.float().to(dtype).double() + op["res"].double()
    rejects(X.expected_bits(twice, dtype, COUT_P), "residual after rounding")
    # one element off by 2 ulp
    bad = good.clone(); bad.view(torch.int16)[40, 5] += 2
    rejects(bad, "2 ulp")
    # one padding column written
    bad = good.clone(); bad[7, COUT + 3] = 1.0
    rejects(bad, "padding column")
    # two rows swapped (a wrong row_perm slot)
    bad = good.clone(); bad[[11, 90]] = good[[90, 11]]
    rejects(bad, "rows swapped")


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32])
def test_bounded_mode_accepts_fp32_reassociation(dtype):
    nbr, op, ref, S = _bounded_case(dtype)
    worst = 0.0
    for split in (1, 4):
        got = _shuffled_fp32(nbr, op, dtype, True, seed=10 + split, split=split)
        worst = max(worst, X.check_bounded(got, ref, S, dtype, "shuffled fp32 split %d" % split))
    print("bounded mode, %s: worst err / bound of fp32 reassociation %.3f" % (dtype, worst))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_bounded_mode_rejects_faults(dtype):
    nbr, op, ref, S = _bounded_case(dtype)
    good = X.expected_bits(ref.float().double(), dtype, COUT_P)
    X.check_bounded(good, ref, S, dtype, "RNE(ref)")

    def rejects(got, what):
        with pytest.raises(AssertionError):
            X.check_bounded(got, ref, S, dtype, what)

    r, k = 17, 3
    nb = nbr.clone(); nb[r, k] = -1
    rejects(X.expected_bits(X.reference(op["x"], op["w"], nb, op["scale"], op["shift"], op["res"], True)[0].float().double(),
                            dtype, COUT_P), "tap dropped")
    x = op["x"].clone(); x[:, CIN - 1] = 0
    rejects(X.expected_bits(X.reference(x, op["w"], nbr, op["scale"], op["shift"], op["res"], True)[0].float().double(),
                            dtype, COUT_P), "channel dropped")
    i = int(torch.argmax(ref.abs()))
    bad = good.clone(); bad.view(torch.int16)[i // COUT, i % COUT] += 2
    rejects(bad, "2 ulp")
    bad = good.clone(); bad[7, COUT + 3] = 1.0
    rejects(bad, "padding column")


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_sentinels_catch_writes_outside_the_slab(dtype):
    count = 100
    nbr, op, ref, S = _exact_case(dtype)
    good = X.expected_bits(ref, dtype, COUT_P)
    o = X.SentinelOut(N_OUT, COUT_P, dtype, "cpu")
    assert o.view.stride(0) > COUT_P
    o.view[:count] = good[:count]
    o.check(count, "rows [0, count)")
    o.view[count] = good[count]                              # one row past the device-side count
    with pytest.raises(AssertionError):
        o.check(count, "row past the count")
    o = X.SentinelOut(N_OUT, COUT_P, dtype, "cpu")
    o.view[:count] = good[:count]
    o.buf[5, o.margin + COUT_P] = 0                          # a column after the slab (a wider out= view)
    with pytest.raises(AssertionError):
        o.check(count, "column after the slab")
    o = X.SentinelOut(N_OUT, COUT_P, dtype, "cpu")
    o.buf[5, o.margin - 1] = 0                               # ... and one before it
    with pytest.raises(AssertionError):
        o.check(count, "column before the slab")
    # permuted rows: the written set is row_perm[:count]
    perm = torch.randperm(N_OUT, generator=torch.Generator().manual_seed(2))
    o = X.SentinelOut(N_OUT, COUT_P, dtype, "cpu")
    o.view[perm[:count]] = good[perm[:count]]
    o.check(perm[:count], "permuted rows")
    o.view[perm[count]] = good[perm[count]]
    with pytest.raises(AssertionError):
        o.check(perm[:count], "a permuted row past the count")


def test_exact_premise_refuses_inexact_operands():
    dtype = torch.bfloat16
    nbr, op, ref, S = _exact_case(dtype)
    args = dict(x=op["x"], w=op["w"], w_unit=op["w_unit"], scale=op["scale"], shift=op["shift"], res=op["res"], ref=ref, S=S)
    X.assert_exact_premise(dtype, **args)
    for key, val in (("scale", op["scale"] * 1.5), ("shift", op["shift"] + 2.0 ** -6), ("res", op["res"] + 0.25),
                     ("x", op["x"] * 2), ("w", op["w"] * 1.25), ("S", S * 2.0 ** 22)):
        with pytest.raises(AssertionError):
            X.assert_exact_premise(dtype, **dict(args, **{key: val}))
