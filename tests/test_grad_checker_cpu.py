"""CPU tier: the gradient and batch-norm references of tests/grad_exact.py against naive restatements and float64 autograd,
and the checkers against planted faults.

Correct "kernel outputs" are built on the CPU (RNE_T of the reference; fp32 sums in a shuffled, split order; an fp32
emulation of bnorm.hip's shifted sums) and must pass; each planted fault -- the kind a norm-ratio tolerance lets through --
must be reported as a failure."""
import pytest
import torch
import torch.nn.functional as F

import conv_exact as X
import grad_exact as G

N_IN, N_OUT, K, CIN, COUT = 170, 150, 27, 40, 36


def _nbr(seed, n_out=N_OUT, n_in=N_IN, k=K):
    g = torch.Generator().manual_seed(seed)
    nbr = torch.randint(0, n_in, (n_out, k), generator=g)
    nbr[torch.rand(n_out, k, generator=g) < 0.4] = -1
    nbr[:, k // 2] = torch.arange(n_out) % n_in
    return nbr


def _naive_wgrad(x, g, nbr):
    x, g = x.double(), g.double()
    dw = torch.zeros(nbr.shape[1], x.shape[1], g.shape[1], dtype=torch.float64)
    for o in range(nbr.shape[0]):
        for k in range(nbr.shape[1]):
            i = int(nbr[o, k])
            if i >= 0:
                dw[k] += torch.outer(x[i], g[o])
    return dw


def _naive_dgrad(g, w, nbr, n_in):
    g, w = g.double(), w.double()
    gx = torch.zeros(n_in, w.shape[1], dtype=torch.float64)
    for o in range(nbr.shape[0]):
        for k in range(nbr.shape[1]):
            i = int(nbr[o, k])
            if i >= 0:
                gx[i] += w[k] @ g[o]
    return gx


def _exact_conv(dtype, seed=0):
    gen = torch.Generator().manual_seed(seed)
    nbr = _nbr(seed)
    x, g = G.exact_ints(gen, N_IN, CIN), G.exact_ints(gen, N_OUT, COUT)
    w, unit = G.exact_weight(gen, (K, CIN, COUT), dtype)
    return nbr, x, g, w, unit


def test_references_equal_naive_loops_and_autograd():
    gen = torch.Generator().manual_seed(1)
    nbr = _nbr(1)
    x, g = torch.randn(N_IN, CIN, generator=gen, dtype=torch.float64), torch.randn(N_OUT, COUT, generator=gen, dtype=torch.float64)
    w = torch.randn(K, CIN, COUT, generator=gen, dtype=torch.float64)
    dw, Sw = G.wgrad_reference(x, g, nbr=nbr)
    gx, Sx = G.dgrad_reference(g, w, nbr, N_IN)
    assert torch.allclose(dw, _naive_wgrad(x, g, nbr), rtol=0, atol=1e-12 * float(Sw.max()))
    assert torch.allclose(gx, _naive_dgrad(g, w, nbr, N_IN), rtol=0, atol=1e-12 * float(Sx.max()))
    # the same through autograd of the forward statement (conv_exact.reference), float64
    xr, wr = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    br = torch.zeros(COUT, dtype=torch.float64, requires_grad=True)
    y, _ = X.reference(xr, wr, nbr)
    ((y + br) * g).sum().backward()
    assert torch.allclose(gx, xr.grad, rtol=0, atol=1e-12 * float(Sx.max()))
    assert torch.allclose(dw, wr.grad, rtol=0, atol=1e-12 * float(Sw.max()))
    assert torch.allclose(G.bias_grad_reference(g), br.grad, rtol=0, atol=1e-12)
    # identity pairs and explicit pair lists
    d1, _ = G.wgrad_reference(x, g[:, :20], n_pairs=N_OUT)
    assert torch.allclose(d1[0], x[:N_OUT].t() @ g[:, :20], rtol=0, atol=1e-10)
    d2, _ = G.wgrad_reference(x, g, pairs=G.pairs_of(nbr))
    assert torch.equal(d2, dw)
    # the layer's own formulation (mirrored offsets of a centred cube, the same map) gives the same input gradient
    K3 = 27
    nb3 = torch.full((N_IN, K3), -1, dtype=torch.long)          # a symmetric map: offset K-1-k is the mirror of offset k
    for k in range(K3 // 2):
        src = torch.randperm(N_IN, generator=gen)[:N_IN // 2]
        dst = torch.randperm(N_IN, generator=gen)[:N_IN // 2]
        nb3[dst, k] = src
        nb3[src, K3 - 1 - k] = dst
    nb3[:, K3 // 2] = torch.arange(N_IN)
    w3 = torch.randn(K3, CIN, COUT, generator=gen, dtype=torch.float64)
    g3 = torch.randn(N_IN, COUT, generator=gen, dtype=torch.float64)
    want, S3 = G.dgrad_reference(g3, w3, nb3, N_IN)
    got = G.dgrad_via_table(g3, w3.flip(0).transpose(1, 2), nb3, N_IN)
    assert torch.allclose(got, want, rtol=0, atol=1e-12 * float(S3.max()))


def _shuffled_wgrad_fp32(x, g, nbr, seed, split):
    """A correct kernel's dW: fp32 sums of the products of each offset's pairs in a random order, in `split` partial sums
    added in order."""
    gen = torch.Generator().manual_seed(seed)
    out = torch.zeros(nbr.shape[1], x.shape[1], g.shape[1])
    for k, (i, o) in enumerate(G.pairs_of(nbr)):
        perm = torch.randperm(len(i), generator=gen)
        parts = []
        for chunk in perm.chunk(split) if len(i) else []:
            acc = torch.zeros(x.shape[1], g.shape[1])
            for p in chunk.tolist():
                acc = acc + torch.outer(x[i[p]].float(), g[o[p]].float())
            parts.append(acc)
        for p in parts:
            out[k] = out[k] + p
    return out


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32])
def test_wgrad_exact_mode_accepts_any_order_and_rejects_faults(dtype):
    nbr, x, g, w, unit = _exact_conv(dtype)
    ref, S = G.wgrad_reference(x, g, nbr=nbr)
    G.assert_grad_exact_premise(dtype, ref, S, 1.0)
    for split in (1, 5):
        G.check_wgrad_exact(_shuffled_wgrad_fp32(x, g, nbr, split, split), ref, "shuffled split %d" % split)

    def rejects(dw, what):
        with pytest.raises(AssertionError):
            G.check_wgrad_exact(dw.float(), ref, what)

    pairs = G.pairs_of(nbr)
    k = 4
    i, o = pairs[k]
    assert len(i) > 3
    drop = list(pairs); drop[k] = (i[1:], o[1:])
    rejects(G.wgrad_reference(x, g, pairs=drop)[0], "one pair dropped")
    dup = list(pairs); dup[k] = (torch.cat([i, i[:1]]), torch.cat([o, o[:1]]))
    rejects(G.wgrad_reference(x, g, pairs=dup)[0], "one pair duplicated")
    rejects(ref[[1, 0] + list(range(2, K))], "two offsets swapped")
    tile = ref.clone(); tile[7, 16:32, 16:32] = 0
    rejects(tile, "one 16-channel tile zeroed")


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32])
def test_dgrad_exact_mode_and_faults(dtype):
    # a symmetric (centred-cube) map so that the layer's mirrored formulation applies
    gen = torch.Generator().manual_seed(3)
    n = N_IN
    nb = torch.full((n, K), -1, dtype=torch.long)
    for k in range(K // 2):
        src, dst = torch.randperm(n, generator=gen)[:n // 2], torch.randperm(n, generator=gen)[:n // 2]
        nb[dst, k] = src
        nb[src, K - 1 - k] = dst
    nb[:, K // 2] = torch.arange(n)
    g = G.exact_ints(gen, n, COUT, lo=-1)
    w, unit = G.exact_weight(gen, (K, CIN, COUT), dtype, lo=-1)
    ref, S = G.dgrad_reference(g, w, nb, n)
    G.assert_grad_exact_premise(dtype, ref, S, unit)
    cin_p = 48
    X.check_exact(X.expected_bits(G.dgrad_via_table(g, w.flip(0).transpose(1, 2), nb, n), dtype, cin_p), ref, dtype, "flipped")
    if dtype == torch.bfloat16:      # the outputs do need rounding: the final RNE is exercised
        assert int((ref.float().to(dtype).double() != ref).sum()) > ref.numel() // 8

    def rejects(v, what):
        with pytest.raises(AssertionError):
            X.check_exact(X.expected_bits(v, dtype, cin_p), ref, dtype, what)

    rejects(G.dgrad_via_table(g, w.transpose(1, 2), nb, n), "dgrad kernel not flipped")
    bad = ref.clone(); bad[:, 16:32] = 0
    rejects(bad, "one 16-channel tile of gx zeroed")
    nb2 = nb.clone(); nb2[5, 3] = -1 if nb[5, 3] >= 0 else 0
    rejects(G.dgrad_reference(g, w, nb2, n)[0], "one pair dropped")
    # bias gradient: exact column sums
    assert torch.equal(G.bias_grad_reference(g), g.double().sum(0))


def test_wgrad_bounded_mode():
    gen = torch.Generator().manual_seed(4)
    nbr = _nbr(4)
    x = torch.randn(N_IN, CIN, generator=gen).to(torch.bfloat16).float()
    g = torch.randn(N_OUT, COUT, generator=gen).to(torch.bfloat16).float()
    ref, S = G.wgrad_reference(x, g, nbr=nbr)
    worst = G.check_wgrad_bounded(_shuffled_wgrad_fp32(x, g, nbr, 9, 3), ref, S, "shuffled fp32")
    print("wgrad bounded mode: worst err / bound of fp32 reassociation %.3f" % worst)
    pairs = G.pairs_of(nbr)
    drop = list(pairs); drop[4] = (pairs[4][0][1:], pairs[4][1][1:])
    with pytest.raises(AssertionError):
        G.check_wgrad_bounded(G.wgrad_reference(x, g, pairs=drop)[0].float(), ref, S, "pair dropped")


# ---- batch norm -----------------------------------------------------------------------------------------------------------

def _emulate_bn_fp32(x, w, b, eps, momentum, rm, rv, res=None, relu=False):
    """csrc/bnorm.hip's forward arithmetic on the CPU: sums about the first row in fp32 chains of bn_chain() terms merged in
    double, statistics in double rounded to fp32, the apply pass in fp32, one rounding to the slab type."""
    dtype = x.dtype
    n, c = x.shape
    xf = x.float()
    d = xf - xf[0]
    L = max(1, G.bn_chain(n, c, dtype) // 2)
    pad = (-n) % L
    dd = torch.cat([d, d.new_zeros(pad, c)], 0).reshape(-1, L, c)
    s1 = torch.zeros(dd.shape[0], c); s2 = torch.zeros(dd.shape[0], c)
    for j in range(L):
        s1 = s1 + dd[:, j]
        s2 = s2 + dd[:, j] * dd[:, j]
    s1, s2 = s1.double().sum(0), s2.double().sum(0)
    dm = s1 / n
    mean = xf[0].double() + dm
    var = (s2 / n - dm * dm).clamp_min(0)
    mean_f, invstd_f = mean.float(), (1.0 / torch.sqrt(var + eps)).float()
    sc = invstd_f * w.float()
    z = (xf - mean_f) * sc + b.float()
    if res is not None:
        z = z + res.float()
    if relu:
        z = z.clamp_min(0)
    unb = var * n / (n - 1)
    return dict(y=z.to(dtype), mean=mean_f, invstd=invstd_f,
                running_mean=((1 - momentum) * rm.double() + momentum * mean).float(),
                running_var=((1 - momentum) * rv.double() + momentum * unb).float())


def _bn_case(dtype, dist, n=3000, c=16, seed=0):
    gen = torch.Generator().manual_seed(seed)
    std = torch.rand(c, generator=gen) + 0.5
    mu = torch.randn(c, generator=gen) * 3
    if dist == "far_mean":
        mu = 1e3 * std * torch.sign(torch.randn(c, generator=gen))
    x = mu + std * torch.randn(n, c, generator=gen)
    if dist == "far_mean":
        x[0] = mu + 0.01 * std
    if dist == "outlier":
        x[0] = mu + 100 * std
    if dist == "constant":
        x[:, ::3] = mu[::3]
    x = x.to(dtype)
    w, b = torch.rand(c, generator=gen) + 0.5, torch.randn(c, generator=gen) * 0.1
    rm, rv = torch.randn(c, generator=gen), torch.rand(c, generator=gen) + 0.5
    res = (torch.randn(n, c, generator=gen) * 0.5).to(dtype)
    dy = torch.randn(n, c, generator=gen).to(dtype)
    return x, w, b, rm, rv, res, dy


@pytest.mark.parametrize("dist", ["normal", "far_mean", "outlier", "constant"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_bn_reference_equals_torch_and_accepts_the_kernel_arithmetic(dtype, dist):
    x, w, b, rm, rv, res, dy = _bn_case(dtype, dist)
    eps, mom = 1e-4, 0.1
    for residual, relu in ((None, False), (res, True)):
        ref = G.bn_reference(x, w, b, eps, mom, rm, rv, residual, relu)
        # against torch in float64 (forward, running statistics, autograd backward)
        xr = x.double().clone().requires_grad_(True)
        wr, br = w.double().clone().requires_grad_(True), b.double().clone().requires_grad_(True)
        rm_t, rv_t = rm.double().clone(), rv.double().clone()
        z = F.batch_norm(xr, rm_t, rv_t, wr, br, training=True, momentum=mom, eps=eps)
        if residual is not None:
            z = z + residual.double()
        y = z.clamp_min(0) if relu else z
        scale = float(ref["y"].abs().max())
        assert torch.allclose(ref["y"], y.detach(), rtol=0, atol=1e-9 * max(scale, 1.0))
        assert torch.allclose(ref["running_mean"], rm_t, rtol=1e-12, atol=1e-12)
        assert torch.allclose(ref["running_var"], rv_t, rtol=1e-12, atol=1e-12)
        mask_y = y.detach()                       # the mask comes from the output itself
        (y * dy.double()).sum().backward()
        bw = G.bn_backward_reference(x, w, dy, ref["mean"], ref["invstd"], y_got=mask_y if relu else None)
        assert torch.allclose(bw["dx"], xr.grad, rtol=0, atol=1e-9 * max(float(xr.grad.abs().max()), 1.0))
        assert torch.allclose(bw["dweight"], wr.grad, rtol=1e-9, atol=1e-9)
        assert torch.allclose(bw["dbias"], br.grad, rtol=1e-9, atol=1e-9)
        # the kernel's arithmetic, emulated in fp32, passes the per-element bounds
        em = _emulate_bn_fp32(x, w, b, eps, mom, rm, rv, residual, relu)
        worst = max(G.check_bn(em["y"], ref["y"], ref["E_y"], dtype, "y"),
                    G.check_bn(em["mean"], ref["mean"], ref["E_mean"], torch.float32, "mean"),
                    G.check_bn(em["invstd"], ref["invstd"], ref["E_invstd"], torch.float32, "invstd"),
                    G.check_bn(em["running_mean"], ref["running_mean"], ref["E_running_mean"], torch.float32, "running_mean"),
                    G.check_bn(em["running_var"], ref["running_var"], ref["E_running_var"], torch.float32, "running_var"))
        print("%s %s relu=%d: worst err / bound of the emulated kernel %.3f" % (dtype, dist, relu, worst))


def test_bn_checker_rejects_faults():
    dtype = torch.float32
    x, w, b, rm, rv, res, dy = _bn_case(dtype, "normal", n=40, c=8, seed=5)
    eps, mom = 1e-4, 0.1
    ref = G.bn_reference(x, w, b, eps, mom, rm, rv)
    bw = G.bn_backward_reference(x, w, dy, ref["mean"], ref["invstd"], ref["mean"].float(), ref["invstd"].float())
    G.check_bn(bw["dx"].float(), bw["dx"], bw["E_dx"], dtype, "dx")
    n = x.shape[0]
    # dx normalised with the unbiased variance
    is_unb = 1.0 / torch.sqrt(ref["var"] * n / (n - 1) + eps)
    bad = G.bn_backward_reference(x, w, dy, ref["mean"], is_unb)["dx"]
    with pytest.raises(AssertionError):
        G.check_bn(bad.float(), bw["dx"], bw["E_dx"], dtype, "dx, unbiased variance")
    # running_var updated with the biased variance
    bad_rv = (1 - mom) * rv.double() + mom * ref["var"]
    with pytest.raises(AssertionError):
        G.check_bn(bad_rv.float(), ref["running_var"], ref["E_running_var"], dtype, "running_var, biased")
    # y normalised with the unbiased variance
    bad_y = (x.double() - ref["mean"]) * is_unb * w.double() + b.double()
    with pytest.raises(AssertionError):
        G.check_bn(bad_y.float(), ref["y"], ref["E_y"], dtype, "y, unbiased variance")
    # the ReLU mask taken from the pre-activation instead of the kernel's y: differs where y rounded to 0
    x2, w2, b2, rm2, rv2, res2, dy2 = _bn_case(torch.bfloat16, "normal", n=400, c=8, seed=6)
    ref2 = G.bn_reference(x2, w2, b2, eps, mom, rm2, rv2, res2, relu=True)
    y_got = ref2["y"].float().to(torch.bfloat16)
    bw2 = G.bn_backward_reference(x2, w2, dy2, ref2["mean"], ref2["invstd"], y_got=y_got)
    G.check_bits(bw2["dres"].float().to(torch.bfloat16), bw2["dres"], "dres")
    bad_res = dy2.clone(); bad_res[y_got.float() <= 0] = 0; bad_res[3, 2] = dy2[3, 2] if y_got[3, 2] <= 0 else 0
    if float(dy2[3, 2]) != 0:
        with pytest.raises(AssertionError):
            G.check_bits(bad_res, bw2["dres"], "dres with one mask bit wrong")


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_sentinel_slab_catches_one_changed_byte(dtype):
    s = G.SentinelSlab(30, 16, dtype, "cpu")
    assert s.view.stride(0) > 16 and (s.view.data_ptr() - s.buf.data_ptr()) % 16 == 0
    s.fill(torch.randn(30, 16))
    s.check("written region only")
    for r, byte in ((2, 0), (30, s.col0 * s.buf.element_size()), (5, (s.col0 + 16) * s.buf.element_size() + 1)):
        t = G.SentinelSlab(30, 16, dtype, "cpu").fill(torch.randn(30, 16))
        t.buf.view(torch.uint8)[r, byte] ^= 1
        with pytest.raises(AssertionError):
            t.check("one byte changed at row %d byte %d" % (r, byte))
    u = G.SentinelSlab(30, 16, dtype, "cpu")
    u.check("untouched", written=False)
    u.view[0, 0] = 1
    with pytest.raises(AssertionError):
        u.check("a refused launch wrote", written=False)
