"""GPU tier: train-mode batch norm (csrc/bnorm.hip: pbn_bn_train_* and pbn_bn_act_train_* with and without residual /
ReLU) pinned to float64 (tests/grad_exact.py) in fp32, bf16 and fp16.

Forward y, save_mean, save_invstd, running_mean / running_var and backward dx, dweight, dbias are checked per element
against the documented bound (grad_exact's module docstring: it has a term for the shift of the first row); dres is the
masked dy bit for bit, masked by the kernel's own y.  x, dy, y, residual, dx and dres are strided column views (ld > c,
16-byte aligned) inside sentinel-filled slabs: nothing outside the written rows x columns may change, inputs not at all.
Row counts around the block size (1, 2, 127..129), BN_MAX_BLOCKS * 128 and one past it, the bench's level 0 and
configs[3]'s ~1.02 M; channels W, 32, 96, 384 (c / W not dividing 256) and the largest accepted (c / W = 256).
Distributions: channel means 1e3 std with the first row near the mean, the first row 100 std out, a constant channel,
outputs straddling the ReLU threshold.  Layouts layout_ok refuses return PBN_ERR_UNSUPPORTED and write nothing."""
import pytest
import torch

import grad_exact as G
import pbnet_amd.MinkowskiEngine as ME
from pbnet_amd import _native as N
from pbnet_amd.MinkowskiEngine.nn import _DT

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = (torch.float32, torch.bfloat16, torch.float16)
EPS, MOM = 1e-5, 0.1
_WORST = {}
_RAN = {}


def W_of(dtype):
    return 4 if dtype == torch.float32 else 8


def make_x(gen, n, c, dtype, dist):
    std = torch.rand(c, generator=gen, dtype=torch.float64) + 0.5
    mu = torch.randn(c, generator=gen, dtype=torch.float64)
    if dist == "far_mean":
        mu = 1e3 * std * torch.sign(torch.randn(c, generator=gen, dtype=torch.float64))
    x = mu + std * torch.randn(n, c, generator=gen, dtype=torch.float64)
    if dist == "far_mean":
        x[0] = mu + 0.01 * std
    elif dist == "outlier":
        x[0] = mu + 100 * std
    elif dist == "constant":
        x[:, ::3] = mu[::3]
    return x.to(dtype)


def stat_buf(vals, margin=4):
    """A float32 vector inside a sentinel-filled buffer: (buffer, view)."""
    buf = torch.empty(len(vals) + 2 * margin, dtype=torch.float32, device=DEV)
    buf.view(torch.int32).fill_(0x5A5A5A5A)
    v = buf[margin:margin + len(vals)]
    if vals is not None:
        v.copy_(vals)
    return buf, v


def stat_margins_ok(buf, margin=4):
    b = buf.view(torch.int32)
    return bool((b[:margin] == 0x5A5A5A5A).all()) and bool((b[-margin:] == 0x5A5A5A5A).all())


def run_case(dtype, n, c, dist, residual, relu, seed=0, label=""):
    gen = torch.Generator().manual_seed(seed * 1000 + n % 997 + c)
    x = make_x(gen, n, c, dtype, dist)
    w = (torch.rand(c, generator=gen) + 0.5)
    b = torch.randn(c, generator=gen) * 0.1
    rm0, rv0 = torch.randn(c, generator=gen), torch.rand(c, generator=gen) + 0.5
    res = None
    if residual:
        res = (torch.randn(n, c, generator=gen) * 0.5).to(dtype)
    if dist == "relu_edge":
        # outputs straddle zero: residual = -(normalised x) + a little noise, in the slab type
        pre = G.bn_reference(x.to(DEV), w, b, EPS, MOM, rm0, rv0)["z"].cpu()
        res = (-pre + 1e-2 * torch.randn(n, c, generator=gen, dtype=torch.float64)).to(dtype)
    dy = torch.randn(n, c, generator=gen).to(dtype)
    lib = N.lib()
    xs = G.SentinelSlab(n, c, dtype, DEV).fill(x.to(DEV))
    ys = G.SentinelSlab(n, c, dtype, DEV, col0=2 * W_of(dtype))
    rs = None if res is None else G.SentinelSlab(n, c, dtype, DEV, extra_cols=3 * W_of(dtype)).fill(res.to(DEV))
    inputs_before = [s.buf.clone() for s in (xs, rs) if s is not None]
    wd, bd = w.to(DEV), b.to(DEV)
    rmb, rm = stat_buf(rm0.to(DEV))
    rvb, rv = stat_buf(rv0.to(DEV))
    smb, sm = stat_buf(torch.zeros(c, device=DEV))
    sib, si = stat_buf(torch.zeros(c, device=DEV))
    wsb = int(lib.pbn_bn_workspace_bytes(c))
    ws = torch.zeros(wsb // 4 + 4, dtype=torch.float32, device=DEV)
    what = "%-8s n %7d c %4d %-9s%s%s %s" % (str(dtype).replace("torch.", ""), n, c, dist, " res" if res is not None else "",
                                            " relu" if relu else "", label)
    if res is None and not relu and seed % 2 == 0:
        rc = lib.pbn_bn_train_forward(N.c_vp(xs.view.data_ptr()), xs.ld, n, c, _DT[dtype], N.ptr(wd), N.ptr(bd), EPS, MOM,
                                      N.ptr(rm), N.ptr(rv), N.c_vp(ys.view.data_ptr()), ys.ld, N.ptr(sm), N.ptr(si),
                                      N.c_vp(ws.data_ptr()), wsb, N.current_stream())
    else:
        rc = lib.pbn_bn_act_train_forward(N.c_vp(xs.view.data_ptr()), xs.ld, n, c, _DT[dtype], N.ptr(wd), N.ptr(bd), EPS, MOM,
                                          N.ptr(rm), N.ptr(rv), None if rs is None else N.c_vp(rs.view.data_ptr()),
                                          0 if rs is None else rs.ld, int(relu), N.c_vp(ys.view.data_ptr()), ys.ld, N.ptr(sm),
                                          N.ptr(si), N.c_vp(ws.data_ptr()), wsb, N.current_stream())
    torch.cuda.synchronize()
    assert rc == 0, "%s: forward rc %d" % (what, rc)
    ref = G.bn_reference(xs.view, w, b, EPS, MOM, rm0, rv0, None if rs is None else rs.view, relu)
    ys.check(what + " y")
    for s, before in zip([s for s in (xs, rs) if s is not None], inputs_before):
        assert torch.equal(s.buf, before), "%s: an input slab changed" % what
    for bb in (rmb, rvb, smb, sib):
        assert stat_margins_ok(bb), "%s: a statistics vector written out of bounds" % what
    worst = {}
    worst["y"] = G.check_bn(ys.view, ref["y"], ref["E_y"], dtype, what + " y")
    worst["mean"] = G.check_bn(sm, ref["mean"], ref["E_mean"], torch.float32, what + " save_mean")
    worst["invstd"] = G.check_bn(si, ref["invstd"], ref["E_invstd"], torch.float32, what + " save_invstd")
    worst["rmean"] = G.check_bn(rm, ref["running_mean"], ref["E_running_mean"], torch.float32, what + " running_mean")
    worst["rvar"] = G.check_bn(rv, ref["running_var"], ref["E_running_var"], torch.float32, what + " running_var")

    # ---- backward: handed the exact statistics rounded to fp32, the kernel's own y as the ReLU mask ----
    mean_f, invstd_f = ref["mean"].float(), ref["invstd"].float()
    dys = G.SentinelSlab(n, c, dtype, DEV, col0=3 * W_of(dtype)).fill(dy.to(DEV))
    dxs = G.SentinelSlab(n, c, dtype, DEV)
    drs = G.SentinelSlab(n, c, dtype, DEV, extra_cols=2 * W_of(dtype)) if (res is not None or relu) else None
    dyb, yb = dys.buf.clone(), ys.buf.clone()
    dwb, dwv = stat_buf(torch.zeros(c, device=DEV))
    dbb, dbv = stat_buf(torch.zeros(c, device=DEV))
    if not relu and drs is None and seed % 2 == 0:
        rc = lib.pbn_bn_train_backward(N.c_vp(xs.view.data_ptr()), xs.ld, N.c_vp(dys.view.data_ptr()), dys.ld, n, c, _DT[dtype],
                                       N.ptr(wd), N.ptr(mean_f), N.ptr(invstd_f), N.c_vp(dxs.view.data_ptr()), dxs.ld, N.ptr(dwv),
                                       N.ptr(dbv), N.c_vp(ws.data_ptr()), wsb, N.current_stream())
    else:
        rc = lib.pbn_bn_act_train_backward(N.c_vp(xs.view.data_ptr()), xs.ld, N.c_vp(dys.view.data_ptr()), dys.ld,
                                           N.c_vp(ys.view.data_ptr()) if relu else None, ys.ld if relu else 0, n, c, _DT[dtype],
                                           N.ptr(wd), N.ptr(mean_f), N.ptr(invstd_f), N.c_vp(dxs.view.data_ptr()), dxs.ld,
                                           None if drs is None else N.c_vp(drs.view.data_ptr()), 0 if drs is None else drs.ld,
                                           N.ptr(dwv), N.ptr(dbv), N.c_vp(ws.data_ptr()), wsb, N.current_stream())
    torch.cuda.synchronize()
    assert rc == 0, "%s: backward rc %d" % (what, rc)
    bw = G.bn_backward_reference(xs.view, w, dys.view, ref["mean"], ref["invstd"], mean_f, invstd_f,
                                 y_got=ys.view if relu else None)
    dxs.check(what + " dx")
    if drs is not None:
        drs.check(what + " dres")
        G.check_bits(drs.view, bw["dres"], what + " dres")
    assert torch.equal(dys.buf, dyb) and torch.equal(ys.buf, yb) and torch.equal(xs.buf, inputs_before[0]), \
        "%s: a backward input changed" % what
    assert stat_margins_ok(dwb) and stat_margins_ok(dbb), "%s: dweight / dbias written out of bounds" % what
    worst["dx"] = G.check_bn(dxs.view, bw["dx"], bw["E_dx"], dtype, what + " dx")
    worst["dweight"] = G.check_bn(dwv, bw["dweight"], bw["E_dweight"], torch.float32, what + " dweight")
    worst["dbias"] = G.check_bn(dbv, bw["dbias"], bw["E_dbias"], torch.float32, what + " dbias")
    for k, v in worst.items():
        key = "%s %s" % (dist, k)
        _WORST[key] = max(_WORST.get(key, 0.0), v)
    _RAN[str(dtype)] = _RAN.get(str(dtype), 0) + 1
    print("%s: worst err/bound %s" % (what, " ".join("%s %.3f" % kv for kv in worst.items())))


SMALL_N = (1, 2, 127, 128, 129)
DISTS = ("normal", "far_mean", "outlier", "constant", "relu_edge")
TAILS = ((False, False), (True, False), (False, True), (True, True))


@pytest.mark.parametrize("dtype", DTYPES)
def test_bn_small_row_counts_every_width(dtype):
    W = W_of(dtype)
    i = 0
    for c in (W, 32, 96, 384, 256 * W):
        for n in SMALL_N:
            dist = DISTS[i % len(DISTS)] if n > 2 else "normal"
            res, relu = TAILS[i % len(TAILS)]
            run_case(dtype, n, c, dist, res or dist == "relu_edge", relu or dist == "relu_edge", seed=i)
            i += 1
    assert i == 25


@pytest.mark.parametrize("dtype", DTYPES)
def test_bn_distributions(dtype):
    """Every distribution with every tail at a block-boundary row count and a width that leaves idle threads."""
    i = 0
    for dist in DISTS:
        for res, relu in TAILS:
            if dist == "relu_edge" and not (res and relu):
                continue
            run_case(dtype, 4099, 96 if dtype != torch.float32 else 36, dist, res, relu, seed=i)
            i += 1
    assert i == 17


@pytest.mark.parametrize("dtype", DTYPES)
def test_bn_large_row_counts(dtype):
    """BN_MAX_BLOCKS * 128 rows and one past it (the last blocks take 129 rows, some none), the bench's level 0, and
    the widest channel count on a few thousand rows."""
    W = W_of(dtype)
    i = 0
    for n, c in ((131072, 96), (131073, 384), (146038, 96), (131073, W), (8191, 256 * W)):
        for dist, res, relu in (("far_mean", False, True), ("outlier", True, True)):
            run_case(dtype, n, c, dist, res, relu, seed=100 + i)
            i += 1
    assert i == 10


def test_bn_configs3_rows():
    """~1.02 M rows (configs[3]) at 32 channels, bf16 and fp32."""
    for dtype in (torch.bfloat16, torch.float32):
        run_case(dtype, 1020000, 32, "far_mean", True, True, seed=1)
        run_case(dtype, 1020000, 32, "outlier", False, False, seed=2)


def test_bn_refused_layouts_write_nothing():
    lib = N.lib()
    ran = 0
    for dtype in DTYPES:
        W = W_of(dtype)
        n = 300
        for c, shift, ldx, why in ((W + 2, 0, None, "c % W"), (2 * W, 1, None, "misaligned x"), (257 * W, 0, None, "c / W > 256"),
                                   (2 * W, 0, 2 * W + 1, "ld not 16-byte")):
            base = torch.randn(n * (c + 2 * W) + 64, device=DEV).to(dtype)
            ld = ldx if ldx is not None else c + 2 * W
            x = base[shift:shift + n * ld].view(n, ld)[:, :c]
            ys = G.SentinelSlab(n, c + (-c) % W, dtype, DEV)
            ws = torch.zeros(int(lib.pbn_bn_workspace_bytes(c)) // 4 + 4, dtype=torch.float32, device=DEV)
            sbufs = [stat_buf(torch.zeros(c, device=DEV)) for _ in range(6)]
            (smb, sm), (sib, si), (rmb, rm), (rvb, rv), (dwb, dw), (dbb, db) = sbufs
            before = [b.clone() for b, _ in sbufs]
            wv = torch.ones(c, device=DEV)
            rc = lib.pbn_bn_act_train_forward(N.c_vp(x.data_ptr()), ld, n, c, _DT[dtype], N.ptr(wv), N.ptr(wv), EPS, MOM,
                                              N.ptr(rm), N.ptr(rv), None, 0, 1, N.c_vp(ys.view.data_ptr()), ys.ld, N.ptr(sm),
                                              N.ptr(si), N.c_vp(ws.data_ptr()), ws.numel() * 4, N.current_stream())
            assert rc == N.PBN_ERR_UNSUPPORTED, "%s %s forward: rc %d" % (dtype, why, rc)
            rc = lib.pbn_bn_act_train_backward(N.c_vp(x.data_ptr()), ld, N.c_vp(x.data_ptr()), ld, None, 0, n, c, _DT[dtype],
                                               N.ptr(wv), N.ptr(wv), N.ptr(wv), N.c_vp(ys.view.data_ptr()), ys.ld, None, 0,
                                               N.ptr(dw), N.ptr(db), N.c_vp(ws.data_ptr()), ws.numel() * 4, N.current_stream())
            assert rc == N.PBN_ERR_UNSUPPORTED, "%s %s backward: rc %d" % (dtype, why, rc)
            torch.cuda.synchronize()
            ys.check("%s %s: refused" % (dtype, why), written=False)
            assert all(torch.equal(b, a) for (b, _), a in zip(sbufs, before)), "%s %s: statistics written" % (dtype, why)
            ran += 1
    assert ran == 12


def test_bn_module_counts_batches_and_matches_torch():
    """ME.MinkowskiBatchNorm on the native train path: num_batches_tracked, running statistics and the output after three
    steps against nn.BatchNorm1d in float64."""
    torch.manual_seed(3)
    c = 48
    mod = ME.MinkowskiBatchNorm(c).to(DEV).train()
    ref = torch.nn.BatchNorm1d(c).double().train()
    with torch.no_grad():
        mod.bn.weight.copy_(torch.rand(c) + 0.5)
        mod.bn.bias.copy_(torch.randn(c) * 0.1)
        ref.weight.copy_(mod.bn.weight.double().cpu())
        ref.bias.copy_(mod.bn.bias.double().cpu())
    i = torch.arange(4000, dtype=torch.int32)
    coords = torch.stack([torch.zeros_like(i), i % 1000, i // 1000, torch.zeros_like(i)], 1)
    for step in range(3):
        x = (torch.randn(4000, c) * 2 + 5).float()
        out = mod(ME.SparseTensor(x.to(DEV), coords.to(DEV))).F
        want = ref(x.double())
        assert float((out.double().cpu() - want).abs().max()) <= 1e-4
    assert int(mod.bn.num_batches_tracked) == 3 == int(ref.num_batches_tracked)
    assert torch.allclose(mod.bn.running_mean.double().cpu(), ref.running_mean, rtol=1e-5, atol=1e-6)
    assert torch.allclose(mod.bn.running_var.double().cpu(), ref.running_var, rtol=1e-5, atol=1e-6)


def test_zz_report():
    print("batch-norm cases per dtype: %s" % _RAN)
    print("worst err / bound per distribution and output: %s" % {k: round(v, 3) for k, v in sorted(_WORST.items())})
    assert all(v <= 1.0 for v in _WORST.values())
