"""GPU tier: the pointwise heads (csrc/heads.hip k_mlp_rows_mfma / k_mlp_rows), the class-score kernel (k_sem_argmax_table), segment
pooling (csrc/pool.hip, both kernels) and the IoU targets (csrc/iou.hip) against the float64 references of tests/heads_ref.py, on the
inputs of tests/heads_cases.py.  Every output element goes through heads_ref.accept (derived bounds; tests/test_heads_ref_cpu.py shows
what they reject) or is compared bit for bit.  Each test prints the figures it measured before it asserts."""
import numpy as np
import pytest
import torch

import heads_cases as C
import heads_ref as R
from pbnet_amd import PB_lib, pbnet_ops, stage_ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TORCH = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
_KEEP = []               # stage_ops caches the folded constants by id(head): keep every head alive so that no id is reused
_X = {}


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t if dtype is None else t.to(TORCH[dtype])


def _host(t):
    return t.detach().double().cpu().numpy()


def _head_x(dtype):
    if dtype not in _X:
        _X[dtype] = _dev(C.head_x(dtype), dtype)
    return _X[dtype]


def _head(hidden, n_out, sigmoid):
    import pbnet_amd.MinkowskiEngine as ME
    p = C.head_params(hidden, n_out)
    layers = [ME.MinkowskiLinear(32, hidden, bias=False), ME.MinkowskiBatchNorm(hidden, eps=C.BN_EPS),
              ME.MinkowskiPReLU(num_parameters=hidden), ME.MinkowskiLinear(hidden, n_out, bias=True)]
    if sigmoid:
        layers.append(ME.MinkowskiSigmoid())
    head = torch.nn.Sequential(*layers).eval()
    t = lambda k: torch.from_numpy(p[k])
    with torch.no_grad():
        head[0].linear.weight.copy_(t("w1"))
        bn = head[1].bn
        bn.weight.copy_(t("bn_weight")); bn.bias.copy_(t("bn_bias")); bn.running_mean.copy_(t("mean")); bn.running_var.copy_(t("var"))
        head[2].module.weight.copy_(t("slope"))
        head[3].linear.weight.copy_(t("w2")); head[3].linear.bias.copy_(t("b2"))
    head = head.to(DEV)
    _KEEP.append(head)
    return head, p


def _folded(head, p):
    """The fp32 (scale, shift) the wrapper folded the BatchNorm into, checked against the float64 fold within the bound of its five
    roundings; the kernel is then judged on the constants as stored."""
    hp = stage_ops._HEADS[id(head)]
    scale, shift = _host(hp.scale), _host(hp.shift)
    s8, h8 = C.fold_bn(p)
    es, eh = C.fold_bn_bounds(p)
    assert (np.abs(scale - s8) <= es).all() and (np.abs(shift - h8) <= eh).all()
    assert np.array_equal(_host(hp.slope), p["slope"].astype(np.float64)) and np.array_equal(_host(hp.w2), p["w2"].astype(np.float64))
    return scale, shift


def _check_head(got, dtype, x, idx_a, idx_b, in_rows, p, scale, shift, sigmoid, what):
    value, bound = R.mlp_rows(x, idx_a, idx_b, in_rows, p["w1"], scale, shift, p["slope"], p["w2"], p["b2"], sigmoid)
    assert got.dtype == TORCH[dtype] and tuple(got.shape) == value.shape
    g = _host(got)
    ok = R.accept(g, value, bound, dtype)
    worst = float((np.abs(g - value) / bound).max())
    assert ok.all(), (what, int((~ok).sum()), worst)
    return worst


@pytest.mark.parametrize("dtype", C.DTYPES)
@pytest.mark.parametrize("hidden", C.HEAD_HIDDEN)
@pytest.mark.parametrize("n_out", C.HEAD_OUT_MFMA + C.HEAD_OUT_SCALAR)
def test_heads(dtype, hidden, n_out):
    """n in {1, 15, 16, 17, 16005} x {no sigmoid, sigmoid} x {no index, idx_a, idx_a + idx_b} of one head; n_out <= 32 runs the matrix-core
    kernel (one or two 16-output tiles), 33 and 40 the scalar kernel.  Distinct slopes (one negative), running_var down to 1e-3."""
    xh, xd = C.head_x(dtype), _head_x(dtype)
    worst = 0.0
    for sigmoid in (False, True):
        head, p = _head(hidden, n_out, sigmoid)
        stage_ops.mlp_rows(head, xd[:1])
        scale, shift = _folded(head, p)
        for n in C.HEAD_N:
            for form in C.HEAD_FORMS:
                idx_a, idx_b = C.head_index(form, n)
                feats = xd[:n] if form == "none" else xd
                got = stage_ops.mlp_rows(head, feats, None if idx_a is None else _dev(idx_a), None if idx_b is None else _dev(idx_b))
                worst = max(worst, _check_head(got, dtype, xh[:n] if form == "none" else xh, idx_a, idx_b, None, p, scale, shift,
                                               sigmoid, (sigmoid, n, form)))
    if dtype == "fp32":                  # a 16-bit output is judged by its rounding interval: the ratio says nothing there
        print("heads fp32 hidden %d n_out %d: largest |got - value| / bound = %.3f" % (hidden, n_out, worst))


@pytest.mark.parametrize("dtype", C.DTYPES)
def test_heads_padded_slab_and_row_capacity(dtype):
    """(a) the 32 channels as a view of a 40-column slab (ld_in = 40; the other 8 columns hold 1e4); (b) the capacity form: a device-side
    row count below the capacity, and rows at or beyond in_rows read as zeros."""
    xh = C.head_x(dtype)[:1000]
    slab = torch.full((1000, 40), 1e4, dtype=TORCH[dtype], device=DEV)
    slab[:, :32] = _head_x(dtype)[:1000]
    view = slab[:, :32]
    assert view.stride(0) == 40 and view.data_ptr() % 16 == 0
    for hidden, n_out, sigmoid in ((16, 3, False), (32, 20, True), (32, 40, False)):
        head, p = _head(hidden, n_out, sigmoid)
        stage_ops.mlp_rows(head, view[:1])
        scale, shift = _folded(head, p)
        idx_a, _ = C.head_index("a", 17)
        idx_a = np.where(idx_a >= 0, idx_a % 1000, idx_a)
        _check_head(stage_ops.mlp_rows(head, view), dtype, xh, None, None, None, p, scale, shift, sigmoid, "ld 40")
        _check_head(stage_ops.mlp_rows(head, view, _dev(idx_a)), dtype, xh, idx_a, None, None, p, scale, shift, sigmoid, "ld 40 + idx")
        # capacity 64, 37 rows exist, the slab holds 600 rows: indices 600 .. 999 name rows that were never computed
        cap_idx = np.random.default_rng(3).integers(0, 1000, 64).astype(np.int64)
        cap_idx[:4] = (599, 600, 999, -1)
        n_dev = torch.tensor([37], dtype=torch.int32, device=DEV)
        got = stage_ops.mlp_rows(head, view, _dev(cap_idx), None, 64, n_dev=n_dev, in_rows=600)
        _check_head(got[:37], dtype, xh, cap_idx[:37], None, 600, p, scale, shift, sigmoid, "capacity")


def test_heads_beyond_the_workgroup_cap():
    """2 097 152 + 21 rows: 8192 workgroups, every wave walks more than 4 row blocks, the last block is partial.  Rows gathered from a
    4096-row slab; the reference computes the slab's rows once and gathers."""
    dtype = "bf16"
    xh, xd = C.head_x(dtype)[:C.CAP_SLAB], _head_x(dtype)[:C.CAP_SLAB]
    idx = C.cap_index()
    idx_d = _dev(idx)
    for sigmoid in (False, True):
        head, p = _head(16, 1, sigmoid)
        got = stage_ops.mlp_rows(head, xd, idx_d)
        scale, shift = _folded(head, p)
        assert got.shape == (C.CAP_ROWS, 1)
        _check_head(got, dtype, xh, idx, None, None, p, scale, shift, sigmoid, "cap")


# ---- class scores -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", C.DTYPES)
@pytest.mark.parametrize("n_cls", C.SEM_CLS)
@pytest.mark.parametrize("nb", (1, C.MAX_SCENES))
def test_class_scores(dtype, n_cls, nb):
    """Arg-max (first maximum), [class, batch] table and per-block histogram exact; own-class probability within its bound.  Inputs
    hold planted ties, all-equal rows, -inf entries and +-80 / +-100 rows."""
    worst = 0.0
    for n in C.SEM_N:
        score, batch = C.sem_scores(dtype, n, n_cls, nb)
        arg, prob, bound, table, hist = R.sem_argmax(score, batch, nb)
        sem_pred, sem_prob, tab, bh = stage_ops.sem_argmax_table(_dev(score, dtype), _dev(batch), nb)
        assert sem_prob.dtype == TORCH[dtype]
        g = _host(sem_prob)
        if dtype == "fp32":
            worst = max(worst, float((np.abs(g - prob) / R.ulp32(prob)).max()))
        assert np.array_equal(sem_pred.cpu().numpy(), arg), n
        assert np.array_equal(tab.cpu().numpy(), table) and np.array_equal(bh.cpu().numpy(), hist), n
        ok = R.accept(g, prob, bound, dtype)
        assert ok.all(), (n, int((~ok).sum()))
    if dtype == "fp32":
        print("class scores fp32 n_cls %d nb %d: largest |prob - float64| = %.3f fp32 ulps" % (n_cls, nb, worst))


# ---- segment pooling ----------------------------------------------------------------------------------------------------

def _pool(feats_d, ss, **kw):
    from pbnet_amd.MinkowskiEngine.nn import segment_pool
    return segment_pool(feats_d, None, len(ss) - 1, seg_start=_dev(np.asarray(ss, np.int32)), **kw)


def _check_pool(feats_h, feats_d, ss, family, what):
    mx, mean, bound = R.segment_pool(feats_h, ss)
    got_mx, got_av = _pool(feats_d, ss)
    assert got_mx.dtype == got_av.dtype == torch.float32
    gm, ga = _host(got_mx), _host(got_av)
    assert R.accept(gm, mx, 0.0, "fp32").all(), what                     # bit-exact, -inf for an empty segment
    ok = R.accept(ga, mean, bound, "fp32")                               # NaN for an empty segment
    assert ok.all(), (what, int((~ok).sum()))
    unequal = 0
    if family == "exact":
        lens = np.diff(ss)[:, None]
        with np.errstate(invalid="ignore", divide="ignore"):
            want = (R.segment_sums(feats_h, ss) / lens).astype(np.float32).astype(np.float64)
        unequal = int((ga != want)[np.broadcast_to(lens > 0, want.shape)].sum())
        assert R.accept(ga, want, R.ulp32(want), "fp32").all(), what
    # one output at a time: the same bits
    only_mx, none_av = _pool(feats_d, ss, want_avg=False)
    none_mx, only_av = _pool(feats_d, ss, want_max=False)
    assert none_av is None and none_mx is None
    assert torch.equal(only_mx, got_mx) and torch.equal(only_av.nan_to_num(7.0), got_av.nan_to_num(7.0))
    return unequal


def _pool_case(dtype, channels, n_seg, pad=0, first=0):
    lens = C.pool_lens(n_seg, channels, dtype)
    assert len(lens) == n_seg
    ss = np.concatenate([[0], np.cumsum(lens)])
    unequal = 0
    for family in ("exact", "normal"):
        slab = C.pool_feats(family, dtype, int(ss[-1]), channels + pad)
        slab_d = _dev(slab, dtype)
        view = slab_d[:, first:first + channels]
        unequal += _check_pool(slab[:, first:first + channels], view, ss, family, (family, dtype, channels, n_seg))
    return unequal, view


@pytest.mark.parametrize("dtype", C.DTYPES)
@pytest.mark.parametrize("channels", C.POOL_CHANNELS)
@pytest.mark.parametrize("n_seg", C.POOL_SEGS)
def test_segment_pool(dtype, channels, n_seg):
    """Splits 64, 64, 60 (two-pass kernels) and 1, 1 (the single-pass kernel, two or three channel chunks at 48 and 96 channels);
    segment lengths 0, 1, split -+ 1, 4 rps k -+ 1, one of 20011 rows.  Exact-sum inputs (k / 8) and unit normal inputs."""
    unequal, _ = _pool_case(dtype, channels, n_seg)
    print("segment pool %s C %d n_seg %d: exact-sum averages that differ from the correctly rounded quotient: %d"
          % (dtype, channels, n_seg, unequal))


@pytest.mark.parametrize("dtype,channels", [("fp32", 6), ("bf16", 34), ("fp16", 34)])
@pytest.mark.parametrize("n_seg", (7, 17, 1024))
def test_segment_pool_rows_that_are_no_whole_vectors(dtype, channels, n_seg):
    """Row bytes not a multiple of 16: the single-pass kernel whatever the split."""
    _pool_case(dtype, channels, n_seg)


@pytest.mark.parametrize("dtype,channels,pad,first", [("fp32", 20, 4, 0), ("bf16", 16, 8, 0), ("fp16", 32, 8, 0), ("fp32", 16, 4, 1)])
def test_segment_pool_padded_leading_dimension(dtype, channels, pad, first):
    """A column view of a wider slab: 16-byte aligned rows (two-pass kernels), and one fp32 view from column 1 whose pointer is only
    4-byte aligned (the single-pass kernel must run)."""
    for n_seg in (7, 17):
        _, view = _pool_case(dtype, channels, n_seg, pad, first)
        assert view.stride(0) == channels + pad and view.data_ptr() % 16 == 4 * first


# ---- IoU targets --------------------------------------------------------------------------------------------------------

def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


@pytest.mark.parametrize("n_inst,n_prop", C.IOU_CASES)
def test_iou_and_mask_label(n_inst, n_prop):
    """Modes -1, 0 and 1 through pbnet_ops and through the in-place PB_lib entry points: IoU bit-exact, mask_label element for element
    (the untouched -1 rows included).  257 instances: strided histogram loops; 20000: more than 64 KB of LDS; 32773 proposals: the
    grid-stride loop; pointnum above 2^24: the (float)uni rounding; planted proposals at the 0.5 threshold and with a tied maximum."""
    c = C.iou_case(n_inst, n_prop)
    idx, off, labels, pn, sc = (_dev(c[k]) for k in ("idx", "off", "labels", "pointnum", "scores"))
    want = R.iou(c["idx"], c["off"], c["labels"], c["pointnum"])
    got = pbnet_ops.get_iou(idx, off, labels, pn)
    assert got.shape == want.shape and np.array_equal(_bits(got.cpu().numpy()), _bits(want))
    out = torch.full((n_prop, n_inst), -7.0, device=DEV)
    PB_lib.get_iou(idx, off, labels, pn, out, n_inst, n_prop)
    assert np.array_equal(_bits(out.cpu().numpy()), _bits(want))
    for mode in (0, 1):
        want = R.iou(c["idx"], c["off"], c["labels"], c["pointnum"], c["scores"], mode)
        want_ml = R.mask_label(c["idx"], c["off"], c["labels"], want)
        iou, ml = pbnet_ops.cal_iou_and_masklabel(idx, off, labels, pn, sc, mode)
        assert np.array_equal(_bits(iou.cpu().numpy()), _bits(want)), mode
        assert ml.shape == sc.shape and np.array_equal(ml.cpu().numpy().reshape(-1), want_ml), mode
        out = torch.full((n_prop, n_inst), -7.0, device=DEV)
        ml2 = torch.full((len(c["idx"]), 1), -1.0, device=DEV)
        PB_lib.cal_iou_and_masklabel(idx, off, labels, pn, out, n_inst, n_prop, sc, ml2, mode)
        assert np.array_equal(_bits(out.cpu().numpy()), _bits(want)) and np.array_equal(ml2.cpu().numpy().reshape(-1), want_ml), mode
        if c["planted"] == 3:
            assert (want_ml[c["off"][0]:c["off"][1]] == -1).all() and (want_ml[c["off"][1]:c["off"][2]] == 1).all()
            assert sorted(np.unique(want_ml[c["off"][2]:c["off"][3]])) == [0.0, 1.0]
