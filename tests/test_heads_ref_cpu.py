"""CPU tier of tests/test_heads_pool_iou_gpu.py: shows without a GPU that those tests would catch a subtly wrong kernel.
(1) tests/heads_ref.py agrees with the restatements the project already has, where they overlap; (2) an honest fp32 evaluation
(numpy float32, both summation orders the two head kernels use) passes `accept` on every input set of tests/heads_cases.py;
(3) each of a list of deliberately wrong variants is rejected on the same inputs."""
import functools

import numpy as np
import pytest
import torch

import heads_cases as C
import heads_ref as R

F4 = np.float32
ORDERS = {"sequential": list(range(32)), "strided": [8 * q + k for k in range(8) for q in range(4)]}   # 0, 8, 16, 24, 1, 9, ...


# ---- (1) the reference against the existing restatements ------------------------------------------------------------------

@pytest.mark.parametrize("n_inst,n_prop", [(1, 64), (37, 64), (257, 64), (37, 1)])
def test_iou_agrees_with_the_oracles(n_inst, n_prop):
    from oracle import loss_ref
    from oracle import pb_cluster_ref as oracle
    c = C.iou_case(n_inst, n_prop)
    mine = R.iou(c["idx"], c["off"], c["labels"], c["pointnum"])
    # the C oracle ignores nothing: labels >= n_inst never equal an instance id there either
    want = oracle.get_iou(c["idx"], c["off"], c["labels"], c["pointnum"])
    assert np.array_equal(mine.view(np.int32), want.view(np.int32))
    assert np.array_equal(mine.view(np.int32), R.iou(c["idx"], c["off"], c["labels"], c["pointnum"], c["scores"], 0).view(np.int32))
    # oracle/loss_ref.get_iou adds the 1e-5 BEFORE it rounds the denominator to fp32, then divides in fp32: two roundings instead of
    # one, so it may differ from the double quotient in the last place and no further -- where uni is exact in fp32.  Above 2^24
    # the 1e-5 breaks the tie of an odd uni upwards where (float)uni rounds to even: not shared ground, left out.
    other = loss_ref.get_iou(c["idx"], c["off"], c["labels"], c["pointnum"])
    small = c["pointnum"] <= 2 ** 24
    assert small.any() and (np.abs(mine.astype(np.float64) - other) <= np.maximum(R.ulp32(mine), R.ulp32(other)))[:, small].all()


@pytest.mark.parametrize("hidden,n_out,sigmoid", [(16, 1, True), (16, 20, False), (32, 32, False), (32, 40, True)])
def test_head_agrees_with_a_float64_torch_module(hidden, n_out, sigmoid):
    p = C.head_params(hidden, n_out)
    layers = [torch.nn.Linear(32, hidden, bias=False), torch.nn.BatchNorm1d(hidden, eps=C.BN_EPS), torch.nn.PReLU(hidden),
              torch.nn.Linear(hidden, n_out)]
    if sigmoid:
        layers.append(torch.nn.Sigmoid())
    head = torch.nn.Sequential(*layers).double().eval()
    t = lambda k: torch.from_numpy(p[k].astype(np.float64))
    with torch.no_grad():
        head[0].weight.copy_(t("w1"))
        head[1].weight.copy_(t("bn_weight")); head[1].bias.copy_(t("bn_bias"))
        head[1].running_mean.copy_(t("mean")); head[1].running_var.copy_(t("var"))
        head[2].weight.copy_(t("slope"))
        head[3].weight.copy_(t("w2")); head[3].bias.copy_(t("b2"))
        x = C.head_x("bf16")[:3000]
        want = head(torch.from_numpy(x.astype(np.float64))).numpy()
    idx_a, idx_b = C.head_index("ab", 17)
    scale, shift = C.fold_bn(p)
    value, bound = R.mlp_rows(x, None, None, None, p["w1"], scale, shift, p["slope"], p["w2"], p["b2"], sigmoid)
    assert np.abs(value - want).max() <= 1e-12 * max(1.0, np.abs(want).max())
    assert (bound > 0).all() and (bound < 1e-3).all()
    # index levels: a -1 at either level reads the zero row
    xs = C.head_x("bf16")
    v2, _ = R.mlp_rows(xs, idx_a, idx_b, None, p["w1"], scale, shift, p["slope"], p["w2"], p["b2"], sigmoid)
    row = np.where(idx_a >= 0, idx_b[np.maximum(idx_a, 0)], -1)
    with torch.no_grad():
        full = head(torch.from_numpy(np.concatenate([xs, np.zeros((1, 32), F4)]).astype(np.float64))).numpy()
    assert (row < 0).any() and np.abs(v2 - full[np.where(row < 0, len(xs), row)]).max() <= 1e-12 * max(1.0, np.abs(full).max())
    # rows >= in_rows read as zeros too
    v3, _ = R.mlp_rows(xs, np.array([5, 2999, 3000, 16004]), None, 3000, p["w1"], scale, shift, p["slope"], p["w2"], p["b2"], sigmoid)
    assert np.array_equal(v3[2], v3[3]) and np.abs(v3[2] - full[len(xs)]).max() <= 1e-12 and not np.array_equal(v3[1], v3[2])


def test_pool_agrees_with_the_sparse_oracle():
    from oracle import sparse_ref
    lens = C.pool_lens(17, 20, "fp32")
    lens = [n for n in lens if n > 0]                          # the oracle divides by a count: no empty segments there
    feats = C.pool_feats("normal", "fp32", sum(lens), 20).astype(np.float64)
    ss = np.concatenate([[0], np.cumsum(lens)])
    mx, mean, bound = R.segment_pool(feats, ss)
    b = np.repeat(np.arange(len(lens)), lens)
    t = torch.from_numpy(feats)
    assert np.array_equal(mx, sparse_ref.global_pool(t, b, len(lens), "max").numpy())
    assert np.abs(mean - sparse_ref.global_pool(t, b, len(lens), "avg").numpy()).max() <= 1e-13
    mx0, mean0, _ = R.segment_pool(feats, np.array([0, 0, 5]))
    assert np.isinf(mx0[0]).all() and np.isnan(mean0[0]).all() and np.isfinite(mean0[1]).all()


def test_rounding_helpers():
    rng = np.random.default_rng(0)
    v = np.concatenate([rng.normal(0, 1, 5000) * np.exp(rng.uniform(-30, 30, 5000)), [0.0, 65504.0, 65519.9, 65520.0, 1e39, -1e39,
                                                                                       2.0 ** -25, 3 * 2.0 ** -25, 1e-45]])
    with np.errstate(over="ignore"):
        assert np.array_equal(R.round_to(v, "fp16"), v.astype(np.float16).astype(np.float64))
        assert np.array_equal(R.round_to(v, "fp32"), v.astype(np.float32).astype(np.float64))
    # bf16 against torch, from values that fp32 holds exactly (so torch's fp32 -> bf16 is a single rounding too)
    with np.errstate(over="ignore"):
        v32 = v.astype(np.float32)
    want = torch.from_numpy(v32).to(torch.bfloat16).double().numpy()
    assert np.array_equal(R.round_to(v32.astype(np.float64), "bf16"), want)
    bits = torch.from_numpy(v32).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    assert np.array_equal(R.widen_bf16(bits), want)
    # one rounding, not two: 1 + 2^-8 + 2^-30 lies above the bf16 midpoint, through fp32 it would fall on it and tie to even
    assert R.round_to(1 + 2.0 ** -8 + 2.0 ** -30, "bf16") == 1 + 2.0 ** -7
    assert R.ulp32(1.0) == 2.0 ** -23 and R.ulp32(0.75) == 2.0 ** -24 and R.ulp32(0.0) == 2.0 ** -149


# ---- (2) + (3) heads --------------------------------------------------------------------------------------------------

def _bf16(a):
    return R.round_to(a.astype(np.float64), "bf16").astype(F4)


def emulate_head(x, p, sigmoid, dtype, order, perm=None, eps=C.BN_EPS, half_hidden=False, bias_shift=False, bf16_layers=False,
                 twice=None):
    """Every step in numpy float32, channels summed in `order`.  The keyword arguments switch on the wrong variants."""
    hid, n_out = p["w1"].shape[0], p["w2"].shape[0]
    scale = (p["bn_weight"] / np.sqrt(p["var"] + F4(eps))).astype(F4)
    shift = (p["bn_bias"] - p["mean"] * scale).astype(F4)
    slope = p["slope"]
    if perm is not None:                                     # (which, permutation of the hidden index)
        which, pi = perm
        scale, shift, slope = (a[pi] if k == which else a for k, a in (("scale", scale), ("shift", shift), ("slope", slope)))
    a = np.zeros((x.shape[0], hid), F4)
    for c in order:
        a = a + x[:, c:c + 1] * p["w1"][:, c][None, :]
    t = a * scale + shift
    h = np.where(t >= 0, t, t * slope).astype(F4)
    if bf16_layers:
        h = _bf16(h)
    b2 = p["b2"]
    if bias_shift:                                           # bias of output o lands on output o - 16
        b2 = np.concatenate([p["b2"][16:], np.zeros(min(16, n_out), F4)])[:n_out]
    o = np.broadcast_to(b2, (x.shape[0], n_out)).astype(F4)
    for k in range(hid // 2 if half_hidden else hid):
        o = o + h[:, k:k + 1] * p["w2"][:, k][None, :]
    if bf16_layers:
        o = _bf16(o)
    if sigmoid:
        with np.errstate(over="ignore"):
            o = (F4(1) / (F4(1) + np.exp(-o))).astype(F4)
    o = o.astype(np.float64)
    if twice is not None:
        o = R.round_to(o, twice)
    return R.round_to(o, dtype)


@functools.lru_cache(maxsize=8)
def _head_setup(dtype, hidden, n_out, sigmoid):
    p = C.head_params(hidden, n_out)
    x = np.concatenate([C.head_x(dtype), np.zeros((1, 32), F4)])           # the zero row every index form can resolve to
    scale = (p["bn_weight"] / np.sqrt(p["var"] + F4(C.BN_EPS))).astype(F4)
    shift = (p["bn_bias"] - p["mean"] * scale).astype(F4)
    value, bound = R.mlp_rows(x, None, None, None, p["w1"], scale, shift, p["slope"], p["w2"], p["b2"], sigmoid)
    return p, x, value, bound


@pytest.mark.parametrize("dtype", C.DTYPES)
@pytest.mark.parametrize("hidden", C.HEAD_HIDDEN)
def test_honest_fp32_heads_are_accepted(dtype, hidden):
    """Every row of the slab (the index forms of the GPU tier only gather from it) and the zero row, every n_out, both orders."""
    for n_out in C.HEAD_OUT_MFMA + C.HEAD_OUT_SCALAR:
        for sigmoid in (False, True):
            p, x, value, bound = _head_setup(dtype, hidden, n_out, sigmoid)
            for name, order in ORDERS.items():
                ok = R.accept(emulate_head(x, p, sigmoid, dtype, order), value, bound, dtype)
                assert ok.all(), (n_out, sigmoid, name, int((~ok).sum()))
    # the folded BatchNorm constants in fp32 lie within their own bound of the float64 ones
    p = C.head_params(hidden, 1)
    s8, h8 = C.fold_bn(p)
    es, eh = C.fold_bn_bounds(p)
    s4 = (p["bn_weight"] / np.sqrt(p["var"] + F4(C.BN_EPS))).astype(F4)
    assert (np.abs(s4 - s8) <= es).all() and (np.abs((p["bn_bias"] - p["mean"] * s4).astype(F4) - h8) <= eh).all()


def _rot(hidden):
    return np.roll(np.arange(hidden), 1)


def _swap_quads(hidden):
    """The layout slip the matrix-core kernel could make: hidden 16 t + 4 kq + i read as 16 t + 4 i + kq."""
    h = np.arange(hidden)
    return 16 * (h // 16) + 4 * (h % 4) + (h % 16) // 4


WRONG_HEADS = {
    "slope from a rotated hidden index": dict(perm=("slope", _rot)),
    "slope with the 4 x 4 lane layout transposed": dict(perm=("slope", _swap_quads)),
    "scale from a permuted hidden index": dict(perm=("scale", _swap_quads)),
    "shift from a permuted hidden index": dict(perm=("shift", _swap_quads)),
    "BatchNorm eps dropped": dict(eps=0.0),
    "hidden units of the second half ignored": dict(half_hidden=True),
    "bias of output o applied to output o - 16": dict(bias_shift=True),
    "rounded to bf16 after each layer": dict(bf16_layers=True),
    "output rounded twice, through fp16": dict(twice="fp16"),
    "output rounded twice, through bf16": dict(twice="bf16"),
}


# a second rounding exists only for a 16-bit output, through the other 16-bit type
WRONG_HEAD_CASES = [(v, d) for v in sorted(WRONG_HEADS) for d in C.DTYPES
                    if "twice" not in WRONG_HEADS[v] or (d != "fp32" and WRONG_HEADS[v]["twice"] != d)]


@pytest.mark.parametrize("variant,dtype", WRONG_HEAD_CASES)
def test_wrong_heads_are_rejected(variant, dtype):
    kw = dict(WRONG_HEADS[variant])
    for hidden in C.HEAD_HIDDEN:
        if "perm" in kw and callable(kw["perm"][1]):
            kw_h = dict(kw, perm=(kw["perm"][0], kw["perm"][1](hidden)))
        else:
            kw_h = kw
        for n_out in (1, 17, 32, 40):
            if kw.get("bias_shift") and n_out <= 16:
                continue
            for sigmoid in (False, True):
                p, x, value, bound = _head_setup(dtype, hidden, n_out, sigmoid)
                ok = R.accept(emulate_head(x, p, sigmoid, dtype, ORDERS["strided"], **kw_h), value, bound, dtype)
                assert not ok.all(), (hidden, n_out, sigmoid)


# ---- (2) + (3) class scores ---------------------------------------------------------------------------------------------

def emulate_sem(score, sub_max=True, last_wins=False):
    s = score.astype(F4)
    arg = (s.shape[1] - 1 - np.argmax(s[:, ::-1], 1)) if last_wins else np.argmax(s, 1)
    best = s[np.arange(len(s)), arg]
    with np.errstate(over="ignore", invalid="ignore"):
        if sub_max:
            e = np.exp(s - best[:, None]).astype(F4)
            tot = np.zeros(len(s), F4)
            for c in range(s.shape[1]):
                tot = tot + e[:, c]
            prob = F4(1) / tot
        else:
            e = np.exp(s).astype(F4)
            tot = np.zeros(len(s), F4)
            for c in range(s.shape[1]):
                tot = tot + e[:, c]
            prob = e[np.arange(len(s)), arg] / tot
    return arg, prob.astype(np.float64)


@pytest.mark.parametrize("dtype", C.DTYPES)
def test_class_scores_honest_accepted_wrong_rejected(dtype):
    seen = set()
    for n in C.SEM_N:
        for n_cls in C.SEM_CLS:
            for nb in (1, C.MAX_SCENES):
                score, batch = C.sem_scores(dtype, n, n_cls, nb)
                arg, prob, bound, table, hist = R.sem_argmax(score, batch, nb)
                assert table.sum() == n and hist.sum() == n and hist.shape[0] == max(-(-n // 1024), 1)
                assert np.array_equal(hist.sum(0), table.sum(1))
                got_arg, got_prob = emulate_sem(score)
                assert np.array_equal(got_arg, arg)
                assert R.accept(R.round_to(got_prob, dtype), prob, bound, dtype).all()
                # what the input holds
                mx = score.max(1, keepdims=True)
                ties = (score == mx).sum(1)
                if (ties > 1).any():
                    seen.add("tie")
                    first = np.argmax(score == mx, 1)
                    seen.update({"tie first"} if (first[ties > 1] == 0).any() else ())
                    seen.update({"tie last"} if (score[ties > 1, -1] == mx[ties > 1, 0]).any() else ())
                if (ties == n_cls).any():
                    seen.add("all equal")
                if np.isinf(score).any():
                    seen.add("-inf")
                    assert not np.isinf(mx).any()
                if n >= 1023:
                    # last maximum wins: a different class on the tied rows
                    bad_arg, _ = emulate_sem(score, last_wins=True)
                    assert not np.array_equal(bad_arg, arg)
                    # no max subtraction: exp overflows at +-100
                    _, bad_prob = emulate_sem(score, sub_max=False)
                    assert not R.accept(R.round_to(bad_prob, dtype), prob, bound, dtype).all()
    assert seen == {"tie", "tie first", "tie last", "all equal", "-inf"}
    assert not np.isnan(C.sem_scores(dtype, 2049, 20, 1)[0]).any()
    if dtype == "fp32":
        assert (np.abs(C.sem_scores(dtype, 2049, 20, 1)[0]) == 80).any()


# ---- (2) + (3) pooling ------------------------------------------------------------------------------------------------

def emulate_pool(feats, ss, split, len_off=0, drop_last=False):
    """fp32: every slice summed in row order, the slices folded in order, one divide (the two-pass kernel's shape)."""
    n_seg = len(ss) - 1
    mx = np.full((n_seg, feats.shape[1]), -np.inf, F4)
    av = np.zeros((n_seg, feats.shape[1]), F4)
    for b in range(n_seg):
        beg, ln = int(ss[b]), int(ss[b + 1] - ss[b])
        tot = np.zeros(feats.shape[1], F4)
        for z in range(split):
            lo, hi = beg + ln * z // split, beg + ln * (z + 1) // split
            if drop_last and hi > lo:
                hi -= 1
            part = np.zeros(feats.shape[1], F4)
            for r in range(lo, hi):
                part = part + feats[r]
            if hi > lo:
                mx[b] = np.maximum(mx[b], feats[lo:hi].max(0))
            tot = tot + part
        with np.errstate(invalid="ignore", divide="ignore"):
            av[b] = tot / F4(ln + len_off)
    return mx.astype(np.float64), av.astype(np.float64)


@pytest.mark.parametrize("dtype", C.DTYPES)
@pytest.mark.parametrize("n_seg,channels", [(7, 20), (17, 4), (1024, 6)])
def test_pool_honest_accepted_wrong_rejected(dtype, n_seg, channels):
    lens = [min(n, 700) for n in C.pool_lens(n_seg, channels, dtype)]      # the row loop above is plain Python: cap the long one
    split = C.pool_split(n_seg)
    assert {0, 1, split + 1} <= set(lens)
    ss = np.concatenate([[0], np.cumsum(lens)])
    for family in ("exact", "normal"):
        feats = C.pool_feats(family, dtype, int(ss[-1]), channels)
        mx, mean, bound = R.segment_pool(feats, ss)
        got_mx, got_av = emulate_pool(feats, ss, split)
        assert R.accept(got_mx, mx, 0.0, "fp32").all() and R.accept(got_av, mean, bound, "fp32").all()
        if family == "exact":
            sums = R.segment_sums(feats, ss)
            assert np.array_equal(sums.astype(F4).astype(np.float64), sums)
            with np.errstate(invalid="ignore", divide="ignore"):
                want = (sums / np.array(lens)[:, None]).astype(F4).astype(np.float64)
            assert R.accept(got_av, want, R.ulp32(want), "fp32").all()
        for kw in (dict(len_off=1), dict(len_off=-1), dict(drop_last=True)):
            bad_mx, bad_av = emulate_pool(feats, ss, split, **kw)
            assert not R.accept(bad_av, mean, bound, "fp32").all(), kw
        bad_mx, _ = emulate_pool(feats, ss, split, drop_last=True)
        assert not R.accept(bad_mx, mx, 0.0, "fp32").all()


# ---- (3) IoU ------------------------------------------------------------------------------------------------------------

def test_iou_cases_hold_their_edges_and_wrong_variants_differ():
    c = C.iou_case(37, 64)
    idx, off, labels, pn, sc = c["idx"], c["off"], c["labels"], c["pointnum"], c["scores"]
    assert c["planted"] == 3 and (labels == -100).any() and (labels >= 37).any() and (pn > 2 ** 24).any()
    assert (np.diff(off) == 0).any() and (sc == 0.5).any() and (sc == np.nextafter(F4(0.5), F4(1))).any()
    for mode in (0, 1):
        iou = R.iou(idx, off, labels, pn, sc, mode)
        ml = R.mask_label(idx, off, labels, iou)
        # planted 0: inter = uni / 2 -> just below 0.5, rows untouched; 1: above; 2: two instances tied, the first wins
        assert iou[0].max() == iou[0, 0] < 0.5 and F4(0.5) - iou[0, 0] < 1e-6 and (ml[off[0]:off[1]] == -1).all()
        assert iou[1, 1] > 0.5 and (ml[off[1]:off[2]] == 1).all()
        assert iou[2, 2] == iou[2, 3] == iou[2].max() > 0.5
        seg = ml[off[2]:off[3]]
        assert (seg[:10] == 0).all() and (seg[10:] == 1).all()           # the points of instance 3 come first and get 0
        assert set(np.unique(ml)) == {-1.0, 0.0, 1.0}
        # last maximum wins
        rev = iou.shape[1] - 1 - np.argmax(iou[:, ::-1], 1)
        assert rev[2] == 3
    # uni not rounded through fp32
    want = R.iou(idx, off, labels, pn)
    inter_total = [R._counts(idx, off, labels, 37, None, -1, p) for p in range(64)]
    bad = np.stack([(i.astype(np.float64) / ((t + pn.astype(np.int64) - i).astype(np.float64) + 1e-5)).astype(F4) for i, t in inter_total])
    assert not np.array_equal(bad.view(np.int32), want.view(np.int32))
    assert np.array_equal(bad[:, pn <= 2 ** 24].view(np.int32), want[:, pn <= 2 ** 24].view(np.int32))
    # mode 1 with the total counting all points
    m1 = R.iou(idx, off, labels, pn, sc, 1)
    bad1 = []
    for p in range(64):
        i, _ = R._counts(idx, off, labels, 37, sc, 1, p)
        bad1.append((i.astype(F4).astype(np.float64) / ((int(off[p + 1] - off[p]) + pn.astype(np.int64) - i).astype(F4).astype(np.float64) + 1e-5)).astype(F4))
    assert not np.array_equal(np.stack(bad1).view(np.int32), m1.view(np.int32))
    assert not np.array_equal(m1.view(np.int32), R.iou(idx, off, labels, pn, sc, 0).view(np.int32))
    # a score of exactly 0.5 is excluded, the next float is not
    one = dict(idx=np.array([0, 1, 2], np.int32), off=np.array([0, 3], np.int32), labels=np.array([0, 0, 0], np.int64),
               pn=np.array([3], np.int32))
    s = np.array([0.5, np.nextafter(F4(0.5), F4(1)), 0.9], F4)
    assert R.iou(one["idx"], one["off"], one["labels"], one["pn"], s, 1)[0, 0] == F4(2.0 / (3.0 + 1e-5))
    big = C.iou_case(3, 32768 + 5)
    assert set(np.diff(big["off"])) == {1, 2}
    assert C.iou_case(20000, 5)["pointnum"].shape[0] * 4 + 4 > 64 * 1024
