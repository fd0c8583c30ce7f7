"""GPU tier: the weight and input gradients of the sparse convolutions pinned to float64 (tests/grad_exact.py).

Weight gradient through the C ABI (pbn_spconv_wgrad_checked), so that the dispatch inputs are chosen, not inherited:
  * exact mode (integer operands: every fp32 partial sum is exact) -- dW must EQUAL the float64 value, for every
    k_wgrad_ring<T, WA, WB, IDENT> of bf16 and fp16 (WA, WB in 1..4, IDENT false / true), the small_level quarter tiles,
    forced pair splits 1 / 2 / 7 / 64 (k_wgrad_reduce; the split count is read back from the workspace), offsets of
    0 / 1 / step - 1 / step + 1 / ~3000 pairs, n_pairs_total = 0, k_wgrad<T> on fp32 slabs and on 16-bit slabs that are
    misaligned or have ld % 8 != 0, strided x / g views; padded host lists and unpadded device lists whose unused tails
    hold VALID row indices (reading past a count changes dW); PBN_WGRAD_FORM=32 in a child process;
  * before every exact case the library is asked what it will launch (pbn_spconv_wgrad_plan, with the call's own arguments
    and under the call's environment): form, WA, WB, small_level and splits must equal the independent Python statement
    (tests/wgrad_plan_ref.py), so "this kernel ran" rests on the library's answer, and the partial slabs found in the
    workspace tie that answer to the launch;
  * dW is written inside a sentinel-filled buffer, nothing around it may change; every call runs twice, bit-identical;
  * bounded mode (|got - ref| <= ulp + 2^-20 S per element) at MinkUNet34C shapes and the bench pyramid's stride-1 map.
Input gradient through the module path (mod(SparseTensor).backward(gy)) for k3, k5, down, up, 1x1 + bias and linear in
bf16 / fp16 / fp32, exact mode: x.grad == RNE_T(float64), kernel.grad == float64, bias.grad == the column sums.  The
batch packer's buffers (training) equal pack_weight byte for byte for every convolution of MinkUNet34C and MinkUNet14A.
Run with -s for the per-form configuration counts and the worst bounded ratios."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import conv_exact as X
import grad_exact as G
from wgrad_plan_ref import cdiv, wgrad_plan
import pbnet_amd.MinkowskiEngine as ME
from pbnet_amd import _native as N
from pbnet_amd import synth
from pbnet_amd.MinkowskiEngine import conv as C

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT16 = (torch.bfloat16, torch.float16)
STEP = 32                                   # pairs per step of k_wgrad_ring
_RAN = {}                                   # form -> configurations run in this process
_WORST = {}                                 # bounded family -> worst err / bound
SENT32 = 0x5A5A5A5A


def library_plan(x, g, K, cin, cout, n_pairs, ident, ws_bytes):
    """pbn_spconv_wgrad_plan for the call run_exact is about to make -> (form, WA, WB, small_level, splits) in the Python
    statement's terms."""
    p = N.WgradPlan()
    rc = N.lib().pbn_spconv_wgrad_plan(C._DT[x.dtype], x.ld, g.ld, int(((x.ptr() | g.ptr()) & 15) == 0), int(ident), K, n_pairs,
                                       cin, cout, 1, ws_bytes, ctypes.byref(p))
    assert rc == 0, rc
    form = ("ring%d%d%s" % (p.wa, p.wb, "i" if ident else "")) if p.form == 1 else "w32"
    return form, p.wa, p.wb, bool(p.small_level), p.splits


def padded_lists(pairs, segment):
    """Host-style lists (pbn_rulebook_pair_fill's layout): every offset's pairs in whole segments, -1 padded."""
    ins, outs, seg_begin = [], [], [0]
    for i, o in pairs:
        n_seg = cdiv(len(i), segment)
        pad = n_seg * segment - len(i)
        ins.append(torch.cat([i.int().cpu(), torch.full((pad,), -1, dtype=torch.int32)]))
        outs.append(torch.cat([o.int().cpu(), torch.full((pad,), -1, dtype=torch.int32)]))
        seg_begin.append(seg_begin[-1] + n_seg)
    cat = lambda l: torch.cat(l).to(DEV) if sum(len(t) for t in l) else torch.zeros(1, dtype=torch.int32, device=DEV)
    counts = torch.tensor([len(i) for i, _ in pairs], dtype=torch.int32, device=DEV)
    return cat(ins), cat(outs), torch.tensor(seg_begin, dtype=torch.int32, device=DEV), counts


def poison_tails(in_idx, out_idx, seg_begin, counts, segment, n_in, n_out):
    """Unpadded lists: every entry behind an offset's count (to the end of its segments) becomes a VALID row index."""
    sb, ct = seg_begin.cpu().long(), counts.cpu().long()
    for k in range(len(ct)):
        lo, hi = int(sb[k]) * segment + int(ct[k]), int(sb[k + 1]) * segment
        if hi > lo:
            r = torch.arange(hi - lo, device=DEV, dtype=torch.int32)
            in_idx[lo:hi] = (r * 7 + k) % n_in
            out_idx[lo:hi] = (r * 5 + 3 * k) % n_out


class Slab(object):
    """A [rows, cols] operand as a view at column col0 of a slab [rows, ld_total] (the rest filled with noise, which the
    kernels must not read as operand values), optionally shifted by `shift` elements (a misaligned base)."""

    def __init__(self, vals, dtype, col0=0, extra=0, ld=None, shift=0):
        rows, cols = vals.shape
        c8 = (cols + 7) // 8 * 8
        self.ld = ld if ld is not None else col0 + c8 + extra
        self.buf = torch.randn(rows * self.ld + shift + 64, device=DEV).to(dtype)
        self.view = self.buf[shift:shift + rows * self.ld].view(rows, self.ld)[:, col0:col0 + cols]
        self.view.copy_(vals.to(DEV).to(dtype))
        if c8 > cols and col0 + c8 <= self.ld:           # the 16-byte chunk tail of a row: zero, as in the package's slabs
            self.buf[shift:shift + rows * self.ld].view(rows, self.ld)[:, col0 + cols:col0 + c8] = 0
        self.rows, self.cols, self.dtype = rows, cols, dtype

    def ptr(self):
        return self.view.data_ptr()


def call_wgrad(x, g, K, cin, cout, lists=None, counts=None, padded=0, segment=0, n_pairs=None, ws_bytes=None, margin=64):
    """One pbn_spconv_wgrad_checked call into a sentinel-filled dW buffer and a sentinel-filled workspace.
    -> (rc, dW [K, cin, cout], splits seen in the workspace, sentinel-ok)."""
    lib = N.lib()
    n_out = K * cin * cout
    buf = torch.empty(n_out + 2 * margin, dtype=torch.float32, device=DEV)
    buf.view(torch.int32).fill_(SENT32)
    dw = buf[margin:margin + n_out]
    wsb = int(lib.pbn_spconv_wgrad_workspace_bytes(K, cin, cout)) if ws_bytes is None else ws_bytes
    ws = torch.empty(max(wsb // 4, 1), dtype=torch.float32, device=DEV)
    ws.view(torch.int32).fill_(SENT32)
    in_idx = out_idx = seg = cnt = None
    if lists is not None:
        in_idx, out_idx, seg, cnt = lists
        if not (not padded if counts is None else counts):      # padded lists are walked as whole segments
            cnt = None
    if n_pairs is None:
        n_pairs = int(lists[3].sum()) if lists is not None else x.rows
    rc = lib.pbn_spconv_wgrad_checked(N.c_vp(x.ptr()), x.ld, x.rows, N.c_vp(g.ptr()), g.ld, g.rows, C._DT[x.dtype],
                                      N.ptr(in_idx), N.ptr(out_idx), N.ptr(seg), N.ptr(cnt), padded, segment, n_pairs, K, cin,
                                      cout, N.c_vp(dw.data_ptr()), N.c_vp(ws.data_ptr()), wsb, N.current_stream())
    torch.cuda.synchronize()
    bits = buf.view(torch.int32)
    sent_ok = bool((bits[:margin] == SENT32).all()) and bool((bits[margin + n_out:] == SENT32).all())
    wbits = ws.view(torch.int32)
    touched = 0
    for s in range(min(64, wsb // (4 * n_out))):
        if bool((wbits[s * n_out:(s + 1) * n_out] != SENT32).any()):
            touched = s + 1
    return rc, dw.view(K, cin, cout).clone(), max(touched, 1), sent_ok


def run_exact(x, g, pairs, K, cin, cout, label, lists=None, counts=None, padded=0, segment=0, n_pairs=None, ident=False,
              expect_splits=None, expect_form=None, ws_bytes=None):
    """Exact-mode weight gradient: twice, bit-identical, sentinels intact, == float64; counts the form it ran."""
    lib = N.lib()
    wsb = int(lib.pbn_spconv_wgrad_workspace_bytes(K, cin, cout)) if ws_bytes is None else ws_bytes
    npl = n_pairs if n_pairs is not None else (int(lists[3].sum()) if lists is not None else x.rows)
    assert ident == (lists is None)
    form, wa, wb, small, splits = library_plan(x, g, K, cin, cout, npl, ident, wsb)
    twin = wgrad_plan(x.dtype, x.ld, g.ld, x.ptr(), g.ptr(), cin, cout, npl, K, ident, wsb)
    assert (form, wa, wb, small, splits) == twin, "%s %d->%d K %d %s: the library plans %r, the Python statement %r" % (
        x.dtype, cin, cout, K, label, (form, wa, wb, small, splits), twin)
    what = "%-8s %-9s %3d->%-3d K %-3d splits %2d%s %s" % (str(x.dtype).replace("torch.", ""), form, cin, cout, K, splits,
                                                           " small" if small else "", label)
    if expect_form is not None:
        assert form == expect_form, "%s: plan says %s" % (what, form)
    ref, S = G.wgrad_reference(x.view, g.view, pairs=pairs) if pairs is not None else \
        G.wgrad_reference(x.view, g.view, n_pairs=npl)
    G.assert_grad_exact_premise(torch.float32, ref, S, 1.0)
    outs = []
    for _ in range(2):
        rc, dw, seen, sent_ok = call_wgrad(x, g, K, cin, cout, lists, counts, padded, segment, n_pairs, ws_bytes)
        assert rc == 0, "%s: rc %d" % (what, rc)
        assert sent_ok, "%s: dW written outside [K, cin, cout]" % what
        outs.append(dw)
    assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32)), "%s: not deterministic" % what
    if npl > 0 and splits > 1:
        assert seen == splits, "%s: %d partial slabs written, the plan says %d" % (what, seen, splits)
    if expect_splits is not None:
        assert splits == expect_splits, "%s: plan gives %d splits" % (what, splits)
    G.check_wgrad_exact(outs[0], ref, what)
    print("%s: exact" % what)
    for key in (form, "small" if small else None, "split" if splits > 1 else None):
        if key:
            _RAN[key] = _RAN.get(key, 0) + 1
    return outs[0]


def rand_pairs(gen, sizes, n_in, n_out):
    return [(torch.randint(0, n_in, (s,), generator=gen), torch.randint(0, n_out, (s,), generator=gen)) for s in sizes]


def operands(gen, n_in, n_out, cin, cout, dtype, **kw):
    x = Slab(G.exact_ints(gen, n_in, cin), dtype, **kw.get("x", {}))
    g = Slab(G.exact_ints(gen, n_out, cout), dtype, **kw.get("g", {}))
    return x, g


# (cin, cout) per WA / WB: cdiv(c, 16) 1-2 -> 1, 3-4 -> 2, 5-6 -> 3, >= 7 -> 4; channel tails on both sides
CH = {1: 20, 2: 56, 3: 90, 4: 120}
CH_OUT = {1: 32, 2: 50, 3: 96, 4: 136}


@pytest.mark.parametrize("dtype", DT16)
def test_wgrad_ring_every_tile_shape(dtype):
    """All 16 (WA, WB) of launch_ring, with pair lists (IDENT false) and identity pairs (IDENT true): 32 kernels."""
    gen = torch.Generator().manual_seed(1)
    seen = set()
    for wa in (1, 2, 3, 4):
        for wb in (1, 2, 3, 4):
            cin, cout = CH[wa], CH_OUT[wb]
            n_in, n_out = 3500, 3300
            x, g = operands(gen, n_in, n_out, cin, cout, dtype)
            pairs = rand_pairs(gen, (3100, 3400, 3031, 3200), n_in, n_out)       # >= 3000 per offset: not small_level
            lists = padded_lists(pairs, 4096)
            run_exact(x, g, pairs, 4, cin, cout, "lists", lists=lists, padded=1, segment=4096,
                      expect_form="ring%d%d" % (wa, wb))
            xi, gi = operands(gen, 3200, 3200, cin, cout, dtype)
            run_exact(xi, gi, None, 1, cin, cout, "identity", ident=True, expect_form="ring%d%di" % (wa, wb))
            seen |= {"ring%d%d" % (wa, wb), "ring%d%di" % (wa, wb)}
    assert len(seen) == 32


@pytest.mark.parametrize("dtype", DT16)
def test_wgrad_small_level_and_forced_splits(dtype, monkeypatch):
    gen = torch.Generator().manual_seed(2)
    # quarter tiles: few pairs per offset, few tiles
    for cin, cout in ((64, 64), (128, 96), (256, 256), (40, 24)):
        x, g = operands(gen, 900, 800, cin, cout, dtype)
        pairs = rand_pairs(gen, [int(v) for v in torch.randint(0, 1500, (27,), generator=gen)], 900, 800)
        lists = padded_lists(pairs, 4096)
        wsb = int(N.lib().pbn_spconv_wgrad_workspace_bytes(27, cin, cout))
        assert wgrad_plan(dtype, x.ld, g.ld, x.ptr(), g.ptr(), cin, cout, int(lists[3].sum()), 27, False, wsb)[3], (cin, cout)
        run_exact(x, g, pairs, 27, cin, cout, "small_level", lists=lists, padded=1, segment=4096)
    # forced splits (the knobs are read per call): s - 1 workgroups per strip and offset, or one split by a pair floor
    monkeypatch.delenv("PBN_WGRAD_DBG", raising=False)
    cin, cout, K = 64, 48, 5
    x, g = operands(gen, 4000, 3900, cin, cout, dtype)
    pairs = rand_pairs(gen, (0, 1, STEP - 1, STEP + 1, 3000), 4000, 3900)
    lists = padded_lists(pairs, 4096)
    strips = cdiv(cdiv(cin, 16), 2 * 2) * cdiv(cdiv(cout, 16), 2 * 2)

    def force(s, per):
        if s == 1:
            monkeypatch.delenv("PBN_WGRAD_WGS", raising=False)
            monkeypatch.setenv("PBN_WGRAD_MIN_PAIRS", str(1 << 30))
        else:
            monkeypatch.setenv("PBN_WGRAD_MIN_PAIRS", "1")
            monkeypatch.setenv("PBN_WGRAD_WGS", str((s - 1) * per))

    for s in (1, 2, 7, 64):
        force(s, strips * K)
        run_exact(x, g, pairs, K, cin, cout, "forced split", lists=lists, padded=1, segment=4096, expect_splits=s)
        xi, gi = operands(gen, 3000, 3000, cin, cout, dtype)
        force(s, strips)
        run_exact(xi, gi, None, 1, cin, cout, "forced split identity", ident=True, expect_splits=s)
    assert _RAN.get("split", 0) >= 6 and _RAN.get("small", 0) >= 4


@pytest.mark.parametrize("dtype", (torch.bfloat16, torch.float16, torch.float32))
def test_wgrad_pair_counts_and_list_formats(dtype):
    """Offsets of 0 / 1 / step - 1 / step + 1 / 63 / 65 / ~3000 pairs, segment sizes that are not multiples of the step;
    padded host lists (walked as whole segments) and unpadded lists (walked by their counts) with VALID indices behind
    every count; n_pairs_total = 0."""
    gen = torch.Generator().manual_seed(3)
    cin, cout = 48, 40
    n_in, n_out = 3300, 3100
    x, g = operands(gen, n_in, n_out, cin, cout, dtype)
    sizes = (0, 1, STEP - 1, STEP + 1, 63, 65, 2999, 0, 517)
    pairs = rand_pairs(gen, sizes, n_in, n_out)
    K = len(sizes)
    for seg in (4096, 100, 33):
        run_exact(x, g, pairs, K, cin, cout, "padded seg %d" % seg, lists=padded_lists(pairs, seg), padded=1, segment=seg)
        in_idx, out_idx, sb, cnt = padded_lists(pairs, seg)
        poison_tails(in_idx, out_idx, sb, cnt, seg, n_in, n_out)
        run_exact(x, g, pairs, K, cin, cout, "unpadded seg %d" % seg, lists=(in_idx, out_idx, sb, cnt), segment=seg)
        # the poisoned tails are visible to a walk that ignores the counts: the test would see an over-read
        rc, dw, _, _ = call_wgrad(x, g, K, cin, cout, (in_idx, out_idx, sb, cnt), counts=False, padded=1, segment=seg,
                                  n_pairs=int(cnt.sum()))
        assert rc == 0
        assert not torch.equal(dw.double(), G.wgrad_reference(x.view, g.view, pairs=pairs)[0]), "poisoned tails invisible"
    # n_pairs_total == 0: dW is zero, nothing else written
    rc, dw, _, ok = call_wgrad(x, g, K, cin, cout, padded_lists(pairs, 4096), padded=1, segment=4096, n_pairs=0)
    assert rc == 0 and ok and float(dw.abs().max()) == 0.0 and not bool(torch.signbit(dw).any())


def test_wgrad_device_lists_of_real_maps():
    """rulebook_pairs (padded) and rulebook_pairs_dev / _multi (unpadded, tails poisoned) of a scene's maps, bf16 / fp16;
    n_pairs_total as wgrad_native passes it (an estimate)."""
    sc = synth.synth_room(seed=61, pitch=0.0225, room=(0.8, 0.6, 0.5), n_boxes=1)
    q, _, _ = synth.voxelize_numpy(sc["xyz"], 0.02)
    coords = np.concatenate([np.zeros((len(q), 1), np.int32), q], 1).astype(np.int32)
    cm = ME.CoordinateManager(torch.from_numpy(coords).to(DEV))
    gen = torch.Generator().manual_seed(4)
    maps = {"k3": (cm.kernel_map(1, 3), cm.num_rows(1), cm.num_rows(1)), "down": (cm.down_map(1), cm.num_rows(1), cm.num_rows(2)),
            "up": (cm.up_map(2), cm.num_rows(2), cm.num_rows(1)), "k5": (cm.kernel_map(1, 5), cm.num_rows(1), cm.num_rows(1))}
    multi = C.rulebook_pairs_dev_multi([m[0] for m in maps.values()])
    for dtype in DT16:
        for (name, (nbr, n_in, n_out)), dev_lists in zip(maps.items(), multi):
            K = nbr.shape[1]
            cin, cout = (6, 32) if name == "k5" else (64, 96)
            x, g = operands(gen, n_in, n_out, cin, cout, dtype)
            pairs = G.pairs_of(nbr, n_in)
            est = max(C.WGRAD_PAIR_SEGMENT, (int(nbr.shape[0]) * K) // (2 if K >= 27 else 4))
            hit = C.rulebook_pairs(nbr)
            lists_h = (hit[0], hit[1], nbr._pbn_pairs[5], nbr._pbn_pairs[6])
            run_exact(x, g, pairs, K, cin, cout, name + " host lists", lists=lists_h, counts=False, padded=1,
                      segment=C.WGRAD_PAIR_SEGMENT, n_pairs=est)
            for label, lst in (("dev", C.rulebook_pairs_dev(nbr)), ("multi", dev_lists)):
                a, b, sb, cnt = [t.clone() for t in lst]
                poison_tails(a, b, sb, cnt, C.WGRAD_PAIR_SEGMENT, n_in, n_out)
                run_exact(x, g, pairs, K, cin, cout, name + " " + label + " lists", lists=(a, b, sb, cnt),
                          segment=C.WGRAD_PAIR_SEGMENT, n_pairs=est)


def test_wgrad_f32_form_and_unaligned_16bit_slabs():
    """k_wgrad<T>: fp32 slabs, and 16-bit slabs reached through a base offset by one element and through ld % 8 != 0;
    strided x / g views (a skip slab's columns) on every form."""
    gen = torch.Generator().manual_seed(5)
    n_in, n_out = 2500, 2600
    for cin, cout in ((32, 64), (20, 36), (96, 130), (6, 32)):
        pairs = rand_pairs(gen, (1200, 0, 33, 2100, 64), n_in, n_out)
        lists = padded_lists(pairs, 4096)
        ga = torch.Generator().manual_seed(cin * cout)
        for dtype, kw, want in ((torch.float32, {}, "w32"),
                                (torch.float32, dict(x=dict(col0=4, extra=12), g=dict(col0=8, extra=4)), "w32"),
                                (torch.bfloat16, dict(x=dict(shift=1)), "w32"),
                                (torch.float16, dict(g=dict(shift=1)), "w32"),
                                (torch.bfloat16, dict(x=dict(ld=(cin + 7) // 8 * 8 + 4)), "w32"),
                                (torch.float16, dict(g=dict(ld=(cout + 7) // 8 * 8 + 2)), "w32"),
                                (torch.bfloat16, dict(x=dict(col0=8, extra=24), g=dict(col0=16, extra=8)), None),
                                (torch.float16, dict(x=dict(col0=32, extra=8), g=dict(col0=8, extra=16)), None)):
            x, g = operands(ga, n_in, n_out, cin, cout, dtype, **kw)
            exp = want if want else wgrad_plan(dtype, x.ld, g.ld, x.ptr(), g.ptr(), cin, cout, 3397, 5, False, 1 << 30)[0]
            run_exact(x, g, pairs, 5, cin, cout, "views %s" % sorted(kw), lists=lists, padded=1, segment=4096, expect_form=exp)
            xi, gi = operands(ga, 1800, 1800, cin, cout, dtype, **kw)
            run_exact(xi, gi, None, 1, cin, cout, "identity views %s" % sorted(kw), ident=True)
    assert _RAN.get("w32", 0) >= 4 * 6 * 2


_FORM_CODE = """
import sys, torch
sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
import test_grad_parity_gpu as T
T.form_cases({form!r})
print("FORM_RUNS", T._RAN)
"""


def form_cases(form):
    """Exact cases for a child process started with PBN_WGRAD_FORM set (static per process)."""
    gen = torch.Generator().manual_seed(6)
    ran = 0
    for dtype in DT16:
        for cin, cout in ((20, 32), (64, 50), (90, 96), (128, 136), (256, 256)):
            x, g = operands(gen, 3000, 2900, cin, cout, dtype)
            pairs = rand_pairs(gen, (0, 1, 33, 3100, 700), 3000, 2900)
            run_exact(x, g, pairs, 5, cin, cout, "FORM=%s" % form, lists=padded_lists(pairs, 4096), padded=1, segment=4096,
                      expect_form="w32")
            xi, gi = operands(gen, 2000, 2000, cin, cout, dtype)
            run_exact(xi, gi, None, 1, cin, cout, "FORM=%s identity" % form, ident=True, expect_form="w32")
            ran += 2
    assert ran == 20


@pytest.mark.parametrize("form", ["32"])
def test_wgrad_static_forms_in_a_child(form):
    code = _FORM_CODE.format(root=ROOT, tests=os.path.join(ROOT, "tests"), form=form)
    env = dict(os.environ, PBN_WGRAD_FORM=form)
    env.pop("PBN_WGRAD_DBG", None)
    p = subprocess.run([sys.executable, "-c", code], env=env, timeout=200, capture_output=True, text=True)
    print(p.stdout[-2000:])
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    assert "FORM_RUNS" in p.stdout


# ---- bounded mode at MinkUNet34C shapes --------------------------------------------------------------------------------

def _bounded(name, nbr, n_in, n_out, cin, cout, dtype, seed):
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(n_in, cin, generator=gen).to(dtype).to(DEV)
    g = torch.randn(n_out, cout, generator=gen).to(dtype).to(DEV)
    got = C.wgrad_native(x, g, nbr, cin, cout)
    again = C.wgrad_native(x, g, nbr, cin, cout)
    assert torch.equal(got.view(torch.int32), again.view(torch.int32)), name
    ref, S = G.wgrad_reference(x, g, nbr=nbr) if nbr is not None else G.wgrad_reference(x, g)
    worst = G.check_wgrad_bounded(got, ref, S, "%s %s" % (name, dtype))
    _WORST[name] = max(_WORST.get(name, 0.0), worst)
    print("bounded %-12s %-8s %3d->%-3d: worst err/bound %.3f" % (name, str(dtype).replace("torch.", ""), cin, cout, worst))


def test_wgrad_bounded_minkunet_shapes():
    sc = synth.synth_room(seed=62, pitch=0.0225, room=(1.6, 1.2, 0.8), n_boxes=2)
    q, _, _ = synth.voxelize_numpy(sc["xyz"], 0.02)
    coords = np.concatenate([np.zeros((len(q), 1), np.int32), q], 1).astype(np.int32)
    cm = ME.CoordinateManager(torch.from_numpy(coords).to(DEV))
    for dtype in DT16 + (torch.float32,):
        _bounded("k5 stem", cm.kernel_map(1, 5), cm.num_rows(1), cm.num_rows(1), 6, 32, dtype, 1)
        for lvl, c in ((1, 32), (2, 64), (4, 128), (8, 256)):
            _bounded("k3", cm.kernel_map(lvl, 3), cm.num_rows(lvl), cm.num_rows(lvl), c, c, dtype, lvl)
        _bounded("down", cm.down_map(1), cm.num_rows(1), cm.num_rows(2), 32, 32, dtype, 3)
        _bounded("up", cm.up_map(4), cm.num_rows(4), cm.num_rows(2), 128, 96, dtype, 4)
        _bounded("1x1", None, cm.num_rows(1), cm.num_rows(1), 96, 20, dtype, 5)


def test_wgrad_bounded_bench_stride1():
    """The bench scene's stride-1 map (146 038 rows) at 96 channels, bf16 (configs[2]'s dtype) and fp16."""
    b, _, _ = synth.make_val_batch(seed=2, copies=1)
    cm = ME.CoordinateManager(torch.from_numpy(b["xyz_voxel"].astype(np.int32)).to(DEV))
    nbr = cm.kernel_map(1, 3)
    n = cm.num_rows(1)
    for dtype in DT16:
        _bounded("bench k3", nbr, n, n, 96, 96, dtype, 7)


# ---- input gradient through the module path, and the batch packer -------------------------------------------------------

def _coords(seed=51):
    sc = synth.synth_room(seed=seed, pitch=0.0225, room=(0.7, 0.6, 0.4), n_boxes=1)
    q, _, _ = synth.voxelize_numpy(sc["xyz"], 0.02)
    parts = [np.concatenate([np.full((len(q), 1), b, np.int32), q + np.array([7 * b, 0, 0], np.int32)], 1) for b in range(2)]
    return np.concatenate(parts, 0).astype(np.int32)


@pytest.mark.parametrize("dtype", (torch.bfloat16, torch.float16, torch.float32))
def test_input_gradient_exact_module_path(dtype):
    coords = _coords()
    cm = ME.CoordinateManager(torch.from_numpy(coords).to(DEV))
    gen = torch.Generator().manual_seed(8)
    ran = 0
    for kind in ("k3", "k5", "down", "up", "1x1", "linear"):
        cin, cout = (6, 32) if kind == "k5" else (40, 56)
        n1, n2 = cm.num_rows(1), cm.num_rows(2)
        if kind in ("k3", "k5", "1x1"):
            k = {"k3": 3, "k5": 5, "1x1": 1}[kind]
            mod = ME.MinkowskiConvolution(cin, cout, kernel_size=k, bias=(kind == "1x1"), dimension=3)
            n_in, n_out, stride = n1, n1, 1
            nbr = None if k == 1 else cm.kernel_map(1, k)
        elif kind == "down":
            mod = ME.MinkowskiConvolution(cin, cout, kernel_size=2, stride=2, dimension=3)
            n_in, n_out, stride, nbr = n1, n2, 1, cm.down_map(1)
        elif kind == "up":
            mod = ME.MinkowskiConvolutionTranspose(cin, cout, kernel_size=2, stride=2, dimension=3)
            n_in, n_out, stride, nbr = n2, n1, 2, cm.up_map(2)
        else:
            mod = ME.MinkowskiLinear(cin, cout, bias=True)
            n_in, n_out, stride, nbr = n1, n1, 1, None
        mod = mod.to(DEV)
        wparam = mod.linear.weight if kind == "linear" else mod.kernel
        kshape = (1, cin, cout) if kind in ("1x1", "linear") else tuple(wparam.shape)
        w3, unit = G.exact_weight(gen, kshape, dtype, lo=-1)
        with torch.no_grad():
            wparam.copy_((w3[0].t() if kind == "linear" else (w3[0] if kind == "1x1" else w3)).to(DEV))
            bias = mod.linear.bias if kind == "linear" else mod.bias
            if bias is not None:
                bias.copy_(G.exact_ints(gen, *bias.shape).to(DEV) * unit)
        x0 = G.exact_ints(gen, n_in, cin)
        gy = G.exact_ints(gen, n_out, cout, lo=-1)
        xd = x0.to(DEV).to(dtype).requires_grad_(True)
        yd = mod(ME.SparseTensor(xd, coordinate_manager=cm, tensor_stride=stride)).F
        yd.backward(gy.to(DEV).to(dtype))
        ref, S = G.dgrad_reference(gy.to(DEV), w3.to(DEV), nbr, n_in)
        G.assert_grad_exact_premise(dtype, ref, S, unit)
        what = "%s %s dgrad" % (kind, dtype)
        X.check_exact(xd.grad, ref, dtype, what)
        want_w, Sw = G.wgrad_reference(x0.to(DEV), gy.to(DEV), nbr=nbr) if nbr is not None else G.wgrad_reference(x0.to(DEV), gy.to(DEV))
        got_w = wparam.grad.t()[None] if kind == "linear" else (wparam.grad[None] if kind == "1x1" else wparam.grad)
        G.check_wgrad_exact(got_w.contiguous(), want_w, "%s %s wgrad" % (kind, dtype))
        if bias is not None:
            assert torch.equal(bias.grad.reshape(-1).double(), G.bias_grad_reference(gy.to(DEV))), "%s bias gradient" % what
        print("%s: x.grad, kernel.grad%s exact" % (what, ", bias.grad" if bias is not None else ""))
        ran += 1
        _RAN["dgrad " + kind] = _RAN.get("dgrad " + kind, 0) + 1
    assert ran == 6


@pytest.mark.parametrize("arch", ["MinkUNet34C", "MinkUNet14A"])
def test_batch_packer_equals_pack_weight(arch):
    from pbnet_amd.network.Mink import Mink_unet
    torch.manual_seed(9)
    net = Mink_unet(6, 32, arch=arch).to(DEV)
    convs = [m for m in net.modules() if isinstance(m, C.MinkowskiConvolutionBase)]
    assert len(convs) >= 20
    checked = 0
    for dtype in (torch.bfloat16, torch.float16, torch.float32):
        for m in convs:
            with torch.no_grad():
                m.kernel.add_(0.0)          # a new parameter version: every layer's packed forms are stale
        C._BATCH.refresh(torch.device(DEV), dtype, True)
        torch.cuda.synchronize()
        for m in convs:
            k3 = m.kernel if m.kernel.dim() == 3 else m.kernel.unsqueeze(0)
            for form, flip, tr in (("f", False, False), ("d", bool(m._dgrad_flip), True)):
                hit = m._cache.store.get((form, dtype))
                assert hit is not None and hit[0][1] == m.kernel._version, "%s: form %s not packed by the batch" % (m, form)
                got = hit[1][0]
                want = C.pack_weight(k3.detach(), dtype, flip=flip, transpose=tr)
                host = C.pack_weight(k3.detach().cpu(), dtype, flip=flip, transpose=tr)
                assert hit[1][1:] == want[1:] == host[1:], (m, form)
                it = torch.int32 if dtype == torch.float32 else torch.int16
                assert torch.equal(got.view(it), want[0].view(it)), "%s form %s: batch packer != pack_weight" % (m, form)
                assert torch.equal(want[0].cpu().reshape(-1).view(it), host[0].reshape(-1).view(it)), \
                    "%s form %s: pbn_pack_weight != torch" % (m, form)
                checked += 1
    print("%s: %d packed buffers equal pack_weight (device and torch statement)" % (arch, checked))
    assert checked == 3 * 2 * len(convs)


def test_zz_report():
    """(report) configurations per kernel form and the worst bounded ratios in this process."""
    print("wgrad configurations per form: %s" % dict(sorted(_RAN.items())))
    print("worst bounded err / bound per family: %s" % {k: round(v, 3) for k, v in sorted(_WORST.items())})
    assert all(v <= 1.0 for v in _WORST.values())
