"""GPU tier of the native losses (csrc/losses.hip through pbnet_amd/losses.py): the seven terms against oracle/loss_ref.py,
the gradients against autograd through the float64 twin (tests/loss_grad_ref.py) on the CPU, the drop-in for model_losses,
run-to-run bits, labels outside the classes, and one model_fn step with cfg.native_losses against the torch path.

Sizes: one row; a wave -+ 1 (63, 65); 259 = a workgroup + 3 (with the mask rows at an address that leaves an unaligned head and
tail); 5000 (test_losses.py's, logits with a leading dimension of 24); 70 001 = 274 workgroups, the last one partial.  K = 13:
rows that are no multiple of 16 bytes (scalar loads, the KMAX = 16 instantiation); K = 20: KMAX = 32."""
import functools

import numpy as np
import pytest
import torch

import loss_grad_ref as G
from oracle import loss_ref
from pbnet_amd import pbnet_ops
from pbnet_amd.config import get_config
from pbnet_amd.losses import LossTerms, model_losses_native
from pbnet_amd.network.PBNet import get_segmented_scores, model_losses

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
CFG = get_config(cluster_epoch=0, native_losses=True)
TOL = 1e-5                                                  # the project's bound for the loss arithmetic (tests/test_losses.py)
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
# One unit in the last place: relative to the value, and never less than the spacing of the format's subnormals.  float16
# needs the second figure: its smallest normal number is 6.1e-5, and d loss / d logit is (softmax - 1) / n_keep, a few 1e-6 at
# 5000 rows (d loss / d offset at 70 001 rows likewise), so those gradients are subnormal and one unit in their last place is
# 2^-24 whatever their size.  bfloat16 has float32's exponent range: no gradient here comes near its subnormals.
ULP = {"bf16": (2.0 ** -8, 0.0), "fp16": (2.0 ** -11, 2.0 ** -24)}
#        N    K    R    P  unaligned mask rows / padded logit rows
SHAPES = [(1, 20, 0, 0, False), (63, 20, 1, 1, False), (65, 13, 3000, 9, False), (259, 20, 3000, 9, True),
          (5000, 20, 3000, 9, True), (70001, 13, 1, 9, False)]
IDS = ["n%d-k%d-r%d-p%d" % s[:4] for s in SHAPES]


@functools.lru_cache(maxsize=None)
def reference(shape, dtype):
    """The case with its predictions rounded to `dtype` (widened back to float32: what the oracle and the twin are fed),
    the oracle's terms and the twin's float64 gradients at grad_loss = 1.  Shared and never written."""
    n, k, r, p, _ = shape
    c = G.case(n + k, n=n, rows=r, n_prop=p, k=k)
    for key in ("sem_score", "offset", "pred_mask", "clt"):
        c[key] = torch.from_numpy(c[key]).to(DTYPES[dtype]).float().numpy()
    want = G.oracle_terms(c, CFG.fg_thresh, CFG.bg_thresh)
    _, grads = G.twin(c, CFG.fg_thresh, CFG.bg_thresh)
    for a in list(c.values()) + [g for g in grads.values() if g is not None]:
        a.setflags(write=False)
    return c, want, grads


def device_inputs(c, dtype, odd=False):
    """Fresh device tensors of a case; odd: pred_mask / gt_mask start one element into their allocation and the logits sit in
    rows of K + 4."""
    t = lambda a: torch.from_numpy(np.array(a)).to(DEV)
    dt = DTYPES[dtype]
    sem = t(c["sem_score"]).to(dt)
    mask, gt = t(c["pred_mask"]).to(dt), t(c["gt_mask"])
    if odd:
        wide = torch.zeros(sem.shape[0], sem.shape[1] + 4, dtype=dt, device=DEV)
        wide[:, :sem.shape[1]] = sem
        sem = wide[:, :sem.shape[1]]
        mask = torch.cat([mask[:1], mask])[1:]
        gt = torch.cat([gt[:1], gt])[1:]
        assert not sem.is_contiguous() and mask.data_ptr() % 8 and gt.data_ptr() % 16
    d = dict(sem=sem.detach().requires_grad_(), off=t(c["offset"]).to(dt).requires_grad_(),
             mask=mask.detach().requires_grad_(), clt=t(c["clt"]).to(dt).requires_grad_(), gt=gt,
             sem_label=t(c["sem"]), ins=t(c["ins"]), info=t(c["info"]), xyz=t(c["xyz"]), pointnum=t(c["pointnum"]))
    d["iou"] = pbnet_ops.get_iou_device(t(c["pidx"]), t(c["off"]), d["ins"], d["pointnum"])
    return d


def run(d, grad_loss=1.0):
    terms, counts, gt_scores = LossTerms.apply(d["sem"], d["off"], d["mask"].view(-1, 1), d["clt"], d["sem_label"], d["ins"],
                                               d["info"], d["xyz"], d["gt"], d["iou"], CFG.fg_thresh, CFG.bg_thresh)
    for x in (d["sem"], d["off"], d["mask"], d["clt"]):
        x.grad = None
    (terms[6] * grad_loss).backward()
    grads = {"sem_score": d["sem"].grad, "offset": d["off"].grad, "pred_mask": d["mask"].grad, "clt": d["clt"].grad}
    return terms, counts, gt_scores, grads


def expected_terms(c, want, k):
    """The oracle's terms; a mean over nothing is NaN (torch's 0 / 0, which model_losses gives today), and so is the sum."""
    keep = (c["sem"] >= 0) & (c["sem"] < k)
    out = {name: want[name] for name in G.TERMS}
    if not keep.any():
        out["semantic_loss"] = float("nan")
    if len(c["pred_mask"]) == 0:
        out["mask_loss"] = float("nan")
    if len(c["clt"]) == 0:
        out["score_loss"] = float("nan")
    if any(np.isnan(out[name]) for name in G.TERMS[:6]):
        out["loss"] = float("nan")
    return out


def check_terms(terms, want):
    got = dict(zip(G.TERMS, terms.tolist()))
    for name in G.TERMS:
        print("%s: %.9g vs %.9g" % (name, got[name], want[name]))
        if np.isnan(want[name]):
            assert np.isnan(got[name]), name
        else:
            assert abs(got[name] - want[name]) <= TOL * max(1.0, abs(want[name])), name


def guarded_rows(c):
    """Rows whose gradient one of the guards makes ~1e8 times an ordinary one: offset predictions of norm zero (-g^ / 1e-8)
    and mask scores with p (1 - p) under BCELoss's 1e-12 -- the planted 0, 1 and 1e-30, and whatever score a 16-bit format
    rounds to exactly 0 or 1."""
    p = c["pred_mask"].astype(np.float64)
    return {"offset": ~c["offset"].any(1), "pred_mask": p * (1 - p) < 1e-12}


def check_grads(grads, want, dtype, c, scale=1.0):
    """Every bound is applied twice where there are guarded rows: to the whole tensor as the bound is stated (its norm or
    its max |want| is then the guarded rows'), and to the ordinary rows with the norm / max |want| of the ordinary rows, so
    that a wrong ordinary row cannot hide below a floor that a guarded row set."""
    guarded = guarded_rows(c)
    for name, w in want.items():
        if w is None:                                      # an empty leaf (R = 0, P = 0)
            assert grads[name] is None or grads[name].numel() == 0
            continue
        w = w * scale
        g = grads[name]
        assert g.dtype == DTYPES[dtype] and tuple(g.shape) == w.shape, name
        g = g.double().cpu().numpy()
        ordinary = ~guarded[name] if name in guarded else np.ones(len(w), bool)
        for what, rows in (("all rows", np.ones(len(w), bool)), ("ordinary rows", ordinary)):
            gr, wr = g[rows], w[rows]
            if what == "ordinary rows" and rows.all():
                continue
            if not wr.any():                               # nothing to be relative to: exact zeros
                assert not gr.any(), (name, what)
                continue
            if dtype == "fp32":
                rel = np.linalg.norm(gr - wr) / np.linalg.norm(wr)
                print("%s, %s (%d): |got - want| / |want| = %.3g" % (name, what, rows.sum(), rel))
                assert rel < 1e-5, (name, what)
            else:
                rel_ulp, tiny = ULP[dtype]
                big = float(torch.finfo(DTYPES[dtype]).max)
                over = np.abs(wr) * (1 - rel_ulp) > big    # rounds to infinity in this format (guarded rows only)
                assert what == "all rows" or not over.any(), name
                assert np.array_equal(gr[over], np.sign(wr[over]) * np.inf), (name, what)
                tol = np.maximum(np.maximum(rel_ulp * np.abs(wr), tiny), 1e-6 * np.abs(wr).max())
                err = np.abs(gr - wr)[~over]
                print("%s, %s (%d): worst error / tolerance = %.3g, max |want| %.3g, median |want| %.3g (%d round to infinity)"
                      % (name, what, rows.sum(), (err / tol[~over]).max(initial=0), np.abs(wr).max(), np.median(np.abs(wr)),
                         int(over.sum())))
                assert (err <= tol[~over]).all(), (name, what)


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_values_and_gradients(shape, dtype):
    c, want, want_grads = reference(shape, dtype)
    n, k, r, p, odd = shape
    d = device_inputs(c, dtype, odd)
    terms, counts, gt_scores, grads = run(d)
    check_terms(terms, expected_terms(c, want, k))
    assert counts.tolist() == [int((c["ins"] != -100).sum()), int((c["gt_mask"] != -1).sum()), int((c["sem"] != -100).sum()), 0]
    assert torch.equal(gt_scores, get_segmented_scores(d["iou"].max(1)[0], CFG.fg_thresh, CFG.bg_thresh) if p else gt_scores[:0])
    if p:
        # and to the oracle's ramp on the same table (its own numpy IoUs round once more than pbn_get_iou's, which
        # tests/test_cluster_gpu.py pins to oracle/pb_cluster_ref.c: they differ in the last bit, and the ramp carries it)
        ramp = loss_ref.segmented_scores(d["iou"].max(1)[0].cpu().numpy(), CFG.fg_thresh, CFG.bg_thresh)
        assert np.array_equal(gt_scores.cpu().numpy().view(np.int32), ramp.view(np.int32))
    assert np.array_equal(d["gt"].cpu().numpy(), want["gt_mask"])
    check_grads(grads, want_grads, dtype, c)
    # the device scalar grad_loss: half the loss, half of every gradient (exactly, in the float64 reference)
    d = device_inputs(c, dtype, odd)
    terms2, _, _, grads = run(d, grad_loss=0.5)
    assert torch.equal(terms2.view(torch.int32), terms.view(torch.int32))
    check_grads(grads, want_grads, dtype, c, scale=0.5)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_two_calls_give_the_same_bits(dtype):
    c, _, _ = reference(SHAPES[5], dtype)
    bits = lambda x: x.contiguous().view(torch.int32 if x.element_size() == 4 else torch.int16)
    a = run(device_inputs(c, dtype))
    b = run(device_inputs(c, dtype))
    assert torch.equal(bits(a[0]), bits(b[0])) and torch.equal(a[1], b[1])
    for name in a[3]:
        assert torch.equal(bits(a[3][name]), bits(b[3][name])), name
    c, _, _ = reference(SHAPES[4], dtype)
    a, b = run(device_inputs(c, dtype, True)), run(device_inputs(c, dtype, True))
    assert torch.equal(bits(a[0]), bits(b[0])) and all(torch.equal(bits(a[3][k]), bits(b[3][k])) for k in a[3])


def _ret(d, c):
    pidx = torch.from_numpy(np.array(c["pidx"])).to(DEV)
    return {"sem_pred_score_p": d["sem"], "offset_pred_p": d["off"], "mask_scores": (d["mask"].view(-1, 1), d["gt"]),
            "clt_scores": d["clt"],
            "proposals": (torch.stack([torch.zeros_like(pidx), pidx], 1), torch.from_numpy(np.array(c["off"])).to(DEV), None, None)}


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("shape", [SHAPES[4], SHAPES[0], SHAPES[1]], ids=[IDS[4], IDS[0], IDS[1]])
@pytest.mark.parametrize("no_label", [False, True], ids=["labels", "all-ignored"])
def test_drop_in_for_model_losses(shape, dtype, no_label):
    """The same device tensors through model_losses and model_losses_native: same keys, same terms (NaN where a mean is
    empty: no class label at all, R = 0, P = 0), the caller's gt_mask object rewritten in place."""
    c, _, _ = reference(shape, dtype)
    out = []
    for fn in (model_losses, model_losses_native):
        d = device_inputs(c, dtype)
        if no_label:
            d["sem_label"].fill_(-100)
        res = fn(_ret(d, c), d["sem_label"], d["ins"], d["info"], d["pointnum"], d["xyz"], 1, CFG)
        assert res[4] is d["gt"] and int((d["gt"] == -1).sum()) == 0
        out.append((res, d))
    (want, dw), (got, dg) = out
    assert list(got[1]) == list(want[1]) and got[0] is got[1]["loss"]
    for name in want[1]:
        w, g = float(want[1][name]), float(got[1][name])
        print("%s: %.9g vs %.9g" % (name, g, w))
        assert (np.isnan(w) and np.isnan(g)) or abs(g - w) <= TOL * max(1.0, abs(w)), name
    if no_label or shape[2] == 0 or shape[3] == 0:
        assert np.isnan(float(got[0]))
    assert torch.equal(dg["gt"], dw["gt"])
    assert float(got[2].sum()) == float(want[2].sum()) and float(got[3].sum()) == float(want[3].sum())
    # below cluster_epoch only the three point terms exist
    d = device_inputs(c, dtype)
    below = get_config(cluster_epoch=128, native_losses=True)
    res = model_losses_native(_ret(d, c), d["sem_label"], d["ins"], d["info"], d["pointnum"], d["xyz"], 1, below)
    ref = model_losses(_ret(d, c), d["sem_label"], d["ins"], d["info"], d["pointnum"], d["xyz"], 1, below)
    assert set(res[1]) == {"semantic_loss", "offset_norm_loss", "offset_dir_loss", "loss"} and res[3] is None and res[4] is None
    for name in ref[1]:
        w, g = float(ref[1][name]), float(res[1][name])
        assert (np.isnan(w) and np.isnan(g)) or abs(g - w) <= TOL * max(1.0, abs(w)), name
    res[0].backward()
    assert d["sem"].grad is not None and d["off"].grad is not None and d["mask"].grad is None


def test_labels_outside_the_classes_are_ignored_and_counted():
    """K = 20 and a label of 25 (and -3, and 2^40) in a few rows: counted in counts[3], the result is the oracle's with those
    rows at -100 and their logit gradient is zero -- the label never becomes an index."""
    shape = SHAPES[4]
    c, _, _ = reference(shape, "fp32")
    bad = {7: 25, 300: -3, 4097: 1 << 40, 4999: 20}
    d = device_inputs(c, "fp32")
    fixed = dict(c, sem=c["sem"].copy())
    for row, label in bad.items():
        d["sem_label"][row] = label
        fixed["sem"][row] = -100
    terms, counts, _, grads = run(d)
    assert counts[3].item() == len(bad) and counts[2].item() == int((fixed["sem"] != -100).sum())
    check_terms(terms, expected_terms(fixed, G.oracle_terms(fixed, CFG.fg_thresh, CFG.bg_thresh), 20))
    _, want_grads = G.twin(fixed, CFG.fg_thresh, CFG.bg_thresh)
    check_grads(grads, want_grads, "fp32", fixed)
    assert not grads["sem_score"][list(bad)].any()


# The stem kernel's gradient under the native losses against the torch losses, |a - b| / |b|, measured on an MI355X: see
# STEM_GRAD_MEASURED; the bound is ten times that (torch's own path sums with atomics, whose order differs between devices).
STEM_GRAD_MEASURED = 1.963e-06                                # a second run on another box of the kind gave 1.487e-06
STEM_GRAD_BOUND = 10 * STEM_GRAD_MEASURED


def test_model_fn_step_with_native_losses():
    """One model_fn training step from the same weights with cfg.native_losses on and off: the logged terms and the gradient
    that reaches the first stem convolution.  The batch is the small two-scene one of tests/test_train_gpu.py::
    test_pbnet_training_step_runs: model_fn needs a whole batch dict with labels, instance statistics and teacher-forced
    heads, and that test is where the suite builds one; tests/test_train_engine_gpu.py drives the U-Net bodies alone
    (features and coordinates of two scenes, no labels), which model_fn cannot take."""
    from pbnet_amd import synth
    from pbnet_amd.network.PBNet import PBNet, model_fn
    torch.manual_seed(22)
    model = PBNet(get_config(batch_size=2, cluster_epoch=0)).to(DEV).train()
    batch_np, teacher_np, _ = synth.make_val_batch(seed=3, copies=2, room=(1.2, 1.0, 0.8), n_boxes=4, pitch=0.03, classes=(17, 10))
    t = torch.from_numpy
    batch = {k: t(v) for k, v in batch_np.items()}
    n, ins = batch["xyz_original"].shape[0], batch["ins"]
    info, pointnum = torch.zeros(n, 9), []
    for i in range(int(ins.max().item()) + 1):
        m = ins == i
        pointnum.append(int(m.sum()))
        if m.any():
            info[m, 0:3] = batch["xyz_original"][m].mean(0)
    batch.update(sem=t(teacher_np["sem_score"].argmax(1)).long(), inst_info=info,
                 instance_pointnum=torch.tensor(pointnum, dtype=torch.int32))
    teacher = {k: t(v) for k, v in teacher_np.items()}
    forward = model.forward
    model.forward = lambda *a, **kw: forward(*a, teacher=teacher, **kw)
    stem = next(p for name, p in model.named_parameters() if name.endswith("conv0p1s1.kernel"))
    seen = {}
    for native in (False, True):
        for p in model.parameters():
            p.grad = None
        cfg = get_config(batch_size=2, cluster_epoch=0, native_losses=native)
        loss, pred, visual, meter = model_fn({k: v.clone() for k, v in batch.items()}, model, 1, cfg, "train")
        loss.backward()
        seen[native] = (visual, stem.grad.detach().double().cpu(), {k: float(v[1]) for k, v in meter.items()},
                        pred["mask_scores"][1].clone())
    assert set(seen[True][0]) == set(seen[False][0]) == {"loss", "semantic_loss", "offset_norm_loss", "offset_dir_loss", "mask_loss"}
    for name, w in seen[False][0].items():
        g = seen[True][0][name]
        print("%s: %.9g vs %.9g" % (name, g, w))
        assert abs(g - w) <= TOL * max(1.0, abs(w)), name
    assert seen[True][2] == seen[False][2] and torch.equal(seen[True][3], seen[False][3])
    rel = float((seen[True][1] - seen[False][1]).norm() / seen[False][1].norm())
    print("stem kernel gradient, native against torch losses: %.3e" % rel)
    assert STEM_GRAD_BOUND <= 1e-3 and rel < STEM_GRAD_BOUND
