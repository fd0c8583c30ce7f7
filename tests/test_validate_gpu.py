"""GPU tier: validate.ValidationEpoch (train.py:123-304) over three synthetic validation scenes at the room size
scripts/eval_loop.py uses, heads teacher-forced through the `model_fn=` hook, against the restatements applied to the `pred`
tensors each step returned and against refine_instances + assign_instances_for_scan called by hand."""
import numpy as np
import pytest
import torch

import metrics_ref as R
from pbnet_amd import evaluate, synth, validate as V
from pbnet_amd.config import get_config
from pbnet_amd.postprocess import refine_instances

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
N_SCENES = 3


def make_scene(i):
    batch_np, teacher_np, _ = synth.make_train_batch(seed=20 + i, copies=3, room=(2.4, 2.0, 1.8), n_boxes=6)
    n = batch_np["xyz_original"].shape[0]
    sem = batch_np["sem"].copy()
    sem[np.random.default_rng(i).random(n) < 0.1] = -100                    # unannotated points
    batch = {k: torch.from_numpy(v) for k, v in dict(batch_np, sem=sem).items()}
    batch["fn"] = ["scene%04d_00" % i] * 3
    batch["sup"] = np.arange(n // 3) // 64                                   # stand-in for the mesh segmentation
    teacher = {k: torch.from_numpy(v) for k, v in teacher_np.items()}
    return batch, teacher


def forced(teachers):
    """model_fn with the two head outputs replaced by the scene's teacher (random weights find no instances)."""
    from pbnet_amd.network.PBNet import model_fn

    def fn(batch, model, epoch, cfg, task="train"):
        teacher = teachers[batch["fn"][0]]
        orig = model.forward
        model.forward = lambda *a, **kw: orig(*a, teacher=teacher, **kw)
        try:
            return model_fn(batch, model, epoch, cfg, task)
        finally:
            del model.forward
    return fn


@pytest.fixture(scope="module")
def setup():
    from pbnet_amd.network.PBNet import PBNet
    cfg = get_config(batch_size=1, cluster_epoch=0)
    torch.manual_seed(22)
    model = PBNet(cfg).to(DEV)
    data = [make_scene(i) for i in range(N_SCENES)]
    teachers = {b["fn"][0]: t for b, t in data}
    return cfg, model, [b for b, _ in data], forced(teachers)


def run_epoch(setup, epoch=1, keep_pred=False):
    cfg, model, batches, fn = setup
    ve = V.ValidationEpoch(model, cfg, epoch, model_fn=fn)
    preds = []
    for batch in batches:
        pred = ve.step(batch)
        if keep_pred:
            preds.append({k: ([x.clone() for x in v] if isinstance(v, (tuple, list)) else v.clone()) for k, v in pred.items()})
    return ve, ve.finish(), preds


def same_matches(a, b):
    assert sorted(a) == sorted(b)
    for name in a:
        for field in evaluate.SceneMatches.__slots__:
            x, y = getattr(a[name], field), getattr(b[name], field)
            assert (x == y) if isinstance(x, str) else np.array_equal(np.asarray(x), np.asarray(y)), (name, field)


def test_epoch_equals_restatements_on_the_returned_pred(setup):
    cfg, model, batches, _ = setup
    ve, out, preds = run_epoch(setup, keep_pred=True)
    assert not model.training and out["scenes"] == N_SCENES
    # semantic: the restatement on pred['sem'] and the batch labels
    K = cfg.sem_num
    want = sum(np.stack(R.sem_counts(p["sem"].cpu().numpy(), b["sem"].numpy(), K)) for p, b in zip(preds, batches))
    sem = out["semantic"]
    assert np.array_equal(np.stack([sem["intersection"], sem["output"], sem["target"]]), want)
    assert want[2].sum() > 0 and want[0].sum() > 0.9 * want[2].sum()                 # teacher-forced heads: mostly right
    ratios = V.semantic_ratios(*want)
    assert out["mIoU"] == ratios["mIoU"] and out["mAcc"] == ratios["mAcc"] and out["allAcc"] == ratios["allAcc"]
    # mask rows: the restatement on pred['mask_scores']
    rows = np.stack([R.mask_row(p["mask_scores"][0].float().cpu().numpy(), p["mask_scores"][1].cpu().numpy()) for p in preds])
    assert rows[:, 0].min() > 0 and np.array_equal(ve.mask.rows(), rows)
    ref = V.mask_ratios(rows)
    for key in ("All_mask_acc", "Tp_acc", "Fp_acc"):
        assert np.array_equal(out[key], ref[key], equal_nan=True)
    # the reference's own statements on a copy of the first scene's tensors (they binarise their input in place)
    a, tp, tf = R.reference_mask_form_torch(preds[0]["mask_scores"][0].float().clone(), preds[0]["mask_scores"][1])
    assert a == rows[0, 1] / rows[0, 0]
    if rows[0, 2]:
        assert abs(float(tp) - rows[0, 3] / rows[0, 2]) <= 2e-6 * float(tp)
    # instance branch: refine_instances + assign_instances_for_scan by hand on the same pred
    by_hand = {}
    for p, b in zip(preds, batches):
        n = b["xyz_original"].shape[0]
        clusters, scores, sem_id = refine_instances(p["sem"], p["proposals"], p["clt_scores"], n, b["sup"], cfg)
        assert clusters.shape[0] > 0
        gt = evaluate.encode_gt_ids(b["sem"].numpy()[:n // 3], b["ins"].numpy()[:n // 3])
        by_hand[b["fn"][0]] = evaluate.assign_instances_for_scan(b["fn"][0], dict(conf=scores, label_id=sem_id, mask=clusters), gt)
    same_matches(out["matches"], by_hand)
    avgs = evaluate.compute_averages(evaluate.evaluate_matches(by_hand))
    assert np.array_equal(out["mAP"], float(avgs["all_ap"]), equal_nan=True)
    assert set(out["losses"]) == {"loss", "semantic_loss", "offset_norm_loss", "offset_dir_loss", "mask_loss"}
    assert all(np.isfinite(v) for v in out["losses"].values())


def test_second_epoch_is_bit_identical(setup):
    _, a, _ = run_epoch(setup)
    _, b, _ = run_epoch(setup)
    for key in ("intersection", "output", "target", "iou_class", "accuracy_class"):
        assert np.array_equal(a["semantic"][key], b["semantic"][key])
    for key in ("mIoU", "mAcc", "allAcc", "All_mask_acc", "Tp_acc", "Fp_acc", "mAP", "AP_50", "AP_25"):
        assert np.array_equal(a[key], b[key], equal_nan=True), key
    assert a["mask"] == b["mask"] or all(np.array_equal(a["mask"][k], b["mask"][k], equal_nan=True) for k in a["mask"])
    assert a["losses"] == b["losses"]
    same_matches(a["matches"], b["matches"])


def test_before_the_cluster_epoch_there_are_no_mask_or_ap_keys(setup):
    cfg, model, batches, fn = setup
    lines = []

    class Log(object):
        def info(self, line):
            lines.append(line)
    ve = V.ValidationEpoch(model, cfg, 0, model_fn=fn, logger=Log())
    pred = ve.step(batches[0])
    assert set(pred) == {"sem", "offseted_xyz"}
    out = ve.finish()
    assert not {"mask", "All_mask_acc", "Tp_acc", "Fp_acc", "avgs", "mAP", "matches"} & set(out)
    want = np.stack(R.sem_counts(pred["sem"].cpu().numpy(), batches[0]["sem"].numpy(), cfg.sem_num))
    assert np.array_equal(out["semantic"]["intersection"], want[0])
    assert lines[-1] == V.format_semantic_line(out["semantic"]) and lines[-1].startswith("mIoU/mAcc/allAcc ")
    assert ve.mask.rows().shape == (0, 8)
