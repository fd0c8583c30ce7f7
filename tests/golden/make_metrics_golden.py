#!/usr/bin/env python3
"""Golden vectors for the validation meters (pbnet_amd/validate.py, csrc/metrics.hip), produced IN THE BUILD CONTAINER by
the reference's own code: `tools.mIOU.intersectionAndUnionGPU` and `tools.log.AverageMeter` are imported from
/root/reference and RUN.  The function ends in `.cuda()`; this process makes `Tensor.cuda` the identity so that it runs on
CPU tensors.  The mask block (train.py:152-168) and the final ratios (train.py:279-283) are statements inside eval_epoch
and cannot be imported: the statements below follow them line by line on CPU tensors.

    python tests/golden/make_metrics_golden.py         # writes tests/golden/metrics_*.npz

Only data is written: labels as int8, the reference's float32 results, and the integer counts they stand for.  Every
running sum of every epoch stays below 2^24, where the reference's float32 sums are still exact integers (asserted)."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, "/root/reference")
torch.Tensor.cuda = lambda self, *a, **k: self          # the reference function ends in .cuda(); run it on CPU tensors
from tools.mIOU import intersectionAndUnionGPU           # noqa: E402  (reference code, executed here only)
from tools.log import AverageMeter                       # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
IGNORE = -100


def runs(rng, n, weights, lo=20, hi=400):
    """Labels in runs of lo..hi points (a scan is spatially coherent), classes drawn with `weights`."""
    out = np.empty(n, np.int64)
    i = 0
    while i < n:
        m = int(rng.integers(lo, hi))
        out[i:i + m] = rng.choice(len(weights), p=weights)
        i += m
    return out


def sem_scene(rng, n, K, ignore_frac=0.2, absent=None, flips=0.1, plant=False):
    w = 1.0 / (1.0 + np.arange(K)) ** 1.3                # skewed: class 0 (floor) >> class K-1
    if absent is not None:
        w[absent] = 0.0
    w /= w.sum()
    target = runs(rng, n, w)
    pred = target.copy()
    f = rng.random(n) < flips
    pred[f] = rng.choice(K, int(f.sum()), p=w)
    if n:
        ign = runs(rng, n, np.array([1 - ignore_frac, ignore_frac]), 10, 200) == 1
        target[ign] = IGNORE
    if plant and n:
        odd = np.array([-1, K, K + 3, -99])              # -99: an ignore-like value that is NOT the ignore value
        for arr in (pred, target):
            at = rng.choice(n, max(4, n // 50), replace=False)
            arr[at] = odd[rng.integers(0, 4, at.shape[0])]
        pred[rng.choice(n, max(1, n // 200), replace=False)] = IGNORE
    return pred, target


def sem_epoch(name, K, scenes):
    """train.py:133-149 and :279-283 over `scenes` = [(pred, target)], with the reference's function and meter."""
    intersection_meter, union_meter, target_meter = AverageMeter(), AverageMeter(), AverageMeter()
    per, acc_val = [], []
    for pred, target in scenes:
        pred_sem, sem_label = torch.from_numpy(pred), torch.from_numpy(target)
        intersection, union, tgt = intersectionAndUnionGPU(pred_sem.detach().clone(), sem_label.detach().clone(), K, -100)
        intersection, union, tgt = intersection.cpu().numpy(), union.cpu().numpy(), tgt.cpu().numpy()
        intersection_meter.update(intersection), union_meter.update(union), target_meter.update(tgt)
        accuracy = sum(intersection_meter.val) / (sum(target_meter.val) + 1e-10)
        per.append(np.stack([intersection, union, tgt]))
        acc_val.append(float(accuracy))
    iou_class = intersection_meter.sum / (union_meter.sum + 1e-10)
    accuracy_class = intersection_meter.sum / (target_meter.sum + 1e-10)
    mIoU = np.mean(iou_class)
    mAcc = np.mean(accuracy_class)
    allAcc = sum(intersection_meter.sum) / (sum(target_meter.sum) + 1e-10)
    sums = np.stack([intersection_meter.sum, union_meter.sum, target_meter.sum])
    per = np.stack(per)
    assert per.dtype == np.float32 and sums.dtype == np.float32
    assert float(sums.max()) < 2 ** 24 and float(sums.sum(1).max()) < 2 ** 24, "float32 sums must stay exact integers"
    assert np.array_equal(per, np.round(per)) and np.array_equal(per.astype(np.int64).sum(0), sums.astype(np.int64))
    lens = np.array([p.shape[0] for p, _ in scenes], np.int64)
    pred = np.concatenate([p for p, _ in scenes]) if len(scenes) else np.zeros(0, np.int64)
    target = np.concatenate([t for _, t in scenes])
    assert np.abs(pred).max(initial=0) < 128 and np.abs(target).max(initial=0) < 128
    path = os.path.join(HERE, "metrics_%s.npz" % name)
    np.savez_compressed(path, K=K, ignore_index=IGNORE, lens=lens, pred=pred.astype(np.int8), target=target.astype(np.int8),
                        scene_f32=per, scene_counts=per.astype(np.int64), sum_f32=sums, sum_counts=sums.astype(np.int64),
                        accuracy_val=np.array(acc_val, np.float64), iou_class=np.asarray(iou_class),
                        accuracy_class=np.asarray(accuracy_class), mIoU=np.asarray(mIoU), mAcc=np.asarray(mAcc),
                        allAcc=np.asarray(allAcc))
    print("%-7s K=%2d scenes %d points %7d  mIoU %.4f mAcc %.4f allAcc %.4f  %d KB" %
          (name, K, len(scenes), int(lens.sum()), mIoU, mAcc, allAcc, os.path.getsize(path) // 1024))


def bf16_grid(x):
    """Round to values that float32, bfloat16 AND float16 all hold exactly (7 mantissa bits, magnitude >= 2^-10 or 0)."""
    x = torch.from_numpy(np.asarray(x, np.float32)).bfloat16().float()
    x[x.abs() < 2.0 ** -10] = 0.0
    assert torch.equal(x, x.bfloat16().float()) and torch.equal(x, x.half().float())
    return x.numpy()


def mask_epoch(name, scenes):
    """train.py:136-138,152-168,298-300 on CPU tensors, statement by statement."""
    All_accm, Tp_accm, Tf_accm = AverageMeter(), AverageMeter(), AverageMeter()
    rows, raised = [], []
    for pred, gt in scenes:
        pred_mask, gt_mask = torch.from_numpy(pred.copy()).view(-1, 1), torch.from_numpy(gt.astype(np.int64))
        try:
            pred_mask = pred_mask.view(-1)
            pred_mask[pred_mask >= 0.5] = 1
            pred_mask[pred_mask < 0.5] = 0
            error_map = pred_mask - gt_mask
            tp_idx = torch.nonzero(error_map == 0).view(-1)
            all_accuracy = tp_idx.shape[0] / gt_mask.shape[0]

            Tp_idx = torch.nonzero(gt_mask == 1)
            tp_acc = pred_mask[Tp_idx].sum() / Tp_idx.shape[0]

            Tf_idx = torch.nonzero(gt_mask == 0)
            tf_acc = 1 - pred_mask[Tf_idx].sum() / Tf_idx.shape[0]
            All_accm.update(all_accuracy)
            Tp_accm.update(tp_acc)
            Tf_accm.update(tf_acc)
        except ZeroDivisionError:                        # a scene without rows: train.py:159 divides by zero
            assert gt_mask.shape[0] == 0
            raised.append(True)
            continue
        raised.append(False)
        rows.append([gt_mask.shape[0], tp_idx.shape[0], Tp_idx.shape[0], int(pred_mask[Tp_idx].sum()), Tf_idx.shape[0],
                     int(pred_mask[Tf_idx].sum()), 0, 0])
    lens = np.array([p.shape[0] for p, _ in scenes], np.int64)
    path = os.path.join(HERE, "metrics_%s.npz" % name)
    np.savez_compressed(path, lens=lens, pred=np.concatenate([p for p, _ in scenes]).astype(np.float32),
                        gt=np.concatenate([g for _, g in scenes]).astype(np.int8), rows=np.array(rows, np.int64),
                        raised=np.array(raised), All_mask_acc=np.float64(All_accm.avg),
                        Tp_acc=np.float32(Tp_accm.avg), Fp_acc=np.float32(Tf_accm.avg))
    print("%-7s scenes %d rows %d  All %.4f Tp %s Fp %.4f  %d KB" % (name, len(scenes), int(lens.sum()), All_accm.avg,
                                                                   float(Tp_accm.avg), float(Tf_accm.avg),
                                                                   os.path.getsize(path) // 1024))


def mask_scene(rng, n, positives=True):
    gt = (runs(rng, n, np.array([0.6, 0.4]), 5, 120) == 1).astype(np.int64) if positives else np.zeros(n, np.int64)
    score = np.where(gt == 1, rng.beta(5, 2, n), rng.beta(2, 5, n))
    score = bf16_grid(score)
    edge = bf16_grid([0.5, 0.5 - 2.0 ** -10, 0.5 + 2.0 ** -8, 0.0, 1.0, 0.49609375, 0.50390625])
    at = rng.choice(n, min(n, 70), replace=False)
    score[at] = edge[np.arange(at.shape[0]) % edge.shape[0]]
    return score, gt


def main():
    rng = np.random.default_rng(20)
    sem_epoch("S1", 20, [sem_scene(rng, n, 20, absent=15) for n in (20011, 60000, 33333, 47001, 25600)])
    sem_epoch("S2", 20, [sem_scene(rng, n, 20, plant=True) for n in (5000, 7013, 3001)])
    s3 = [sem_scene(rng, 2000, 20), sem_scene(rng, 1500, 20), sem_scene(rng, 1, 20, ignore_frac=0.0), sem_scene(rng, 0, 20),
          sem_scene(rng, 900, 20)]
    s3[1][1][:] = IGNORE                                 # every target ignored
    sem_epoch("S3", 20, s3)
    sem_epoch("S4_K2", 2, [sem_scene(rng, n, 2, flips=0.3) for n in (4099, 2048)])
    sem_epoch("S4_K13", 13, [sem_scene(rng, n, 13, plant=True) for n in (6001, 3000, 1023)])
    empty = (np.zeros(0, np.float32), np.zeros(0, np.int64))
    mask_epoch("M1", [mask_scene(rng, 9001), mask_scene(rng, 70003), mask_scene(rng, 4096, positives=False), empty,
                      mask_scene(rng, 2500)])


if __name__ == "__main__":
    main()
