"""Independent restatements for the validation meters (tests only).

`sem_counts` / `mask_row`: the integer form of tools/mIOU.py:18-31 and train.py:153-168 in numpy (`bincount`, boolean
sums).  `reference_form_torch` / `reference_mask_form_torch`: the reference's OWN sequence of torch operations (clone,
masked write, .float().cpu(), histc, .cuda(); nonzero, index, sum) on whatever device the inputs live on -- the timing
baseline of DESIGN.md section 10 and the check for sizes too big to commit as fixtures."""
import numpy as np
import torch


def sem_counts(pred, target, K, ignore_index=-100, confusion=False):
    """(intersection, output, target) int64 [K] each (+ confusion int64 [K, K], row = target, col = pred)."""
    pred = np.asarray(pred).astype(np.int64).reshape(-1)
    target = np.asarray(target).astype(np.int64).reshape(-1)
    out = np.where(target == ignore_index, ignore_index, pred)            # mIOU.py:24

    def hist(v):                                                          # histc(bins=K, min=0, max=K-1) of integers
        return np.bincount(v[(v >= 0) & (v < K)], minlength=K).astype(np.int64)
    res = (hist(out[out == target]), hist(out), hist(target))
    if confusion:
        ok = (target != ignore_index) & (target >= 0) & (target < K) & (pred >= 0) & (pred < K)
        res += (np.bincount(target[ok] * K + pred[ok], minlength=K * K).reshape(K, K).astype(np.int64),)
    return res


def mask_row(pred, gt, threshold=0.5):
    """int64 [8]: n, agree, n_pos, pos_pred1, n_neg, neg_pred1, n_nan, 0 (pred widened to float32 first)."""
    pred = np.asarray(pred, np.float32).reshape(-1)
    gt = np.asarray(gt).astype(np.int64).reshape(-1)
    nan = np.isnan(pred)
    with np.errstate(invalid="ignore"):
        one = pred >= np.float32(threshold)
    pos, neg = gt == 1, gt == 0
    agree = ~nan & np.where(one, pos, neg)
    return np.array([pred.shape[0], agree.sum(), pos.sum(), (pos & one).sum(), neg.sum(), (neg & one).sum(), nan.sum(), 0],
                    np.int64)


def reference_form_torch(pred, target, K, ignore_index=-100):
    """train.py:146-147 + tools/mIOU.py:18-31, operation for operation.  Returns three float32 numpy [K] vectors."""
    output, target = pred.detach().clone(), target.detach().clone()
    dev = output.device
    output = output.view(-1)
    target = target.view(-1)
    output[target == ignore_index] = ignore_index
    intersection = output[output == target]
    area_intersection = torch.histc(intersection.float().cpu(), bins=K, min=0, max=K - 1)
    area_output = torch.histc(output.float().cpu(), bins=K, min=0, max=K - 1)
    area_target = torch.histc(target.float().cpu(), bins=K, min=0, max=K - 1)
    area_union = area_output + area_target - area_intersection
    intersection, union, target = area_intersection.to(dev), area_union.to(dev), area_target.to(dev)
    return intersection.cpu().numpy(), union.cpu().numpy(), target.cpu().numpy()


def reference_mask_form_torch(pred_mask, gt_mask):
    """train.py:153-165 (binarises `pred_mask` in place, as upstream).  Returns (all_accuracy, tp_acc, tf_acc)."""
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
    return all_accuracy, tp_acc, tf_acc
