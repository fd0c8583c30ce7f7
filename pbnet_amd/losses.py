"""The loss terms of model_fn on the device: one forward and one backward call of csrc/losses.hip in place of the few hundred
small torch launches of `model_losses` and its autograd chain (pbnet_amd/network/PBNet.py).  Off by default: set
`cfg.native_losses = True` (get_config(native_losses=True)) and `model_fn` goes through `model_losses_native`."""
import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from . import _native as N

TERMS = ("semantic_loss", "offset_norm_loss", "offset_dir_loss", "mask_loss", "dice_loss", "score_loss", "loss")


def _rows(t):
    """A [n, k] prediction as (tensor, leading dimension): rows may be strided, columns are adjacent."""
    if t.stride(1) != 1 or t.stride(0) < t.shape[1]:
        t = t.contiguous()
    return t, t.stride(0) if t.shape[0] > 1 else t.shape[1]


class LossTerms(Function):
    """(sem_score [N,K], offset_pred [N,3], pred_mask [R] or None, clt_scores [P] or None; labels, targets, the IoU table)
    -> terms f32[8], counts i64[4], gt_scores f32[P] (see pbn_losses_forward in include/pbnet_hip.h).  The predictions go in
    in the dtype they have (float32 / bfloat16 / float16) and get their gradients back in it.  Only terms[6], the loss,
    carries the graph: backward takes d/d terms[6] and ignores the other entries' gradients.  `gt_mask` is rewritten in
    place (-1 -> 0).  pred_mask None: below cluster_epoch, the three point terms only."""

    @staticmethod
    def forward(ctx, sem_score, offset_pred, pred_mask, clt_scores, sem_label, ins_label, inst_info, xyz, gt_mask, iou, fg, bg):
        N.require_cuda(sem_score, offset_pred, pred_mask, clt_scores, sem_label, ins_label, inst_info, xyz, gt_mask, iou)
        dev = sem_score.device
        n, k = sem_score.shape
        sem, ld = _rows(sem_score)
        off = offset_pred.contiguous()
        assert off.shape == (n, 3) and inst_info.shape == (n, 9) and xyz.shape == (n, 3)
        assert inst_info.dtype == torch.float32 and xyz.dtype == torch.float32
        assert sem_label.dtype == torch.int64 and ins_label.dtype == torch.int64
        info, xyz, sem_label, ins_label = inst_info.contiguous(), xyz.contiguous(), sem_label.contiguous(), ins_label.contiguous()
        clustered = pred_mask is not None
        if clustered:
            assert gt_mask.dtype == torch.int64 and gt_mask.is_contiguous() and iou.dtype == torch.float32
            mask, clt, iou = pred_mask.contiguous().view(-1), clt_scores.contiguous().view(-1), iou.contiguous()
            r, p = mask.shape[0], clt.shape[0]
            assert gt_mask.numel() == r and iou.shape[0] == p
            weight = torch.empty(r, dtype=torch.uint8, device=dev)
        else:
            mask = clt = iou = weight = gt_mask = None
            r, p = -1, 0
        gt_scores = torch.empty(p, dtype=torch.float32, device=dev)
        terms = torch.empty(8, dtype=torch.float32, device=dev)
        counts = torch.empty(4, dtype=torch.int64, device=dev)
        state = torch.empty(8, dtype=torch.float64, device=dev)
        lib = N.lib()
        ws = torch.empty(lib.pbn_losses_workspace_bytes(n, r, p), dtype=torch.uint8, device=dev)
        dt = lambda t: N.DT[t.dtype] if t is not None else 0
        rc = lib.pbn_losses_forward(
            N.c_vp(sem.data_ptr()), dt(sem), ld, N.ptr(sem_label), N.ptr(off), dt(off), N.ptr(info), N.ptr(xyz), N.ptr(ins_label), n, k,
            N.ptr(mask), dt(mask), N.ptr(gt_mask), N.ptr(weight), r, N.ptr(iou), iou.shape[1] if clustered else 0, N.ptr(clt),
            dt(clt), p, float(fg), float(bg), N.ptr(gt_scores), N.ptr(terms), N.ptr(counts), N.ptr(state), N.ptr(ws),
            ws.numel(), N.current_stream())
        N.check(rc, "pbn_losses_forward")
        ctx.save_for_backward(sem, off, mask, clt, sem_label, ins_label, info, xyz, gt_mask, weight, gt_scores, state)
        ctx.shapes = (ld, pred_mask.shape if clustered else None, clt_scores.shape if clustered else None)
        ctx.mark_non_differentiable(counts, gt_scores)
        return terms, counts, gt_scores

    @staticmethod
    @once_differentiable
    def backward(ctx, g_terms, _g_counts, _g_scores):
        sem, off, mask, clt, sem_label, ins_label, info, xyz, gt_mask, weight, gt_scores, state = ctx.saved_tensors
        ld, mask_shape, clt_shape = ctx.shapes
        n, k = sem.shape
        clustered = mask is not None
        r, p = (mask.shape[0], clt.shape[0]) if clustered else (-1, 0)
        grad_loss = g_terms.float().contiguous()[6:7]                  # stays on the device
        g_sem = torch.empty(n, k, dtype=sem.dtype, device=sem.device)
        g_off = torch.empty_like(off)
        g_mask = torch.empty_like(mask) if clustered else None
        g_clt = torch.empty_like(clt) if clustered else None
        dt = lambda t: N.DT[t.dtype] if t is not None else 0
        rc = N.lib().pbn_losses_backward(
            N.c_vp(sem.data_ptr()), dt(sem), ld, N.ptr(sem_label), N.ptr(off), dt(off), N.ptr(info), N.ptr(xyz), N.ptr(ins_label), n, k,
            N.ptr(mask), dt(mask), N.ptr(gt_mask), N.ptr(weight), r, N.ptr(clt), dt(clt), N.ptr(gt_scores), p, N.ptr(state),
            N.ptr(grad_loss), N.ptr(g_sem), N.ptr(g_off), N.ptr(g_mask), N.ptr(g_clt), N.current_stream())
        N.check(rc, "pbn_losses_backward")
        return (g_sem, g_off, g_mask.view(mask_shape) if clustered else None, g_clt.view(clt_shape) if clustered else None,
                None, None, None, None, None, None, None, None)


def model_losses_native(ret, sem_label, ins_label, instance_info, instance_pointnum, xyz_original, epoch, cfg):
    """`model_losses` (pbnet_amd/network/PBNet.py) through LossTerms: the same five-tuple (loss, parts, valid, weight,
    gt_mask) with the same keys in `parts`, the same in-place rewrite of gt_mask (-1 -> 0; the same tensor object is
    returned and travels on in pred['mask_scores']) and the same NaN for an empty mean.  Differences a caller can see:
    `parts` are 0-d views of one float32[8] tensor, detached except parts['loss'] (= the returned loss), which alone
    carries the graph; `valid` and `weight` are not the per-row masks but 0-d int64 tensors whose .sum() is what the
    masks' .sum() was (rows with an instance label / mask rows that are not ignored) -- all model_fn reads of them.  A
    semantic label that is neither -100 nor a class is ignored (torch's kernel asserts on it)."""
    clustered = epoch > cfg.cluster_epoch
    pred_mask = clt = gt_mask = iou = None
    if clustered:
        from . import pbnet_ops as ops
        pred_mask, gt_mask = ret["mask_scores"]
        proposals_idx, proposals_offset, _, _ = ret["proposals"]
        iou = ops.get_iou(proposals_idx[:, 1].contiguous(), proposals_offset, ins_label, instance_pointnum)
        clt = ret["clt_scores"]
    terms, counts, _ = LossTerms.apply(ret["sem_pred_score_p"], ret["offset_pred_p"], pred_mask, clt, sem_label, ins_label,
                                       instance_info, xyz_original, gt_mask, iou, cfg.fg_thresh, cfg.bg_thresh)
    logged = terms.detach()
    names = TERMS if clustered else TERMS[:3]
    parts = {name: logged[i] for i, name in enumerate(TERMS) if name in names}
    parts["loss"] = loss = terms[6]
    return loss, parts, counts[0], counts[1] if clustered else None, gt_mask
