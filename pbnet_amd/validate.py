"""The validation epoch of /root/reference/train.py:123-304 (`eval_epoch`) on this package: semantic mIoU / mAcc / allAcc
(`tools/mIOU.py:18-31` intersectionAndUnionGPU, train.py:133-149,279-283), the mask-branch accuracies All / Tp / Tf
(train.py:152-168) and the AP of the instance branch (train.py:171-253,286-288 = postprocess.refine_instances, or
with cfg.device_post its device-resident form, + evaluate.*), as meters whose counters are int64 and live on the device
(csrc/metrics.hip).

What changes against the reference is where the counting happens and in what type, not what is counted:

* the reference clones both label vectors, copies three float vectors to the host, bins them there with `histc`, copies the
  three histograms back and out again, and forms the mask ratios through two `nonzero` calls: nine host<->device round
  trips per scene.  Here one launch adds a scene's counts into device counters and one writes a scene's mask row; nothing is
  read back until `result()` (or `accuracy_val()`, when somebody wants the per-iteration number).
* the reference's AverageMeter sums float32 count vectors, so a class whose running count passes 2^24 stops growing
  (float32(2^24) + 1 == float32(2^24)); ScanNet val passes that for wall / floor.  Integer counters are exact, and the
  ratios are formed from them in float64 with the reference's formulas (both `+ 1e-10` kept).
"""
import os
import time

import numpy as np
import torch

from . import _native as N

_LABEL_DTYPES = (torch.int32, torch.int64)
_SCORE_CODES = {torch.float32: 0, torch.bfloat16: 1, torch.float16: 2}      # PBN_F32 / PBN_BF16 / PBN_F16


def _check_classes(n_class):
    n_class = int(n_class)
    if n_class < 2 or n_class > 64:
        # K = 1: histc(min=0, max=0) takes its range from the data, there is nothing to restate; K > 64: the K x K table
        # no longer fits the kernel's LDS budget
        raise ValueError("n_class must be in [2, 64], got %d" % n_class)
    return n_class


def _flat_labels(t, what):
    """1-D int32 / int64 view of `t` with unit stride (a strided view is copied; any element offset is fine)."""
    if t.dtype not in _LABEL_DTYPES:
        raise TypeError("%s must be int32 or int64, got %s" % (what, t.dtype))
    t = t.detach().reshape(-1)
    return t if t.numel() == 0 or t.stride(0) == 1 else t.contiguous()


def _sem_confusion(pred, target, n_class, ignore_index, acc3k, conf):
    N.require_cuda(pred, target, acc3k, conf)
    p, t = _flat_labels(pred, "pred"), _flat_labels(target, "target")
    if p.shape != t.shape:
        raise ValueError("pred has %d labels, target %d" % (p.numel(), t.numel()))
    N.check(N.lib().pbn_sem_confusion(p.data_ptr(), int(p.dtype == torch.int64), t.data_ptr(), int(t.dtype == torch.int64),
                                      p.numel(), n_class, int(ignore_index), acc3k.data_ptr(),
                                      None if conf is None else conf.data_ptr(), N.current_stream()), "pbn_sem_confusion")


def intersectionAndUnionGPU(output, target, K, ignore_index=-100):
    """tools/mIOU.py:18-31, same signature and return form: (area_intersection, area_union, area_target), float32 [K] on
    `output`'s device; `output[target == ignore_index] = ignore_index` is applied in place as upstream (mIOU.py:24).  The
    counting is one kernel on integer counters; the float32 conversion of the result is exact below 2^24 per class."""
    K = _check_classes(K)
    N.require_cuda(output, target)
    assert output.dim() in [1, 2, 3, 4]
    assert output.shape == target.shape
    acc = torch.zeros(3 * K, dtype=torch.int64, device=output.device)
    _sem_confusion(output, target, K, ignore_index, acc, None)
    output.view(-1)[target.view(-1) == ignore_index] = ignore_index
    inter, out, tgt = acc[:K], acc[K:2 * K], acc[2 * K:]
    return inter.float(), (out + tgt - inter).float(), tgt.float()


def semantic_ratios(intersection, output, target):
    """train.py:279-283 in float64 from integer counts: dict(union, iou_class, accuracy_class, mIoU, mAcc, allAcc)."""
    inter, out, tgt = (np.asarray(a, np.int64) for a in (intersection, output, target))
    union = out + tgt - inter
    iou_class = inter.astype(np.float64) / (union.astype(np.float64) + 1e-10)
    accuracy_class = inter.astype(np.float64) / (tgt.astype(np.float64) + 1e-10)
    return dict(union=union, iou_class=iou_class, accuracy_class=accuracy_class, mIoU=float(np.mean(iou_class)),
                mAcc=float(np.mean(accuracy_class)), allAcc=float(inter.sum()) / (float(tgt.sum()) + 1e-10))


class SemanticMeter(object):
    """intersection / output / target counts of an epoch (and the K x K confusion table when asked for) as int64 counters.

    One buffer: total[3K] | confusion[K*K] | before[3K].  `update` copies total -> before and adds the scene into total: two
    launches, no synchronisation, no allocation; the LAST scene's counts (train.py:149 reads `.val`) are total - before, formed
    on the host when `accuracy_val()` is asked for.  With device="cpu" the counters are host memory: `merge_`, `all_reduce`
    (gloo) and `result()` work there, `update` needs device tensors and raises."""

    def __init__(self, n_class, ignore_index=-100, device=None, confusion=False):
        self.n_class = _check_classes(n_class)
        self.ignore_index = int(ignore_index)
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        k = self.n_class
        self._n_conf = k * k if confusion else 0
        self._buf = torch.zeros(6 * k + self._n_conf, dtype=torch.int64, device=self.device)
        self._total = self._buf[:3 * k]
        self._conf = self._buf[3 * k:3 * k + self._n_conf] if confusion else None
        self._before = self._buf[3 * k + self._n_conf:]
        self.updates = 0

    def reset(self):
        self._buf.zero_()
        self.updates = 0

    def update(self, pred, target):
        N.require_cuda(pred, target, self._buf)
        self._before.copy_(self._total)
        _sem_confusion(pred, target, self.n_class, self.ignore_index, self._total, self._conf)
        self.updates += 1

    def merge_(self, other, confusion=None):
        """Add another meter, or integer counts ([3K] or [3, K]: intersection | output | target, plus an optional [K, K]
        table).  The merged counts become the `last update` that accuracy_val() reports."""
        if isinstance(other, SemanticMeter):
            if other.n_class != self.n_class or (other._conf is None) != (self._conf is None):
                raise ValueError("meters of different shape")
            counts, confusion = other._total, other._conf
        else:
            counts = torch.as_tensor(np.asarray(other.cpu() if torch.is_tensor(other) else other).astype(np.int64)).reshape(-1)
            if counts.numel() != 3 * self.n_class:
                raise ValueError("expected %d counts, got %d" % (3 * self.n_class, counts.numel()))
        self._before.copy_(self._total)
        self._total.add_(counts.to(self.device))
        if confusion is not None:
            if self._conf is None:
                raise ValueError("this meter keeps no confusion table")
            conf = torch.as_tensor(np.asarray(confusion.cpu() if torch.is_tensor(confusion) else confusion).astype(np.int64))
            self._conf.add_(conf.reshape(-1).to(self.device))
        self.updates += 1
        return self

    def all_reduce(self, group=None):
        """SUM of the counters over the ranks: one collective over total | confusion.  The last-update counts stay local."""
        import torch.distributed as dist
        if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size(group) == 1:
            return self
        head = self._buf[:3 * self.n_class + self._n_conf]
        old = self._total.clone()
        if head.is_cuda and dist.get_backend(group) == "gloo":
            host = head.cpu()
            dist.all_reduce(host, op=dist.ReduceOp.SUM, group=group)
            head.copy_(host)
        else:
            dist.all_reduce(head, op=dist.ReduceOp.SUM, group=group)
        self._before.add_(self._total - old)
        return self

    def accuracy_val(self):
        """train.py:149: sum(intersection.val) / (sum(target.val) + 1e-10) of the last update.  One read-back."""
        k = self.n_class
        h = self._buf.cpu().numpy()
        last = h[:3 * k] - h[3 * k + self._n_conf:]
        return float(last[:k].sum()) / (float(last[2 * k:].sum()) + 1e-10)

    def result(self):
        """One read-back; ratios in float64 from the integers (train.py:279-283)."""
        k = self.n_class
        h = self._buf.cpu().numpy()
        inter, out, tgt = h[:k].copy(), h[k:2 * k].copy(), h[2 * k:3 * k].copy()
        res = dict(intersection=inter, output=out, target=tgt, **semantic_ratios(inter, out, tgt))
        if self._conf is not None:
            res["confusion"] = h[3 * k:3 * k + self._n_conf].reshape(k, k).copy()
        return res


def mask_ratios(rows):
    """train.py:159-168,298-300 from integer rows [S, 8] (n, agree, n_pos, pos_pred1, n_neg, neg_pred1, n_nan, 0), in the
    reference's own precisions: `all` is a Python float per scene, `tp` / `tf` are float32 quotients (a float32 tensor sum
    divided by a Python int), each averaged by AverageMeter's running sum.  A scene without positive rows gives 0/0 = NaN
    as upstream and poisons Tp_acc; the *_pooled ratios over the summed counts do not."""
    rows = np.asarray(rows, np.int64).reshape(-1, 8)
    all_sum, tp_sum, tf_sum = 0.0, np.float32(0), np.float32(0)
    with np.errstate(invalid="ignore", divide="ignore"):
        for n, agree, n_pos, pos1, n_neg, neg1 in rows[:, :6].tolist():
            all_sum += agree / n
            tp_sum = np.float32(tp_sum + np.float32(pos1) / np.float32(n_pos))
            tf_sum = np.float32(tf_sum + (np.float32(1) - np.float32(neg1) / np.float32(n_neg)))
        s = rows.shape[0]
        tot = rows.sum(0)

        def ratio(a, b):
            return float(a) / float(b) if b else float("nan")
        return {"All_mask_acc": all_sum / s if s else 0.0,
                "Tp_acc": float(tp_sum / np.float32(s)) if s else 0.0,
                "Fp_acc": float(tf_sum / np.float32(s)) if s else 0.0,
                "All_mask_acc_pooled": ratio(tot[1], tot[0]), "Tp_acc_pooled": ratio(tot[3], tot[2]),
                "Fp_acc_pooled": 1.0 - ratio(tot[5], tot[4]), "n_nan": int(tot[6]), "scenes": int(s)}


class MaskAccuracyMeter(object):
    """One int64 row of eight counts per scene in a device buffer [capacity, 8] (doubling growth); `update` is one launch
    (two above 65 536 rows), no synchronisation.  `pred_mask` is not modified (the reference binarises it in place,
    train.py:155-156; nothing reads it afterwards).  A scene without rows (PBNet._empty_stage) is skipped and counted in
    `skipped`: the reference divides by zero there (train.py:159)."""

    def __init__(self, threshold=0.5, capacity=64):
        self.threshold = float(threshold)
        self._cap = int(capacity)
        self._rows = None
        self._n = 0
        self._host = []
        self.skipped = 0

    def update(self, pred_mask, gt_mask):
        N.require_cuda(pred_mask, gt_mask)
        p = pred_mask.detach().reshape(-1)
        g = gt_mask.detach().reshape(-1)
        if p.numel() != g.numel():
            raise ValueError("pred_mask has %d rows, gt_mask %d" % (p.numel(), g.numel()))
        if p.numel() == 0:
            self.skipped += 1
            return
        if p.dtype not in _SCORE_CODES:
            p = p.float()
        if g.dtype not in _LABEL_DTYPES:
            g = g.long()                     # float / bool targets: converted here, not in the kernel
        p = p if p.stride(0) == 1 else p.contiguous()
        g = g if g.stride(0) == 1 else g.contiguous()
        if self._rows is None:
            self._rows = torch.zeros(self._cap, 8, dtype=torch.int64, device=p.device)
        elif self._n == self._cap:
            grown = torch.zeros(2 * self._cap, 8, dtype=torch.int64, device=self._rows.device)
            grown[:self._cap].copy_(self._rows)
            self._rows, self._cap = grown, 2 * self._cap
        N.check(N.lib().pbn_mask_accuracy(p.data_ptr(), _SCORE_CODES[p.dtype], g.data_ptr(), int(g.dtype == torch.int64),
                                          p.numel(), self.threshold, self._rows[self._n].data_ptr(), N.current_stream()),
                "pbn_mask_accuracy")
        self._n += 1

    def merge_(self, other):
        """Append another meter's scenes, or integer rows [S, 8]."""
        if isinstance(other, MaskAccuracyMeter):
            self._host.append(other.rows())
            self.skipped += other.skipped
        else:
            rows = np.asarray(other, np.int64).reshape(-1, 8)
            self._host.append(rows[rows[:, 0] > 0])
            self.skipped += int((rows[:, 0] <= 0).sum())          # a scene without rows, as in update()
        return self

    def rows(self):
        """Every scene's row on the host, int64 [S, 8].  One read-back."""
        parts = list(self._host)
        if self._n:
            parts.append(self._rows[:self._n].cpu().numpy())
        return np.concatenate(parts) if parts else np.zeros((0, 8), np.int64)

    def gather_(self, group=None):
        """Every rank ends with the rows of all ranks, in rank order (the mean over scenes needs the scenes, not a sum)."""
        import torch.distributed as dist
        if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size(group) == 1:
            return self
        parts = [None] * dist.get_world_size(group)
        dist.all_gather_object(parts, (self.rows(), self.skipped), group=group)
        self._host, self._n = [r for r, _ in parts], 0
        self.skipped = sum(s for _, s in parts)
        return self

    def result(self):
        res = mask_ratios(self.rows())
        res["skipped"] = self.skipped
        return res


class AverageMeter(object):
    """tools/log.py:16-30."""

    def __init__(self):
        self.val = self.avg = self.sum = self.count = 0

    def update(self, val, n=1):
        self.val = val
        self.sum += val * n
        self.count += n
        self.avg = self.sum / self.count


def format_semantic_line(res):
    """train.py:291."""
    return "mIoU/mAcc/allAcc {:.4f}/{:.4f}/{:.4f}.".format(res["mIoU"], res["mAcc"], res["allAcc"])


def _default_model_fn(*a, **kw):
    from .network.PBNet import model_fn
    return model_fn(*a, **kw)


class ValidationEpoch(object):
    """train.py:123-304 against this package: `step(batch)` once per validation scene (its 3 copies), then `finish()`.

    `model_fn` is called as model_fn(batch, model, epoch, cfg, task='eval') and may be wrapped by the caller (teacher
    forcing, a DDP module).  `gt`: a val_gt directory (one `<scene>.txt` per scene), a callable scene name -> ids, or None =
    evaluate.encode_gt_ids of the batch's own first-copy labels.  `reduce=True` sums the meters over the ranks and merges the
    per-scene matches on rank 0 when a process group exists; the reference logs rank 0's shard only (`reduce=False`).

    `cfg.device_ap` (needs `cfg.device_post`): the tail of a step -- post-processing, AP association, loss averages -- reads
    nothing back and allocates nothing once its buffers fit.  Each scene appends one record to an `evaluate.AssociationLog`
    (`ap_log_words` int32 words) and the loss terms go to a `train_epoch.LossMeter`, both gated on the device by n_keep > 0;
    `finish()` reads the log and the meter once.  One visible difference: the `no cluster` lines (same text, same count) are
    printed by `finish()`, not by the step that met the scene.  `progress=True` still works but reads n_keep and the meters
    back every step, which gives up the point of the mode.

    `cfg.device_ap_table` (needs `cfg.device_ap`): `finish()` does not read the log either -- an `evaluate.APTable` matches and
    integrates on the device and the averages come from its table; `out["matches"]` is then None and `out["ap"]` holds the
    cells.  Under a process group with more than one rank the epoch keeps the host path and says so in one line."""

    def __init__(self, model, cfg, epoch, model_fn=None, gt=None, logger=None, writer=None, reduce=True, device=None,
                 progress=False, ap_log_words=4 << 20):
        self.model, self.cfg, self.epoch = model, cfg, int(epoch)
        self.model_fn = _default_model_fn if model_fn is None else model_fn
        self.gt, self.logger, self.writer, self.reduce, self.progress = gt, logger, writer, reduce, progress
        self.cluster = self.epoch > cfg.cluster_epoch
        self.device_post = bool(getattr(cfg, "device_post", False))     # absent = off: postprocess.refine_instances
        self.device_ap = bool(getattr(cfg, "device_ap", False))         # absent = off: evaluate.assign_instances_for_scan
        if self.device_ap and not self.device_post:
            raise ValueError("cfg.device_ap needs cfg.device_post: the association reads what refine_instances_device leaves")
        self.device_ap_table = bool(getattr(cfg, "device_ap_table", False))     # absent = off: evaluate.evaluate_matches
        if self.device_ap_table and not self.device_ap:
            raise ValueError("cfg.device_ap_table needs cfg.device_ap: the table reads the association log where it lies")
        self._post_ws, self._staging, self._empty_buf = None, {}, None
        self._ap_log, self._ap_log_words, self._loss_meter, self._meter_in = None, int(ap_log_words), None, None
        self.semantic = SemanticMeter(cfg.sem_num, -100, device=device)
        self.mask = MaskAccuracyMeter(0.5)
        self.am_dict, self.visual_keys, self.matches = {}, set(), {}
        self.steps = self.no_cluster = 0
        self.start_time = time.time()
        if model is not None:
            model.eval()

    def _info(self, line):
        (print if self.logger is None else self.logger.info)(line)

    def _gt_ids(self, name, batch, n_fold):
        if self.gt is None:
            from . import evaluate
            sem, ins = batch["sem"], batch["ins"]
            sem = sem.cpu().numpy() if torch.is_tensor(sem) else np.asarray(sem)
            ins = ins.cpu().numpy() if torch.is_tensor(ins) else np.asarray(ins)
            return evaluate.encode_gt_ids(sem[:n_fold], ins[:n_fold])
        if callable(self.gt):
            return self.gt(name)
        return os.path.join(self.gt, name + ".txt")

    @staticmethod
    def _read_weights(weights, scalars):
        """The loss-meter weights that are device scalars (and, with them, the int32 scalars of the device post-processing) in
        ONE read-back: (weights as Python floats, scalars as ints)."""
        dev_w = [w.detach().double().reshape(()) for w in weights if torch.is_tensor(w)]
        parts = ([torch.stack(dev_w)] if dev_w else []) + ([scalars.double()] if scalars is not None else [])
        host = torch.cat(parts).tolist() if parts else []
        return host[:len(dev_w)], [int(v) for v in host[len(dev_w):]]

    def _upload_ids(self, ids, dev, slot="sup"):
        """Host ids -> device int64 through a pinned staging buffer and an asynchronous copy (a copy from pageable memory would
        hold the host until it is done).  One pair of buffers per `slot` (superpoint ids, ground-truth ids, ...), growing only.
        A staging buffer is written again only after the copy that last read it: the event recorded behind that copy is waited
        for first.  Every forward reads something back after the previous step's copies were enqueued, so the wait finds
        the event done; it is there for a caller whose model_fn does not."""
        ids = np.ascontiguousarray(ids).reshape(-1)
        n = int(ids.shape[0])
        st = self._staging.get(slot)
        if st is None or st[0].numel() < n or st[1].device != dev:
            st = self._staging[slot] = [torch.empty(max(n, 1), dtype=torch.int64).pin_memory(),
                                        torch.empty(max(n, 1), dtype=torch.int64, device=dev), None]
        pin, out, copied = st
        if copied is not None:
            copied.synchronize()
        pin[:n].copy_(torch.from_numpy(ids))
        out[:n].copy_(pin[:n], non_blocking=True)
        if copied is None:
            copied = st[2] = torch.cuda.Event()
        copied.record()
        return out[:n]

    def _refine_on_device(self, pred, point_num, sup, meter_dict):
        """cfg.device_post: postprocess.refine_instances_device; n_keep and the status word travel with the loss-meter weights."""
        from .postprocess import PostWorkspace, refine_instances_device
        dev = pred["sem"].device
        n_fold = point_num // 3
        n_sp = None
        if not (torch.is_tensor(sup) and sup.is_cuda):          # host ids: their bound costs no device read-back
            sup = np.asarray(sup)
            n_sp = int(sup.max()) + 1 if sup.size else 1
            sup = self._upload_ids(sup, dev)
        elif sup.dtype != torch.int64:
            sup = sup.long()
        need = (int(pred["proposals"][1].shape[0]) - 1, n_fold, n_fold if n_sp is None else n_sp)
        ws = self._post_ws
        if ws is None or ws.device != dev or not ws.fits(*need):
            grown = need if ws is None else (max(need[0], ws.n_prop), max(need[1], ws.n_fold), max(need[2], ws.n_superpoints))
            ws = self._post_ws = PostWorkspace(grown[0], grown[1], grown[2], dev)
        res = refine_instances_device(pred["sem"], pred["proposals"], pred["clt_scores"], point_num, sup, self.cfg,
                                      n_superpoints=n_sp, workspace=ws)
        if self.device_ap:                                       # cfg.device_ap: nothing is read back, _associate_on_device goes on
            return res, None
        host_w, scalars = self._read_weights([meter_dict[k][1] for k in meter_dict], res.scalars)
        return res.sliced(scalars), host_w

    def _device_gt(self, name, batch, n_fold, sem_dev, dev):
        """cfg.device_ap: the scene's ground truth as device tensors -- the id vector, or with gt=None the (sem, ins) pair of the
        first copy that pbn_gt_encode_dev turns into ids.  Host arrays go through the pinned staging path, once per scene."""
        from . import evaluate
        if self.gt is None:
            ins = batch["ins"]
            if torch.is_tensor(ins) and ins.is_cuda:
                ins = ins[:n_fold] if ins.dtype in _LABEL_DTYPES else ins[:n_fold].long()
            else:
                ins = self._upload_ids((ins.numpy() if torch.is_tensor(ins) else np.asarray(ins))[:n_fold], dev, "ins")
            sem = sem_dev.reshape(-1)[:n_fold]
            return (sem if sem.dtype in _LABEL_DTYPES else sem.long()), ins
        ids = self.gt(name) if callable(self.gt) else os.path.join(self.gt, name + ".txt")
        if isinstance(ids, (str, bytes)) or hasattr(ids, "__fspath__"):
            ids = evaluate.load_gt_ids(ids)
        if torch.is_tensor(ids) and ids.is_cuda:
            return ids if ids.dtype in _LABEL_DTYPES else ids.long()
        return self._upload_ids(ids.numpy() if torch.is_tensor(ids) else np.asarray(ids), dev, "gt")

    def _associate_on_device(self, name, refined, gt):
        """cfg.device_ap: one record of the epoch's association log; the log's work buffers follow the post-processing's."""
        from . import evaluate
        ws = self._post_ws
        if self._ap_log is None:
            self._ap_log = evaluate.AssociationLog(ws.n_prop, ws.n_fold, log_words=self._ap_log_words, device=ws.device)
        self._ap_log.append_refined(name, refined, gt)

    def _empty(self, dev):
        """cfg.device_ap: the bool [1] that holds a step's `n_keep <= 0`, allocated once."""
        if self._empty_buf is None or self._empty_buf.device != dev:
            self._empty_buf = torch.zeros(1, dtype=torch.bool, device=dev)
        return self._empty_buf

    def _meter_on_device(self, meter_dict, empty, dev):
        """cfg.device_ap: train.py:258-261 on a train_epoch.LossMeter.  `empty` (device bool [1] = `n_keep <= 0`, or None) keeps
        a scene without clusters out of the averages (train.py:217-219): term and weight both become 0 -- a NaN term times a
        zero weight would still be NaN.  Terms and weights are staged into two vectors allocated with the meter, so a step
        allocates nothing; a host number travels as a launch argument, not as a copy."""
        from .train_epoch import LossMeter
        keys = list(meter_dict)
        if self._loss_meter is None:
            self._loss_meter = LossMeter(keys, device=dev)
            self._meter_in = (torch.zeros(len(keys), dtype=torch.float32, device=dev),
                              torch.zeros(len(keys), dtype=torch.float64, device=dev))
        elif self._loss_meter.names != keys:
            raise ValueError("the logged terms changed within the epoch: %s, then %s" % (self._loss_meter.names, keys))

        terms, weights = self._meter_in
        for i, k in enumerate(keys):                            # in place: a device scalar is copied, a host number filled in
            for buf, v in ((terms, meter_dict[k][0]), (weights, meter_dict[k][1])):
                if torch.is_tensor(v) and v.is_cuda:
                    buf[i].copy_(v.detach().reshape(()))
                else:
                    buf[i].fill_(float(v))
        if empty is not None:                                   # torch.where(n_keep > 0, x, 0), in place
            terms.masked_fill_(empty, 0.0)
            weights.masked_fill_(empty, 0.0)
        self._loss_meter.update(terms, weights)

    def step(self, batch):
        from . import evaluate
        from .postprocess import refine_instances
        fn = batch.get("fn") or ["scene%04d" % self.steps]
        if len(fn) > 3:
            raise ValueError("ValidationEpoch takes one scene (3 copies) per step, as batch_size_v = 1 upstream; this batch "
                             "holds %d copies and model_fn has no n_batch keyword to tell the forward so" % len(fn))
        with torch.no_grad():
            loss, pred, visual_dict, meter_dict = self.model_fn(batch, self.model, self.epoch, self.cfg, task="eval")
            self.steps += 1
            host_w = empty = None
            # train.py:144-149
            sem_label = torch.as_tensor(batch["sem"]).to(pred["sem"].device)
            self.semantic.update(pred["sem"], sem_label if sem_label.dtype in _LABEL_DTYPES else sem_label.long())
            if self.cluster:
                # train.py:152-168
                self.mask.update(*pred["mask_scores"])
                # train.py:171-253
                name = fn[0]
                point_num = int(batch["xyz_original"].shape[0])
                if self.device_ap:
                    # the whole tail stays on the device: n_keep == 0 (train.py:217-219) is a header-only record and a closed gate
                    refined, _ = self._refine_on_device(pred, point_num, batch["sup"], meter_dict)
                    n_fold = point_num // 3
                    self._associate_on_device(name, refined, self._device_gt(name, batch, n_fold, sem_label, sem_label.device))
                    empty = torch.le(refined.n_keep.reshape(1), 0, out=self._empty(sem_label.device))
                else:
                    if self.device_post:
                        refined, host_w = self._refine_on_device(pred, point_num, batch["sup"], meter_dict)
                        clusters, scores, sem_id = refined
                    else:
                        clusters, scores, sem_id = refine_instances(pred["sem"], pred["proposals"], pred["clt_scores"],
                                                                    point_num, batch["sup"], self.cfg)
                    if clusters.shape[0] == 0:
                        # train.py:217-219: the `continue` sits ABOVE the loss-meter update (:258-261), so a scene without
                        # clusters is missing from the loss averages too; kept
                        print("no cluster")
                        self.no_cluster += 1
                        return pred
                    self.matches[name] = evaluate.assign_instances_for_scan(
                        name, dict(conf=scores, label_id=sem_id, mask=clusters), self._gt_ids(name, batch, point_num // 3))
            self.visual_keys.update(visual_dict)
            if self.device_ap:
                self._meter_on_device(meter_dict, empty, pred["sem"].device)
                # two read-backs per step are the price of the line; as in the host form, a scene without clusters logs none
                if self.progress and not (empty is not None and bool(empty)):
                    val, avg = self._loss_meter.read()["loss"]
                    self._info("iter: {} loss: {:.4f}({:.4f}) Accuracy {accuracy:.4f} ".format(
                        self.steps, val, avg, accuracy=self.semantic.accuracy_val()))
                return pred
            # train.py:258-261 on Python floats; the weights are device scalars: one read-back for all of them
            keys = list(meter_dict)
            weights = [meter_dict[k][1] for k in keys]
            if host_w is None:
                host_w = self._read_weights(weights, None)[0]
            host_w = iter(host_w)
            for k, w in zip(keys, weights):
                v = meter_dict[k][0]
                self.am_dict.setdefault(k, AverageMeter()).update(float(v), next(host_w) if torch.is_tensor(w) else float(w))
            if self.progress:
                self._info("iter: {} loss: {:.4f}({:.4f}) Accuracy {accuracy:.4f} ".format(
                    self.steps, self.am_dict["loss"].val, self.am_dict["loss"].avg, accuracy=self.semantic.accuracy_val()))
        return pred

    def finish(self):
        """train.py:269-303.  Returns one dict; on a rank other than 0 of a reduced epoch the AP keys are absent."""
        import torch.distributed as tdist
        from . import dist as pdist, evaluate
        world = tdist.get_world_size() if (tdist.is_available() and tdist.is_initialized()) else 1
        rank = tdist.get_rank() if world > 1 else 0
        table_ap = None
        if self.device_ap:
            # the epoch's two read-backs: the association log (records in step order) and the loss meter
            use_table = self.device_ap_table and self._ap_log is not None
            if use_table and world > 1:
                self._info("device_ap_table: %d ranks, matching and integration stay on the host" % world)
                use_table = False
            if use_table:
                table_ap, dropped, failed, _, _ = evaluate.ap_table_of_logs([self._ap_log])
                for scene, reasons in failed:             # as collect() raises for a record with status bits
                    raise ValueError("%s: %s" % (scene, "; ".join(reasons)))
                self.matches = None
                self.no_cluster = len(dropped)
                for _ in dropped:
                    print("no cluster")
            elif self._ap_log is not None:
                self.matches, dropped = self._ap_log.collect()
                self.no_cluster = len(dropped)
                for _ in dropped:
                    print("no cluster")
            self.am_dict = {}
            if self._loss_meter is not None and self.steps > self.no_cluster:      # no counted scene: no meter, as the host form
                _, total, count = self._loss_meter.raw().tolist()
                for k, s, c in zip(self._loss_meter.names, total, count):
                    meter = self.am_dict[k] = AverageMeter()
                    meter.sum, meter.count = s, c
        matches, am = self.matches, {k: (m.sum, m.count) for k, m in self.am_dict.items()}
        if world > 1 and self.reduce:
            self.semantic.all_reduce()
            self.mask.gather_()
            parts = [None] * world
            tdist.all_gather_object(parts, am)
            am = {}
            for part in parts:
                for k, (s, c) in part.items():
                    am[k] = (am.get(k, (0, 0))[0] + s, am.get(k, (0, 0))[1] + c)
            matches = pdist.gather_scene_results(matches)
        speaks = rank == 0
        losses = {k: (s / c if c else 0.0) for k, (s, c) in am.items()}
        out = {"epoch": self.epoch, "scenes": self.steps, "no_cluster": self.no_cluster, "losses": losses,
               "time": time.time() - self.start_time}
        if speaks and "loss" in losses:
            self._info("epoch: {}/{}, val loss: {:.4f},  time: {}s".format(self.epoch, getattr(self.cfg, "epochs", self.epoch),
                                                                          losses["loss"], out["time"]))
        sem = self.semantic.result()
        out.update(semantic=sem, mIoU=sem["mIoU"], mAcc=sem["mAcc"], allAcc=sem["allAcc"])
        scalars = [(k + "_eval", v) for k, v in losses.items() if k in self.visual_keys]
        scalars += [("val/mIOU_eval", sem["mIoU"]), ("val/mAcc_eval", sem["mAcc"]), ("val/allACC_eval", sem["allAcc"])]
        avgs = None
        if self.cluster:
            mask = self.mask.result()
            out.update(mask=mask, All_mask_acc=mask["All_mask_acc"], Tp_acc=mask["Tp_acc"], Fp_acc=mask["Fp_acc"])
            scalars += [("val/All_mask_acc", mask["All_mask_acc"]), ("val/Tp_acc", mask["Tp_acc"]), ("val/Fp_acc", mask["Fp_acc"])]
            if table_ap is not None:
                out["ap"] = table_ap                      # matches stays None: the records never came to the host
            if matches is not None or table_ap is not None:
                avgs = evaluate.compute_averages(evaluate.evaluate_matches(matches) if table_ap is None else table_ap)
                out.update(matches=matches, avgs=avgs, mAP=float(avgs["all_ap"]), AP_50=float(avgs["all_ap_50%"]),
                           AP_25=float(avgs["all_ap_25%"]))
                scalars += [("val/mAP", avgs["all_ap"]), ("val/AP_50", avgs["all_ap_50%"]), ("val/AP_25", avgs["all_ap_25%"])]
        if speaks:
            self._info(format_semantic_line(sem))
            if avgs is not None:
                evaluate.print_results(avgs, self.logger)
            if self.writer is not None:
                for tag, value in scalars:
                    self.writer.add_scalar(tag, value, self.epoch)
        return out
