"""The training epoch of /root/reference/train.py:27-120 (`cosine_lr_after_step`, `train_epoch`) on this package: the
learning-rate schedule, forward + losses through `model_fn`, backward, the gradient exchange, the optimizer step, the running
loss averages, the reference's progress and epoch lines, its tensorboard scalars and its checkpoint call.

What changes against the reference is where the averages are kept, not what is averaged: with `cfg.device_meters` model_fn
returns the logged terms and their weights as device tensors and `LossMeter` adds them up on the device in float64 (one
small launch of csrc/optim.hip per step); nothing is read back until a line is due.  With `log_every=0` that is once, in
`finish()`.  The reference also calls `torch.cuda.empty_cache()` before every step (train.py:48); this loop does not: it
returns every cached block to the driver and makes the next step allocate again."""
import math
import sys
import time

import numpy as np
import torch

from . import _native as N


def cosine_lr_after_step(optimizer, base_lr, epoch, step_epoch, total_epochs, clip=1e-6):
    """train.py:27-33: base_lr up to step_epoch, then half a cosine down to `clip` at total_epochs.  Sets every group's lr
    and returns it."""
    if epoch < step_epoch:
        lr = base_lr
    else:
        lr = clip + 0.5 * (base_lr - clip) * (1 + math.cos(math.pi * ((epoch - step_epoch) / (total_epochs - step_epoch))))
    for param_group in optimizer.param_groups:
        param_group["lr"] = lr
    return lr


class LossMeter(object):
    """tools/log.py:16-30 (AverageMeter) for k named terms at once, in float64: acc[3k] = val | sum | count with
    val = term, sum += term * weight, count += weight.  On the device (the default) `update` takes a float32 [k] tensor of
    terms and a [k] tensor of weights and is one launch without synchronisation; `read()` is the one read-back.  With
    device="cpu" the terms and weights are host numbers and the same three float64 operations run in numpy."""

    def __init__(self, names, device=None):
        self.names = list(names)
        k = len(self.names)
        self.host = device is not None and torch.device(device).type == "cpu"
        if self.host:
            self._acc = np.zeros(3 * k, np.float64)
        else:
            self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
            self._acc = torch.zeros(3 * k, dtype=torch.float64, device=self.device)
        self.updates = 0

    def update(self, terms, weights):
        k = len(self.names)
        if self.host:
            v = np.array([float(x) for x in terms], np.float64)
            w = np.array([float(x) for x in weights], np.float64)
            assert v.shape == (k,) and w.shape == (k,)
            self._acc[:k] = v
            self._acc[k:2 * k] = self._acc[k:2 * k] + v * w
            self._acc[2 * k:] = self._acc[2 * k:] + w
        else:
            N.require_cuda(terms, weights)
            if terms.dtype != torch.float32 or terms.numel() != k or weights.numel() != k:
                raise ValueError("LossMeter.update takes %d float32 terms and %d weights, got %s %s and %s" %
                                 (k, k, terms.dtype, tuple(terms.shape), tuple(weights.shape)))
            t = terms.detach().reshape(-1).contiguous()
            w = weights.detach().reshape(-1).to(torch.float64).contiguous()
            N.check(N.lib().pbn_loss_meter_update(N.ptr(t), N.ptr(w), N.ptr(self._acc), k, N.current_stream()),
                    "pbn_loss_meter_update")
        self.updates += 1

    def raw(self):
        """float64 [3, k] on the host: val, sum, count.  One read-back."""
        acc = self._acc if self.host else self._acc.cpu().numpy()
        return np.array(acc, np.float64).reshape(3, len(self.names))

    def read(self):
        """{name: (val, avg)} with avg = sum / count (0 before the first weight), as AverageMeter.  One read-back."""
        val, total, count = self.raw().tolist()
        return {n: (v, s / c if c else 0.0) for n, v, s, c in zip(self.names, val, total, count)}


class _Clock(object):
    """AverageMeter of a duration (train.py:40-41)."""

    def __init__(self):
        self.val = self.sum = self.avg = 0.0
        self.count = 0

    def update(self, val):
        self.val = val
        self.sum += val
        self.count += 1
        self.avg = self.sum / self.count


def format_remain(seconds):
    """train.py:73-75."""
    t_m, t_s = divmod(seconds, 60)
    t_h, t_m = divmod(t_m, 60)
    return "{:02d}:{:02d}:{:02d}".format(int(t_h), int(t_m), int(t_s))


def format_progress_line(epoch, epochs, it, n_iters, meters, batch_time, iter_time, remain_time, clustered):
    """train.py:77-90; `meters` = {name: (val, avg)}, the two times = (val, avg); `clustered` = epoch > cfg.cluster_epoch."""
    if not clustered:
        return ("epoch: {}/{} iter: {}/{} loss: {:.4f}({:.4f})  data_time: {:.2f}({:.2f}) "
                "iter_time: {:.2f}({:.2f}) remain_time: {remain_time}\n"
                .format(epoch, epochs, it, n_iters, meters["loss"][0], meters["loss"][1], batch_time[0], batch_time[1],
                        iter_time[0], iter_time[1], remain_time=remain_time))
    return ("epoch: {}/{} iter: {}/{} loss: {:.4f}({:.4f})  mask_loss: {:.4f}({:.4f})   "
            " data_time: {:.2f}({:.2f}) iter_time: {:.2f}({:.2f}) remain_time: {remain_time}\n"
            .format(epoch, epochs, it, n_iters, meters["loss"][0], meters["loss"][1], meters["mask_loss"][0],
                    meters["mask_loss"][1], batch_time[0], batch_time[1], iter_time[0], iter_time[1], remain_time=remain_time))


def format_epoch_line(epoch, epochs, averages, seconds, clustered):
    """train.py:102-107."""
    if not clustered:
        return "epoch: {}/{}, train loss: {:.4f},  time: {}s".format(epoch, epochs, averages["loss"], seconds)
    return "epoch: {}/{}, train loss: {:.4f}, mask_loss: {:.4f},  time: {}s".format(epoch, epochs, averages["loss"],
                                                                                     averages["mask_loss"], seconds)


def _default_model_fn(*a, **kw):
    from .network.PBNet import model_fn
    return model_fn(*a, **kw)


class TrainEpoch(object):
    """train.py:36-120 against this package: `step(batch)` once per batch of the loader, then `finish()`.

    `model_fn` is called as model_fn(batch, model, epoch, cfg, task='train') and may be wrapped by the caller.  `reducer`: a
    dist.GradientReducer whose hooks exchange the gradients during backward; its `finish()` is waited for before the optimizer
    step.  `n_iters` = len(train_loader) (the progress line and the remaining time need it).  The lines go to sys.stdout
    (progress) and `logger.info` (epoch, checkpoint; print without a logger) on rank 0 only: `cfg.dist` false, or
    `cfg.local_rank == 0`.  `log_every`: a progress line, hence a read-back of the meters, every that many iterations; 0 =
    none, the meters are read in `finish()` only.  The learning-rate scalar is written once, not once per term as train.py:115
    does."""

    def __init__(self, model, cfg, epoch, optimizer, n_iters, model_fn=None, reducer=None, logger=None, writer=None, log_every=1,
                 save=True):
        self.model, self.cfg, self.epoch, self.optimizer = model, cfg, int(epoch), optimizer
        self.n_iters = int(n_iters)
        self.model_fn = _default_model_fn if model_fn is None else model_fn
        self.reducer, self.logger, self.writer, self.log_every, self.save = reducer, logger, writer, int(log_every), save
        self.clustered = self.epoch > cfg.cluster_epoch
        self.speaks = (not getattr(cfg, "dist", False)) or getattr(cfg, "local_rank", 0) == 0
        self.meter, self.visual_keys = None, set()
        self.steps = 0
        model.train()
        self.iter_time, self.batch_time = _Clock(), _Clock()
        self.start_time = time.time()
        self.end_time = time.time()

    def _info(self, line):
        (print if self.logger is None else self.logger.info)(line)

    def _update_meters(self, meter_dict):
        keys = list(meter_dict)
        values = [meter_dict[k][0] for k in keys]
        weights = [meter_dict[k][1] for k in keys]
        on_device = bool(values) and all(torch.is_tensor(v) and v.is_cuda for v in values)
        if self.meter is None:
            self.meter = LossMeter(keys, device=None if on_device else "cpu")
        if self.meter.names != keys or self.meter.host == on_device:
            raise ValueError("model_fn changed its meter terms within an epoch: %s, then %s" % (self.meter.names, keys))
        if on_device:
            dev = values[0].device
            w = torch.stack([(x if torch.is_tensor(x) else torch.tensor(float(x), device=dev)).detach().reshape(()).double()
                             for x in weights])
            self.meter.update(torch.stack([v.detach().float().reshape(()) for v in values]), w)
        else:
            # train.py:62-65 on Python floats; weights that are device scalars come back in ONE read-back
            dev_w = [x.detach().double().reshape(()) for x in weights if torch.is_tensor(x)]
            host_w = iter(torch.stack(dev_w).tolist() if dev_w else [])
            self.meter.update([float(v) for v in values], [next(host_w) if torch.is_tensor(x) else float(x) for x in weights])

    def step(self, batch):
        cfg = self.cfg
        self.batch_time.update(time.time() - self.end_time)
        cosine_lr_after_step(self.optimizer, cfg.lr, self.epoch, cfg.step_epoch, cfg.epochs, clip=1e-6)
        loss, _, visual_dict, meter_dict = self.model_fn(batch, self.model, self.epoch, cfg, task="train")
        self.optimizer.zero_grad(set_to_none=True)
        loss.backward()
        if self.reducer is not None:
            self.reducer.finish()
        self.optimizer.step()
        self._update_meters(meter_dict)
        self.visual_keys.update(visual_dict)
        i = self.steps
        self.steps += 1
        # train.py:67-75
        current_iter = (self.epoch - 1) * self.n_iters + i + 1
        max_iter = cfg.epochs * self.n_iters
        remain_iter = max_iter - current_iter
        self.iter_time.update(time.time() - self.end_time)
        self.end_time = time.time()
        if self.speaks and self.log_every > 0 and (i + 1) % self.log_every == 0:
            remain_time = format_remain(remain_iter * self.iter_time.avg)
            sys.stdout.write(format_progress_line(self.epoch, cfg.epochs, i + 1, self.n_iters, self.meter.read(),
                                                  (self.batch_time.val, self.batch_time.avg),
                                                  (self.iter_time.val, self.iter_time.avg), remain_time, self.clustered))
            if i == self.n_iters - 1:
                print()
        return loss

    def finish(self):
        """train.py:101-119.  Returns {term: average} (0.0 for `loss` / `mask_loss` when no step ran)."""
        from . import checkpoint
        averages = {k: avg for k, (_, avg) in (self.meter.read() if self.meter is not None else {}).items()}
        averages.setdefault("loss", 0.0)
        if self.clustered:
            averages.setdefault("mask_loss", 0.0)
        if self.speaks:
            self._info(format_epoch_line(self.epoch, self.cfg.epochs, averages, time.time() - self.start_time, self.clustered))
            if self.writer is not None:
                logged = [k for k in (self.meter.names if self.meter is not None else []) if k in self.visual_keys]
                for k in logged:
                    self.writer.add_scalar(k + "_train", averages[k], self.epoch)
                if logged:
                    self.writer.add_scalar("train/learning_rate", self.optimizer.param_groups[0]["lr"], self.epoch)
            if self.save:
                pretrain_file = checkpoint.checkpoint_save(self.model, self.optimizer, self.cfg.logpath, self.epoch,
                                                           self.cfg.save_freq)
                self._info("Saving {}".format(pretrain_file))
        return averages
