#!/usr/bin/env python3
"""Golden values for the training epoch (pbnet_amd/train_epoch.py), produced IN THE BUILD CONTAINER by the reference's own
code: `train.cosine_lr_after_step`, `train.train_epoch` and `tools.log.AverageMeter` are imported from /root/reference and
RUN.  train.py imports tensorboardX, which is absent here: this process registers an empty stand-in module under that name
before the import (train_epoch only calls `writer.add_scalar`, on the recording object below).

    python tests/golden/make_train_golden.py         # writes tests/golden/train_lr.json, train_lines.json, train_meter.json

train_epoch runs whole, on the CPU, with stand-ins for what it is handed: a loader that is a list, a one-parameter model, a
model_fn that returns the recorded terms, torch's SGD, a logger and a writer that record their calls, and a clock (the
module's `time`) that returns a fixed list of instants, so that the printed durations are data too.  Only data is written:
the inputs (terms, weights, instants) and what the reference printed, logged and wrote for them."""
import io
import json
import os
import sys
import tempfile
import types
from contextlib import redirect_stdout

import numpy as np
import torch

sys.path.insert(0, "/root/reference")
sys.modules.setdefault("tensorboardX", types.SimpleNamespace(SummaryWriter=object))
import train as R                                        # noqa: E402  (reference code, executed here only)
from tools.log import AverageMeter                       # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))


def lr_table():
    out = []
    for base_lr, step_epoch, epochs in ((0.001, 50, 520), (0.01, 3, 10)):
        opt = types.SimpleNamespace(param_groups=[{"lr": None}, {"lr": None}])
        values = []
        for epoch in range(epochs + 1):
            R.cosine_lr_after_step(opt, base_lr, epoch, step_epoch, epochs, clip=1e-6)
            assert opt.param_groups[0]["lr"] == opt.param_groups[1]["lr"]
            values.append(opt.param_groups[0]["lr"])
        out.append({"base_lr": base_lr, "step_epoch": step_epoch, "epochs": epochs, "clip": 1e-6, "lr": values})
    return out


def meter_table(rng):
    """Six steps of five terms (float32 values, as model_fn's terms are) with weights up to 3e5, through AverageMeter in
    float64."""
    names = ["loss", "semantic_loss", "offset_norm_loss", "offset_dir_loss", "mask_loss"]
    terms = (rng.random((6, 5)) * np.array([4.0, 2.5, 0.7, 1.0, 0.9])).astype(np.float32)
    terms[:, 3] *= -1.0                                   # the direction term is negative
    weights = np.floor(rng.random((6, 5)) * 3e5)
    weights[:, :4] = weights[:, :1]                       # the four point terms share the count of valid points
    weights[2, 4] = 0.0                                   # a step without mask rows
    weights[5, 0:4] = 3e5
    meters = [AverageMeter() for _ in names]
    after = []
    for t, w in zip(terms, weights):
        for m, v, n in zip(meters, t, w):
            m.update(float(v), float(n))
        after.append({"val": [m.val for m in meters], "sum": [m.sum for m in meters], "count": [m.count for m in meters],
                      "avg": [m.avg for m in meters]})
    return {"names": names, "terms": [[float(x) for x in row] for row in terms], "weights": weights.tolist(), "after": after}


class Recorder(object):
    def __init__(self):
        self.lines, self.scalars = [], []

    def info(self, line):
        self.lines.append(str(line))

    def add_scalar(self, tag, value, step):
        self.scalars.append([tag, float(value), int(step)])


def epoch_case(rng, epoch, cluster_epoch, n_iters, dist, local_rank=0):
    names = ["loss", "semantic_loss", "offset_norm_loss", "offset_dir_loss"] + (["mask_loss"] if epoch > cluster_epoch else [])
    steps = []
    for _ in range(n_iters):
        n_valid = float(rng.integers(1000, 200000))
        row = {k: [float(np.float32(rng.random() * 3)), n_valid] for k in names}
        if "mask_loss" in row:
            row["mask_loss"][1] = float(rng.integers(100, 90000))
        steps.append(row)
    clock = np.cumsum(np.round(rng.random(2 + 3 * n_iters + 1) * 1.7 + 0.004, 3)) + 1000.0
    clock = [float(np.round(c, 3)) for c in clock]
    tmp = tempfile.mkdtemp()
    cfg = types.SimpleNamespace(lr=0.001, step_epoch=4, epochs=12, cluster_epoch=cluster_epoch, dist=dist, local_rank=local_rank,
                                logpath=tmp + "/", save_freq=4)
    model = torch.nn.Linear(3, 1)
    optimizer = torch.optim.SGD(model.parameters(), lr=cfg.lr)
    it = iter(steps)

    def model_fn(batch, model, epoch, cfg, task="train"):
        row = next(it)
        loss = model(torch.ones(1, 3)).sum()
        visual = {k: v[0] for k, v in row.items()}
        return loss, None, visual, {k: (v[0], v[1]) for k, v in row.items()}

    ticks = iter(clock)
    rec = Recorder()
    R.cfg, R.logger, R.writer = cfg, rec, rec
    R.time = types.SimpleNamespace(time=lambda: next(ticks))
    out = io.StringIO()
    with redirect_stdout(out):
        R.train_epoch([None] * n_iters, model, model_fn, optimizer, epoch)
    speaks = not dist or local_rank == 0                  # the other ranks do not take the epoch line's instant
    assert len(list(ticks)) == (0 if speaks else 1), "the clock list does not match the reference's calls"
    return {"epoch": epoch, "n_iters": n_iters,
            "cfg": {k: v for k, v in vars(cfg).items() if k != "logpath"}, "names": names, "steps": steps, "clock": clock,
            "stdout": out.getvalue(), "logged": [line.replace(tmp + "/", "{logpath}") for line in rec.lines],
            "scalars": rec.scalars, "lr_after": optimizer.param_groups[0]["lr"]}


def main():
    rng = np.random.default_rng(27)
    with open(os.path.join(HERE, "train_lr.json"), "w") as f:
        json.dump(lr_table(), f)
    with open(os.path.join(HERE, "train_meter.json"), "w") as f:
        json.dump(meter_table(rng), f)
    cases = [epoch_case(rng, 3, 8, 4, False), epoch_case(rng, 9, 8, 3, False), epoch_case(rng, 9, 8, 2, True, 0),
             epoch_case(rng, 9, 8, 2, True, 1)]
    with open(os.path.join(HERE, "train_lines.json"), "w") as f:
        json.dump(cases, f, indent=1)
    for name in ("train_lr.json", "train_meter.json", "train_lines.json"):
        print(name, os.path.getsize(os.path.join(HERE, name)), "bytes")
    print(cases[0]["stdout"] + cases[1]["stdout"], cases[1]["logged"])


if __name__ == "__main__":
    main()
