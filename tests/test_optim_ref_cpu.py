"""CPU tier of the training epoch: the numpy float32 restatement of csrc/optim.hip's contract (tests/optim_ref.py) against
torch.optim on float64 twins, state-dict round trips between pbnet_amd.optim.Adam and torch.optim.Adam, and
pbnet_amd/train_epoch.py (schedule, meters, lines, scalars, checkpoint call) against what the reference's own train.py and
tools/log.py produced for the same inputs (tests/golden/make_train_golden.py -> train_lr.json, train_meter.json,
train_lines.json)."""
import io
import json
import os
import types
from contextlib import redirect_stdout

import numpy as np
import pytest
import torch

import optim_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
SHAPES = [(7,), (33, 5), (4, 3, 2), (1,), (130,)]
STEPS = 20
ABSENT = (2, range(5, 10))          # parameter 2 has no gradient on steps 5-9 (0-based)
LR = 1e-3
# The largest relative gap (optim_ref.relative_gap over parameters and state after 20 steps) between the float32 restatement
# and torch.optim on float64 twins, measured with the gradients of seed 5 below, weight decay 0 and 1e-2:
#     Adam  2.357e-07      AdamW  9.482e-07 (weight decay 1e-2; 2.357e-07 without)      SGD  2.673e-07
# The assertion allows 4 x that: the margin covers other seeds, not other arithmetic.
MEASURED_GAP = {"Adam": 2.357e-07, "AdamW": 9.482e-07, "SGD": 2.673e-07}


def problem(seed=5):
    rng = np.random.default_rng(seed)
    params = [rng.standard_normal(s).astype(np.float32) for s in SHAPES]
    grads = [[rng.standard_normal(s).astype(np.float32) for s in SHAPES] for _ in range(STEPS)]
    for t in ABSENT[1]:
        grads[t][ABSENT[0]] = None
    return params, grads


def hyper(rule, weight_decay):
    return dict(lr=LR, weight_decay=weight_decay, **({"momentum": 0.9} if rule == "SGD" else {"betas": (0.9, 0.99)}))


def run_twin(rule, params, grads, weight_decay):
    """torch.optim on float64 copies of the float32 problem: (parameters, state0, state1) as float64 arrays."""
    twins = [torch.nn.Parameter(torch.from_numpy(p.astype(np.float64))) for p in params]
    opt = R.torch_twin(rule, twins, **hyper(rule, weight_decay))
    for step in grads:
        for p, g in zip(twins, step):
            p.grad = None if g is None else torch.from_numpy(g.astype(np.float64))
        opt.step()
    names = ("momentum_buffer", None) if rule == "SGD" else ("exp_avg", "exp_avg_sq")
    state = [[opt.state[p][n].numpy() if n else None for p in twins] for n in names]
    return [p.detach().numpy() for p in twins], state[0], state[1], opt


def gaps(rule, weight_decay, seed=5):
    params, grads = problem(seed)
    ref = R.RefOptimizer(rule, params, **hyper(rule, weight_decay))
    for step in grads:
        ref.step(step)
    p64, s0, s1, opt = run_twin(rule, params, grads, weight_decay)
    out = [R.relative_gap(a, b) for a, b in zip(ref.p, p64)] + [R.relative_gap(a, b) for a, b in zip(ref.s0, s0)]
    if rule != "SGD":
        out += [R.relative_gap(a, b) for a, b in zip(ref.s1, s1)]
        assert ref.t == [int(opt.state[p]["step"]) for p in opt.param_groups[0]["params"]] == [20, 20, 15, 20, 20]
    return max(out)


@pytest.mark.parametrize("rule", ["Adam", "AdamW", "SGD"])
@pytest.mark.parametrize("weight_decay", [0.0, 1e-2])
def test_restatement_against_torch_float64(rule, weight_decay):
    gap = gaps(rule, weight_decay)
    print("%s weight_decay %g: relative gap %.3e (bound %.3e)" % (rule, weight_decay, gap, 4 * MEASURED_GAP[rule]))
    assert gap <= 4 * MEASURED_GAP[rule]


def test_restatement_rounds_every_operation_to_float32():
    """The restatement is not float64 in disguise: it differs from the float64 twin by about one float32 rounding, and a
    zero gradient on a zero state moves nothing (d = eps, m = 0)."""
    assert gaps("Adam", 0.0) > 1e-9
    p, m, v = R.adam_step(np.ones(3, np.float32), np.zeros(3, np.float32), np.zeros(3, np.float32), np.zeros(3, np.float32), LR,
                          (0.9, 0.999), 1e-8, 0.0, 1, False)
    assert np.array_equal(p, np.ones(3, np.float32)) and not m.any() and not v.any()


# ---- state dicts ------------------------------------------------------------------------------------------------------------------
def _params(seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter(torch.randn(s, generator=g)) for s in SHAPES]


def _torch_steps(opt, params, steps, seed, skip=None):
    g = torch.Generator().manual_seed(seed)
    for _ in range(steps):
        for i, p in enumerate(params):
            grad = torch.randn(p.shape, generator=g)
            p.grad = None if i == skip else grad
        opt.step()


def test_state_dict_round_trips_with_torch_adam():
    """torch.optim.Adam -> pbnet_amd.optim.Adam -> torch.optim.Adam on CPU tensors (the dict logic needs no library): the
    tensors land in the flat buffers as views, come out with torch's keys, and a torch optimizer that loads them continues
    exactly as the one that never stopped.  Parameter 1 never had a gradient: it has no state on either side."""
    from pbnet_amd import optim as O
    a = _params(1)
    t_a = torch.optim.Adam(a, lr=LR, weight_decay=1e-2)
    _torch_steps(t_a, a, 3, 7, skip=1)
    saved = t_a.state_dict()

    b = [torch.nn.Parameter(p.detach().clone()) for p in a]
    mine = O.Adam(b, lr=5e-2)
    mine.load_state_dict(saved)
    assert mine.param_groups[0]["lr"] == LR and mine.param_groups[0]["weight_decay"] == 1e-2
    for i, p in enumerate(b):
        if i == 1:
            assert not mine.state.get(p)
            continue
        st = mine.state[p]
        assert float(st["step"]) == 3.0 and not st["step"].is_cuda
        for k, name in enumerate(("exp_avg", "exp_avg_sq")):
            assert torch.equal(st[name], t_a.state[a[i]][name]) and st[name].shape == p.shape
            base = mine._flat[k]
            assert st[name].untyped_storage().data_ptr() == base.untyped_storage().data_ptr()      # a view of the flat buffer
            assert (st[name].data_ptr() - base.data_ptr()) % 16 == 0                               # on a 16-byte boundary
    out = mine.state_dict()
    assert out["param_groups"][0].keys() == saved["param_groups"][0].keys()
    assert out["state"].keys() == saved["state"].keys()
    for k, st in saved["state"].items():
        assert out["state"][k].keys() == st.keys()
        for name, v in st.items():
            assert torch.equal(out["state"][k][name], v), (k, name)

    # and back: through torch.save / torch.load into a fresh torch optimizer that then steps in lockstep with the original
    buf = io.BytesIO()
    torch.save(out, buf)
    buf.seek(0)
    c = [torch.nn.Parameter(p.detach().clone()) for p in a]
    t_c = torch.optim.Adam(c, lr=9.0)
    t_c.load_state_dict(torch.load(buf))
    _torch_steps(t_a, a, 2, 11)
    _torch_steps(t_c, c, 2, 11)
    for p, q in zip(a, c):
        assert torch.equal(p, q)


def test_state_dict_of_own_state_survives_reload():
    """Loading the optimizer's own state_dict (whose tensors ARE the views) must not destroy it."""
    from pbnet_amd import optim as O
    b = _params(2)
    mine = O.Adam(b, lr=LR)
    t = torch.optim.Adam([torch.nn.Parameter(p.detach().clone()) for p in b], lr=LR)
    _torch_steps(t, t.param_groups[0]["params"], 2, 3)
    mine.load_state_dict(t.state_dict())
    before = {k: {n: v.clone() for n, v in st.items()} for k, st in mine.state_dict()["state"].items()}
    mine.load_state_dict(mine.state_dict())
    after = mine.state_dict()["state"]
    for k, st in before.items():
        for n, v in st.items():
            assert torch.equal(after[k][n], v)


def test_constructor_errors_and_build_optimizer():
    from pbnet_amd import optim as O
    with pytest.raises(TypeError, match="bfloat16"):
        O.Adam([torch.nn.Parameter(torch.zeros(4, dtype=torch.bfloat16))])
    ps = _params(3)
    ps[2].requires_grad_(False)
    cfg = types.SimpleNamespace(optimizer="AdamW", lr=2e-3, momentum=0.8, weight_decay=1e-4)
    for native, module in ((True, "pbnet_amd.optim"), (False, "torch.optim")):
        opt = O.build_optimizer(cfg, ps, native=native)
        assert type(opt).__name__ == "AdamW" and type(opt).__module__.startswith(module)
        g = opt.param_groups[0]
        assert (g["lr"], tuple(g["betas"]), g["weight_decay"], len(g["params"])) == (2e-3, (0.9, 0.99), 1e-4, len(ps) - 1)
    cfg.optimizer = "SGD"
    g = O.build_optimizer(cfg, ps, native=True).param_groups[0]
    assert (g["lr"], g["momentum"], g["weight_decay"], g["dampening"], g["nesterov"]) == (2e-3, 0.8, 1e-4, 0, False)
    cfg.optimizer = "Adam"
    g = O.build_optimizer(cfg, ps, native=True).param_groups[0]
    assert (g["lr"], tuple(g["betas"]), g["eps"], g["weight_decay"]) == (2e-3, (0.9, 0.999), 1e-8, 0)
    cfg.native_optimizer = True
    assert type(O.build_optimizer(cfg, ps)).__module__ == "pbnet_amd.optim"
    cfg.optimizer = "RMSprop"
    with pytest.raises(ValueError):
        O.build_optimizer(cfg, ps)
    with pytest.raises(RuntimeError):                      # no CPU path for the step itself
        opt = O.Adam(_params(4))
        for p in opt.param_groups[0]["params"]:
            p.grad = torch.zeros_like(p)
        opt.step()


# ---- schedule, meters, lines ------------------------------------------------------------------------------------------------------
def _golden(name):
    with open(os.path.join(HERE, "golden", name)) as f:
        return json.load(f)


def test_cosine_lr_after_step_against_reference():
    from pbnet_amd.train_epoch import cosine_lr_after_step
    tables = _golden("train_lr.json")
    assert [(t["step_epoch"], t["epochs"]) for t in tables] == [(50, 520), (3, 10)]
    for t in tables:
        opt = types.SimpleNamespace(param_groups=[{"lr": None}, {"lr": None}])
        assert len(t["lr"]) == t["epochs"] + 1
        for epoch, want in enumerate(t["lr"]):
            got = cosine_lr_after_step(opt, t["base_lr"], epoch, t["step_epoch"], t["epochs"], clip=t["clip"])
            assert got == want == opt.param_groups[0]["lr"] == opt.param_groups[1]["lr"], (epoch, got, want)
        assert t["lr"][0] == t["base_lr"] and t["lr"][-1] == t["clip"]


def test_host_loss_meter_against_average_meter():
    """LossMeter(device='cpu') is AverageMeter's three float64 operations: equal to the recorded results, not merely close."""
    from pbnet_amd.train_epoch import LossMeter
    g = _golden("train_meter.json")
    meter = LossMeter(g["names"], device="cpu")
    for terms, weights, want in zip(g["terms"], g["weights"], g["after"]):
        meter.update(terms, weights)
        val, total, count = meter.raw().tolist()
        assert (val, total, count) == (want["val"], want["sum"], want["count"])
        assert [meter.read()[n] for n in g["names"]] == list(zip(want["val"], want["avg"]))
    assert max(max(w) for w in g["weights"]) == 3e5 and len(g["terms"]) == 6 and len(g["names"]) == 5


class _Recorder(object):
    def __init__(self):
        self.lines, self.scalars = [], []

    def info(self, line):
        self.lines.append(str(line))

    def add_scalar(self, tag, value, step):
        self.scalars.append([tag, float(value), int(step)])


@pytest.mark.parametrize("case", range(4))
def test_train_epoch_lines_against_reference(case, tmp_path, monkeypatch):
    """TrainEpoch on the CPU with stand-ins (a one-layer model, torch's SGD, a model_fn that hands out the recorded terms as
    host floats, the recorded clock) prints, logs and writes what the reference's train_epoch did for the same inputs: the
    progress lines in both cluster_epoch branches, the epoch line, the scalars, the checkpoint file and its line; a rank
    other than 0 stays silent."""
    from pbnet_amd import train_epoch as T
    c = _golden("train_lines.json")[case]
    cfg = types.SimpleNamespace(logpath=str(tmp_path) + "/", **c["cfg"])
    model = torch.nn.Linear(3, 1)
    optimizer = torch.optim.SGD(model.parameters(), lr=123.0)
    rows = iter(c["steps"])

    def model_fn(batch, model, epoch, cfg, task="train"):
        row = next(rows)
        assert task == "train" and model.training
        loss = model(torch.ones(1, 3)).sum()
        return loss, None, {k: v[0] for k, v in row.items()}, {k: (v[0], v[1]) for k, v in row.items()}

    ticks = iter(c["clock"])
    monkeypatch.setattr(T, "time", types.SimpleNamespace(time=lambda: next(ticks)))
    rec = _Recorder()
    out = io.StringIO()
    with redirect_stdout(out):
        ep = T.TrainEpoch(model, cfg, c["epoch"], optimizer, c["n_iters"], model_fn=model_fn, logger=rec, writer=rec, log_every=1)
        for _ in range(c["n_iters"]):
            ep.step(None)
            assert all(p.grad is not None for p in model.parameters())
        averages = ep.finish()
    speaks = not c["cfg"]["dist"] or c["cfg"]["local_rank"] == 0
    assert out.getvalue() == c["stdout"]
    assert rec.lines == [line.replace("{logpath}", cfg.logpath) for line in c["logged"]]
    assert bool(out.getvalue()) == bool(rec.lines) == speaks
    # the reference repeats the learning-rate scalar once per term (train.py:115); here it is written once
    want = []
    for s in c["scalars"]:
        if s not in want:
            want.append(s)
    assert sorted(rec.scalars) == sorted(want) and len(rec.scalars) == len({s[0] for s in rec.scalars})
    assert optimizer.param_groups[0]["lr"] == c["lr_after"]
    assert os.path.isfile(cfg.logpath + "%09d.pth" % c["epoch"]) == speaks
    # the averages are AverageMeter's
    for k in c["names"]:
        total = sum(r[k][0] * r[k][1] for r in c["steps"])
        count = sum(r[k][1] for r in c["steps"])
        assert abs(averages[k] - total / count) <= 1e-12 * abs(total / count)
    assert ("mask_loss" in c["stdout"]) == (c["epoch"] > c["cfg"]["cluster_epoch"] and speaks)


def test_train_epoch_without_steps_and_without_logging(tmp_path):
    from pbnet_amd import train_epoch as T
    cfg = types.SimpleNamespace(logpath=str(tmp_path) + "/", lr=1e-3, step_epoch=4, epochs=12, cluster_epoch=8, save_freq=4)
    model = torch.nn.Linear(3, 1)
    rec = _Recorder()
    ep = T.TrainEpoch(model, cfg, 9, torch.optim.SGD(model.parameters(), lr=1.0), 0, logger=rec, writer=rec, log_every=0, save=False)
    assert ep.finish() == {"loss": 0.0, "mask_loss": 0.0}
    assert len(rec.lines) == 1 and rec.lines[0].startswith("epoch: 9/12, train loss: 0.0000, mask_loss: 0.0000,  time: ")
    assert rec.scalars == [] and not os.listdir(str(tmp_path))
    assert T.format_remain(3 * 3600 + 62.9) == "03:01:02"
