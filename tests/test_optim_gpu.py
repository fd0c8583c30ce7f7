"""GPU tier: the multi-tensor step kernels of csrc/optim.hip (through pbnet_amd.optim) against the numpy float32
restatement of their contract (tests/optim_ref.py) BIT FOR BIT, their closeness to torch.optim on float64 twins (the bound
measured in tests/test_optim_ref_cpu.py; not re-measured here, the kernel equals the restatement), the launches and uploads
of a steady step, the error paths, and pbn_loss_meter_update against float64 sums and the reference's AverageMeter."""
import json
import os

import numpy as np
import pytest
import torch

import optim_ref as R
from test_optim_ref_cpu import MEASURED_GAP

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HERE = os.path.dirname(os.path.abspath(__file__))
LR = 1e-3
NO_GRAD, LATE, EMPTY = 9, 10, 11            # indices of the special parameters
LATE_FROM = 2                               # the late parameter's gradient first appears at step 3 (0-based 2)


class Problem(object):
    """Parameters of 1, 3, 4, 5, 17, C-1, C, C+1, 2C+7 elements (C = pbn_optim_chunk()), one that never has a gradient, one
    whose gradient first appears at step 3 and an empty one.  The gradients are views of ONE flat buffer at element offsets
    0 (even parameters) and 1 (odd parameters) modulo 4, so that some chunks are 16-byte aligned and some are not; values
    include zeros, denormal-sized gradients (1e-40) and elements whose gradient is zero in every step."""

    def __init__(self, seed=3):
        from pbnet_amd import _native as N
        self.C = C = N.lib().pbn_optim_chunk()
        self.sizes = [1, 3, 4, 5, 17, C - 1, C, C + 1, 2 * C + 7, 6, 9, 0]
        rng = np.random.default_rng(seed)
        self.init = [rng.standard_normal(n).astype(np.float32) for n in self.sizes]
        self.offsets, at = [], 0
        for k, n in enumerate(self.sizes):
            at = -(-at // 4) * 4 + (k % 2)
            self.offsets.append(at)
            at += n
        self.total = at
        self.steps = []
        for s in range(5):
            gs = []
            for k, n in enumerate(self.sizes):
                g = (rng.standard_normal(n) * 10.0 ** rng.integers(-3, 2)).astype(np.float32)
                g[::7] = 0.0                              # zero in every step: m = v = 0, d = eps, the update is exactly 0
                g[3::11] = np.float32(1e-40)              # denormal-sized: g * g underflows to 0
                if n > 5:
                    g[5] = 0.0 if s < 3 else g[5]         # zero at first, then not
                gs.append(g)
            self.steps.append(gs)

    def grads_of_step(self, s):
        return [None if k == NO_GRAD or (k == LATE and s < LATE_FROM) else g for k, g in enumerate(self.steps[s])]


@pytest.fixture(scope="module")
def problem():
    return Problem()


def _make(rule, weight_decay, params):
    from pbnet_amd import optim as O
    if rule == "SGD":
        return O.SGD(params, lr=LR, momentum=0.9, weight_decay=weight_decay)
    return (O.AdamW if rule == "AdamW" else O.Adam)(params, lr=LR, betas=(0.9, 0.99), weight_decay=weight_decay)


def _hyper(rule, weight_decay):
    return dict(lr=LR, weight_decay=weight_decay, **({"momentum": 0.9} if rule == "SGD" else {"betas": (0.9, 0.99)}))


def _run(rule, weight_decay, pr, check_at=(1, 2, 5)):
    params = [torch.nn.Parameter(torch.from_numpy(a.copy()).to(DEV)) for a in pr.init]
    opt = _make(rule, weight_decay, params)
    flat = torch.zeros(pr.total + 4, device=DEV)
    assert flat.data_ptr() % 16 == 0
    views = [flat[o:o + n] for o, n in zip(pr.offsets, pr.sizes)]
    ref = R.RefOptimizer(rule, pr.init, **_hyper(rule, weight_decay))
    names = ("momentum_buffer",) if rule == "SGD" else ("exp_avg", "exp_avg_sq")
    launches, uploads = [], []
    for s in range(5):
        grads = pr.grads_of_step(s)
        host = np.zeros(pr.total + 4, np.float32)
        for o, g in zip(pr.offsets, grads):
            if g is not None:
                host[o:o + g.shape[0]] = g
        flat.copy_(torch.from_numpy(host))
        for p, v, g in zip(params, views, grads):
            p.grad = None if g is None else v
        opt.step()
        ref.step(grads)
        launches.append(opt.launches_last_step)
        uploads.append(opt.table_uploads)
        if s + 1 in check_at:
            for k, p in enumerate(params):
                assert torch.equal(p.detach().cpu(), torch.from_numpy(ref.p[k])), (rule, weight_decay, s + 1, k, "p")
                if ref.s0[k] is None:
                    assert not opt.state.get(p), (k, "a parameter without a gradient has no state")
                    continue
                st = opt.state[p]
                for name, want in zip(names, (ref.s0[k], ref.s1[k])):
                    assert torch.equal(st[name].cpu(), torch.from_numpy(want)), (rule, weight_decay, s + 1, k, name)
                if rule != "SGD":
                    assert float(st["step"]) == ref.t[k] and not st["step"].is_cuda
    return params, opt, ref, views, launches, uploads


@pytest.mark.parametrize("rule", ["Adam", "AdamW", "SGD"])
@pytest.mark.parametrize("weight_decay", [0.0, 1e-2])
def test_kernel_equals_restatement_bit_for_bit(rule, weight_decay, problem):
    pr = problem
    params, opt, ref, views, launches, uploads = _run(rule, weight_decay, pr)
    # both access paths were taken, as the table the host built says: even parameters 16-byte vectors, odd ones dwords
    rec = opt.table_records()
    addr_vec = {int(a): int(v) for a, v in zip(rec[:, 1], rec[:, 5])}
    for k, v in enumerate(views):
        if k in (NO_GRAD, EMPTY):
            continue
        assert addr_vec[v.data_ptr()] == (1 if k % 2 == 0 else 0) == int(v.data_ptr() % 16 == 0), k
    assert set(rec[:, 5].tolist()) == {0, 1}
    assert rec[:, 4].max() == pr.C and rec[:, 4].min() == 1 and rec[:, 4].sum() == sum(pr.sizes) - pr.sizes[NO_GRAD]
    assert rec.shape[0] == sum(-(-n // pr.C) for k, n in enumerate(pr.sizes) if k != NO_GRAD)
    # the parameter without a gradient and the empty one never moved, the late one moved from step 3 on
    assert torch.equal(params[NO_GRAD].detach().cpu(), torch.from_numpy(pr.init[NO_GRAD])) and ref.t[LATE] == 3
    if weight_decay == 0.0:
        for k, p in enumerate(params):                   # g = 0 in every step with m = v = 0: the update is exactly 0
            assert torch.equal(p.detach().cpu()[::7], torch.from_numpy(pr.init[k][::7])), k
    # launches: one per step-count group.  The late parameter makes a second group at step 3; Adam's two groups keep different
    # step counts for good, SGD's new buffers step like the others after their first step (one launch again)
    assert launches == ([1, 1, 2, 2, 2] if rule != "SGD" else [1, 1, 2, 1, 1])
    # uploads: the first step, and step 3 when a gradient appeared: never in a steady step
    assert uploads == [1, 1, 2, 2, 2]
    # ... and again when a gradient address changes, and only then
    opt.step()
    assert opt.table_uploads == 2
    params[4].grad = params[4].grad.clone()
    opt.step()
    assert opt.table_uploads == 3
    opt.step()
    assert opt.table_uploads == 3


@pytest.mark.parametrize("rule", ["Adam", "AdamW", "SGD"])
def test_kernel_close_to_torch_float64(rule, problem):
    pr = problem
    params, opt, ref, _, _, _ = _run(rule, 1e-2, pr, check_at=())
    twins = [torch.nn.Parameter(torch.from_numpy(a.astype(np.float64))) for a in pr.init]
    topt = R.torch_twin(rule, twins, **_hyper(rule, 1e-2))
    for s in range(5):
        for p, g in zip(twins, pr.grads_of_step(s)):
            p.grad = None if g is None else torch.from_numpy(g.astype(np.float64))
        topt.step()
    gap = max(R.relative_gap(p.detach().cpu().numpy(), t.detach().numpy()) for p, t in zip(params, twins))
    print("%s: relative gap to the float64 twin %.3e (bound %.3e)" % (rule, gap, 4 * MEASURED_GAP[rule]))
    assert gap <= 4 * MEASURED_GAP[rule]


def test_steady_step_is_one_launch_and_no_copy(problem):
    """A profiled steady step: exactly `launches_last_step` device kernels, all k_optim_step, and no memory copy."""
    from torch.profiler import ProfilerActivity, profile
    params, opt, _, _, _, _ = _run("Adam", 0.0, problem, check_at=())
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        opt.step()
        torch.cuda.synchronize()
    # (torch's own "Optimizer.step#Adam.step" range is mirrored on the device timeline as an annotation: not a launch)
    dev = [e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and not e.name.startswith("Optimizer.step#")]
    names = [e.name for e in dev]
    assert opt.launches_last_step == 2 and opt.table_uploads == 2
    assert len(names) == 2 and all("k_optim_step" in n for n in names), names
    assert not [e.name for e in prof.events() if "memcpy" in e.name.lower()]


def test_schedule_is_read_every_step_and_errors():
    from pbnet_amd import optim as O
    p = torch.nn.Parameter(torch.ones(8, device=DEV))
    opt = O.SGD([p], lr=0.5)
    p.grad = torch.ones(8, device=DEV)
    opt.step()
    opt.param_groups[0]["lr"] = 0.25
    opt.step()
    assert torch.equal(p.detach().cpu(), torch.full((8,), 0.25)) and opt.table_uploads == 1
    with pytest.raises(TypeError, match="bfloat16"):
        O.Adam([torch.nn.Parameter(torch.zeros(4, device=DEV, dtype=torch.bfloat16))])
    q = torch.nn.Parameter(torch.zeros(4, 6, device=DEV))
    q.grad = torch.zeros(6, 4, device=DEV).t()
    with pytest.raises(ValueError, match="not contiguous"):
        O.Adam([q]).step()
    from pbnet_amd import _native as N
    lib = N.lib()
    assert lib.pbn_optim_adam(None, 1, 1e-3, 0.9, 0.1, 0.99, 0.01, 1e-8, 0.0, 1e-2, 0.1, 0, None) == N.PBN_ERR_ARG
    assert lib.pbn_optim_adam(None, 0, 1e-3, 0.9, 0.1, 0.99, 0.01, 1e-8, 0.0, 1e-2, 0.1, 0, None) == N.PBN_OK
    assert lib.pbn_optim_sgd(None, -1, 1e-3, 0.9, 0.0, 0, None) == N.PBN_ERR_ARG
    assert lib.pbn_optim_sgd(None, 0, float("nan"), 0.9, 0.0, 0, None) == N.PBN_ERR_ARG


def test_loss_meter_update_against_float64_and_average_meter():
    """Six steps of five terms with weights up to 3e5: the device sums agree with numpy float64 and with the reference's
    AverageMeter (recorded by tests/golden/make_train_golden.py) to 1e-14 relative."""
    from pbnet_amd.train_epoch import LossMeter
    with open(os.path.join(HERE, "golden", "train_meter.json")) as f:
        g = json.load(f)
    meter = LossMeter(g["names"])
    terms, weights = np.array(g["terms"], np.float32), np.array(g["weights"], np.float64)
    assert np.array_equal(terms.astype(np.float64), np.array(g["terms"])) and weights.max() == 3e5 and terms.shape == (6, 5)
    for s, (t, w) in enumerate(zip(terms, weights)):
        # weights as the dtypes model_fn hands over: int64 counts, then float32 sums
        wt = torch.from_numpy(w).to(DEV).long() if s % 2 == 0 else torch.from_numpy(w).to(DEV).float()
        meter.update(torch.from_numpy(t).to(DEV), wt)
    raw = meter.raw()
    want64 = np.stack([terms[-1].astype(np.float64), (terms.astype(np.float64) * weights).sum(0), weights.sum(0)])
    last = g["after"][-1]
    recorded = np.array([last["val"], last["sum"], last["count"]])
    for want in (want64, recorded):
        assert np.all(np.abs(raw - want) <= 1e-14 * np.abs(want)), (raw, want)
    got = meter.read()
    for n, v, a in zip(g["names"], last["val"], last["avg"]):
        assert got[n][0] == v and abs(got[n][1] - a) <= 1e-14 * abs(a)
