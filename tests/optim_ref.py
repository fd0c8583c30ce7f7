"""The arithmetic contract of csrc/optim.hip (include/pbnet_hip.h) restated in numpy float32: every line below is ONE float32
operation rounded once (numpy float32 arrays against float32 scalars; no fused multiply-add, correctly rounded division and
square root, denormals kept), in the kernel's order.  The scalars are formed in Python float64 and rounded to float32 once,
exactly as pbnet_amd/optim.py hands them to ctypes.  Not a test module: tests/test_optim_ref_cpu.py compares this file with
torch.optim on float64 twins, tests/test_optim_gpu.py compares the kernels with this file bit for bit."""
import math

import numpy as np

F = np.float32


def adam_scalars(lr, beta1, beta2, eps, weight_decay, t):
    """The kernel arguments of pbn_optim_adam for step count t >= 1, each rounded to float32 once."""
    return dict(lr=F(lr), beta1=F(beta1), one_minus_beta1=F(1.0 - beta1), beta2=F(beta2), one_minus_beta2=F(1.0 - beta2),
                eps=F(eps), weight_decay=F(weight_decay), step_size=F(lr / (1.0 - beta1 ** t)),
                bc2_sqrt=F(math.sqrt(1.0 - beta2 ** t)))


def adam_step(p, g, m, v, lr, betas, eps, weight_decay, t, decoupled):
    """One Adam / AdamW step of one tensor; float32 arrays in, new (p, m, v) out."""
    s = adam_scalars(lr, betas[0], betas[1], eps, weight_decay, t)
    p, g, m, v = (np.asarray(a, F) for a in (p, g, m, v))
    if s["weight_decay"] != 0:
        if decoupled:
            shrink = s["lr"] * s["weight_decay"]
            p = p * (F(1.0) - shrink)
        else:
            wp = s["weight_decay"] * p
            g = g + wp
    dm = g - m
    sm = dm * s["one_minus_beta1"]
    m = m + sm
    vb = v * s["beta2"]
    gg = g * g
    sg = gg * s["one_minus_beta2"]
    v = vb + sg
    r = np.sqrt(v)
    q = r / s["bc2_sqrt"]
    d = q + s["eps"]
    u = m / d
    su = s["step_size"] * u
    p = p - su
    assert p.dtype == F and m.dtype == F and v.dtype == F
    return p, m, v


def sgd_step(p, g, buf, lr, momentum, weight_decay, first):
    """One SGD step of one tensor (no dampening, no Nesterov); float32 arrays in, new (p, buf) out."""
    lr, momentum, weight_decay = F(lr), F(momentum), F(weight_decay)
    p, g, buf = (np.asarray(a, F) for a in (p, g, buf))
    if weight_decay != 0:
        wp = weight_decay * p
        g = g + wp
    if first:
        buf = g.copy()
    else:
        bm = buf * momentum
        buf = bm + g
    sb = lr * buf
    p = p - sb
    assert p.dtype == F and buf.dtype == F
    return p, buf


class RefOptimizer(object):
    """The rule over a list of float32 arrays with per-tensor step counts: a tensor whose gradient is None in a step is
    left out (no state, no decay, its count does not advance).  rule in {'Adam', 'AdamW', 'SGD'}."""

    def __init__(self, rule, params, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, momentum=0.0):
        self.rule, self.lr, self.betas, self.eps, self.weight_decay, self.momentum = rule, lr, betas, eps, weight_decay, momentum
        self.p = [np.array(a, F) for a in params]
        self.s0 = [None] * len(self.p)
        self.s1 = [None] * len(self.p)
        self.t = [0] * len(self.p)

    def step(self, grads):
        for i, g in enumerate(grads):
            if g is None or self.p[i].size == 0:
                continue
            first = self.s0[i] is None
            if first:
                self.s0[i], self.s1[i] = np.zeros_like(self.p[i]), np.zeros_like(self.p[i])
            self.t[i] += 1
            if self.rule == "SGD":
                self.p[i], self.s0[i] = sgd_step(self.p[i], g, self.s0[i], self.lr, self.momentum, self.weight_decay, first)
            else:
                self.p[i], self.s0[i], self.s1[i] = adam_step(self.p[i], g, self.s0[i], self.s1[i], self.lr, self.betas, self.eps,
                                                               self.weight_decay, self.t[i], self.rule == "AdamW")


def torch_twin(rule, params64, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, momentum=0.0):
    """torch.optim's optimizer of the same rule over float64 CPU parameters (single-tensor path)."""
    import torch
    if rule == "SGD":
        return torch.optim.SGD(params64, lr=lr, momentum=momentum, weight_decay=weight_decay, foreach=False)
    cls = torch.optim.AdamW if rule == "AdamW" else torch.optim.Adam
    return cls(params64, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, foreach=False)


def relative_gap(got, want):
    """max |got - want| / max |want| over one tensor (0 for an empty one)."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    if want.size == 0:
        return 0.0
    return float(np.abs(got - want).max() / max(np.abs(want).max(), 1e-300))
