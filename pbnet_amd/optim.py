"""The optimizers of the reference's training program (train.py:350-357: Adam, SGD with momentum, AdamW) over flat state
storage, stepped by csrc/optim.hip: ONE launch for all tensors that share a step count, in place of torch's per-dtype /
per-device multi-tensor chains.

* State lives in flat float32 buffers (every tensor's segment starts on a 16-byte boundary); `self.state[p]` exposes
  `step`, `exp_avg`, `exp_avg_sq` / `momentum_buffer` as views, so `state_dict()` is what `torch.optim` writes and
  `load_state_dict()` of a torch-written dict copies the tensors into the flat buffers.  checkpoint.checkpoint_save /
  checkpoint_restore work unchanged.
* A parameter whose `grad is None` in a step is left out: no state, no decay, its step count does not advance (what
  DistributedDataParallel(find_unused_parameters=True) and dist.GradientReducer preserve: before cluster_epoch the mask
  and score branches are such parameters).
* The kernel reads a device table with one record per chunk of at most pbn_optim_chunk() elements.  The table is cached
  on the signature (parameter and gradient addresses) and uploaded again only when that changes (`table_uploads`); a
  steady step does no host-to-device copy and no synchronisation, the scalars travel as kernel arguments, formed here in
  Python float64 and rounded to float32 once.  `lr` is read from `param_groups` at every step.

The arithmetic is the C ABI's contract (include/pbnet_hip.h; tests/optim_ref.py restates it in numpy float32)."""
import math

import numpy as np
import torch

from . import _native as N

NATIVE_DEFAULT = False          # build_optimizer's choice when cfg.native_optimizer is not set
_ALIGN = 4                      # elements: every tensor's state segment starts on a 16-byte boundary


def adam_scalars(lr, beta1, beta2, t):
    """The per-launch scalars of the Adam rule in float64: (step_size, bc2_sqrt) for step count t >= 1."""
    return lr / (1.0 - beta1 ** t), math.sqrt(1.0 - beta2 ** t)


def chunk_records(p_addr, g_addr, s0_addr, s1_addr, numel, chunk):
    """int64 [n, 5] records of one tensor: param, grad, state0, state1 addresses of each chunk and n | vec << 32 (the layout of
    pbn_optim_chunk_rec).  vec = 1 when all addresses of the chunk are multiples of 16."""
    starts = np.arange(0, numel, chunk, dtype=np.int64)
    rec = np.empty((starts.shape[0], 5), np.int64)
    rec[:, 0] = p_addr + 4 * starts
    rec[:, 1] = g_addr + 4 * starts
    rec[:, 2] = s0_addr + 4 * starts
    rec[:, 3] = (s1_addr + 4 * starts) if s1_addr else 0
    vec = ((rec[:, 0] | rec[:, 1] | rec[:, 2] | rec[:, 3]) % 16 == 0).astype(np.int64)
    rec[:, 4] = np.minimum(numel - starts, chunk) | (vec << 32)
    return rec


class _Launch(object):
    """Tensors of one param group that step together: a contiguous run of the table."""
    __slots__ = ("group", "key", "first_chunk", "n_chunks", "index", "ones")

    def __init__(self, group, key, first_chunk, n_chunks, index):
        self.group, self.key, self.first_chunk, self.n_chunks, self.index = group, key, first_chunk, n_chunks, index


class _FlatOptimizer(torch.optim.Optimizer):
    STATE = ()                  # names of the flat state tensors, state0 first
    HAS_STEP = False

    def __init__(self, params, defaults):
        super().__init__(params, defaults)
        self._params = [p for g in self.param_groups for p in g["params"]]
        self._group_of = [gi for gi, g in enumerate(self.param_groups) for _ in g["params"]]
        devices = {p.device for p in self._params}
        if len(devices) > 1:
            raise ValueError("all parameters must live on one device, got %s" % sorted(map(str, devices)))
        self._device = devices.pop()
        self._offsets, total = [], 0
        for p in self._params:
            if p.dtype != torch.float32:
                raise TypeError("pbnet_amd.optim steps float32 parameters only (PBN_ERR_ARG), got %s of shape %s"
                                % (p.dtype, tuple(p.shape)))
            self._offsets.append(total)
            total += -(-p.numel() // _ALIGN) * _ALIGN
        self._flat = [torch.zeros(total, dtype=torch.float32, device=self._device) for _ in self.STATE]
        self._steps = torch.zeros(len(self._params), dtype=torch.float32)       # host, as torch keeps `step`
        self._installed = [None] * len(self._params)                            # name -> the view this class put into state[p]
        self._used = [False] * len(self._params)                                # the segment has held a state
        self._signature = None
        self._table = None
        self._table_host = None                                                 # int64 [n_chunks, 5], what was uploaded
        self._launches = []
        self.table_uploads = 0
        self.launches_last_step = 0

    # ---- state as views ---------------------------------------------------------------------------------------------
    def _segment(self, k, i):
        p = self._params[i]
        return self._flat[k][self._offsets[i]:self._offsets[i] + p.numel()].view(p.shape)

    def _install(self, i, source=None):
        """Make self.state[p] the views of parameter i; `source` (a state dict of foreign tensors) is copied in first."""
        p = self._params[i]
        views = {}
        if self.HAS_STEP:
            self._steps[i] = float(source["step"]) if source is not None else 0.0
            views["step"] = self._steps[i]
        for k, name in enumerate(self.STATE):
            views[name] = self._segment(k, i)
            if source is not None:
                views[name].copy_(source[name])
            elif self._used[i]:
                views[name].zero_()                     # a segment that held another state before (load_state_dict)
        self._used[i] = True
        self._installed[i] = dict(views)
        views.update({k: v for k, v in (source or {}).items() if k not in views})
        self.state[p] = views
        return views

    def _adopt_foreign_state(self):
        """State entries this class did not create (load_state_dict, checkpoint_restore's device move) -> the flat buffers."""
        for i, p in enumerate(self._params):
            st = self.state.get(p)
            if not st or all(v is None for v in st.values()):      # torch's SGD without momentum writes a None buffer
                self._installed[i] = None
                continue
            mine = self._installed[i]
            if mine is not None and all(st.get(name) is t for name, t in mine.items()):
                continue
            missing = [name for name in (("step",) if self.HAS_STEP else ()) + self.STATE if st.get(name) is None]
            if missing:
                raise ValueError("optimizer state of a parameter lacks %s" % missing)
            self._install(i, dict(st))

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        self._installed = [None] * len(self._params)
        self._adopt_foreign_state()
        self._signature = None

    def add_param_group(self, param_group):
        if getattr(self, "_flat", None) is not None:
            raise NotImplementedError("pbnet_amd.optim lays its state out at construction: pass every group to the constructor")
        super().add_param_group(param_group)

    # ---- the table --------------------------------------------------------------------------------------------------
    def _key(self, i, has_state):
        raise NotImplementedError

    def _check_group(self, group):
        pass

    def _rebuild(self, grads):
        N.require_cuda(*self._params)
        for g in self.param_groups:
            self._check_group(g)
        self._adopt_foreign_state()
        chunk = N.lib().pbn_optim_chunk()
        steps = self._steps.tolist()
        order = []
        for i, (p, g) in enumerate(zip(self._params, grads)):
            if g is None or p.numel() == 0:
                continue
            if g.dtype != torch.float32 or g.device != p.device or g.shape != p.shape or g.is_sparse:
                raise TypeError("gradient of a %s %s parameter is %s %s on %s: float32 dense gradients on the parameter's device "
                                "only (PBN_ERR_ARG)" % (tuple(p.shape), p.dtype, tuple(g.shape), g.dtype, g.device))
            if not g.is_contiguous() or not p.is_contiguous():
                raise ValueError("parameter %d (shape %s): the %s is not contiguous (strides %s); the step kernel reads flat "
                                 "storage" % (i, tuple(p.shape), "gradient" if p.is_contiguous() else "parameter",
                                              (g if p.is_contiguous() else p).stride()))
            has_state = self._installed[i] is not None
            order.append((self._group_of[i], self._key(steps[i], has_state), i))
        order.sort()
        records, launches, at = [], [], 0
        for gi, key, i in order:
            if self._installed[i] is None:
                self._install(i)
            p = self._params[i]
            off = 4 * self._offsets[i]
            rec = chunk_records(p.data_ptr(), grads[i].data_ptr(), self._flat[0].data_ptr() + off,
                                self._flat[1].data_ptr() + off if len(self._flat) > 1 else 0, p.numel(), chunk)
            records.append(rec)
            if launches and launches[-1].group == gi and launches[-1].key == key:
                launches[-1].n_chunks += rec.shape[0]
                launches[-1].index.append(i)
            else:
                launches.append(_Launch(gi, key, at, rec.shape[0], [i]))
            at += rec.shape[0]
        for la in launches:
            la.index = torch.tensor(la.index, dtype=torch.int64)
            la.ones = torch.ones(la.index.shape[0])
        self._launches = launches
        if records:
            self._table_host = np.concatenate(records)
            self._table = torch.from_numpy(self._table_host).to(self._device)
            self.table_uploads += 1
        else:
            self._table_host, self._table = np.zeros((0, 5), np.int64), None

    def table_records(self):
        """The table as uploaded: int64 [n_chunks, 6] = param, grad, state0, state1 addresses, n, vec."""
        t = self._table_host if self._table_host is not None else np.zeros((0, 5), np.int64)
        return np.concatenate([t[:, :4], t[:, 4:] & 0xffffffff, t[:, 4:] >> 32], 1)

    def _launch(self, la, group, table_ptr):
        raise NotImplementedError

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        grads = [p.grad for p in self._params]
        signature = tuple([p.data_ptr() for p in self._params] + [0 if g is None else g.data_ptr() for g in grads])
        if signature != self._signature:
            self._rebuild(grads)
            self._signature = signature
        self.launches_last_step = 0
        base = self._table.data_ptr() if self._table is not None else 0
        for la in self._launches:
            self._launch(la, self.param_groups[la.group], N.c_vp(base + 40 * la.first_chunk))
            self.launches_last_step += 1
        self._merge_launches()
        return loss

    def _merge_launches(self):
        pass


class Adam(_FlatOptimizer):
    """torch.optim.Adam(params, lr, betas, eps, weight_decay) without amsgrad / maximize (train.py:351)."""
    STATE = ("exp_avg", "exp_avg_sq")
    HAS_STEP = True
    DECOUPLED = False

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0):
        if lr < 0 or eps < 0 or weight_decay < 0 or not (0 <= betas[0] < 1) or not (0 <= betas[1] < 1):
            raise ValueError("invalid Adam hyper-parameters: lr %r betas %r eps %r weight_decay %r" % (lr, betas, eps, weight_decay))
        # the keys torch.optim.Adam writes into a state dict, so that either class loads the other's
        super().__init__(params, dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay, amsgrad=False,
                                      maximize=False, foreach=None, capturable=False, differentiable=False, fused=None,
                                      decoupled_weight_decay=self.DECOUPLED))

    def _check_group(self, group):
        if group.get("amsgrad") or group.get("maximize"):
            raise NotImplementedError("pbnet_amd.optim.Adam has no amsgrad / maximize form (the reference uses neither)")
        if torch.is_tensor(group["lr"]):
            raise TypeError("lr must be a Python float: it travels as a kernel argument")

    def _key(self, step, has_state):
        return int(step)

    def _launch(self, la, group, table_ptr):
        t = la.key + 1
        lr, (beta1, beta2), wd = float(group["lr"]), group["betas"], float(group["weight_decay"])
        step_size, bc2_sqrt = adam_scalars(lr, beta1, beta2, t)
        N.check(N.lib().pbn_optim_adam(table_ptr, la.n_chunks, lr, beta1, 1.0 - beta1, beta2, 1.0 - beta2, float(group["eps"]), wd,
                                       step_size, bc2_sqrt, int(bool(group.get("decoupled_weight_decay", self.DECOUPLED))),
                                       N.current_stream()), "pbn_optim_adam")
        la.key = t
        self._steps.index_add_(0, la.index, la.ones)


class AdamW(Adam):
    """torch.optim.AdamW: the decay multiplies the parameter by 1 - lr * weight_decay before the Adam update (train.py:356)."""
    DECOUPLED = True

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2):
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)


class SGD(_FlatOptimizer):
    """torch.optim.SGD(params, lr, momentum, weight_decay) without dampening and Nesterov (train.py:353)."""
    STATE = ("momentum_buffer",)

    def __init__(self, params, lr=1e-3, momentum=0.0, weight_decay=0.0):
        if lr < 0 or momentum < 0 or weight_decay < 0:
            raise ValueError("invalid SGD hyper-parameters: lr %r momentum %r weight_decay %r" % (lr, momentum, weight_decay))
        super().__init__(params, dict(lr=lr, momentum=momentum, dampening=0, weight_decay=weight_decay, nesterov=False,
                                      maximize=False, foreach=None, differentiable=False, fused=None))

    def _check_group(self, group):
        if group.get("dampening") or group.get("nesterov") or group.get("maximize"):
            raise NotImplementedError("pbnet_amd.optim.SGD has no dampening / Nesterov / maximize form (train.py:353 uses none)")

    def _key(self, step, has_state):
        return 0 if has_state else 1                    # `first`: the buffer starts as the gradient

    def _launch(self, la, group, table_ptr):
        N.check(N.lib().pbn_optim_sgd(table_ptr, la.n_chunks, float(group["lr"]), float(group["momentum"]),
                                      float(group["weight_decay"]), la.key, N.current_stream()), "pbn_optim_sgd")
        la.key = 0

    def _merge_launches(self):
        # after their first step the new tensors step like the others: adjacent runs of the table become one launch
        merged = []
        for la in self._launches:
            if merged and merged[-1].group == la.group and merged[-1].key == la.key and \
                    merged[-1].first_chunk + merged[-1].n_chunks == la.first_chunk:
                merged[-1].n_chunks += la.n_chunks
                merged[-1].index = torch.cat([merged[-1].index, la.index])
                merged[-1].ones = torch.cat([merged[-1].ones, la.ones])
            else:
                merged.append(la)
        self._launches = merged


def build_optimizer(cfg, params, native=None):
    """train.py:350-357: cfg.optimizer in {'Adam', 'SGD', 'AdamW'} over the parameters that require a gradient, with the
    reference's arguments (Adam: lr only; SGD: momentum, weight_decay; AdamW: betas (0.9, 0.99), weight_decay).  `native`
    (default cfg.native_optimizer, else NATIVE_DEFAULT) picks this module's classes or torch.optim's."""
    params = [p for p in params if p.requires_grad]
    if native is None:
        native = getattr(cfg, "native_optimizer", NATIVE_DEFAULT)
    name = getattr(cfg, "optimizer", "Adam")
    on_gpu = bool(params) and params[0].is_cuda
    if name == "Adam":
        return Adam(params, lr=cfg.lr) if native else torch.optim.Adam(params, lr=cfg.lr, fused=on_gpu)
    if name == "SGD":
        kw = dict(lr=cfg.lr, momentum=cfg.momentum, weight_decay=cfg.weight_decay)
        return SGD(params, **kw) if native else torch.optim.SGD(params, **kw)
    if name == "AdamW":
        kw = dict(lr=cfg.lr, betas=(0.9, 0.99), weight_decay=cfg.weight_decay)
        return AdamW(params, **kw) if native else torch.optim.AdamW(params, fused=on_gpu, **kw)
    raise ValueError("cfg.optimizer must be 'Adam', 'SGD' or 'AdamW', got %r" % (name,))
