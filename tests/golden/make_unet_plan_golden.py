"""Generates tests/golden/unet_plans.json: the static plans of the MinkUNet body as the two native executors receive them
(MinkUNet._build_plan -> csrc/executor.hip, train_engine.TrainPlan -> csrc/train_exec.hip), integers only.

Recorded at the commit BEFORE the plans became consumers of one walk of the body; tests/test_unet_plan_cpu.py rebuilds the
plans and compares them field for field, so whoever restates the topology has to reproduce every op, view and offset.
Uses nothing but Mink_unet, net._build_plan(dtype), MinkUNet.FOLD_SHORTCUT and TrainPlan.  Weights come from
torch.manual_seed on the CPU generator (bit-reproducible for a fixed torch version): the fixture records torch.__version__
and the packed-weight hashes count only under that version.  The inference plans build without the native library, the
training plans ask it for the weight-gradient workspace size.

Run from the repo root:  python tests/golden/make_unet_plan_golden.py
"""
import ctypes
import hashlib
import json
import os
import struct
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from pbnet_amd.network import train_engine as TE  # noqa: E402
from pbnet_amd.network.Mink import Mink_unet  # noqa: E402
from pbnet_amd.network.mink_unet import MinkUNet  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "unet_plans.json")
ARCHS = ("MinkUNet14A", "MinkUNet34C")
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
CIN, COUT, SEED = 6, 20, 3


def build(arch, extreme=False):
    """Seeded network in eval mode; BatchNorm statistics and affine parameters as tests/test_backbone_gpu.py randomises them.
    extreme: every other shortcut block gets the statistics of test_fold_guard_extreme_batchnorm_statistics, so the fp16 fold
    guard declines those blocks and folds the rest."""
    torch.manual_seed(SEED)
    net = Mink_unet(CIN, COUT, arch=arch).eval()
    g = torch.Generator().manual_seed(7)
    for mod in net.modules():
        if isinstance(mod, torch.nn.BatchNorm1d):
            mod.running_mean.copy_(torch.randn(mod.num_features, generator=g) * 0.1)
            mod.running_var.copy_(torch.rand(mod.num_features, generator=g) * 0.5 + 0.75)
            mod.weight.data.copy_(torch.rand(mod.num_features, generator=g) + 0.5)
            mod.bias.data.copy_(torch.randn(mod.num_features, generator=g) * 0.1)
    if extreme:
        blocks = [m for m in net.modules() if getattr(m, "downsample", None) is not None]
        with torch.no_grad():
            for i, blk in enumerate(blocks):
                if i % 2:
                    continue
                bn = (blk.norm2 if i % 4 == 0 else blk.downsample[1]).bn
                if i % 8 < 4:
                    bn.weight.fill_(3e6)             # scale ~ 1e9: the scaled weights overflow fp16
                    bn.running_var.fill_(1e-2)
                else:
                    bn.running_var.fill_(1e12)       # scale ~ 1e-6: the scaled weights are fp16 subnormals
    return net


def _fields(struct_type):
    """Names of every non-pointer field of a ctypes op, in declaration order."""
    return [name for name, ctype in struct_type._fields_ if ctype is not ctypes.c_void_p and not name.startswith("_")]


def _ints(op):
    """The values of _fields(type(op)); floats as their bit patterns."""
    kinds = dict(op._fields_)
    return [struct.unpack("<i", struct.pack("<f", getattr(op, name)))[0] if kinds[name] is ctypes.c_float
            else int(getattr(op, name)) for name in _fields(type(op))]


def inference_plan(net, dtype, fold):
    old = MinkUNet.FOLD_SHORTCUT
    MinkUNet.FOLD_SHORTCUT = fold
    try:
        plan = net._build_plan(dtype)
    finally:
        MinkUNet.FOLD_SHORTCUT = old
    by_ptr = {t.data_ptr(): t for t in plan["keep"] if t is not None}
    ops, hashes = [], []
    for i in range(plan["n_ops"]):
        o = plan["ops"][i]
        ops.append(_ints(o) + [int(not o.scale), int(not o.shift)])
        h = hashlib.sha256()
        for p in (o.w, o.scale, o.shift):
            if p:
                h.update(by_ptr[p].contiguous().view(torch.uint8).numpy().tobytes())
        hashes.append(h.hexdigest())
    bufs = [[plan["bufs"][b].level, plan["bufs"][b].width] for b in range(plan["n_bufs"])]
    return dict(op_fields=_fields(type(plan["ops"][0])) + ["scale_null", "shift_null"], ops=ops, sha256=hashes, bufs=bufs,
                out_buf=plan["out_buf"], cin_p=plan["cin_p"], out_width=plan["out_width"],
                true_io=[list(t) for t in plan["true_io"]], folded_io=[list(t) for t in plan["folded_io"]])


def training_plan(net, dtype, want_input_grad):
    plan = TE.TrainPlan(net, dtype, want_input_grad)
    return dict(op_fields=_fields(TE.N.TrainOp), ops=[_ints(plan.ops[i]) for i in range(len(plan.recs))],
                bufs=[list(b) for b in plan.bufs], out_view=list(plan.out_view), split_sizes=list(plan.split_sizes), grad_floats=plan.grad_floats,
                stat_floats=plan.stat_floats, pair_slots=list(plan.pair_slots), wgrad_ws_bytes=plan.wgrad_ws_bytes,
                dinput_width=plan.dinput_width)


def inference_cases():
    """name -> (arch, extreme, dtype name, fold)."""
    cases = {}
    for arch in ARCHS:
        for dn in DTYPES:
            for fold in (True, False):
                cases["%s-%s-%s" % (arch, dn, "fold" if fold else "sep")] = (arch, False, dn, fold)
    cases["MinkUNet14A-f16-fold-extreme"] = ("MinkUNet14A", True, "f16", True)
    return cases


def training_cases():
    """name -> (arch, dtype name, want_input_grad)."""
    return {"%s-%s-%s" % (arch, dn, "dx" if dx else "nodx"): (arch, dn, dx)
            for arch in ARCHS for dn in ("bf16", "f32") for dx in (False, True)}


def record(inference=None, training=None):
    """The fixture's content for the named cases (default: all of them); networks are built once per (arch, extreme)."""
    nets = {}

    def net(arch, extreme=False):
        if (arch, extreme) not in nets:
            nets[(arch, extreme)] = build(arch, extreme)
        return nets[(arch, extreme)]

    ic, tc = inference_cases(), training_cases()
    out = {"torch_version": torch.__version__, "inference": {}, "training": {}}
    for name in (ic if inference is None else inference):
        arch, extreme, dn, fold = ic[name]
        out["inference"][name] = inference_plan(net(arch, extreme), DTYPES[dn], fold)
    for name in (tc if training is None else training):
        arch, dn, dx = tc[name]
        out["training"][name] = training_plan(net(arch), DTYPES[dn], dx)
    return out


def main():
    data = record()
    with open(OUT, "w") as f:
        json.dump(data, f, sort_keys=True, separators=(",", ":"))
        f.write("\n")
    for kind in ("inference", "training"):
        for name, p in sorted(data[kind].items()):
            print(kind, name, len(p["ops"]), "ops", len(p["bufs"]), "bufs", len(p.get("folded_io", ())), "folded")


if __name__ == "__main__":
    main()
