#!/usr/bin/env python3
"""The optimizer step over the full PBNet(cfg) parameter list with random gradients: pbnet_amd.optim.Adam (csrc/optim.hip, one
launch) against torch.optim.Adam(fused=True), timed with device events on one MI355X.

Protocol: each optimizer owns a copy of the parameters and of the gradients; 10 warm-up steps of each, then the two alternate
in blocks of 20 steps until each has at least --seconds of timed steps; the figure is the median block.  A block's time runs
from the first launch to the end of the last kernel, so it is the larger of the host's pace and the device's.  A profiler pass
(5 steps of each; the profiler slows the host, its kernel sum is not the step time) counts the device launches of a step and
sums their time, which is set against the 28 bytes per parameter a step must move (read p, g, m, v; write p, m, v) and the HBM
peak.  Prints one JSON line and writes it to --out; needs the GPU."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

BLOCK = 20
HBM_PEAK = 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=2.0, help="timed steps per optimizer, at least")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r08_optim_timing.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "optim_timing.py measures on the GPU; there is no CPU form of it"
    from torch.profiler import ProfilerActivity, profile
    from pbnet_amd import optim as O
    from pbnet_amd.config import get_config
    from pbnet_amd.network.PBNet import PBNet
    dev = torch.device("cuda:0")
    torch.manual_seed(22)
    model = PBNet(get_config(batch_size=1, cluster_epoch=0)).to(dev)
    shapes = [p.shape for p in model.parameters() if p.requires_grad]
    sets = {}
    for key in ("native", "torch_fused"):
        g = torch.Generator(device=dev).manual_seed(5)
        params = [torch.nn.Parameter(torch.randn(s, device=dev, generator=g)) for s in shapes]
        for p in params:
            p.grad = torch.randn(p.shape, device=dev, generator=g) * 1e-2
        sets[key] = params
    opts = {"native": O.Adam(sets["native"], lr=1e-3), "torch_fused": torch.optim.Adam(sets["torch_fused"], lr=1e-3, fused=True)}
    n_elem = sum(p.numel() for p in sets["native"])

    def block(opt):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        start.record()
        for _ in range(BLOCK):
            opt.step()
        stop.record()
        torch.cuda.synchronize()
        return start.elapsed_time(stop) / BLOCK

    for opt in opts.values():
        for _ in range(10):
            opt.step()
    times = {key: [] for key in opts}
    while min(sum(v) * BLOCK for v in times.values()) < args.seconds * 1e3:
        for key, opt in opts.items():
            times[key].append(block(opt))
    result = {"metric": "optimizer step over the PBNet parameter list, ms per step (median block of %d)" % BLOCK,
              "tensors": len(shapes), "elements": n_elem, "bytes_to_move_per_step": 28 * n_elem, "hbm_peak_GBps": HBM_PEAK / 1e9}
    for key, opt in opts.items():
        launches, sums = [], []
        for _ in range(5):
            torch.cuda.synchronize()
            with profile(activities=[ProfilerActivity.CUDA]) as prof:
                opt.step()
                torch.cuda.synchronize()
            kernels = [e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA
                       and not e.name.startswith("Optimizer.step#")]          # torch's range annotation is not a launch
            launches.append(len(kernels))
            sums.append(sum(e.device_time for e in kernels))
        us = statistics.median(sums)
        v = times[key]
        result[key] = {"ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4),
                       "blocks": len(v), "launches_per_step": int(statistics.median(launches)), "kernel_us_sum": round(us, 2),
                       "kernel_GBps": round(28 * n_elem / (us * 1e-6) / 1e9, 1), "kernel_frac_hbm": round(28 * n_elem / (us * 1e-6) / HBM_PEAK, 4),
                       "step_frac_hbm": round(28 * n_elem / (statistics.median(v) * 1e-3) / HBM_PEAK, 4)}
    result["native"]["table_uploads"] = opts["native"].table_uploads
    result["native"]["chunks"] = int(opts["native"].table_records().shape[0])
    result["native_over_torch"] = round(result["native"]["ms"] / result["torch_fused"]["ms"], 3)
    # the two hold the same numbers up to the arithmetic both are allowed (torch's fused kernel contracts to FMA)
    worst = max(float((a.detach() - b.detach()).abs().max() / b.detach().abs().max().clamp_min(1e-30))
                for a, b in zip(sets["native"], sets["torch_fused"]) if a.numel())
    result["max_relative_difference_of_parameters"] = worst
    line = json.dumps(result)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
