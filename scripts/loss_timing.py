#!/usr/bin/env python3
"""Forward + backward of the training losses at the configs[2] shape: torch (`model_losses` + autograd) against the native
path (`model_losses_native`, csrc/losses.hip), timed with device events.

The shape comes from one batch of scripts/train_step.py (a ScanNet-sized synthetic scene, teacher-forced heads): PBNet runs
once, its outputs are detached and become the leaves both paths differentiate to, in bfloat16 and in float32.  Protocol: 10
warm-up calls of each path, then the two paths alternate in blocks of 20 calls until each has at least 2 s of timed calls; the
figure is the median block.  A profiler pass (9 calls of each path, medians; the profiler slows the host, so its kernel sum is
not the call time) counts the launches and gives the time of the two large kernels (k_loss_points, k_loss_points_bwd), whose achieved bytes per second are set against the bytes they must move.  Prints one
JSON line; needs the GPU."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

PROFILED_CALLS = 9                                          # kernel times are the median of this many profiled calls


def leaves_of(ret, dtype):
    out = dict(ret)
    for key in ("sem_pred_score_p", "offset_pred_p", "clt_scores"):
        out[key] = ret[key].detach().to(dtype).requires_grad_()
    out["mask_scores"] = (ret["mask_scores"][0].detach().to(dtype).requires_grad_(), ret["mask_scores"][1].clone())
    return out


def profile_calls(paths, fresh_leaves, fixed, entry, dtype, n, k, keep, valid):
    """Launch count and summed kernel time of a forward + backward of each path, and the two large native kernels against
    the bytes they must move (logits of the labelled rows, both labels of every row, offsets / targets of the valid rows;
    the backward also writes both gradients)."""
    from torch.profiler import ProfilerActivity, profile
    es = torch.empty(0, dtype=dtype).element_size()
    must = {"k_loss_points_bwd": keep * k * es + n * 16 + valid * (3 * es + 24) + n * k * es + n * 3 * es,
            "k_loss_points": keep * k * es + n * 16 + valid * (3 * es + 24)}
    for key, fn in paths.items():
        launches, sums, per_kernel = [], [], {kern: [] for kern in must}
        for _ in range(PROFILED_CALLS):
            lv = fresh_leaves()
            torch.cuda.synchronize()
            with profile(activities=[ProfilerActivity.CUDA]) as prof:
                fn(lv, *fixed)[0].backward()
                torch.cuda.synchronize()
            kernels = [e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
            launches.append(len(kernels))
            sums.append(sum(e.device_time for e in kernels) / 1e3)
            for kern in must:
                per_kernel[kern] += [e.device_time for e in kernels if kern in e.name and (kern + "_bwd") not in e.name][:1]
        entry[key]["launches"] = int(statistics.median(launches))
        entry[key]["kernel_ms_sum"] = round(statistics.median(sums), 4)
        for kern, nbytes in must.items() if key == "native" else ():
            us = statistics.median(per_kernel[kern])
            entry[key][kern] = {"us": round(us, 2), "min_us": round(min(per_kernel[kern]), 2), "profiled_calls": PROFILED_CALLS,
                                "bytes_to_move": nbytes, "achieved_GBps": round(nbytes / (us * 1e-6) / 1e9, 1),
                                "hbm_peak_GBps": 8000.0}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=2.0, help="timed calls per path and dtype, at least")
    ap.add_argument("--small", action="store_true", help="a 20 k-point room (rehearsal; not a measurement)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "loss_timing.py measures on the GPU; there is no CPU form of it"
    from pbnet_amd import synth
    from pbnet_amd.config import get_config
    from pbnet_amd.losses import model_losses_native
    from pbnet_amd.network.PBNet import PBNet, model_losses
    dev = torch.device("cuda:0")
    cfg = get_config(batch_size=1, cluster_epoch=0)
    torch.manual_seed(22)
    model = PBNet(cfg).to(dev).train()
    kw = dict(room=(1.6, 1.3, 1.2), n_boxes=4, pitch=0.03, classes=(17, 10)) if args.small else {}
    batch_np, teacher_np, _ = synth.make_train_batch(seed=10, copies=1, **kw)
    batch = {k: torch.from_numpy(v).to(dev) for k, v in batch_np.items()}
    batch["feat_voxel"] = batch["feat_voxel"].to(torch.bfloat16)
    teacher = {k: torch.from_numpy(v).to(dev) for k, v in teacher_np.items()}
    with torch.no_grad():
        ret = model(batch["feat_voxel"], batch["xyz_voxel"], batch["xyz_original"], batch["v2p_index"], batch["ins"], 1, "train",
                    teacher=teacher)
    fixed = (batch["sem"], batch["ins"], batch["inst_info"], batch["instance_pointnum"], batch["xyz_original"].float(), 1, cfg)
    n, k = ret["sem_pred_score_p"].shape
    r, p = ret["mask_scores"][0].shape[0], ret["clt_scores"].shape[0]
    keep = int(((batch["sem"] >= 0) & (batch["sem"] < k)).sum())
    valid = int((batch["ins"] != -100).sum())
    result = {"metric": "training losses, forward + backward, ms per call", "n_points": n, "n_class": k, "mask_rows": r,
              "proposals": p, "dtypes": {}}

    for name, dtype in (("bf16", torch.bfloat16), ("fp32", torch.float32)):
        def call(fn):
            lv = leaves_of(ret, dtype)
            loss = fn(lv, *fixed)[0]
            loss.backward()
            return loss

        def block(fn, calls=20):
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            lvs = [leaves_of(ret, dtype) for _ in range(calls)]          # the casts are not part of either path
            torch.cuda.synchronize()
            start.record()
            for lv in lvs:
                fn(lv, *fixed)[0].backward()
            stop.record()
            torch.cuda.synchronize()
            return start.elapsed_time(stop) / calls

        paths = {"torch": model_losses, "native": model_losses_native}
        for fn in paths.values():
            for _ in range(10):
                call(fn)
        times = {key: [] for key in paths}
        while min(sum(v) * 20 for v in times.values()) < args.seconds * 1e3:
            for key, fn in paths.items():
                times[key].append(block(fn))
        entry = {key: {"ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4),
                       "blocks_of_20": len(v)} for key, v in times.items()}
        assert abs(float(call(model_losses)) - float(call(model_losses_native))) <= 1e-4 * max(1.0, abs(float(call(model_losses))))
        profile_calls(paths, lambda: leaves_of(ret, dtype), fixed, entry, dtype, n, k, keep, valid)
        entry["speedup"] = round(entry["torch"]["ms"] / entry["native"]["ms"], 2)
        result["dtypes"][name] = entry
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
