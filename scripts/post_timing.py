#!/usr/bin/env python3
"""Per-scene cost of the evaluation-time post-processing in its two forms, at the sizes of the configs[1] scene (seed 2, 3 x
161 517 points, the proposals of a teacher-forced task='eval' forward): `refine_instances` (host form) against
`refine_instances_device(...)` followed by `.sliced()` (device form: one read-back of four scalars at the end).

Like for like: both forms are timed on the same inputs.  Rows `*_device_ids`: the superpoint ids are a device tensor already
(the host form takes one as it is).  Rows `*_host_ids`: both forms are handed the numpy ids and upload them inside the timed
call.  `device_enqueue_only_device_ids` is the device form without `.sliced()`.  A second size repeats the forward's proposals
`--replicate` times (distinct scores), for a scene with several hundred proposals.

Protocol: 10 warm-up calls of each form, then the forms alternate in blocks of 20 calls until each has at least `--seconds` of
timed calls.  Per block: device events around the 20 calls and a host clock around the same calls ending in a synchronise;
`enqueue_ms` is the host clock until the last call RETURNS (before the synchronise).  The figure is the median block, with min
and max.  A profiler pass (9 calls, medians; the profiler slows the host, so its kernel sum is not the call time) counts kernel
launches and the copy events in each direction; `host_syncs` counts the synchronising calls torch itself reports under
`torch.cuda.set_sync_debug_mode("warn")` in one call.  Prints one JSON line and, with a path, writes it there; needs the GPU."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

PROFILED_CALLS = 9
BLOCK = 20


def count_events(fn):
    from torch.profiler import ProfilerActivity, profile
    counts = {"launches": [], "d2h_copies": [], "h2d_copies": [], "kernel_ms_sum": []}
    for _ in range(PROFILED_CALLS):
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        dev = [e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
        copies = [e for e in dev if "memcpy" in e.name.lower()]
        kernels = [e for e in dev if "memcpy" not in e.name.lower() and "memset" not in e.name.lower()]
        counts["launches"].append(len(kernels))
        counts["d2h_copies"].append(sum("dtoh" in e.name.lower() for e in copies))
        counts["h2d_copies"].append(sum("htod" in e.name.lower() for e in copies))
        counts["kernel_ms_sum"].append(sum(e.device_time for e in kernels) / 1e3)
    out = {k: (round(statistics.median(v), 4) if k == "kernel_ms_sum" else int(statistics.median(v))) for k, v in counts.items()}
    import warnings
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as seen:
            warnings.simplefilter("always")
            fn()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    out["host_syncs"] = sum("synchroniz" in str(w.message).lower() for w in seen)
    return out


def block(fn):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    start.record()
    for _ in range(BLOCK):
        fn()
    stop.record()
    t1 = time.perf_counter()
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    return start.elapsed_time(stop) / BLOCK, (t2 - t0) * 1e3 / BLOCK, (t1 - t0) * 1e3 / BLOCK


def replicated(pred, copies):
    """The forward's proposals `copies` times over (proposal ids shifted, scores scaled by distinct factors so that no tie
    appears): a scene with several hundred proposals of realistic extent and overlap."""
    idx, off, clt = pred["proposals"][0], pred["proposals"][1], pred["clt_scores"].view(-1).float()
    if copies == 1:
        return (idx, off), clt
    n_prop, n_entries = int(off.shape[0]) - 1, int(idx.shape[0])
    shift = torch.tensor([n_prop, 0], dtype=idx.dtype, device=idx.device)
    idx_all = torch.cat([idx + k * shift for k in range(copies)])
    off_all = torch.cat([off[:-1] + k * n_entries for k in range(copies)] + [off[-1:] + (copies - 1) * n_entries])
    clt_all = torch.cat([clt * (1.0 - 0.003 * k) for k in range(copies)])
    return (idx_all.contiguous(), off_all.contiguous()), clt_all.contiguous()


def measure(pred, copies, point_num, n_fold, n_sp, sup_host, sup_dev, cfg, seconds):
    from pbnet_amd.postprocess import PostWorkspace, refine_instances, refine_instances_device
    proposals, clt = replicated(pred, copies)
    n_prop = int(proposals[1].shape[0]) - 1
    common = (pred["sem"], proposals, clt, point_num)
    ws = PostWorkspace(n_prop, n_fold, n_sp, sup_dev.device)

    def upload():
        return torch.from_numpy(sup_host.astype(np.int64, copy=False)).to(sup_dev.device)

    # like for like: both forms get the SAME ids.  Rows `*_device_ids`: the ids are already on the device (the host form takes
    # a device tensor as it is).  Rows `*_host_ids`: both forms are handed numpy ids and upload them inside the timed call.
    forms = {"host_device_ids": lambda: refine_instances(*common, sup_dev, cfg),
             "device_device_ids": lambda: refine_instances_device(*common, sup_dev, cfg, n_superpoints=n_sp, workspace=ws).sliced(),
             "device_enqueue_only_device_ids": lambda: refine_instances_device(*common, sup_dev, cfg, n_superpoints=n_sp,
                                                                              workspace=ws),
             "host_host_ids": lambda: refine_instances(*common, sup_host, cfg),
             "device_host_ids": lambda: refine_instances_device(*common, upload(), cfg, n_superpoints=n_sp, workspace=ws).sliced()}
    a = forms["host_device_ids"]()
    b = tuple(t.clone() for t in forms["device_device_ids"]())
    same = all(x.shape == y.shape and bool((x == y).all()) for x, y in zip(a, b))
    for fn in forms.values():
        for _ in range(10):
            fn()
    times = {k: [] for k in forms}
    while min(sum(t[1] for t in v) * BLOCK for v in times.values()) < seconds * 1e3:
        for key, fn in forms.items():
            times[key].append(block(fn))
    out = {"proposals": n_prop, "proposal_copies": copies, "clusters_kept": int(a[0].shape[0]), "forms_agree": same, "forms": {}}
    for key, v in times.items():
        entry = {"blocks": len(v)}
        for i, name in enumerate(("event_ms", "wall_ms", "enqueue_ms")):
            col = [t[i] for t in v]
            entry[name] = {"median": round(statistics.median(col), 4), "min": round(min(col), 4), "max": round(max(col), 4)}
        entry.update(count_events(forms[key]))
        out["forms"][key] = entry
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?", help="write the JSON line here too")
    ap.add_argument("--seconds", type=float, default=2.0, help="timed calls per form, at least")
    ap.add_argument("--replicate", type=int, default=8, help="second size: the forward's proposals this many times over")
    ap.add_argument("--small", action="store_true", help="a small room (rehearsal; not a measurement)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "post_timing.py measures on the GPU; there is no CPU form of it"
    from pbnet_amd import synth
    from pbnet_amd.config import get_config
    from pbnet_amd.network.PBNet import PBNet, model_fn
    dev = torch.device("cuda:0")
    cfg = get_config(batch_size=1, cluster_epoch=0)
    torch.manual_seed(22)
    model = PBNet(cfg).to(dev).eval()
    kw = dict(room=(2.4, 2.0, 1.8), n_boxes=6) if args.small else {}
    batch_np, teacher_np, _ = synth.make_train_batch(seed=2, copies=3, **kw)
    batch = {k: torch.from_numpy(v) for k, v in batch_np.items()}
    teacher = {k: torch.from_numpy(v).to(dev) for k, v in teacher_np.items()}
    forward = model.forward
    model.forward = lambda *a, **k: forward(*a, teacher=teacher, **k)
    with torch.no_grad():
        _, pred, _, _ = model_fn(batch, model, 1, cfg, task="eval")
    point_num = int(batch["xyz_original"].shape[0])
    n_fold = point_num // 3
    n_prop = int(pred["proposals"][1].shape[0]) - 1
    sup_host = np.arange(n_fold) // 64                          # stand-in for the mesh segmentation, as scripts/eval_loop.py
    n_sp = int(sup_host.max()) + 1
    sup_dev = torch.from_numpy(sup_host.astype(np.int64)).to(dev)
    result = {"metric": "evaluation post-processing of one scene, ms per call", "n_fold": n_fold, "n_superpoints": n_sp,
              "block_calls": BLOCK, "rehearsal_size": bool(args.small), "sizes": []}
    for copies in (1, args.replicate):
        result["sizes"].append(measure(pred, copies, point_num, n_fold, n_sp, sup_host, sup_dev, cfg, args.seconds))
    line = json.dumps(result)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
