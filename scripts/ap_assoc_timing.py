#!/usr/bin/env python3
"""Per-scene cost of the tail of a validation step AFTER refine_instances_device, in its two forms, at the sizes of the
configs[1] scene (seed 2, n_fold 161 517, the RefinedInstances of a teacher-forced task='eval' forward):

  A  the host tail: `.sliced()` (one read-back of four scalars), then evaluate.assign_instances_for_scan with host ids
     (np.unique on the host, index upload, pbn_instance_overlap, read-back of the [P, U] table);
  B  evaluate.AssociationLog.append_refined with device ids (no read-back); the read-back is paid once per block of scenes by
     `collect()`, inside the timed window.

Protocol: 10 warm-up scenes of each form, then the forms alternate in blocks of `--block` scenes until each has at least
`--seconds` of timed scenes.  Per block a host clock around the scenes, ending in a synchronise (A) or in `collect()` (B):
`wall_ms` per scene; `enqueue_ms` is the same clock when the last call RETURNS (before the synchronise / the collect).  The
figure is the median block, with min and max.  A profiler pass (9 scenes, medians) counts kernel launches and copies per scene;
`host_syncs` counts the synchronising calls torch reports in one scene.  Prints one JSON line and, with a path, writes it there;
needs the GPU."""
import argparse
import json
import os
import statistics
import sys
import time
import warnings

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

PROFILED_CALLS = 9


def count_events(fn):
    from torch.profiler import ProfilerActivity, profile
    counts = {"launches": [], "d2h_copies": [], "h2d_copies": []}
    for _ in range(PROFILED_CALLS):
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        dev = [e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
        copies = [e for e in dev if "memcpy" in e.name.lower()]
        counts["launches"].append(len([e for e in dev if "memcpy" not in e.name.lower() and "memset" not in e.name.lower()]))
        counts["d2h_copies"].append(sum("dtoh" in e.name.lower() for e in copies))
        counts["h2d_copies"].append(sum("htod" in e.name.lower() for e in copies))
    out = {k: int(statistics.median(v)) for k, v in counts.items()}
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as seen:
            warnings.simplefilter("always")
            fn()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    out["host_syncs"] = sum("synchroniz" in str(w.message).lower() for w in seen)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?", help="write the JSON line here too")
    ap.add_argument("--seconds", type=float, default=2.0, help="timed scenes per form, at least")
    ap.add_argument("--block", type=int, default=20, help="scenes per block (B pays one collect() per block)")
    ap.add_argument("--small", action="store_true", help="a small room (rehearsal; not a measurement)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "ap_assoc_timing.py measures on the GPU; there is no CPU form of it"
    from pbnet_amd import evaluate, synth
    from pbnet_amd.config import get_config
    from pbnet_amd.network.PBNet import PBNet, model_fn
    from pbnet_amd.postprocess import PostWorkspace, refine_instances_device
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
    sup = torch.from_numpy(sup_host.astype(np.int64)).to(dev)
    ws = PostWorkspace(n_prop, n_fold, n_sp, dev)
    res = refine_instances_device(pred["sem"], pred["proposals"], pred["clt_scores"], point_num, sup, cfg, n_superpoints=n_sp,
                                  workspace=ws)
    gt_host = evaluate.encode_gt_ids(batch_np["sem"][:n_fold], batch_np["ins"][:n_fold])
    gt_dev = torch.from_numpy(gt_host).to(dev)
    log = evaluate.AssociationLog(n_prop, n_fold, device=dev)

    def scene_a():
        clusters, scores, sem_id = res.sliced()
        return evaluate.assign_instances_for_scan("scene", dict(conf=scores, label_id=sem_id, mask=clusters), gt_host)

    def scene_b():
        log.append_refined("scene", res, gt_dev)

    def block_a():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.block):
            scene_a()
        t1 = time.perf_counter()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / args.block, (t1 - t0) * 1e3 / args.block

    def block_b():
        log.reset()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.block):
            scene_b()
        t1 = time.perf_counter()
        log.collect()
        return (time.perf_counter() - t0) * 1e3 / args.block, (t1 - t0) * 1e3 / args.block

    want = scene_a()
    log.reset()
    scene_b()
    got = log.collect()[0]["scene"]
    same = all(np.array_equal(np.asarray(getattr(want, f)), np.asarray(getattr(got, f)))
               for f in evaluate.SceneMatches.__slots__ if f != "scene")
    record_words = int(log.state[0].item())
    for _ in range(10):
        scene_a()
        scene_b()
    log.reset()
    legs = {"A_host_tail": block_a, "B_device_log": block_b}
    times = {k: [] for k in legs}
    while min(sum(t[0] for t in v) * args.block for v in times.values()) < args.seconds * 1e3:
        for key, fn in legs.items():
            times[key].append(fn())
    result = {"metric": "tail of one validation step after refine_instances_device, ms per scene", "n_fold": n_fold,
              "proposals": n_prop, "clusters_kept": int(want.pred_id.shape[0]),
              "n_keep": int(res.n_keep.item()), "n_gt": int(log.scalars[0].item()), "record_words": record_words,
              "block_scenes": args.block, "rehearsal_size": bool(args.small), "forms_agree": bool(same),
              "box": {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "hip": torch.version.hip}, "legs": {}}
    log.reset()
    for key, v in times.items():
        entry = {"blocks": len(v)}
        for i, name in enumerate(("wall_ms", "enqueue_ms")):
            col = [t[i] for t in v]
            entry[name] = {"median": round(statistics.median(col), 4), "min": round(min(col), 4), "max": round(max(col), 4)}
        entry.update(count_events(scene_a if key.startswith("A") else scene_b))
        result["legs"][key] = entry
    line = json.dumps(result)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
