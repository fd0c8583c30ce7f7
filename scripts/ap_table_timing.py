#!/usr/bin/env python3
"""The tail of an evaluation epoch AFTER the association log is complete, in its two forms, on a 312-record epoch:

  A  the host tail: `AssociationLog.read_log()` + `decode_association_log` + `evaluate_matches`;
  B  the device tail: `APTable.add(log)` + `APTable.finish()`, its one read-back included.

The epoch: the record of the configs[1] scene (seed 2, the teacher-forced task='eval' forward, refine_instances_device,
`AssociationLog.append_refined` -- the record a validation step or the serving front appends for that scene), appended 312
times under 312 names.  Every record has the real scene's size; the scenes are not distinct, so the score ties of a real epoch
are overstated.  Protocol: 3 warm-up rounds of each form, then the forms alternate until each has `--rounds` timed rounds; a
host clock from a synchronised start to the returned AP table.  Medians with min and max, and the bytes each form reads back.
Prints one JSON line and, with a path, writes it there; needs the GPU."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?", help="write the JSON line here too")
    ap.add_argument("--records", type=int, default=312)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--small", action="store_true", help="a small room (rehearsal; not a measurement)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "ap_table_timing.py measures on the GPU; there is no CPU form of it"
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
    gt_dev = torch.from_numpy(evaluate.encode_gt_ids(batch_np["sem"][:n_fold], batch_np["ins"][:n_fold])).to(dev)
    probe = evaluate.AssociationLog(n_prop, n_fold, device=dev)
    probe.append_refined("probe", res, gt_dev)
    record_words = int(probe.state[0].item())
    log = evaluate.AssociationLog(n_prop, n_fold, log_words=args.records * record_words + 8, device=dev)
    for i in range(args.records):
        log.append_refined("scene%04d_00" % i, res, gt_dev)
    n_keep, n_gt = int(res.n_keep.item()), int(log.scalars[0].item())
    table = evaluate.APTable(args.records, 12 * max(n_keep, 1) * args.records, device=dev)
    host_bytes = [0]

    def tail_a():
        words = log.read_log()
        host_bytes[0] = int(words.nbytes) + 16
        return evaluate.evaluate_matches(evaluate.decode_association_log(words, log.names)[0])

    def tail_b():
        table.reset()
        table.add(log)
        return table.finish()[0]

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        return (time.perf_counter() - t0) * 1e3, out

    legs = {"A_host_tail": tail_a, "B_device_table": tail_b}
    for fn in legs.values():
        for _ in range(3):
            fn()
    times, last = {k: [] for k in legs}, {}
    for _ in range(args.rounds):
        for key, fn in legs.items():
            ms, last[key] = timed(fn)
            times[key].append(ms)
    a, b = last["A_host_tail"], last["B_device_table"]
    live = ~np.isnan(a)
    result = {"metric": "tail of an evaluation epoch after the association log is complete, ms per epoch",
              "records": args.records, "n_keep": n_keep, "n_gt": n_gt, "record_words": record_words, "n_fold": n_fold,
              "rehearsal_size": bool(args.small),
              "forms_agree": bool(np.array_equal(np.isnan(a), np.isnan(b)) and
                                  float(np.abs(a[live].astype(np.float64) - b[live].astype(np.float64)).max(initial=0.0)) <= 1.2e-7),
              "readback_bytes": {"A_host_tail": host_bytes[0], "B_device_table": table.readback_bytes},
              "box": {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "hip": torch.version.hip}, "legs": {}}
    for key, v in times.items():
        result["legs"][key] = {"rounds": len(v), "wall_ms": {"median": round(statistics.median(v), 3), "min": round(min(v), 3),
                                                             "max": round(max(v), 3)}}
    line = json.dumps(result)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
