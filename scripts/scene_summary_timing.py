#!/usr/bin/env python3
"""The scene summary of one merged forward (folded semantic labels, class vote, box and centre per kept instance) two ways, on two
configs[1] evaluation units (3 copies each, six batch elements, bf16 features, teacher forced, the stand-in segmentation of
scripts/served_tta_timing.py), both starting from the results of `refine_tta_merged_device` on that forward:

    native : `postprocess.summarize_merged_device` (pbn_scene_summary: three launches, no read-back) on a pre-allocated workspace;
    torch  : the same quantities composed from torch ops on the parent commit's results, per scene: `view(copies, n, K).float()`
             summed in copy order, `argmax`, a `bincount` over (instance, class) for the vote, `scatter_reduce` amin / amax for the
             box and an int64 `index_add_` of the same 16.16 fixed point for the centre -- and a `.item()` for the number of kept
             instances, which sizes those tables.

Neither form ends in a read-back of its results; the torch form's synchronising calls are the ones it cannot do without.
Protocol of scripts/post_timing.py: 10 warm-up calls per form, alternating blocks of 20 calls until each form has run for
--seconds, median block (device events; host clock next to it), a profiler pass for launches and copies, torch's sync debug mode
for synchronising calls.  The two forms' results are compared before anything is timed.

Prints one JSON line and, with a path, writes it there; needs the GPU."""
import argparse
import json
import os
import platform
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402

from post_timing import BLOCK, block, count_events  # noqa: E402

C2 = dict(room=(4.0, 3.2, 2.6), n_boxes=12, pitch=0.0225, voxel=0.02)      # bench.py WORKLOADS["c2"] = BASELINE configs[1]
SMALL = dict(room=(1.6, 1.3, 1.2), n_boxes=6, pitch=0.03)
COPIES = 3


def spread(col, digits=4):
    return {"median": round(statistics.median(col), digits), "min": round(min(col), digits), "max": round(max(col), digits)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?", help="write the JSON line here too")
    ap.add_argument("--seconds", type=float, default=2.0, help="timed calls per form, at least")
    ap.add_argument("--small", action="store_true", help="small rooms (rehearsal; not a measurement)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "scene_summary_timing.py measures on the GPU; there is no CPU form of it"
    from pbnet_amd import postprocess as PP
    from pbnet_amd import synth
    from pbnet_amd.config import get_config
    from pbnet_amd.network.PBNet import PBNet
    from pbnet_amd.serving import merge_tta_units
    dev = torch.device("cuda:0")
    cfg = get_config(test=True)
    torch.manual_seed(22)
    model = PBNet(cfg).to(dev).eval()
    units, teachers = [], []
    for sd in (2, 3):
        bt, tc, _ = synth.make_val_batch(copies=COPIES, seed=sd, **(SMALL if args.small else C2))
        u = {k: torch.from_numpy(bt[k]).to(dev) for k in ("xyz_voxel", "feat_voxel", "xyz_original", "v2p_index")}
        u["feat_voxel"] = u["feat_voxel"].to(torch.bfloat16)
        n = int(u["xyz_original"].shape[0]) // COPIES
        u["sup"] = torch.arange(n, device=dev) // 64
        u["n_superpoints"] = (n - 1) // 64 + 1
        units.append(u)
        teachers.append({k: torch.from_numpy(v).to(dev) for k, v in tc.items()})
    batch, starts, (sup, sp_starts) = merge_tta_units(units, COPIES, teachers)
    with torch.no_grad():
        ret = model(batch["feat_voxel"], batch["xyz_voxel"], batch["xyz_original"], batch["v2p_index"], None, 1, "test",
                    teacher=batch["teacher"], n_batch=2 * COPIES)
    rb = PP.refine_tta_merged_device(ret["sem_pred_p"], ret["proposals"], ret["clt_scores"], starts, sp_starts, sup, cfg, copies=COPIES)
    score = ret["sem_pred_score_p"]
    n_cls = int(score.shape[1])
    xyz = torch.cat([u["xyz_original"][:starts[j + 1] - starts[j]] for j, u in enumerate(units)]).contiguous()
    labels = rb.workspace.label_table
    ws = PP.SummaryWorkspace(rb.n_prop, starts[-1], 2, n_cls, dev)
    torch.cuda.synchronize()

    def native():
        return PP.summarize_merged_device(score, rb, starts, copies=COPIES, xyz=xyz, workspace=ws)

    def composed():
        out = []
        for j in range(2):
            p0, p1 = starts[j], starts[j + 1]
            n = p1 - p0
            s = score[COPIES * p0:COPIES * p1].view(COPIES, n, n_cls).float()
            tot = s[0]
            for c in range(1, COPIES):
                tot = tot + s[c]
            fold = tot.argmax(1)
            k = int(rb.scalars[j].item())                                      # sizes the per-instance tables
            pi = rb.point_instance[p0:p1].long()
            member = pi >= 0
            ids, pts = pi[member], xyz[p0:p1][member]
            hist = torch.bincount(ids * n_cls + fold[member], minlength=k * n_cls).view(k, n_cls)
            count, cls = hist.max(1)
            lo = torch.full((k, 3), float("inf"), device=dev).scatter_reduce(0, ids[:, None].expand(-1, 3), pts, "amin")
            hi = torch.full((k, 3), float("-inf"), device=dev).scatter_reduce(0, ids[:, None].expand(-1, 3), pts, "amax")
            q = torch.zeros(k, 3, dtype=torch.int64, device=dev).index_add_(0, ids, torch.round(pts * 65536.0).long())
            centre = (q.double() / hist.sum(1).double()[:, None] / 65536.0).float()
            out.append(dict(sem_fold=fold, class_vote=labels[cls], class_points=count, box=torch.cat([lo, hi], 1), centroid=centre))
        return out

    sm = native()
    scalars = sm.readback()
    got, want = [sm.scene(j, scalars) for j in range(2)], composed()
    agree = all(torch.equal(g["sem_fold"].long(), w["sem_fold"]) and torch.equal(g["class_vote"], w["class_vote"])
                and torch.equal(g["class_points"].long(), w["class_points"]) and torch.equal(g["box"], w["box"])
                and torch.equal(g["centroid"], w["centroid"]) for g, w in zip(got, want))
    forms = {"native": native, "torch": composed}
    for fn in forms.values():
        for _ in range(10):
            fn()
    times = {k: [] for k in forms}
    while min(sum(t[1] for t in v) * BLOCK for v in times.values()) < args.seconds * 1e3:
        for key, fn in forms.items():
            times[key].append(block(fn))
    result = {"device": torch.cuda.get_device_name(0), "host": platform.node(), "torch": torch.__version__,
              "rehearsal_size": bool(args.small), "copies": COPIES, "metric": "post-processing results -> scene summary of two TTA "
              "units in one merged forward, ms per call", "points": [starts[1], starts[2] - starts[1]], "classes": n_cls,
              "score_dtype": str(score.dtype), "proposals": rb.n_prop, "kept_per_unit": scalars[:2],
              "lds_instances": int(PP.N.lib().pbn_scene_summary_lds_instances(n_cls)),
              "workspace_kib": round(ws.nbytes / 1024, 1), "forms_agree": bool(agree), "block_calls": BLOCK, "forms": {}}
    for key, v in times.items():
        entry = {"blocks": len(v)}
        for i, name in enumerate(("event_ms", "wall_ms", "enqueue_ms")):
            entry[name] = spread([t[i] for t in v])
        entry.update(count_events(forms[key]))
        result["forms"][key] = entry
    line = json.dumps(result)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
