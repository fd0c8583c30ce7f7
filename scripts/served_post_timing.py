#!/usr/bin/env python3
"""From a merged forward's result to per-scene instances, in two forms, on the merged forward of four distinct configs[1] scenes
(seeds 2..5 of the `served` leg's stream, bf16 features, teacher forced) with the stand-in segmentation of scripts/eval_loop.py
(ids = point // 64):

  composition : what a caller of the serving front had to do before `SceneServer(refine=...)`: `split_results`, then four
                `refine_instances_device(...).sliced()` calls (point_num = 3 n_j switches the fold off), each on its own
                pre-allocated workspace;
  batched     : `refine_merged_device` on the merged result (the concatenation of the four scenes' ids included), one read-back
                of n_keep[B] / status[B], four `.scene(j, scalars)` slices.

Protocol and counters are those of scripts/post_timing.py (10 warm-up calls per form, alternating blocks of 20 calls, median block;
a profiler pass counts launches, summed kernel time and copies; torch's sync debug mode counts synchronising calls).  Prints one
JSON line and, with a path, writes it there; needs the GPU."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402

from post_timing import BLOCK, block, count_events  # noqa: E402

C2 = dict(room=(4.0, 3.2, 2.6), n_boxes=12, pitch=0.0225, voxel=0.02)      # bench.py WORKLOADS["c2"] = BASELINE configs[1]
SMALL = dict(room=(1.6, 1.3, 1.2), n_boxes=6, pitch=0.03)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?", help="write the JSON line here too")
    ap.add_argument("--seconds", type=float, default=2.0, help="timed calls per form, at least")
    ap.add_argument("--scenes", type=int, default=4)
    ap.add_argument("--small", action="store_true", help="small rooms (rehearsal; not a measurement)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "served_post_timing.py measures on the GPU; there is no CPU form of it"
    from pbnet_amd import postprocess as PP
    from pbnet_amd import synth
    from pbnet_amd.config import get_config
    from pbnet_amd.network.PBNet import PBNet
    from pbnet_amd.serving import merge_scenes, split_results
    dev = torch.device("cuda:0")
    cfg = get_config(test=True)
    torch.manual_seed(22)
    model = PBNet(cfg).to(dev).eval()
    scenes, teachers = [], []
    for sd in range(2, 2 + args.scenes):
        bt, tc, _ = synth.make_val_batch(copies=1, seed=sd, **(SMALL if args.small else C2))
        sc = {k: torch.from_numpy(bt[k]).to(dev) for k in ("xyz_voxel", "feat_voxel", "xyz_original", "v2p_index")}
        sc["feat_voxel"] = sc["feat_voxel"].to(torch.bfloat16)
        n = int(sc["xyz_original"].shape[0])
        sc["sup"] = torch.arange(n, device=dev) // 64
        sc["n_superpoints"] = (n - 1) // 64 + 1
        scenes.append(sc)
        teachers.append({k: torch.from_numpy(v).to(dev) for k, v in tc.items()})
    batch, teacher, starts = merge_scenes(scenes, teachers)
    with torch.no_grad():
        ret = model(batch["feat_voxel"], batch["xyz_voxel"], batch["xyz_original"], batch["v2p_index"], None, 1, "test",
                    teacher=teacher, n_batch=len(scenes))
    torch.cuda.synchronize()
    b = len(scenes)
    n_prop = int(ret["proposals"][1].shape[0]) - 1
    sizes = [starts[j + 1] - starts[j] for j in range(b)]
    sp_starts = PP.superpoint_starts(starts, [True] * b, [s["n_superpoints"] for s in scenes])
    per_scene_ws = None
    batch_ws = PP.PostBatchWorkspace(n_prop, starts[-1], b, sp_starts[-1], dev)

    def composition():
        parts = split_results(ret, starts)
        out = []
        for j, r in enumerate(parts):
            res = PP.refine_instances_device(r["sem_pred_p"], r["proposals"], r["clt_scores"], 3 * sizes[j], scenes[j]["sup"], cfg,
                                             n_superpoints=scenes[j]["n_superpoints"], workspace=per_scene_ws[j])
            out.append(res.sliced())
        return out

    def batched():
        sup = torch.cat([s["sup"] for s in scenes])
        rb = PP.refine_merged_device(ret["sem_pred_p"], ret["proposals"], ret["clt_scores"], starts, sp_starts, sup, cfg,
                                     workspace=batch_ws)
        scalars = rb.scalars.tolist()
        return rb, scalars, [rb.scene(j, scalars) for j in range(b)]

    props = [int(r["proposals"][1].shape[0]) - 1 for r in split_results(ret, starts)]
    per_scene_ws = [PP.PostWorkspace(props[j], sizes[j], scenes[j]["n_superpoints"], dev) for j in range(b)]
    want = composition()
    rb, scalars, got = batched()
    same = all(torch.equal(rb.dense(j, scalars), want[j][0]) and torch.equal(got[j]["scores"], want[j][1].float())
               and torch.equal(got[j]["semantic_id"], want[j][2]) for j in range(b))
    forms = {"composition": composition, "batched": batched}
    for fn in forms.values():
        for _ in range(10):
            fn()
    times = {k: [] for k in forms}
    while min(sum(t[1] for t in v) * BLOCK for v in times.values()) < args.seconds * 1e3:
        for key, fn in forms.items():
            times[key].append(block(fn))
    result = {"metric": "merged forward's result -> per-scene instances, ms per merged forward", "scenes": b, "points": sizes,
              "proposals": n_prop, "proposals_per_scene": props, "superpoint_rows": sp_starts[-1], "kept_per_scene": scalars[:b],
              "forms_agree": same, "block_calls": BLOCK, "rehearsal_size": bool(args.small),
              "batch_workspace_mib": round(batch_ws.nbytes / 2 ** 20, 1), "forms": {}}
    for key, v in times.items():
        entry = {"blocks": len(v)}
        for i, name in enumerate(("event_ms", "wall_ms", "enqueue_ms")):
            col = [t[i] for t in v]
            entry[name] = {"median": round(statistics.median(col), 4), "min": round(min(col), 4), "max": round(max(col), 4)}
        entry.update(count_events(forms[key]))
        result["forms"][key] = entry
    line = json.dumps(result)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
