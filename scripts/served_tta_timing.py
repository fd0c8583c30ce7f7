#!/usr/bin/env python3
"""The reference's evaluation unit (three rotated copies of a scene through one forward, then the folding post-processing,
eval_map.py:48-123) served two ways, on configs[1] scenes (seeds 2.. of the `served` leg's stream, bf16 features, teacher forced)
with the stand-in segmentation of scripts/eval_loop.py (ids = point // 64):

  (a) post-processing alone, from forward results to per-scene instances on the host's side of one synchronise:
        per_scene : what the parent commit offers: one `refine_instances_device(...).sliced()` per unit, on the unit's own
                    3-copy forward, each on its own pre-allocated workspace;
        batched   : `refine_tta_merged_device` on the merged forward of two units (six batch elements), one read-back of
                    n_keep[2] / status[2], two `.scene(j, scalars)` slices.
      Protocol and counters of scripts/post_timing.py: 10 warm-up calls per form, alternating blocks of 20 calls, median block
      (device events; host clock next to it), a profiler pass for launches / copies, torch's sync debug mode for synchronising calls.
  (b) the unit end to end, scenes/s over a stream of units (host clock from the first submit to the last result; every result
      ends in a synchronise):
        loop      : the parent commit's path, unit after unit: `model(..., n_batch=3)`, `refine_instances_device`, `.sliced()`;
        served    : `SceneServer(refine, tta=3)` with 1 and 2 units per forward and F = 1, 2, 4 forwards in flight.
      One warm-up pass per path, then the paths alternate pass by pass; median pass (min-max).

Prints one JSON line and, with a path, writes it there; needs the GPU."""
import argparse
import json
import os
import platform
import statistics
import sys
import time

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
    ap.add_argument("--seconds", type=float, default=2.0, help="part (a): timed calls per form, at least")
    ap.add_argument("--passes", type=int, default=15, help="part (b): timed passes over the stream per path")
    ap.add_argument("--distinct", type=int, default=4, help="distinct scenes")
    ap.add_argument("--stream", type=int, default=8, help="part (b): units per pass (the distinct scenes in turn)")
    ap.add_argument("--small", action="store_true", help="small rooms (rehearsal; not a measurement)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "served_tta_timing.py measures on the GPU; there is no CPU form of it"
    from pbnet_amd import postprocess as PP
    from pbnet_amd import synth
    from pbnet_amd.config import get_config
    from pbnet_amd.network.PBNet import PBNet
    from pbnet_amd.serving import SceneServer, merge_tta_units
    dev = torch.device("cuda:0")
    worker_streams = [torch.cuda.Stream(dev) for _ in range(4)]            # the process's first streams: distinct hardware queues
    cfg = get_config(test=True)
    torch.manual_seed(22)
    model = PBNet(cfg).to(dev).eval()
    units, teachers = [], []
    for sd in range(2, 2 + args.distinct):
        bt, tc, _ = synth.make_val_batch(copies=COPIES, seed=sd, **(SMALL if args.small else C2))
        u = {k: torch.from_numpy(bt[k]).to(dev) for k in ("xyz_voxel", "feat_voxel", "xyz_original", "v2p_index")}
        u["feat_voxel"] = u["feat_voxel"].to(torch.bfloat16)
        n = int(u["xyz_original"].shape[0]) // COPIES
        u["sup"] = torch.arange(n, device=dev) // 64
        u["n_superpoints"] = (n - 1) // 64 + 1
        units.append(u)
        teachers.append({k: torch.from_numpy(v).to(dev) for k, v in tc.items()})
    sizes = [int(u["xyz_original"].shape[0]) // COPIES for u in units]

    def forward(batch, teacher, n_batch):
        with torch.no_grad():
            return model(batch["feat_voxel"], batch["xyz_voxel"], batch["xyz_original"], batch["v2p_index"], None, 1, "test",
                         teacher=teacher, n_batch=n_batch)

    # ---- (a) the post-processing alone, two units --------------------------------------------------------------------------------
    own = [forward(units[j], teachers[j], COPIES) for j in range(2)]
    batch, starts, (sup, sp_starts) = merge_tta_units(units[:2], COPIES, teachers[:2])
    ret = forward(batch, batch["teacher"], 2 * COPIES)
    torch.cuda.synchronize()
    props = [int(r["proposals"][1].shape[0]) - 1 for r in own]
    n_prop = int(ret["proposals"][1].shape[0]) - 1
    per_scene_ws = [PP.PostWorkspace(props[j], sizes[j], units[j]["n_superpoints"], dev) for j in range(2)]
    batch_ws = PP.PostBatchWorkspace(n_prop, starts[-1], 2, sp_starts[-1], dev)

    def per_scene():
        out = []
        for j, r in enumerate(own):
            res = PP.refine_instances_device(r["sem_pred_p"], r["proposals"], r["clt_scores"], COPIES * sizes[j], units[j]["sup"], cfg,
                                             n_superpoints=units[j]["n_superpoints"], workspace=per_scene_ws[j])
            out.append(res.sliced())
        return out

    def batched():
        rb = PP.refine_tta_merged_device(ret["sem_pred_p"], ret["proposals"], ret["clt_scores"], starts, sp_starts, sup, cfg,
                                         copies=COPIES, workspace=batch_ws)
        scalars = rb.scalars.tolist()
        return rb, scalars, [rb.scene(j, scalars) for j in range(2)]

    want = per_scene()
    rb, scalars, got = batched()
    same = all(torch.equal(rb.dense(j, scalars), want[j][0]) and torch.equal(got[j]["semantic_id"], want[j][2]) for j in range(2))
    score_diff = max([float((got[j]["scores"] - want[j][1].float()).abs().max()) for j in range(2) if scalars[j] == want[j][1].numel()
                      and scalars[j]] or [float("nan")])
    # the two forms on the SAME inputs (each unit's own forward as a merged forward of one unit): must agree exactly
    same_inputs = True
    for j, r in enumerate(own):
        one = PP.refine_tta_merged_device(r["sem_pred_p"], r["proposals"], r["clt_scores"], [0, sizes[j]], [0, units[j]["n_superpoints"]],
                                          units[j]["sup"], cfg, copies=COPIES)
        sc = one.scalars.tolist()
        inst = one.scene(0, sc)
        same_inputs &= (torch.equal(one.dense(0, sc), want[j][0]) and torch.equal(inst["scores"], want[j][1].float())
                        and torch.equal(inst["semantic_id"], want[j][2]))
    forms = {"per_scene": per_scene, "batched": batched}
    for fn in forms.values():
        for _ in range(10):
            fn()
    times = {k: [] for k in forms}
    while min(sum(t[1] for t in v) * BLOCK for v in times.values()) < args.seconds * 1e3:
        for key, fn in forms.items():
            times[key].append(block(fn))
    part_a = {"metric": "forward results -> per-scene instances of two TTA units, ms per pair of units", "points": sizes[:2],
              "proposals_own_forwards": props, "proposals_merged_forward": n_prop, "superpoint_rows": sp_starts[-1],
              "kept_per_unit": scalars[:2], "kept_per_unit_per_scene_form": [int(w[1].numel()) for w in want],
              "forms_agree_on_the_same_forward": bool(same_inputs), "merged_vs_own_forwards_clusters_and_classes_agree": same,
              "merged_vs_own_forwards_scores_max_abs_diff": score_diff, "block_calls": BLOCK,
              "batch_workspace_mib": round(batch_ws.nbytes / 2 ** 20, 1), "forms": {}}
    for key, v in times.items():
        entry = {"blocks": len(v)}
        for i, name in enumerate(("event_ms", "wall_ms", "enqueue_ms")):
            entry[name] = spread([t[i] for t in v])
        entry.update(count_events(forms[key]))
        part_a["forms"][key] = entry

    # ---- (b) the evaluation unit end to end ----------------------------------------------------------------------------------------
    stream_units = [j % len(units) for j in range(args.stream)]
    loop_ws = [PP.PostWorkspace(4 * max(props), sizes[j], units[j]["n_superpoints"], dev) for j in range(len(units))]

    def loop_pass():
        kept = []
        for j in stream_units:
            r = forward(units[j], teachers[j], COPIES)
            res = PP.refine_instances_device(r["sem_pred_p"], r["proposals"], r["clt_scores"], COPIES * sizes[j], units[j]["sup"], cfg,
                                             n_superpoints=units[j]["n_superpoints"], workspace=loop_ws[j])
            kept.append(int(res.sliced()[0].shape[0]))
        return kept

    servers = {}
    for f in (1, 2, 4):
        for b in (1, 2):
            servers["served_b%d_f%d" % (b, f)] = SceneServer(model, max_batch=b, refine=cfg, tta=COPIES, streams=worker_streams[:f])

    def served_pass(server):
        def run():
            futs = [server.submit(units[j], teachers[j]) for j in stream_units]
            return [int(f.result(timeout=600)["instances"]["scores"].shape[0]) for f in futs]
        return run

    paths = {"loop": loop_pass}
    paths.update({k: served_pass(s) for k, s in servers.items()})
    kept = {k: fn() for k, fn in paths.items()}                            # the warm-up pass
    forwards0 = {k: s.forwards for k, s in servers.items()}
    secs = {k: [] for k in paths}
    for _ in range(args.passes):
        for key, fn in paths.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            secs[key].append(time.perf_counter() - t0)
    part_b = {"metric": "evaluation units (3 copies, forward + folding post-processing) per second, host clock per pass",
              "units_per_pass": args.stream, "distinct_scenes": len(units), "points": sizes, "passes": args.passes,
              "kept_agree_with_loop": {k: v == kept["loop"] for k, v in kept.items() if k != "loop"}, "paths": {}}
    for key, v in secs.items():
        entry = {"scenes_per_s": spread([args.stream / t for t in v], 2), "pass_ms": spread([t * 1e3 for t in v], 2)}
        if key in servers:
            entry["forwards_per_pass"] = round((servers[key].forwards - forwards0[key]) / args.passes, 2)
        part_b["paths"][key] = entry
    for s in servers.values():
        s.close()
    result = {"device": torch.cuda.get_device_name(0), "host": platform.node(), "torch": torch.__version__,
              "rehearsal_size": bool(args.small), "copies": COPIES, "post_processing": part_a, "end_to_end": part_b}
    line = json.dumps(result)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
