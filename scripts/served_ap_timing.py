#!/usr/bin/env python3
"""The AP association behind the batched post-processing of one merged forward, two ways, on configs[1] scenes (seeds 2, 3 of the
`served` leg's stream, bf16 features, teacher forced, three copies per unit, two units per forward; the method of
scripts/served_tta_timing.py part (a)).  Ground truth is a stand-in: the id of the 50 cm cell column a point stands in.

  (a) parent    : what the parent commit offers behind `refine_tta_merged_device`: read n_keep back, then per unit
                  `RefinedBatch.dense(j)` (k_j x n_j int32) and `AssociationLog.append` into one log;
  (b) batched   : `AssociationLog.append_batch` on the RefinedBatch: no read-back, no dense table.
      and (b) with ONE unit in the forward, for the launch count's independence of B.

10 warm-up calls per form, alternating blocks of 20 calls, median block (device events; host clock next to it), a profiler pass for
launches / copies, torch's sync debug mode for synchronising calls.  The post-processing itself is not in the timed region: both
forms start from the same RefinedBatch.  Prints one JSON line and, with a path, writes it there; needs the GPU."""
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
CODES = [0, 3001, 4002, 5003, 7004, 39005, 1006, 2007, 8008, 9009, 10010, 11011, 12012, 14013, 16014, 24015]


def spread(col, digits=4):
    return {"median": round(statistics.median(col), digits), "min": round(min(col), digits), "max": round(max(col), digits)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?", help="write the JSON line here too")
    ap.add_argument("--seconds", type=float, default=2.0, help="timed calls per form, at least")
    ap.add_argument("--small", action="store_true", help="small rooms (rehearsal; not a measurement)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "served_ap_timing.py measures on the GPU; there is no CPU form of it"
    from pbnet_amd import evaluate as E
    from pbnet_amd import postprocess as PP
    from pbnet_amd import synth
    from pbnet_amd.config import get_config
    from pbnet_amd.network.PBNet import PBNet
    from pbnet_amd.serving import merge_tta_units
    dev = torch.device("cuda:0")
    cfg = get_config(test=True)
    torch.manual_seed(22)
    model = PBNet(cfg).to(dev).eval()
    codes = torch.tensor(CODES, dtype=torch.int64, device=dev)
    units, teachers, gts = [], [], []
    for sd in (2, 3):
        bt, tc, _ = synth.make_val_batch(copies=COPIES, seed=sd, **(SMALL if args.small else C2))
        u = {k: torch.from_numpy(bt[k]).to(dev) for k in ("xyz_voxel", "feat_voxel", "xyz_original", "v2p_index")}
        u["feat_voxel"] = u["feat_voxel"].to(torch.bfloat16)
        n = int(u["xyz_original"].shape[0]) // COPIES
        u["sup"] = torch.arange(n, device=dev) // 64
        u["n_superpoints"] = (n - 1) // 64 + 1
        units.append(u)
        teachers.append({k: torch.from_numpy(v).to(dev) for k, v in tc.items()})
        cell = torch.floor(u["xyz_original"][:n] / 0.5).long()
        gts.append(codes[(cell[:, 0] + 5 * cell[:, 1]) % len(CODES)].contiguous())
    sizes = [int(g.shape[0]) for g in gts]

    def refined(sel):
        batch, starts, (sup, sp_starts) = merge_tta_units([units[j] for j in sel], COPIES, [teachers[j] for j in sel])
        with torch.no_grad():
            ret = model(batch["feat_voxel"], batch["xyz_voxel"], batch["xyz_original"], batch["v2p_index"], None, 1, "test",
                        teacher=batch["teacher"], n_batch=COPIES * len(sel))
        return PP.refine_tta_merged_device(ret["sem_pred_p"], ret["proposals"], ret["clt_scores"], starts, sp_starts, sup, cfg,
                                           copies=COPIES)

    rb2, rb1 = refined([0, 1]), refined([0])
    torch.cuda.synchronize()
    kept = rb2.scalars.tolist()[:2]
    log_kw = dict(u_cap=1024, id_cap=65536, log_words=8 << 20, device=dev)
    parent_log = E.AssociationLog(max(rb2.n_prop, 1), max(sizes), **log_kw)
    batch_log, one_log = E.AssociationLog(1, 1, **log_kw), E.AssociationLog(1, 1, **log_kw)
    dense_bytes = []

    def parent():
        parent_log.reset()
        scalars = rb2.scalars.tolist()                          # the host stop: n_keep sizes the dense tables
        del dense_bytes[:]
        for j in range(2):
            dense = rb2.dense(j, scalars)
            dense_bytes.append(dense.numel() * 4)
            k = scalars[j]
            parent_log.append("u%d" % j, dense, rb2.scores[j, :k], rb2.semantic_id[j, :k], None, None, gts[j])

    def batched():
        batch_log.reset()
        batch_log.append_batch(["u0", "u1"], rb2, gts, copies=COPIES)

    def batched_one():
        one_log.reset()
        one_log.append_batch(["u0"], rb1, gts[:1], copies=COPIES)

    parent(), batched(), batched_one()
    torch.cuda.synchronize()
    used = int(parent_log.state[0])
    same = parent_log.state.tolist() == batch_log.state.tolist() and torch.equal(parent_log.log[:used], batch_log.log[:used])
    forms = {"parent": parent, "batched": batched, "batched_one_unit": batched_one}
    for fn in forms.values():
        for _ in range(10):
            fn()
    times = {k: [] for k in forms}
    while min(sum(t[1] for t in v) * BLOCK for v in times.values()) < args.seconds * 1e3:
        for key, fn in forms.items():
            times[key].append(block(fn))
    result = {"device": torch.cuda.get_device_name(0), "host": platform.node(), "torch": torch.__version__,
              "rehearsal_size": bool(args.small), "copies": COPIES,
              "metric": "RefinedBatch of one merged forward -> records in the epoch log, ms per forward (two units; one for the last form)",
              "points": sizes, "proposals_merged_forward": rb2.n_prop, "kept_per_unit": kept, "log_words_used": used,
              "forms_write_the_same_log_bytes": bool(same), "block_calls": BLOCK, "forms": {}}
    for key, v in times.items():
        entry = {"blocks": len(v)}
        for i, name in enumerate(("event_ms", "wall_ms", "enqueue_ms")):
            entry[name] = spread([t[i] for t in v])
        entry.update(count_events(forms[key]))
        entry["dense_table_bytes"] = sum(dense_bytes) if key == "parent" else 0
        result["forms"][key] = entry
    f = result["forms"]
    result["event_ms_ratio_parent_over_batched"] = round(f["parent"]["event_ms"]["median"] / f["batched"]["event_ms"]["median"], 3)
    result["acceptance"] = {"batched_makes_no_synchronising_call": f["batched"]["host_syncs"] == 0 and f["batched"]["d2h_copies"] == 0,
                            "batched_allocates_no_dense_table": f["batched"]["dense_table_bytes"] == 0,
                            "batched_launches_do_not_depend_on_B": f["batched"]["launches"] == f["batched_one_unit"]["launches"]}
    line = json.dumps(result)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
