"""Stage times of the raw-scan front (csrc/thin.hip) on a raw-sensor-sized cloud: the synthetic room of pbnet_amd/synth.py
replicated with jitter to about 2 M points, plus 1 % far outliers.  HIP events per stage of pbn_thin_points_timed, torch
events around knn_graph on the thinned points, outlier_mask and raw_index; medians of --runs after --warmup.  The numpy
restatement (tests/thin_ref.py) is timed once on the same host for scale, and its bytes are compared with the device's.
Writes one JSON file.

    python scripts/thin_timing.py --out profiles/r18_thin_timing.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import thin_ref  # noqa: E402
from pbnet_amd import mesh, synth  # noqa: E402


def raw_scan(target, jitter, outliers, seed=0):
    """synth_room's points `copies` times over with `jitter` m of Gaussian noise, then `outliers` x as many points
    scattered through three times the room's box."""
    scene = synth.synth_room()
    base = scene["xyz"].astype(np.float64)
    rng = np.random.default_rng(seed)
    copies = max(1, round(target / base.shape[0]))
    xyz = np.concatenate([base + rng.normal(scale=jitter, size=base.shape) for _ in range(copies)])
    lo, hi = base.min(0), base.max(0)
    far = rng.uniform(lo - (hi - lo), hi + (hi - lo), (int(outliers * xyz.shape[0]), 3))
    xyz = np.concatenate([xyz, far]).astype(np.float32)
    rgb = rng.integers(0, 256, xyz.shape).astype(np.float32)
    order = rng.permutation(xyz.shape[0])                    # a sensor does not deliver cell by cell
    return xyz[order], rgb[order], copies, far.shape[0]


def timed(fn):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    out = fn()
    ev[1].record()
    torch.cuda.synchronize()
    return out, ev[0].elapsed_time(ev[1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=2000000)
    ap.add_argument("--pitch", type=float, default=0.02)
    ap.add_argument("--jitter", type=float, default=0.004)
    ap.add_argument("--outliers", type=float, default=0.01)
    ap.add_argument("--ratio", type=float, default=2.0)
    ap.add_argument("--k", type=int, default=16)
    ap.add_argument("--runs", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    xyz, rgb, copies, n_far = raw_scan(a.points, a.jitter, a.outliers)
    x, c = torch.from_numpy(xyz).to(dev), torch.from_numpy(rgb).to(dev)
    rows = []
    for it in range(a.warmup + a.runs):
        t = {}
        th = mesh.thin_points(x, c, a.pitch, times=t)
        (idx, d2), t["knn_graph on the thinned points"] = timed(lambda: mesh.knn_graph(th["xyz"], k=a.k))
        (keep, stats), t["outlier_mask"] = timed(lambda: mesh.outlier_mask(d2, a.ratio))
        raw, t["raw_index"] = timed(lambda: mesh.raw_index(th["inverse"], keep, idx))
        if it >= a.warmup:
            rows.append(t)
    stages = {s: float(np.median([r[s] for r in rows])) for s in rows[0]}
    m, kept = int(th["xyz"].shape[0]), int(keep.sum().item())
    w0 = time.perf_counter()
    ref = thin_ref.thin(xyz, rgb, a.pitch)
    w1 = time.perf_counter()
    ref_keep, ref_stats = thin_ref.outlier(d2.cpu().numpy(), a.ratio)
    w2 = time.perf_counter()
    same = all(ref[k].tobytes() == th[k].cpu().numpy().tobytes() for k in ref)
    same_mask = bool(np.array_equal(ref_keep, keep.cpu().numpy()) and ref_stats.tobytes() == stats.cpu().numpy().tobytes())
    result = {"what": "raw-scan front, ms (HIP events; medians)", "device": torch.cuda.get_device_name(0),
              "raw_points": int(xyz.shape[0]), "room_copies": copies, "jitter_m": a.jitter, "far_points": n_far,
              "pitch": a.pitch, "k": a.k, "ratio": a.ratio, "runs": a.runs, "warmup": a.warmup,
              "stages_ms": stages, "thin_device_ms": sum(stages[s] for s in mesh.THIN_STAGES),
              "M": m, "fullest_cell": int(th["count"].max().item()), "mean_cell": float(xyz.shape[0]) / m,
              "kept": kept, "fraction_removed_by_the_mask": 1.0 - kept / m,
              "raw_points_without_a_row": int((raw < 0).sum().item()),
              "stats_mu_sigma_nvalid": [float(v) for v in stats.cpu().numpy()],
              "numpy_restatement_ms": {"thin": 1e3 * (w1 - w0), "outlier": 1e3 * (w2 - w1),
                                       "threads": len(os.sched_getaffinity(0))},
              "device_equals_restatement": {"thin": bool(same), "outlier": same_mask}}
    line = json.dumps(result, indent=1)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
