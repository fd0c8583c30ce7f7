"""Stage times of the label vote (csrc/vote.hip) on the raw-sensor-sized scan of scripts/thin_timing.py: the synthetic room
of pbnet_amd/synth.py replicated with jitter to about 2 M points plus 1 % far outliers, its sem / ins replicated with the
points (the far points are unannotated).  The scan is thinned (pitch), masked (ratio) and routed (raw_index) on the
device; vote_labels then runs over that raw_index.  HIP events per stage of pbn_cloud_vote_labels_timed and of
pbn_thin_points_timed in the same run; medians of --runs after --warmup.  The numpy restatement (tests/vote_ref.py) is
timed once on the same host for scale, and its bytes are compared with the device's.  Writes one JSON file.

    python scripts/vote_timing.py --out profiles/r19_vote_timing.json
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

import vote_ref  # noqa: E402
from pbnet_amd import mesh, synth  # noqa: E402


def raw_scan(target, jitter, outliers, seed=0):
    """thin_timing.raw_scan (the same draws in the same order, so the same points) with the labels carried along."""
    scene = synth.synth_room()
    base = scene["xyz"].astype(np.float64)
    rng = np.random.default_rng(seed)
    copies = max(1, round(target / base.shape[0]))
    xyz = np.concatenate([base + rng.normal(scale=jitter, size=base.shape) for _ in range(copies)])
    lo, hi = base.min(0), base.max(0)
    far = rng.uniform(lo - (hi - lo), hi + (hi - lo), (int(outliers * xyz.shape[0]), 3))
    xyz = np.concatenate([xyz, far]).astype(np.float32)
    rng.integers(0, 256, xyz.shape)                          # thin_timing draws the colours here
    order = rng.permutation(xyz.shape[0])
    none = np.full(far.shape[0], -100, np.int32)
    sem = np.concatenate([np.tile(np.asarray(scene["sem"], np.int32), copies), none])
    ins = np.concatenate([np.tile(np.asarray(scene["ins"], np.int32), copies), none])
    return xyz[order], sem[order], ins[order], copies, far.shape[0]


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
    xyz, sem, ins, copies, n_far = raw_scan(a.points, a.jitter, a.outliers)
    x, s, q = (torch.from_numpy(v).to(dev) for v in (xyz, sem, ins))
    th = mesh.thin_points(x, None, a.pitch)
    idx, d2 = mesh.knn_graph(th["xyz"], k=a.k)
    keep, _ = mesh.outlier_mask(d2, a.ratio)
    rows = mesh.raw_index(th["inverse"], keep, idx)
    m = int(keep.sum().item())
    vote_rows, thin_rows = [], []
    for it in range(a.warmup + a.runs):
        tv, tt = {}, {}
        mesh.thin_points(x, None, a.pitch, times=tt)
        got = mesh.vote_labels(rows, s, q, m=m, times=tv)
        if it >= a.warmup:
            vote_rows.append(tv)
            thin_rows.append(tt)
    stages = {k: float(np.median([r[k] for r in vote_rows])) for k in mesh.VOTE_STAGES}
    thin_ms = float(np.median([sum(r[k] for k in mesh.THIN_STAGES) for r in thin_rows]))
    got = {k: v.cpu().numpy() for k, v in got.items()}
    rows_h = rows.cpu().numpy()
    w0 = time.perf_counter()
    ref = vote_ref.vote(rows_h, sem, ins, m)
    w1 = time.perf_counter()
    same = all(ref[k].dtype == got[k].dtype and ref[k].tobytes() == got[k].tobytes() for k in ref)
    raw_ids = np.unique(ins[ins >= 0])
    result = {"what": "label vote over a raw scan's raw_index, ms (HIP events; medians)", "device": torch.cuda.get_device_name(0),
              "raw_points": int(xyz.shape[0]), "room_copies": copies, "jitter_m": a.jitter, "far_points": n_far,
              "pitch": a.pitch, "k": a.k, "ratio": a.ratio, "runs": a.runs, "warmup": a.warmup, "kept_rows": m,
              "stages_ms": stages, "vote_device_ms": float(np.median([sum(r.values()) for r in vote_rows])),
              "thin_points_device_ms_same_run": thin_ms,
              "numpy_restatement_ms": {"vote": 1e3 * (w1 - w0), "threads": len(os.sched_getaffinity(0))},
              "device_equals_restatement": bool(same),
              "raw_points_that_vote": int((rows_h >= 0).sum()),
              "share_of_rows_with_votes_eq_members": float((got["votes"] == got["members"]).mean()),
              "most_members_in_a_row": int(got["members"].max()),
              "raw_instances": int(raw_ids.shape[0]), "surviving_instances": int(got["old_id"].shape[0]),
              "vanished_instances": int(raw_ids.shape[0] - got["old_id"].shape[0])}
    line = json.dumps(result, indent=1)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
