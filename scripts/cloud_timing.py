"""Stage times of the point-cloud front (csrc/cloud.hip) on the bench-sized synthetic room of pbnet_amd/synth.py
(~162 k points, k = 16): HIP events per stage of pbn_cloud_knn_timed (box + grid, keys + sort, cell table, search), torch
events around point_normals and knn_edges, events + host clock around segment_point (which synchronises for its host
sweep); medians of --runs after --warmup.  The search's candidate tests and cell reads per query are recounted on the
host from the same grid rule (h from the box's area and n / k) and the kernel's stopping rule.  Writes one JSON file.

    python scripts/cloud_timing.py --out profiles/r17_cloud_timing.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pbnet_amd import mesh, synth  # noqa: E402


def grid_rule(p, k, t_cap):
    """cloud.hip's k_cloud_grid in float64 numpy: (min, inv, dims)."""
    mn, mx = p.min(0).astype(np.float64), p.max(0).astype(np.float64)
    ext = mx - mn
    area = 2.0 * (ext[0] * ext[1] + ext[1] * ext[2] + ext[0] * ext[2])
    h = np.sqrt(area * k / (2.0 * p.shape[0])) if area > 0 else (ext.sum() * k / p.shape[0] if ext.sum() > 0 else 1.0)
    h = max(h, ext.max() / 1023.0 * (1.0 + 1.0e-9))
    for _ in range(64):
        inv = 1.0 / h
        dims = np.minimum(np.floor((mx - mn) * inv), 1023).astype(np.int64) + 1
        if dims.prod() <= t_cap:
            return mn, inv, dims, h
        h *= 1.25
    return mn, 0.0, np.ones(3, np.int64), h


def search_work(p, d2k, k):
    """Candidate tests and cell reads per query under the kernel's rule: shells grow until the k-th d2 is strictly below
    the squared distance to the nearest inner face of the scanned block, or the block covers the grid."""
    n = p.shape[0]
    t_cap = int(min(1 << 20, max(4096, 4 * n)))
    mn, inv, dims, h = grid_rule(p, k, t_cap)
    t = (p.astype(np.float64) - mn) * inv
    c = np.minimum(np.floor(t).astype(np.int64), dims - 1)
    occ = np.zeros(tuple(dims), np.int64)
    np.add.at(occ, (c[:, 0], c[:, 1], c[:, 2]), 1)
    integral = np.zeros(tuple(dims + 1), np.int64)
    integral[1:, 1:, 1:] = occ.cumsum(0).cumsum(1).cumsum(2)

    def box(lo, hi):                      # points in cells [lo, hi] (inclusive, clipped), per query
        a, b = np.clip(lo, 0, dims - 1), np.clip(hi, 0, dims - 1) + 1
        s = 0
        for sx, ix in ((1, b[:, 0]), (-1, a[:, 0])):
            for sy, iy in ((1, b[:, 1]), (-1, a[:, 1])):
                for sz, iz in ((1, b[:, 2]), (-1, a[:, 2])):
                    s = s + sx * sy * sz * integral[ix, iy, iz]
        return s, np.prod(b - a, axis=1)

    cand = np.zeros(n, np.int64)
    cells = np.zeros(n, np.int64)
    rings = np.zeros(n, np.int64)
    live = np.ones(n, bool)
    for r in range(1024):
        pts_in, cells_in = box(c - r, c + r)
        cand[live], cells[live], rings[live] = pts_in[live] - 1, cells_in[live], r
        lo_gap = np.where(c - r > 0, t - (c - r), np.inf)
        hi_gap = np.where(c + r < dims - 1, (c + r + 1) - t, np.inf)
        gap = np.minimum(lo_gap, hi_gap).min(1)
        bound2 = (gap / inv) ** 2 if inv > 0 else np.full(n, np.inf)
        live &= ~(np.isinf(gap) | (d2k < bound2))
        if not live.any():
            break
    return {"cell_size": float(h), "grid": [int(d) for d in dims], "occupied_cells": int((occ > 0).sum()),
            "candidates_per_query_mean": float(cand.mean()), "candidates_per_query_max": int(cand.max()),
            "cells_per_query_mean": float(cells.mean()), "shells_mean": float(rings.mean() + 1),
            "queries_stopping_after_shell_1": float(np.mean(rings <= 1))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=16)
    ap.add_argument("--runs", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    pts = synth.synth_room()["xyz"]
    pts = (pts - pts.mean(0)).astype(np.float32)
    x = torch.from_numpy(pts).to(dev)
    rows = []
    for it in range(a.warmup + a.runs):
        t = {}
        idx, d2 = mesh.knn_graph(x, k=a.k, times=t)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        ev[0].record()
        nl = mesh.point_normals(x, idx)
        ev[1].record()
        edges = mesh.knn_edges(idx)
        ev[2].record()
        torch.cuda.synchronize()
        w0 = time.perf_counter()
        sup = mesh.segment_point(x, nl, edges)
        torch.cuda.synchronize()
        w1 = time.perf_counter()
        t["normals"] = ev[0].elapsed_time(ev[1])
        t["knn_edges (torch)"] = ev[1].elapsed_time(ev[2])
        t["segment_point (call wall time, host sweep inside)"] = (w1 - w0) * 1e3
        if it >= a.warmup:
            rows.append(t)
    stages = {s: float(np.median([r[s] for r in rows])) for s in rows[0]}
    work = search_work(pts, d2[:, -1].cpu().numpy().astype(np.float64), a.k)
    # per query: candidates x 16 B (float4, sorted order: neighbouring lanes share them), cells x 8 B, its own point and
    # key 24 B, its row out 8 B x k
    work["bytes_per_query_mean"] = work["candidates_per_query_mean"] * 16 + work["cells_per_query_mean"] * 8 + 24 + 8 * a.k
    result = {"what": "point-cloud front, HIP events per stage, ms", "device": torch.cuda.get_device_name(0),
              "points": int(pts.shape[0]), "k": a.k, "runs": a.runs, "warmup": a.warmup, "stages_ms": stages,
              "knn_device_ms": sum(stages[s] for s in mesh.CLOUD_STAGES), "segments": int(sup.max().item()) + 1,
              "search": work}
    try:
        from scipy.spatial import cKDTree
        ts = []
        threads = min(16, len(os.sched_getaffinity(0)))
        for _ in range(3):
            w0 = time.perf_counter()
            tree = cKDTree(pts)
            w1 = time.perf_counter()
            tree.query(pts, k=a.k + 1, workers=threads)
            ts.append((w1 - w0, time.perf_counter() - w1))
        result["host_ckdtree_ms"] = {"build": 1e3 * float(np.median([t[0] for t in ts])),
                                     "query": 1e3 * float(np.median([t[1] for t in ts])),
                                     "threads": threads}
    except ImportError:
        result["host_ckdtree_ms"] = None
    line = json.dumps(result, indent=1)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
