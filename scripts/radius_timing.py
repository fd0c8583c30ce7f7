"""Stage times of the radius filter (csrc/cloud.hip: radius_count / radius_outlier_mask / radius_raw_index) on the raw scan
of scripts/thin_timing.py (the synthetic room replicated with jitter to about 2 M points plus 1 % far points), and the
whole raw-scan front -- thin_points, the mask, the raw index, the compaction -- under outlier_radius= and under
outlier_ratio= in the same run, alternating.  HIP events per stage of pbn_cloud_radius_count_timed, torch events around
the rest; medians of --runs after --warmup.  The script plants the far points, so it knows them: it reports what each
filter drops.  The walk's candidate tests per query are recounted on the host from the kernel's grid and stopping rule
(without the cap, which only shortens a walk), and at cap = k the count is compared with the kNN graph's d2.  Writes one
JSON file.

    python scripts/radius_timing.py --out profiles/r21_radius_timing.json
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import thin_timing  # noqa: E402
from pbnet_amd import mesh, synth  # noqa: E402
from thin_timing import timed  # noqa: E402


def raw_scan_with_far(target, jitter, outliers, seed=0):
    """thin_timing.raw_scan, draw for draw, which also says which points are the planted far ones."""
    base = synth.synth_room()["xyz"].astype(np.float64)
    rng = np.random.default_rng(seed)
    copies = max(1, round(target / base.shape[0]))
    xyz = np.concatenate([base + rng.normal(scale=jitter, size=base.shape) for _ in range(copies)])
    lo, hi = base.min(0), base.max(0)
    far = rng.uniform(lo - (hi - lo), hi + (hi - lo), (int(outliers * xyz.shape[0]), 3))
    is_far = np.concatenate([np.zeros(xyz.shape[0], bool), np.ones(far.shape[0], bool)])
    xyz = np.concatenate([xyz, far]).astype(np.float32)
    rgb = rng.integers(0, 256, xyz.shape).astype(np.float32)
    order = rng.permutation(xyz.shape[0])
    return xyz[order], rgb[order], is_far[order], copies


def walk_work(p, radius):
    """Candidate tests, cell reads and shells per query of k_radius_count without the cap: cloud.hip's grid rule with the
    cell a hair above the radius, shells until the bound of the scanned block is strictly above r2 or the block covers
    the grid (scripts/cloud_timing.py's recount with the radius in the k-th neighbour's place)."""
    n = p.shape[0]
    t_cap = int(min(1 << 20, max(4096, 4 * n)))
    mn, mx = p.min(0).astype(np.float64), p.max(0).astype(np.float64)
    h = max(float(np.float32(radius) * np.float32(1.0 + 2.0 ** -10)), (mx - mn).max() / 1023.0 * (1.0 + 1.0e-9))
    for _ in range(64):
        inv = 1.0 / h
        dims = np.minimum(np.floor((mx - mn) * inv), 1023).astype(np.int64) + 1
        if dims.prod() <= t_cap:
            break
        h *= 1.25
    h = 1.0 / inv
    t = (p.astype(np.float64) - mn) * inv
    c = np.minimum(np.floor(t).astype(np.int64), dims - 1)
    occ = np.zeros(tuple(dims), np.int64)
    np.add.at(occ, (c[:, 0], c[:, 1], c[:, 2]), 1)
    integral = np.zeros(tuple(dims + 1), np.int64)
    integral[1:, 1:, 1:] = occ.cumsum(0).cumsum(1).cumsum(2)

    def box(lo, hi):
        a, b = np.clip(lo, 0, dims - 1), np.clip(hi, 0, dims - 1) + 1
        s = 0
        for sx, ix in ((1, b[:, 0]), (-1, a[:, 0])):
            for sy, iy in ((1, b[:, 1]), (-1, a[:, 1])):
                for sz, iz in ((1, b[:, 2]), (-1, a[:, 2])):
                    s = s + sx * sy * sz * integral[ix, iy, iz]
        return s, np.prod(b - a, axis=1)

    r2 = float(np.float32(radius) * np.float32(radius))
    cand, cells, rings = np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(n, np.int64)
    live = np.ones(n, bool)
    for r in range(1024):
        pts_in, cells_in = box(c - r, c + r)
        cand[live], cells[live], rings[live] = pts_in[live] - 1, cells_in[live], r
        lo_gap = np.where(c - r > 0, t - (c - r), np.inf)
        hi_gap = np.where(c + r < dims - 1, (c + r + 1) - t, np.inf)
        gap = np.minimum(lo_gap, hi_gap).min(1)
        live &= ~(np.isinf(gap) | ((gap / inv) ** 2 > r2))
        if not live.any():
            break
    return {"cell_size": float(h), "grid": [int(d) for d in dims], "occupied_cells": int((occ > 0).sum())}, cand, cells, rings


def per_query(cand, cells, rings, which):
    return {"queries": int(which.sum()), "candidates_mean": float(cand[which].mean()), "candidates_max": int(cand[which].max()),
            "cells_mean": float(cells[which].mean()), "shells_mean": float(rings[which].mean() + 1),
            "stopping_after_shell_0": float(np.mean(rings[which] == 0)), "stopping_by_shell_1": float(np.mean(rings[which] <= 1))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=2000000)
    ap.add_argument("--pitch", type=float, default=0.02)
    ap.add_argument("--jitter", type=float, default=0.004)
    ap.add_argument("--outliers", type=float, default=0.01)
    ap.add_argument("--radius", type=float, default=None, help="default: 3 x pitch")
    ap.add_argument("--min-pts", type=int, default=6)
    ap.add_argument("--ratio", type=float, default=2.0)
    ap.add_argument("--k", type=int, default=16)
    ap.add_argument("--runs", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    radius = 3.0 * a.pitch if a.radius is None else a.radius
    dev = torch.device("cuda:0")
    xyz, rgb, is_far, copies = raw_scan_with_far(a.points, a.jitter, a.outliers)
    assert np.array_equal(xyz, thin_timing.raw_scan(a.points, a.jitter, a.outliers)[0])      # §9b's scan, point for point
    x, c = torch.from_numpy(xyz).to(dev), torch.from_numpy(rgb).to(dev)

    def front_radius():
        th = mesh.thin_points(x, c, a.pitch)
        keep = mesh.radius_outlier_mask(th["xyz"], radius, a.min_pts)
        raw = mesh.radius_raw_index(th["inverse"], keep, th["xyz"], radius)
        return th, keep, raw, th["xyz"][keep], th["rgb"][keep], th["count"][keep]

    def front_ratio():
        th = mesh.thin_points(x, c, a.pitch)
        idx, d2 = mesh.knn_graph(th["xyz"], k=a.k)
        keep, _ = mesh.outlier_mask(d2, a.ratio)
        raw = mesh.raw_index(th["inverse"], keep, idx)
        return th, keep, raw, th["xyz"][keep], th["rgb"][keep], th["count"][keep]

    rows = []
    for it in range(a.warmup + a.runs):
        t = {}
        th = mesh.thin_points(x, c, a.pitch)
        p = th["xyz"]
        count = mesh.radius_count(p, radius, cap=a.min_pts, times=t)
        t = {"radius_count(cap=min_pts): " + s: v for s, v in t.items()}
        t["radius_count(cap=min_pts), device"] = sum(t.values())
        full_t = {}
        full = mesh.radius_count(p, radius, times=full_t)
        t["radius_count(no cap): count stage"] = full_t["count"]
        keep, t["radius_outlier_mask (call: count, read-back, compare)"] = timed(
            lambda: mesh.radius_outlier_mask(p, radius, a.min_pts))
        raw, t["radius_raw_index (call: front, route, gather, read-back)"] = timed(
            lambda: mesh.radius_raw_index(th["inverse"], keep, p, radius))
        (idx, d2), t["knn_graph on the thinned points"] = timed(lambda: mesh.knn_graph(p, k=a.k))
        order = (front_radius, front_ratio) if it % 2 == 0 else (front_ratio, front_radius)
        for fn in order:
            out, t["whole front, " + ("outlier_radius" if fn is front_radius else "outlier_ratio")] = timed(fn)
            if fn is front_radius:
                f_rad = out
            else:
                f_rat = out
        if it >= a.warmup:
            rows.append(t)
    stages = {s: float(np.median([r[s] for r in rows])) for s in rows[0]}
    spread = {s: [float(min(r[s] for r in rows)), float(max(r[s] for r in rows))] for s in rows[0] if s.startswith("whole")}

    m = int(p.shape[0])
    inverse = th["inverse"].cpu().numpy()
    far_cell = np.zeros(m, bool)
    far_cell[inverse[is_far]] = True                         # cells that hold a planted far point

    def dropped(keep_d, raw_d):
        k, r = keep_d.cpu().numpy(), raw_d.cpu().numpy()
        return {"kept_cells": int(k.sum()), "cells_dropped": int((~k).sum()), "fraction_of_cells_dropped": float((~k).mean()),
                "planted_far_points": int(is_far.sum()), "planted_far_points_dropped": int((~k[inverse[is_far]]).sum()),
                "room_points_dropped": int((~k[inverse[~is_far]]).sum()), "raw_points_without_a_row": int((r < 0).sum()),
                "room_points_without_a_row": int((r[~is_far] < 0).sum())}

    r2 = np.float32(radius) * np.float32(radius)
    capk = mesh.radius_count(p, radius, cap=a.k)
    same_as_knn = bool(torch.equal(capk, (d2 <= float(r2)).sum(1).to(torch.int32)))
    same_mask = bool(torch.equal(keep, full >= a.min_pts) and torch.equal(count, full.clamp(max=a.min_pts)))
    grid, cand, cells, rings = walk_work(p.cpu().numpy(), radius)
    parent_path = os.path.join(ROOT, "profiles", "r18_thin_timing.json")
    parent = json.load(open(parent_path))["stages_ms"] if os.path.exists(parent_path) else None
    result = {"what": "radius filter on the raw-scan front, ms (HIP events; medians)", "device": torch.cuda.get_device_name(0),
              "raw_points": int(xyz.shape[0]), "room_copies": copies, "jitter_m": a.jitter, "pitch": a.pitch, "M": m,
              "radius": radius, "radius_over_pitch": radius / a.pitch, "min_pts": a.min_pts, "k": a.k, "ratio": a.ratio,
              "runs": a.runs, "warmup": a.warmup, "stages_ms": stages, "whole_front_min_max_ms": spread,
              "whole_front_is": "thin_points + mask + raw index + compaction of xyz / rgb / count, one torch event pair, "
                                "read-backs included; the two fronts alternate inside every run",
              "neighbours_within_radius": {"median": float(full.float().median().item()), "max": int(full.max().item()),
                                           "median_of_cells_with_a_far_point": float(np.median(full.cpu().numpy()[far_cell]))},
              "outlier_radius_drops": dropped(f_rad[1], f_rad[2]), "outlier_ratio_drops": dropped(f_rat[1], f_rat[2]),
              "walk_without_cap": dict(grid, all=per_query(cand, cells, rings, np.ones(m, bool)),
                                       cells_with_a_far_point=per_query(cand, cells, rings, far_cell),
                                       room_cells=per_query(cand, cells, rings, ~far_cell)),
              "checks": {"count_at_cap_k_equals_the_knn_graphs_d2_within_r2": same_as_knn,
                         "mask_and_capped_count_follow_the_full_count": same_mask},
              "parent_r18_thin_timing_stages_ms": parent}
    line = json.dumps(result, indent=1)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
