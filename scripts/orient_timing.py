"""What the normal orientation (csrc/orient.hip) costs on the bench-sized synthetic room of pbnet_amd/synth.py (~162 k
points, k = 16), by the method of scripts/cloud_timing.py: medians of --runs after --warmup, HIP events per stage of
pbn_cloud_orient_timed (edge codes, rounds, tail), the Boruvka rounds that merged something, knn_graph and point_normals
timed in the same run for scale, and segment_point's call time and segment count with and without the oriented normals.
When scipy imports, scipy.sparse.csgraph.minimum_spanning_tree over the same edges is the host figure.  With --variants the
library builds of `make orient_variant` (no read before the atomic, no reduction within the wave, neither) are timed too,
each in a process of its own.  Writes one JSON file.

    python scripts/orient_timing.py --out profiles/r22_orient_timing.json
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pbnet_amd import mesh, synth  # noqa: E402

VARIANTS = {"nopeek": "no read before the atomic", "nowave": "no reduction within the wave", "neither": "neither"}


def median_rows(rows):
    return {s: float(np.median([r[s] for r in rows])) for s in rows[0]}


def measure(x, k, runs, warmup, full):
    rows, seg = [], {}
    for it in range(warmup + runs):
        t = {}
        idx, _ = mesh.knn_graph(x, k=k, times=t)
        t["knn_graph"] = sum(t.pop(s) for s in mesh.CLOUD_STAGES)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        nl = mesh.point_normals(x, idx)
        ev[1].record()
        o = mesh.orient_normals(nl, idx, times=t)                            # synchronises
        t["point_normals"] = ev[0].elapsed_time(ev[1])
        t["orient_normals"] = sum(t[s] for s in mesh.ORIENT_STAGES)
        if full:
            edges = mesh.knn_edges(idx)
            for name, normals in (("viewpoint", nl), ("graph", o["nl"])):
                torch.cuda.synchronize()
                w0 = time.perf_counter()
                sup = mesh.segment_point(x, normals, edges)
                torch.cuda.synchronize()
                t["segment_point, %s normals (call wall time)" % name] = (time.perf_counter() - w0) * 1e3
                seg[name] = int(sup.max().item()) + 1
        if it >= warmup:
            rows.append(t)
    return median_rows(rows), o, nl, idx, seg


def host_mst_ms(nl, idx):
    try:
        from scipy.sparse import csr_matrix
        from scipy.sparse.csgraph import minimum_spanning_tree
    except ImportError:
        return None
    n, k = idx.shape
    i = np.repeat(np.arange(n), k)
    j = idx.reshape(-1).astype(np.int64)
    ok = (j >= 0) & (j != i)
    i, j = i[ok], j[ok]
    ts = []
    for _ in range(3):
        w0 = time.perf_counter()
        w = 1.0 - np.abs(np.einsum("ij,ij->i", nl[i], nl[j])) + 1.0e-9       # a stored zero would be no edge
        minimum_spanning_tree(csr_matrix((w, (i, j)), shape=(n, n)))
        ts.append(time.perf_counter() - w0)
    return 1e3 * float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=16)
    ap.add_argument("--runs", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    ap.add_argument("--variants", action="store_true")
    ap.add_argument("--stages-only", action="store_true", help="print the stage medians as one JSON line (a variant's child run)")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    pts = synth.synth_room()["xyz"]
    pts = (pts - pts.mean(0)).astype(np.float32)
    x = torch.from_numpy(pts).to(dev)
    stages, o, nl, idx, seg = measure(x, a.k, a.runs, a.warmup, not a.stages_only)
    if a.stages_only:
        print(json.dumps({s: stages[s] for s in mesh.ORIENT_STAGES + ("orient_normals",)}))
        return
    stats = o["stats"].tolist()
    result = {"what": "normal orientation over the kNN graph, HIP events per stage, ms", "device": torch.cuda.get_device_name(0),
              "points": int(pts.shape[0]), "k": a.k, "edge_slots": int(pts.shape[0]) * a.k, "runs": a.runs, "warmup": a.warmup,
              "stages_ms": stages, "rounds_launched": max(1, int(np.ceil(np.log2(max(pts.shape[0], 2))))),
              "rounds_that_merged": int(o["rounds"]), "trees": stats[0], "flipped": stats[1], "null": stats[2],
              "segments": seg, "host_scipy_mst_ms": host_mst_ms(nl.cpu().numpy().astype(np.float64), idx.cpu().numpy())}
    if a.variants:
        result["min_kernel_variants_ms"] = {}
        for name, what in VARIANTS.items():
            lib = os.path.join(ROOT, "pbnet_amd", "libpbnet_hip_orient_%s.so" % name)
            if not os.path.exists(lib):
                continue
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--stages-only", "--k", str(a.k), "--runs", str(a.runs),
                                  "--warmup", str(a.warmup)], env=dict(os.environ, PBNET_HIP_LIB=lib), capture_output=True,
                                 text=True, timeout=300, check=True).stdout
            result["min_kernel_variants_ms"][what] = json.loads(out.strip().splitlines()[-1])
    line = json.dumps(result, indent=1)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
