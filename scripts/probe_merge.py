#!/usr/bin/env python3
"""Time DeviceMerge.train_merge (pbnet_amd/loader.py) on a batch of four configs[1]-sized scenes with mix-up against the
float64 numpy restatement of the reference's trainMerge (tests/merge_ref.py) on the host.

    python scripts/probe_merge.py [--iters 20] [--warmup 3] [--cpu-iters 2]

GPU: CUDA events around each merge (generator draws, everything up to the batch dict), median of --iters after --warmup.
CPU: the restatement with the same draws, BLAS / OpenMP limited to 16 threads (numpy runs most of it on one).  Prints one
JSON line; DESIGN.md section 7 records the numbers."""
import argparse
import json
import os
import sys
import time

for v in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):
    os.environ.setdefault(v, "16")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np        # noqa: E402
import torch              # noqa: E402

import merge_ref          # noqa: E402
from pbnet_amd.config import get_config                            # noqa: E402
from pbnet_amd.loader import DeviceMerge, MergeDraws, SceneCache    # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cpu-iters", type=int, default=2)
    args = ap.parse_args()
    torch.set_num_threads(16)
    dev = torch.device("cuda:0")
    scenes = merge_ref.synth_scenes(range(2, 8))
    names = sorted(scenes)
    cache = SceneCache(scenes, dev, train=names, val=names)
    cfg = get_config(batch_size=4)
    merge = DeviceMerge(cache, cfg, seed=1)
    ids = [0, 1, 2, 3]
    times, points, reads = [], [], []
    for it in range(args.warmup + args.iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        out = merge.train_merge(ids)
        b.record()
        torch.cuda.synchronize()
        if it >= args.warmup:
            times.append(a.elapsed_time(b))
            points.append(int(out["xyz_original"].shape[0]))
            reads.append(merge.readbacks)
    # host restatement on the same kind of draws
    cpu = []
    for it in range(args.cpu_iters):
        gen = torch.Generator().manual_seed(100 + it)
        d = MergeDraws.draw_train(gen, 4, len(names), lambda i, m: cache.host[names[ids[i]]]["n"] + cache.host[names[m]]["n"],
                                  cfg.max_crop_p)
        merge.train_merge(ids, d)             # draws the noise grids (their shapes come from the device)
        t0 = time.perf_counter()
        merge_ref.train_merge(scenes, names, ids, d, cfg)
        cpu.append((time.perf_counter() - t0) * 1e3)
    res = dict(probe="train_merge", scenes=4, points_in=[int(cache.host[n]["n"]) for n in names[:4]],
               points_out_median=int(np.median(points)), gpu_ms_median=round(float(np.median(times)), 3),
               gpu_ms_min=round(float(np.min(times)), 3), gpu_ms_max=round(float(np.max(times)), 3), iters=args.iters,
               readbacks_per_merge=int(np.max(reads)), cpu_restatement_ms=[round(c, 1) for c in cpu], cpu_threads=16)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
