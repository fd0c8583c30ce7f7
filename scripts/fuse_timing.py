"""What depth-frame fusion (csrc/tsdf.hip) costs on the synthetic sequence of scripts/frames_timing.py (300 frames of
480 x 640, uint16 depth with about 20 % holes, colour on) at 2 cm voxels: medians of --runs after --warmup.

  fuse_frames   HIP events per stage of the measurement entries (the raw cloud's three, box + keys, point blocks, dilation +
                blocks, integrate, extract count, extract write), M_b, the voxel-frame pairs before and after the cull and
                the depth bytes gathered;
  torch         a plain torch statement of the same arithmetic done a frame at a time over the allocated voxels -- read S
                and Wt, project, gather, update, write back -- which is how tensor libraries integrate; its volume is
                compared with fuse_frames'.

No target is fixed: the two times and their ratio are reported where they land.  Writes one JSON file.

    python scripts/fuse_timing.py --out profiles/r28_fuse_timing.json
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
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from pbnet_amd import frames  # noqa: E402
from frames_timing import F, H, INTR, W, sequence  # noqa: E402


def torch_integrate(depth, colour, pose, origin, block_key, voxel, trunc):
    """Frame at a time over the allocated voxels, float64: the volume is read and written once per frame."""
    dev = depth.device
    m = block_key.shape[0]
    mask = (1 << 21) - 1
    b = torch.stack([block_key & mask, (block_key >> 21) & mask, (block_key >> 42) & mask], dim=1)
    idx = torch.arange(512, device=dev)
    i = torch.stack([idx & 7, (idx >> 3) & 7, idx >> 6], dim=1)
    p = torch.from_numpy(origin).to(dev)[None, None, :] + ((8 * b[:, None, :] + i[None]).double() + 0.5) * voxel
    p = p.reshape(-1, 3)
    S = torch.zeros(m * 512, dtype=torch.float64, device=dev)
    Wt = torch.zeros(m * 512, dtype=torch.int32, device=dev)
    C = torch.zeros(m * 512, 3, dtype=torch.float64, device=dev)
    fx, fy, cx, cy = INTR
    for f in range(depth.shape[0]):
        Rt = torch.from_numpy(np.ascontiguousarray(pose[f, :3, :3].T)).to(dev)
        t = pose[f, :3, 3]
        tc = [-((float(Rt[r, 0]) * t[0] + float(Rt[r, 1]) * t[1]) + float(Rt[r, 2]) * t[2]) for r in range(3)]
        pc = [((Rt[r, 0] * p[:, 0] + Rt[r, 1] * p[:, 1]) + Rt[r, 2] * p[:, 2]) + tc[r] for r in range(3)]
        zc = pc[2]
        ur, vr = torch.round((fx * pc[0]) / zc + cx), torch.round((fy * pc[1]) / zc + cy)
        ok = (zc > 0) & (ur >= 0) & (ur <= W - 1) & (vr >= 0) & (vr <= H - 1)
        u, v = torch.where(ok, ur, 0.0).long(), torch.where(ok, vr, 0.0).long()
        z = depth[f].to(torch.int32)[v, u].double() / 1000.0
        s = z - zc
        ok &= (z > 0) & ~(s < -trunc)
        S = torch.where(ok, S + torch.clamp(s / trunc, max=1.0), S)
        Wt = Wt + ok.to(torch.int32)
        C = torch.where(ok[:, None], C + colour[f][v, u].double(), C)
    seen = Wt > 0
    tsdf = torch.where(seen, S / Wt.double(), 0.0).float()
    return tsdf.reshape(m, 512), Wt.reshape(m, 512)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--frames", type=int, default=F)
    ap.add_argument("--voxel", type=float, default=0.02)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    depth, colour, pose = sequence(dev, a.frames)
    trunc = 4.0 * a.voxel
    rows, out = [], None
    for it in range(a.warmup + a.runs):
        t = {}
        try:
            out = frames.fuse_frames(depth, pose, INTR, colour, voxel=a.voxel, return_volume=True, times=t)   # synchronises
        except ValueError as refusal:                          # too many blocks for this voxel size: report it, time nothing
            line = json.dumps({"what": "depth-frame fusion", "frames": a.frames, "voxel": a.voxel, "refused": str(refusal)}, indent=1)
            print(line)
            if a.out:
                with open(a.out, "w") as fh:
                    fh.write(line + "\n")
            return
        if it >= a.warmup:
            rows.append(t)
    names = frames.FRAMES_STAGES + frames.FUSE_STAGES
    stages = {s: float(np.median([r[s] for r in rows])) for s in names}
    stages["total"] = sum(stages.values())
    stats = rows[-1]["stats"]
    m_b = out["n_blocks"]
    live = int((~out["skipped"]).sum())

    def torch_run():
        return torch_integrate(depth, colour, pose, out["origin"], out["block_key"], a.voxel, trunc)

    walls = []
    for it in range(a.warmup + a.runs):
        torch.cuda.synchronize()
        w0 = time.perf_counter()
        tsdf, wt = torch_run()
        torch.cuda.synchronize()
        if it >= a.warmup:
            walls.append(1e3 * (time.perf_counter() - w0))
    torch_ms = float(np.median(walls))
    result = {"what": "depth-frame fusion, ms (medians)", "device": torch.cuda.get_device_name(0), "frames": a.frames, "height": H,
              "width": W, "voxel": a.voxel, "trunc": trunc, "runs": a.runs, "warmup": a.warmup, "form": "256 lanes x 2 voxels",
              "stages_ms": stages, "n_blocks": m_b, "surface_rows": int(out["xyz"].shape[0]),
              "voxel_frame_pairs": {"before_cull": m_b * 512 * live, "after_cull": stats["block_frame_pairs"] * 512},
              "depth_bytes_gathered": stats["depth_samples"] * depth.element_size(),
              "torch_frame_at_a_time_ms": torch_ms, "torch_over_integrate": torch_ms / stages["integrate"],
              "torch_agreement": {"same_weights": bool(torch.equal(wt, out["vol_weight"])),
                                  "max_abs_tsdf_diff": float((tsdf - out["tsdf"]).abs().max()) if m_b else 0.0}}
    line = json.dumps(result, indent=1)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
