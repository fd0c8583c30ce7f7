"""What the posed-depth-frames front end (csrc/frames.hip) costs on a synthetic sequence of 300 frames of 480 x 640 (uint16
depth with about 20 % holes, colour on), by the method of scripts/upright_timing.py: medians of --runs after --warmup.

  frames_to_points   HIP events per stage of the measurement entries (count, scan + starts, write) and the wall time of the
                     plain call, its one read-back included; once more with the edge test on, which is what the neighbour
                     reads cost when they come straight from the cache;
  torch              the same cloud by the plain torch expression a user writes today -- meshgrid, mask, nonzero, gathers,
                     matmul -- in float64 (the same arithmetic; its result is compared) and in float32 (what is usually
                     written);
  copy               a device-to-device copy that moves exactly the bytes the write pass reads (every depth sample, the
                     colour of the survivors) and writes (xyz, rgb, pixel): the bandwidth yardstick.

Writes one JSON file.

    python scripts/frames_timing.py --out profiles/r27_frames_timing.json
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

from pbnet_amd import frames  # noqa: E402

F, H, W = 300, 480, 640
INTR = (577.87, 577.87, 319.5, 239.5)             # ScanNet's depth camera
HOLES, EDGE = 0.2, 0.05


def sequence(dev, n_frames):
    """Slanted planes with ripples between 0.8 and 4.5 m, 20 % holes in blocks of 8 x 8 (holes come in patches), random colour,
    a camera that walks a circle."""
    g = torch.Generator(device=dev).manual_seed(7)
    v = torch.arange(H, device=dev, dtype=torch.float32)[None, :, None]
    u = torch.arange(W, device=dev, dtype=torch.float32)[None, None, :]
    f = torch.arange(n_frames, device=dev, dtype=torch.float32)[:, None, None]
    z = 2.6 + 1.2 * torch.sin(0.004 * u + 0.1 * f) + 0.6 * torch.cos(0.006 * v - 0.07 * f) + 0.02 * torch.rand(n_frames, H, W, device=dev, generator=g)
    holes = torch.rand(n_frames, H // 8, W // 8, device=dev, generator=g) < HOLES
    holes = holes.repeat_interleave(8, 1).repeat_interleave(8, 2)
    depth = (z * 1000.0).round().clamp(1, 65535).to(torch.int32)
    depth[holes] = 0
    depth = depth.to(torch.uint16)
    colour = torch.randint(0, 256, (n_frames, H, W, 3), device=dev, dtype=torch.uint8, generator=g)
    a = np.linspace(0.0, 2.0 * np.pi, n_frames, endpoint=False)
    pose = np.tile(np.eye(4), (n_frames, 1, 1))
    pose[:, 0, 0], pose[:, 0, 2], pose[:, 2, 0], pose[:, 2, 2] = np.cos(a), np.sin(a), -np.sin(a), np.cos(a)
    pose[:, 0, 3], pose[:, 1, 3], pose[:, 2, 3] = 2.0 * np.cos(a), 0.1 * np.sin(3 * a), 2.0 * np.sin(a)
    return depth, colour, pose


def torch_expression(depth, colour, pose_d, intr, dtype):
    """What a user writes today: [F, H, W] temporaries, a mask, nonzero, gathers and a batched matmul."""
    n_f = depth.shape[0]
    fx, fy, cx, cy = intr
    d32 = depth.to(torch.int32)                                # torch has no uint16 arithmetic
    z = d32.to(dtype) / 1000.0
    v, u = torch.meshgrid(torch.arange(H, device=depth.device, dtype=dtype), torch.arange(W, device=depth.device, dtype=dtype),
                          indexing="ij")
    cam = torch.stack([(u - cx) * z / fx, (v - cy) * z / fy, z], dim=-1)                     # [F, H, W, 3]
    world = torch.matmul(cam.reshape(n_f, H * W, 3), pose_d[:, :3, :3].to(dtype).transpose(1, 2)) + pose_d[:, None, :3, 3].to(dtype)
    mask = (d32 > 0).reshape(-1)
    pixel = torch.nonzero(mask).reshape(-1)
    xyz = world.reshape(-1, 3)[pixel].float()
    rgb = colour.reshape(-1, 3)[pixel].float()
    return xyz, rgb, pixel.to(torch.int32)


def wall_ms(fn, runs, warmup):
    rows = []
    for it in range(warmup + runs):
        torch.cuda.synchronize()
        w0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        if it >= warmup:
            rows.append(1e3 * (time.perf_counter() - w0))
    return float(np.median(rows)), out


def staged_ms(depth, colour, pose, edge, runs, warmup):
    rows = []
    for it in range(warmup + runs):
        t = {}
        out = frames.frames_to_points(depth, pose, INTR, colour, edge=edge, times=t)        # synchronises
        if it >= warmup:
            rows.append(t)
    med = {s: float(np.median([r[s] for r in rows])) for s in frames.FRAMES_STAGES}
    med["total"] = sum(med.values())
    return med, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--frames", type=int, default=F)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    depth, colour, pose = sequence(dev, a.frames)
    pose_d = torch.from_numpy(pose).to(dev)
    pixels = depth.numel()

    stages, out = staged_ms(depth, colour, pose, None, a.runs, a.warmup)
    stages_edge, out_edge = staged_ms(depth, colour, pose, EDGE, a.runs, a.warmup)
    plain, _ = wall_ms(lambda: frames.frames_to_points(depth, pose, INTR, colour), a.runs, a.warmup)
    n = int(out["xyz"].shape[0])

    torch_ms, agree = {}, {}
    for name, dtype in (("float64", torch.float64), ("float32", torch.float32)):
        torch_ms[name], (xyz, rgb, pixel) = wall_ms(lambda: torch_expression(depth, colour, pose_d, INTR, dtype), a.runs, a.warmup)
        agree[name] = {"same_pixels": bool(torch.equal(pixel, out["pixel"])), "same_rgb": bool(torch.equal(rgb, out["rgb"])),
                       "max_abs_xyz_diff": float((xyz - out["xyz"]).abs().max()) if n else 0.0,
                       "same_xyz_bytes": bool(torch.equal(xyz, out["xyz"]))}
        del xyz, rgb, pixel

    read_bytes = pixels * depth.element_size() + 3 * n
    write_bytes = n * (12 + 12 + 4)
    half = (read_bytes + write_bytes) // 2                    # a copy of b bytes reads b and writes b
    src = torch.empty(half, dtype=torch.uint8, device=dev)
    dst = torch.empty_like(src)
    copy_ms, _ = wall_ms(lambda: dst.copy_(src), a.runs + 4, a.warmup)
    traffic = float(read_bytes + write_bytes)

    result = {"what": "posed depth frames to a compacted cloud, ms (medians)", "device": torch.cuda.get_device_name(0),
              "frames": a.frames, "height": H, "width": W, "pixels": pixels, "points": n, "holes": 1.0 - n / pixels,
              "runs": a.runs, "warmup": a.warmup, "block_pixels": 1024, "neighbour_depths": "straight from the cache (no LDS tile)",
              "stages_ms": stages, "stages_edge_ms": dict(stages_edge, edge=EDGE, points=int(out_edge["xyz"].shape[0])),
              "frames_to_points_wall_ms": plain, "torch_expression_wall_ms": torch_ms, "torch_agreement": agree,
              "speedup_over_torch": {k: v / plain for k, v in torch_ms.items()},
              "write_pass_bytes": {"read": read_bytes, "written": write_bytes},
              "copy_ms": copy_ms, "copy_gb_per_s": traffic / (copy_ms * 1e-3) / 1e9,
              "write_gb_per_s": traffic / (stages["write"] * 1e-3) / 1e9,
              "write_fraction_of_copy": copy_ms / stages["write"],
              "edge_cost_ms": {s: stages_edge[s] - stages[s] for s in ("count", "write")}}
    line = json.dumps(result, indent=1)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
