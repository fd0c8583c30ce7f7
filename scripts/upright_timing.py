"""What the floor plane and upright frame (csrc/upright.hip) cost on the bench-sized synthetic room of pbnet_amd/synth.py
(~161 k points) tilted by a fixed rotation, at H = 1024, by the method of scripts/orient_timing.py: medians of --runs after
--warmup, HIP events per stage of pbn_cloud_upright_timed (hypotheses, score, select + refit, apply).  The score stage is
also given as point-plane tests per second (from a second run without a hint, in which no hypothesis dies by the tilt
rule), next to the VALU bound derived from the instruction count of the score kernel's inner loop in the built code
object (llvm-objdump on the library; None when the tool is missing), and next to the wall time of the numpy restatement
(tests/upright_ref.py) on the host.  With --variants the library build of
`make upright_variant` (the other point-staging form: wave-uniform global loads, no LDS) is timed too, in a process of its
own.  Writes one JSON file.

    python scripts/upright_timing.py --variants --out profiles/r24_upright_timing.json
"""
import argparse
import glob
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from pbnet_amd import _native, mesh, synth  # noqa: E402

VARIANTS = {"uniform": "wave-uniform global loads, no LDS"}
TILT_AXIS, TILT_DEG = (1.0, 2.0, 0.5), 25.0
THRESHOLD, HYPOTHESES = 0.02, 1024
# MI355X: 256 CUs x 4 SIMDs; a wave64 VALU instruction issues over 2 cycles of its SIMD; 2.4 GHz
SIMDS, CYCLES_PER_VALU, CLOCK_HZ = 256 * 4, 2, 2.4e9


def tilted_room():
    import upright_ref as U
    pts = synth.synth_room()["xyz"].astype(np.float64)
    pts = pts - pts.mean(0)
    R = U._rot(TILT_AXIS, TILT_DEG)
    return (pts @ R.T).astype(np.float32), R @ np.array([0.0, 0.0, 1.0])


def measure(x, up, runs, warmup):
    rows = []
    for it in range(warmup + runs):
        t = {}
        out = mesh.upright(x, THRESHOLD, hypotheses=HYPOTHESES, up_hint=up, times=t)       # synchronises
        t["upright"] = sum(t[s] for s in mesh.UPRIGHT_STAGES)
        if it >= warmup:
            rows.append(t)
    return {s: float(np.median([r[s] for r in rows])) for s in rows[0]}, out


def inner_loop_valu(lib):
    """(VALU instructions, points) of the score kernel's hottest loop block in the library's gfx950 code object."""
    objdump = shutil.which("llvm-objdump") or "/opt/rocm/llvm/bin/llvm-objdump"
    if not os.path.exists(objdump):
        return None
    with tempfile.TemporaryDirectory() as tmp:
        local = os.path.join(tmp, "lib.so")
        shutil.copy(lib, local)
        try:
            subprocess.run([objdump, "--offloading", local], cwd=tmp, capture_output=True, timeout=300, check=True)
            text = None
            for obj in sorted(glob.glob(os.path.join(tmp, "lib.so*gfx950*"))):      # one code object per translation unit
                symbol = score_symbol(objdump, obj)
                if symbol:
                    text = subprocess.run([objdump, "-d", "--disassemble-symbols=" + symbol, obj], capture_output=True,
                                          text=True, timeout=300, check=True).stdout
                    break
            if text is None:
                return None
        except (subprocess.SubprocessError, OSError, LookupError):
            return None
    # basic blocks end at a branch; the inner loop is the block with the most compares against t that branches backwards
    best = None
    block = []
    for line in text.splitlines():
        m = re.match(r"\s+([sv]_\w+|ds_\w+|global_\w+|buffer_\w+|flat_\w+)\b", line)
        if not m:
            continue
        block.append(m.group(1))
        if m.group(1).startswith(("s_cbranch", "s_branch", "s_endpgm")):
            valu = [i for i in block if i.startswith("v_")]
            points = sum(1 for i in valu if i.startswith("v_cmp_gt_f32") or i.startswith("v_cmp_lt_f32")) or 0
            if points and (best is None or len(valu) > best[0]):
                best = (len(valu), points)
            block = []
    return best


def score_symbol(objdump, obj):
    syms = subprocess.run([objdump, "-t", obj], capture_output=True, text=True, timeout=300, check=True).stdout
    for line in syms.splitlines():
        name = line.split()[-1] if line.split() else ""
        if "k_upr_score" in name and "." not in name:          # the function, not its .kd / .num_vgpr / ... companions
            return name
    return None


def host_ms(pts, up):
    import upright_ref as U
    w0 = time.perf_counter()
    ref = U.upright_ref(pts, THRESHOLD, HYPOTHESES, up_hint=up)
    return 1e3 * (time.perf_counter() - w0), ref


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    ap.add_argument("--variants", action="store_true")
    ap.add_argument("--stages-only", action="store_true", help="print the stage medians as one JSON line (a variant's child run)")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    pts, up = tilted_room()
    x = torch.from_numpy(pts).to(dev)
    stages, out = measure(x, tuple(up), a.runs, a.warmup)
    # without a hint no hypothesis dies by the tilt rule, so every lane of the score kernel works: the rate to hold the bound to
    free, free_out = measure(x, None, a.runs, a.warmup)
    n = int(pts.shape[0])
    tests = float(n) * HYPOTHESES
    if a.stages_only:
        print(json.dumps(dict(stages, info=out["info"].tolist(), score_no_hint=free["score"])))
        return
    import upright_ref as U
    loop = inner_loop_valu(_native.LIB_PATH if hasattr(_native, "LIB_PATH") else os.path.join(ROOT, "pbnet_amd", "libpbnet_hip.so"))
    bound = None
    if loop:
        per_point = loop[0] / loop[1]                          # VALU instructions per (point, wave of 64 hypotheses)
        bound = SIMDS * CLOCK_HZ / (CYCLES_PER_VALU * per_point) * 64
    ms, ref = host_ms(pts, tuple(up))
    result = {"what": "floor plane and upright frame, HIP events per stage, ms", "device": torch.cuda.get_device_name(0),
              "points": n, "hypotheses": HYPOTHESES, "threshold": THRESHOLD, "tilt_deg": TILT_DEG, "runs": a.runs, "warmup": a.warmup,
              "point_staging": "LDS float4 rows, broadcast reads", "stages_ms": stages, "info": out["info"].tolist(),
              "angle_to_true_up_deg": float(np.rad2deg(U.angle_to(out["plane"][:3].cpu().numpy(), up))),
              "no_hint_stages_ms": free, "no_hint_info": free_out["info"].tolist(),
              "point_plane_tests": tests, "score_tests_per_s": tests / (free["score"] * 1e-3),
              "inner_loop": None if not loop else {"valu_instructions": loop[0], "points": loop[1]},
              "valu_bound_tests_per_s": bound,
              "score_fraction_of_valu_bound": None if not bound else tests / (free["score"] * 1e-3) / bound,
              "host_numpy_restatement_ms": ms,
              "host_agrees": bool(np.array_equal(ref["info"], out["info"].cpu().numpy())
                                  and ref["moments"].tobytes() == out["moments"].cpu().numpy().tobytes())}
    if a.variants:
        result["point_staging_variants_ms"] = {}
        for name, what in VARIANTS.items():
            lib = os.path.join(ROOT, "pbnet_amd", "libpbnet_hip_upright_%s.so" % name)
            if not os.path.exists(lib):
                continue
            child = subprocess.run([sys.executable, os.path.abspath(__file__), "--stages-only", "--runs", str(a.runs),
                                    "--warmup", str(a.warmup)], env=dict(os.environ, PBNET_HIP_LIB=lib), capture_output=True,
                                   text=True, timeout=300, check=True).stdout
            row = json.loads(child.strip().splitlines()[-1])
            vloop = inner_loop_valu(lib)
            result["point_staging_variants_ms"][what] = dict(
                row, score_tests_per_s=tests / (row["score_no_hint"] * 1e-3),
                inner_loop=None if not vloop else {"valu_instructions": vloop[0], "points": vloop[1]},
                same_info=row["info"] == result["info"])
    line = json.dumps(result, indent=1)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
