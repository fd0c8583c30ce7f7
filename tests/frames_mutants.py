"""A second statement of the posed-depth-frames contract, written the way csrc/frames.hip works -- one pixel at a time, the
validity rules in the kernel's order, Python floats (IEEE float64, one rounding per operation), rows appended in the order
the workgroups, chunks and lanes emit them -- with one switch per deliberate mistake.  With mutant=None it must equal
tests/frames_ref.py bit for bit on every designed case of tests/frames_cases.py; a mutant that equals it on every case shows
that the set is too weak (tests/test_frames_cases_cpu.py holds the kill matrix)."""
import math

import numpy as np

F32 = np.float32

MUTANTS = ("centre_half", "r_transposed", "z_over_fx", "stride_neighbours", "border_is_edge", "invalid_neighbour_is_edge",
           "edge_times_zn", "skip_reads_bottom_row", "depth_max_exclusive", "column_major")


def _z(d, is_u16, scale):
    return float(d) / scale if is_u16 else float(d)


def _measured(z, lo, hi, mutant):
    top = z < hi if mutant == "depth_max_exclusive" else z <= hi
    return math.isfinite(z) and z > 0.0 and z >= lo and top


def _f32(x):
    with np.errstate(over="ignore"):
        return F32(x)


def decode(case, mutant=None):
    """The dict of tests/frames_ref.py's frames_ref for a case of tests/frames_cases.py."""
    assert mutant is None or mutant in MUTANTS, mutant
    depth = np.asarray(case["depth"])
    is_u16 = depth.dtype == np.uint16
    n_f, h, w = depth.shape
    pose = np.asarray(case["pose"], np.float64).reshape(n_f, 4, 4)
    intr = np.broadcast_to(np.asarray(case["intr"], np.float64), (n_f, 4))
    colour = case.get("colour")
    kw = case.get("kw", {})
    scale, lo, hi = float(kw.get("depth_scale", 1000.0)), float(kw.get("depth_min", 0.0)), float(kw.get("depth_max", math.inf))
    stride, edge = int(kw.get("stride", 1)), kw.get("edge")
    edge = 0.0 if edge is None else float(edge)
    d = depth.tolist()
    rows = []                                                  # (order key, pixel id, X, Y, Z)
    starts = [0]
    for f in range(n_f):
        P = pose[f].tolist()
        checked = P[:4] if mutant == "skip_reads_bottom_row" else P[:3]
        pose_ok = all(math.isfinite(x) for row in checked for x in row)
        R = [[P[c][r] for c in range(3)] for r in range(3)] if mutant == "r_transposed" else [P[r][:3] for r in range(3)]
        t = [P[r][3] for r in range(3)]
        fx, fy, cx, cy = intr[f].tolist()
        count = 0
        for v in range(0, h, stride):
            for u in range(0, w, stride):
                if not pose_ok:
                    continue
                z = _z(d[f][v][u], is_u16, scale)
                if not _measured(z, lo, hi, mutant):
                    continue
                if edge > 0.0:
                    step = stride if mutant == "stride_neighbours" else 1
                    is_edge = False
                    for vn, un in ((v, u - step), (v, u + step), (v - step, u), (v + step, u)):
                        if not (0 <= vn < h and 0 <= un < w):
                            is_edge |= mutant == "border_is_edge"
                            continue
                        zn = _z(d[f][vn][un], is_u16, scale)
                        if not _measured(zn, lo, hi, mutant):
                            is_edge |= mutant == "invalid_neighbour_is_edge"
                            continue
                        is_edge |= abs(zn - z) > edge * (zn if mutant == "edge_times_zn" else z)
                    if is_edge:
                        continue
                half = 0.5 if mutant == "centre_half" else 0.0
                if mutant == "z_over_fx":
                    xc, yc = ((float(u) + half) - cx) * (z / fx), ((float(v) + half) - cy) * (z / fy)
                else:
                    xc, yc = (((float(u) + half) - cx) * z) / fx, (((float(v) + half) - cy) * z) / fy
                world = [_f32(((R[r][0] * xc + R[r][1] * yc) + R[r][2] * z) + t[r]) for r in range(3)]
                if not all(np.isfinite(world)):
                    continue
                pid = (f * h + v) * w + u
                rows.append(((f, u, v) if mutant == "column_major" else (pid,), pid, world))
                count += 1
        starts.append(starts[-1] + count)
    rows.sort(key=lambda r: r[0])
    pixel = np.array([r[1] for r in rows], np.int32).reshape(-1)
    out = {"xyz": np.array([r[2] for r in rows], F32).reshape(-1, 3), "pixel": pixel, "n": len(rows),
           "frame_start": np.array(starts, np.int32)}
    if colour is not None:
        out["rgb"] = np.asarray(colour, np.uint8).reshape(-1, 3)[pixel].astype(F32).reshape(-1, 3)
    return out


def same(a, b):
    """Bit for bit: floats by their bits, integers by value."""
    if set(a) != set(b):
        return False
    for k in a:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        if x.shape != y.shape or x.dtype != y.dtype or x.tobytes() != y.tobytes():
            return False
    return True
