"""numpy restatement of csrc/cloud.hip's fixed-radius contract (pbnet_amd.mesh.radius_count / radius_outlier_mask /
radius_raw_index), and the designed cases as data (every one generated from a seed: nothing is committed as a fixture).

d2       d2(i, j) = ((dx*dx + dy*dy) + dz*dz), dx = x[j] - x[i], in float32 (tests/cloud_ref.py's: numpy's element-wise
         float32 arithmetic is IEEE-rounded per operation and never fused).
radius   rf = float32(radius), r2 = float32(rf * rf); j is a neighbour of i when j != i and d2(i, j) <= r2.
count    count[i] = min(number of neighbours, cap); cap None = 2^31 - 1.
mask     keep[i] = count with cap = min_pts >= min_pts.
route    rank = the exclusive scan of keep, t = inverse[i]: rank[t] when keep[t]; else rank[j*], j* the KEPT point with the
         smallest key (bits of d2(t, j), j) among those with d2 <= r2; else -1.

`wrong=` names a mistake the kernels could make (COUNT_WRONG, ROUTE_WRONG); tests/test_radius_ref_cpu.py shows for each a
designed case on which the restatement with that mistake differs.
"""
import numpy as np

import cloud_cases

F32 = np.float32
I32 = np.int32
MAX_CAP = (1 << 31) - 1
COUNT_WRONG = ("lt", "self", "nocap", "r2_f64", "d2_f64")
ROUTE_WRONG = ("lt", "any", "tie_high", "beyond", "rank_all")


def r2_of(radius):
    with np.errstate(over="ignore", under="ignore"):
        rf = F32(radius)
        if not (np.isfinite(rf) and rf > 0):
            raise ValueError("radius must be positive and finite as a float32, got %r" % (radius,))
        return F32(rf * rf)


def d2_rows(xyz, lo, hi, f64=False):
    """d2(i, j) for i in [lo, hi) and every j: float32 [hi - lo, N] (float64 sums of the float32 differences with f64)."""
    q = xyz[lo:hi]
    with np.errstate(over="ignore", under="ignore"):
        dx = xyz[None, :, 0] - q[:, None, 0]
        dy = xyz[None, :, 1] - q[:, None, 1]
        dz = xyz[None, :, 2] - q[:, None, 2]
        if f64:
            dx, dy, dz = dx.astype(np.float64), dy.astype(np.float64), dz.astype(np.float64)
        return (dx * dx + dy * dy) + dz * dz


def radius_count_ref(xyz, radius, cap=None, wrong=None, chunk=512):
    """count int32 [N]."""
    assert wrong is None or wrong in COUNT_WRONG
    xyz = np.ascontiguousarray(xyz, F32).reshape(-1, 3)
    cap = MAX_CAP if cap is None else int(cap)
    if not 1 <= cap <= MAX_CAP:
        raise ValueError("cap must lie in 1..2^31 - 1, got %r" % (cap,))
    r2 = r2_of(radius)
    if wrong == "r2_f64":
        r2 = np.float64(F32(radius)) * np.float64(F32(radius))
    n = xyz.shape[0]
    out = np.zeros(n, np.int64)
    for lo in range(0, n, chunk):
        d2 = d2_rows(xyz, lo, min(lo + chunk, n), f64=wrong == "d2_f64")
        assert d2.dtype == (np.float64 if wrong == "d2_f64" else F32)
        near = d2 < r2 if wrong == "lt" else d2 <= r2
        if wrong != "self":
            rows = np.arange(near.shape[0])
            near[rows, lo + rows] = False                    # self: excluded by index
        out[lo:lo + chunk] = near.sum(1)
    if wrong != "nocap":
        out = np.minimum(out, cap)
    return out.astype(I32)


def radius_mask_ref(xyz, radius, min_pts, wrong=None):
    """keep bool [N]."""
    if int(min_pts) < 1:
        raise ValueError("min_pts must be at least 1, got %r" % (min_pts,))
    return radius_count_ref(xyz, radius, cap=int(min_pts), wrong=wrong) >= int(min_pts)


def radius_raw_index_ref(inverse, keep, xyz, radius, wrong=None):
    """int32 [N_raw]."""
    assert wrong is None or wrong in ROUTE_WRONG
    xyz = np.ascontiguousarray(xyz, F32).reshape(-1, 3)
    keep = np.asarray(keep, bool)
    inverse = np.asarray(inverse, I32)
    r2 = r2_of(radius)
    m = xyz.shape[0]
    rank = np.arange(m, dtype=I32) if wrong == "rank_all" else (np.cumsum(keep) - keep).astype(I32)
    route = np.full(m, -1, I32)
    route[keep] = rank[keep]
    j = np.arange(m, dtype=np.uint64)
    none = np.uint64(0xffffffffffffffff)
    for t in np.flatnonzero(~keep):
        d2 = d2_rows(xyz, t, t + 1)[0]
        ok = np.ones(m, bool) if wrong == "beyond" else (d2 < r2 if wrong == "lt" else d2 <= r2)
        ok &= np.arange(m) != t if wrong == "any" else keep
        bits = d2.view(np.uint32).astype(np.uint64)
        key = (bits << np.uint64(32)) | (np.uint64(m) - j if wrong == "tie_high" else j)
        key = np.where(ok, key, none)
        best = int(np.argmin(key))
        if key[best] != none:
            route[t] = rank[best]
    out = np.full(inverse.shape[0], -1, I32)
    ok = (inverse >= 0) & (inverse < m)
    out[ok] = route[inverse[ok]]
    return out


# ------------------------------------------------------------------------------------------------ plain Python loops
def d2_scalar(p, q):
    """d2 from point q to point p, one float32 operation at a time."""
    dx, dy, dz = F32(p[0] - q[0]), F32(p[1] - q[1]), F32(p[2] - q[2])
    return F32(F32(F32(dx * dx) + F32(dy * dy)) + F32(dz * dz))


def radius_count_loop(xyz, radius, cap=None, rows=None):
    """The count said a second way: a double loop over float32 scalars that stops at cap.  `rows` limits the queries."""
    xyz = np.asarray(xyz, F32)
    n = xyz.shape[0]
    cap = MAX_CAP if cap is None else cap
    rf = F32(radius)
    with np.errstate(over="ignore", under="ignore"):
        r2 = F32(rf * rf)
        out = {}
        for i in (range(n) if rows is None else rows):
            c = 0
            for j in range(n):
                if j != i and d2_scalar(xyz[j], xyz[i]) <= r2:
                    c += 1
                    if c == cap:
                        break
            out[i] = c
    return out


def radius_raw_index_loop(inverse, keep, xyz, radius):
    xyz = np.asarray(xyz, F32)
    rf = F32(radius)
    r2 = F32(rf * rf)
    rank, c = [], 0
    for kept in keep:
        rank.append(c)
        c += int(kept)
    out = []
    for t in inverse:
        if keep[t]:
            out.append(rank[t])
            continue
        best = None
        for j in range(xyz.shape[0]):
            d = d2_scalar(xyz[j], xyz[t])
            if keep[j] and d <= r2:
                key = (int(np.array(d, F32).view(np.uint32)), j)
                if best is None or key < best:
                    best = key
        out.append(-1 if best is None else rank[best[1]])
    return np.array(out, I32).reshape(-1)


# --------------------------------------------------------------------------------------------------- designed cases
BELOW_ONE = float(np.nextafter(F32(1.0), F32(0.0)))          # one float32 ulp below 1
CELLS = (None, "radius", 1e-30, 1e30)                        # the GPU tier's cell sizes; "radius" = the case's radius
CAPS = (1, 4, None)


def _square_rounds(up):
    """The first float32 radius above 1.5 whose float32 square is above (`up`) / below the exact square."""
    for i in range(1, 200):
        rf = F32(1.5) + F32(i) * F32(2.0 ** -23)
        exact = np.float64(rf) * np.float64(rf)
        if (np.float64(F32(rf * rf)) > exact) if up else (np.float64(F32(rf * rf)) < exact):
            return rf
    raise AssertionError("no such radius")


def _pair(rf):
    """Two points rf apart along x: their computed d2 is exactly float32(rf * rf) = r2."""
    return np.array([[0, 0, 0], [rf, 0, 0]], F32)


def _count_cases():
    """name -> (xyz float32 [N, 3], radius)."""
    g = cloud_cases
    c = {"n0": (np.zeros((0, 3), F32), 1.0), "n1": (g.gauss(1), 1.0), "n2": (g.gauss(2), 3.0)}
    for n in (63, 64, 65, 255, 256, 257):
        c["n%d" % n] = (g.gauss(n), 0.7)
    c["coincident"] = (g.coincident(), 0.1)
    c["coincident_r2_zero"] = (np.concatenate([g.coincident(), g.coincident() + F32(1e-3)]), 1e-30)   # r2 underflows to 0
    c["lattice_r1"] = (g.lattice(), 1.0)                     # neighbours exactly at d2 == r2, points on cell faces
    c["lattice_r1.5"] = (g.lattice(), 1.5)
    c["lattice_below1"] = (g.lattice(), BELOW_ONE)
    c["sheet"] = (g.sheet(), 0.05)
    c["blob"] = (g.blob_and_outlier(), g.BLOB_CELL)          # the last point is 40 cells of the radius away
    c["line"] = (g.line(), g.LINE_CELL)
    c["offset"] = (g.offset(), 0.5)
    c["room_5cm"] = (g.room(1), 0.05)
    c["room_20cm"] = (g.room(1), 0.2)
    c["r2_rounds_up"] = (_pair(_square_rounds(True)), float(_square_rounds(True)))
    c["r2_rounds_down"] = (_pair(_square_rounds(False)), float(_square_rounds(False)))
    return c


def _route_cases():
    """name -> (inverse int32 [N_raw], keep bool [M], xyz float32 [M, 3], radius)."""
    def case(points, keep, radius=1.0, inverse=None):
        xyz = np.array(points, F32).reshape(-1, 3)
        inv = np.arange(xyz.shape[0]) if inverse is None else inverse
        return np.asarray(inv, I32), np.array(keep, bool), xyz, radius
    c = {}
    # point 0 is dropped and precedes its answer: a rank is not an index
    c["one_kept"] = case([[0.5, 0, 0], [0, 0, 0], [5, 0, 0]], [0, 1, 1])
    c["none_within"] = case([[0.5, 0, 0], [2, 0, 0], [5, 0, 0]], [0, 1, 1])
    c["tie"] = case([[9, 9, 9], [0.5, 0, 0], [-0.5, 0, 0], [0, 0, 0]], [1, 1, 1, 0])
    # 2 and 3 are each other's nearest and both dropped; their own rank (2) is not their answer's (1)
    c["nearest_is_dropped"] = case([[7, 0, 0], [0.6, 0, 0], [0, 0, 0], [0.1, 0, 0]], [1, 1, 0, 0])
    c["at_r2"] = case([[0, 0, 0], [1, 0, 0]], [0, 1])
    c["all_kept"] = case(cloud_cases.gauss(65), np.ones(65, bool), 0.5)
    c["none_kept"] = case(cloud_cases.gauss(65), np.zeros(65, bool), 0.5)
    c["repeated_rows"] = case([[0.5, 0, 0], [0, 0, 0], [5, 0, 0], [5.2, 0, 0]], [0, 1, 1, 0],
                              inverse=[3, 3, 0, 1, 1, 2, 0, 3, 2])
    c["n_raw0"] = case([[0.5, 0, 0], [0, 0, 0]], [0, 1], inverse=np.zeros(0, I32))
    room = cloud_cases.room(1)
    rng = np.random.default_rng(77)
    keep = radius_mask_ref(room, 0.2, 4) & (rng.uniform(size=room.shape[0]) > 0.2)       # holes in the dense parts too
    c["room"] = case(room, keep, 0.2, inverse=rng.integers(0, room.shape[0], 5000))
    return c


COUNT = _count_cases()
ROUTE = _route_cases()
