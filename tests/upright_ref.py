"""The numpy twin of csrc/upright.hip, written from include/pbnet_hip.h ("Floor plane and upright frame"): one rounded
operation per line or per numpy call, float32 values in np.float32 and float64 values in np.float64, the generator in
Python integers, the fixed-shape sum restated.  One function per stage; a later stage takes the earlier stage's output as
its input, so each stage is pinned on its own.  Below them: the designed cases (a few thousand points at most)."""
import functools
import math

import numpy as np

F32, F64 = np.float32, np.float64
MAX_HYP = 4096
SCORE_CHUNK = 1024                                           # csrc/upright.hip: UPR_CHUNK = pbn_cloud_upright_chunk()
HYP_BLOCK = 256                                              # csrc/upright.hip: UPR_HYP_BLOCK
SUM_BLOCK = 256                                              # csrc/scan_dev.h: SUM_BLOCK
JACOBI_SWEEPS = 10                                           # csrc/scan_dev.h
HYPOTHESES = (1, 63, 64, 65, HYP_BLOCK - 1, HYP_BLOCK, HYP_BLOCK + 1, MAX_HYP)
_M64 = (1 << 64) - 1


# ------------------------------------------------------------------------------------------------------------ draws
def mix64(z):
    z ^= z >> 30
    z = (z * 0xbf58476d1ce4e5b9) & _M64
    z ^= z >> 27
    z = (z * 0x94d049bb133111eb) & _M64
    z ^= z >> 31
    return z


def draws(seed, n_hyp, n):
    """int64 [H, 3]: hypothesis h's three point indices."""
    return np.array([[((mix64((seed + 3 * h + j) & _M64) >> 32) * n) >> 32 for j in range(3)] for h in range(n_hyp)],
                    np.int64).reshape(n_hyp, 3)


def unit_hint(hint):
    """The host's float64 normalisation of up_hint (pbnet_amd/mesh.py)."""
    h = np.asarray(hint, F64).reshape(3)
    return h / np.sqrt((h[0] * h[0] + h[1] * h[1]) + h[2] * h[2])


def cos_tilt(max_tilt):
    return float(np.cos(np.deg2rad(F64(max_tilt))))


# ------------------------------------------------------------------------------------------------------- hypotheses
def hypotheses_ref(xyz, n_hyp, seed, hint=None, cos_t=None):
    """(planes f32 [H, 4], live bool [H]); `hint` is the unit float64 hint or None.  Dead rows are zero."""
    xyz = np.asarray(xyz, F32).reshape(-1, 3)
    n = xyz.shape[0]
    planes, live = np.zeros((n_hyp, 4), F32), np.zeros(n_hyp, bool)
    if n < 3:
        return planes, live
    idx = draws(seed, n_hyp, n)
    distinct = (idx[:, 0] != idx[:, 1]) & (idx[:, 0] != idx[:, 2]) & (idx[:, 1] != idx[:, 2])
    p = xyz.astype(F64)
    p0, p1, p2 = p[idx[:, 0]], p[idx[:, 1]], p[idx[:, 2]]
    with np.errstate(all="ignore"):
        e1 = p1 - p0
        e2 = p2 - p0
        nx = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
        ny = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
        nz = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
        q = (nx * nx + ny * ny) + nz * nz
        ok = distinct & (q > 0) & np.isfinite(q)
        r = np.sqrt(q)
        ux, uy, uz = nx / r, ny / r, nz / r
        d = -((ux * p0[:, 0] + uy * p0[:, 1]) + uz * p0[:, 2])
        if hint is not None:
            g = (ux * hint[0] + uy * hint[1]) + uz * hint[2]
            neg = g < 0
            ux, uy, uz, d = (np.where(neg, -v, v) for v in (ux, uy, uz, d))
            ok = ok & ~(np.abs(g) < cos_t)
        full = np.stack([ux, uy, uz, d], axis=1).astype(F32)
    planes[ok] = full[ok]
    return planes, ok


# ------------------------------------------------------------------------------------------------------------ score
def plane_s(plane, xyz):
    """s = ((a*x + b*y) + c*z) + d in float32 for one plane [4] or planes [B, 4] against xyz [N, 3] -> [N] or [B, N]."""
    plane = np.asarray(plane, F32)
    x, y, z = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    if plane.ndim == 1:
        a, b, c, d = plane
    else:
        a, b, c, d = (plane[:, j, None] for j in range(4))
    with np.errstate(all="ignore"):
        t0 = a * x
        t1 = b * y
        t2 = t0 + t1
        t3 = c * z
        t4 = t2 + t3
        return t4 + d


def score_ref(xyz, planes, live, t, s_of=plane_s, inside=np.less_equal):
    """(in int64 [H], above int64 [H], nonfinite bool); dead hypotheses count nothing.  s_of and inside are the
    contract's; the mutants of tests/test_upright_ref_cpu.py replace them."""
    xyz = np.asarray(xyz, F32).reshape(-1, 3)
    t = F32(t)
    cin, cab = np.zeros(len(planes), np.int64), np.zeros(len(planes), np.int64)
    for b in range(0, len(planes), HYP_BLOCK):
        rows = np.flatnonzero(live[b:b + HYP_BLOCK]) + b
        if rows.size == 0 or xyz.shape[0] == 0:
            continue
        s = s_of(planes[rows], xyz)
        with np.errstate(invalid="ignore"):
            cin[rows] = inside(np.abs(s), t).sum(1)
            cab[rows] = (s > t).sum(1)
    return cin, cab, bool(not np.all(np.isfinite(xyz)))


# ----------------------------------------------------------------------------------------------------------- select
def select_ref(planes, live, cin, cab, n, hinted, max_below, highest=False):
    """dict: found, h, in, above, below, alive, plane0 f32 [4].  highest = the mutant that breaks ties the other way."""
    best, alive = None, 0
    for h in range(len(planes)):
        if not live[h]:
            continue
        above, below = int(cab[h]), n - int(cin[h]) - int(cab[h])
        flip = (not hinted) and below > above
        if flip:
            above, below = below, above
        if max_below >= 0 and below > max_below:
            continue
        alive += 1
        key = (int(cin[h]) << 12) | (h if highest else MAX_HYP - 1 - h)
        if best is None or key > best[0]:
            best = (key, h, int(cin[h]), above, below, flip)
    if best is None:
        return {"found": 0, "h": 0, "in": 0, "above": 0, "below": 0, "alive": alive, "plane0": np.zeros(4, F32)}
    _, h, cnt, above, below, flip = best
    plane0 = -planes[h] if flip else planes[h].copy()
    return {"found": 1, "h": h, "in": cnt, "above": above, "below": below, "alive": alive, "plane0": plane0.astype(F32)}


# ---------------------------------------------------------------------------------------------------------- moments
def fixed_sum(v):
    """The contract's sum of a float64 vector over ALL its indices: blocks of 256, the tree, partials in block order."""
    v = np.asarray(v, F64)
    nb = -(-v.shape[0] // SUM_BLOCK)
    b = np.zeros(nb * SUM_BLOCK, F64)
    b[:v.shape[0]] = v
    b = b.reshape(nb, SUM_BLOCK)
    s = SUM_BLOCK // 2
    while s > 0:
        b[:, :s] = b[:, :s] + b[:, s:2 * s]
        s //= 2
    total = F64(0.0)
    for part in b[:, 0]:
        total = total + part
    return total


def index_order_sum(v):
    """The mutant: the same numbers added in plain index order."""
    total = F64(0.0)
    for e in np.asarray(v, F64):
        total = total + e
    return total


def inlier_mask(xyz, plane0, t):
    with np.errstate(invalid="ignore"):
        return np.abs(plane_s(plane0, np.asarray(xyz, F32).reshape(-1, 3))) <= F32(t)


def moments_ref(xyz, floor_mask, total=fixed_sum):
    """float64 [10]: the count, the centroid, the six centred second-moment sums over the points of floor_mask."""
    p = np.asarray(xyz, F32).reshape(-1, 3).astype(F64)
    m = np.asarray(floor_mask, bool)
    out = np.zeros(10, F64)
    cnt = F64(int(m.sum()))
    out[0] = cnt
    with np.errstate(all="ignore"):
        for a in range(3):
            out[1 + a] = total(np.where(m, p[:, a], 0.0)) / cnt
        dx, dy, dz = p[:, 0] - out[1], p[:, 1] - out[2], p[:, 2] - out[3]
        for j, (u, v) in enumerate(((dx, dx), (dx, dy), (dx, dz), (dy, dy), (dy, dz), (dz, dz))):
            out[4 + j] = total(np.where(m, u * v, 0.0))
    return out


# ------------------------------------------------------------------------------------------------------------ refit
def _jacobi_rot(a, v, p, q, r):
    """csrc/scan_dev.h's jacobi_rot on the symmetric a (dict of pairs) and the columns p, q of v; r is the third axis."""
    apq = a[p, q]
    if apq == 0.0:
        return
    theta = (a[q, q] - a[p, p]) / (2.0 * apq)
    tt = (-1.0 if theta < 0.0 else 1.0) / (abs(theta) + math.sqrt(theta * theta + 1.0))
    c = 1.0 / math.sqrt(tt * tt + 1.0)
    s = tt * c
    a[p, p] = a[p, p] - tt * apq
    a[q, q] = a[q, q] + tt * apq
    a[p, q] = 0.0
    pr, qr = min(p, r), max(p, r)
    qq, rr = min(q, r), max(q, r)
    apr, aqr = a[pr, qr], a[qq, rr]
    a[pr, qr] = c * apr - s * aqr
    a[qq, rr] = s * apr + c * aqr
    for row in range(3):
        vp, vq = v[row][p], v[row][q]
        v[row][p] = c * vp - s * vq
        v[row][q] = s * vp + c * vq


def jacobi_smallest(m6):
    """The unit eigenvector of the smallest eigenvalue of the symmetric matrix (xx, xy, xz, yy, yz, zz), as the device
    finds it: fixed sweeps, Python floats (IEEE float64, one rounding per operation)."""
    a = {(0, 0): float(m6[0]), (0, 1): float(m6[1]), (0, 2): float(m6[2]), (1, 1): float(m6[3]), (1, 2): float(m6[4]),
         (2, 2): float(m6[5])}
    v = [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]
    for _ in range(JACOBI_SWEEPS):
        _jacobi_rot(a, v, 0, 1, 2)
        _jacobi_rot(a, v, 0, 2, 1)
        _jacobi_rot(a, v, 1, 2, 0)
    col = 2 if a[2, 2] < min(a[0, 0], a[1, 1]) else 1 if a[1, 1] < a[0, 0] else 0
    nx, ny, nz = v[0][col], v[1][col], v[2][col]
    length = math.sqrt((nx * nx + ny * ny) + nz * nz)
    if length > 0.0 and math.isfinite(length):
        return nx / length, ny / length, nz / length
    return 1.0, 0.0, 0.0


def refit_ref(moments, plane0):
    """plane float64 [4] from the moments and the winner's float32 plane."""
    a0, b0, c0, d0 = (float(v) for v in np.asarray(plane0, F32))
    if not moments[0] >= 3.0:
        return np.array([a0, b0, c0, d0], F64)
    nx, ny, nz = jacobi_smallest(moments[4:])
    if (nx * a0 + ny * b0) + nz * c0 < 0.0:
        nx, ny, nz = -nx, -ny, -nz
    d = -((nx * float(moments[1]) + ny * float(moments[2])) + nz * float(moments[3]))
    return np.array([nx, ny, nz, d], F64)


# --------------------------------------------------------------------------------------------------------- rotation
def rotation_ref(plane):
    """R float64 [9], row-major: the minimal rotation of plane[0..2] onto +z."""
    a, b, c = (F64(v) for v in np.asarray(plane, F64)[:3])
    k = F64(1.0) + c
    if not k > 0.0:
        return np.array([1.0, 0.0, 0.0, 0.0, -1.0, 0.0, 0.0, 0.0, -1.0], F64)
    ab = -((a * b) / k)
    return np.array([F64(1.0) - (a * a) / k, ab, -a, ab, F64(1.0) - (b * b) / k, -b, a, b, c], F64)


def apply_ref(xyz, plane, R, t, s_of=plane_s):
    """(xyz_out f32 [N, 3], floor bool [N], height f32 [N]) under the float32 roundings of plane and R."""
    xyz = np.asarray(xyz, F32).reshape(-1, 3)
    r32 = np.asarray(R, F64).reshape(9).astype(F32)
    p32 = np.asarray(plane, F64).astype(F32)
    x, y, z = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    out = np.empty_like(xyz)
    with np.errstate(all="ignore"):
        for r in range(3):
            t0 = r32[3 * r] * x
            t1 = r32[3 * r + 1] * y
            t2 = t0 + t1
            t3 = r32[3 * r + 2] * z
            out[:, r] = t2 + t3
        height = s_of(p32, xyz).astype(F32)
        return out, np.abs(height) <= F32(t), height


# ------------------------------------------------------------------------------------------------------ whole chain
def max_below_of(below_frac, n):
    return -1 if below_frac is None else int(float(below_frac) * n)


def tail_ref(xyz, sel, t):
    """Everything behind the select stage: the dict pbnet_amd.mesh.upright returns, as host arrays."""
    xyz = np.asarray(xyz, F32).reshape(-1, 3)
    n = xyz.shape[0]
    info = np.array([sel["found"], sel["h"], sel["in"], sel["above"], sel["below"], 0, sel["alive"], 0], np.int32)
    if not sel["found"]:
        return {"info": info, "plane0": np.zeros(4, F32), "moments": np.zeros(10, F64), "plane": np.zeros(4, F64),
                "R": np.eye(3).reshape(9), "xyz": xyz.copy(), "floor": np.zeros(n, bool), "height": np.zeros(n, F32)}
    moments = moments_ref(xyz, inlier_mask(xyz, sel["plane0"], t))
    info[5] = int(moments[0])
    plane = refit_ref(moments, sel["plane0"])
    R = rotation_ref(plane)
    out, floor, height = apply_ref(xyz, plane, R, t)
    return {"info": info, "plane0": sel["plane0"], "moments": moments, "plane": plane, "R": R, "xyz": out, "floor": floor,
            "height": height}


def upright_ref(xyz, threshold, hypotheses=1024, seed=0, up_hint=None, max_tilt=30.0, below_frac=0.01):
    """pbnet_amd.mesh.upright's arguments through every stage."""
    xyz = np.asarray(xyz, F32).reshape(-1, 3)
    hint = None if up_hint is None else unit_hint(up_hint)
    planes, live = hypotheses_ref(xyz, hypotheses, seed, hint, cos_tilt(max_tilt))
    cin, cab, _ = score_ref(xyz, planes, live, threshold)
    sel = select_ref(planes, live, cin, cab, xyz.shape[0], hint is not None, max_below_of(below_frac, xyz.shape[0]))
    return tail_ref(xyz, sel, threshold)


# ------------------------------------------------------------------------------------------------------------ cases
def _rot(axis, deg):
    """Rodrigues' rotation matrix, float64."""
    k = np.asarray(axis, F64) / np.linalg.norm(axis)
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]], F64)
    a = np.deg2rad(deg)
    return np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * (K @ K)


def _grid(nx, ny, x0, x1, y0, y1):
    gx, gy = np.meshgrid(np.linspace(x0, x1, nx), np.linspace(y0, y1, ny), indexing="ij")
    return gx.reshape(-1), gy.reshape(-1)


def _slab(n, seed):
    """n points: four fifths within +-0.005 of a plane tilted 20 degrees about (1, 1, 0), the rest clutter above it."""
    rng = np.random.default_rng(seed)
    m = n - n // 5
    p = np.concatenate([np.column_stack([rng.uniform(-2, 2, m), rng.uniform(-2, 2, m), rng.uniform(-0.005, 0.005, m)]),
                        np.column_stack([rng.uniform(-2, 2, n - m), rng.uniform(-2, 2, n - m), rng.uniform(0.1, 2, n - m)])])
    return (p[rng.permutation(n)] @ _rot((1, 1, 0), 20).T).astype(F32)


ROOM_L, ROOM_T = 4.0, 0.02
ROOM_ROT = _rot((1.0, 2.0, 0.5), 25.0)
ROOM_UP = ROOM_ROT @ np.array([0.0, 0.0, 1.0])


def _room():
    """Floor (noise-free, 4 x 4), two walls, ceiling and clutter, about 3000 points, rotated 25 degrees about a skew axis."""
    rng = np.random.default_rng(7)
    fx, fy = _grid(40, 40, 0.0, ROOM_L, 0.0, ROOM_L)
    floor = np.column_stack([fx, fy, np.zeros_like(fx)])
    wy, wz = _grid(20, 20, 0.0, ROOM_L, 0.05, 2.5)
    wall_a = np.column_stack([rng.normal(0.0, 0.004, wy.size), wy, wz])
    wall_b = np.column_stack([wy, rng.normal(0.0, 0.004, wy.size) + ROOM_L, wz])
    cx, cy = _grid(20, 20, 0.0, ROOM_L, 0.0, ROOM_L)
    ceiling = np.column_stack([cx, cy, 2.5 + rng.normal(0.0, 0.004, cx.size)])
    clutter = np.column_stack([rng.uniform(0.2, 3.8, 200), rng.uniform(0.2, 3.8, 200), rng.uniform(0.05, 1.8, 200)])
    p = np.concatenate([floor, wall_a, wall_b, ceiling, clutter])
    return (p[rng.permutation(p.shape[0])] @ ROOM_ROT.T).astype(F32)


def _two_slabs():
    x, y = _grid(16, 16, 0.0, 3.75, 0.0, 3.75)               # multiples of 1/4: every operation on them is exact
    p = np.concatenate([np.column_stack([x, y, np.zeros_like(x)]), np.column_stack([x, y, np.full_like(x, 2.5)])])
    return p[np.random.default_rng(3).permutation(p.shape[0])].astype(F32)


def _big_wall():
    x, y = _grid(20, 20, 0.0, 4.75, 0.0, 4.75)
    wy, wz = _grid(30, 30, 0.0, 4.75, 0.125, 3.75)
    p = np.concatenate([np.column_stack([x, y, np.zeros_like(x)]), np.column_stack([np.zeros_like(wy), wy, wz])])
    return p[np.random.default_rng(4).permutation(p.shape[0])].astype(F32)


def _table():
    x, y = _grid(15, 15, 0.0, 3.5, 0.0, 3.5)
    tx, ty = _grid(20, 20, 1.0, 2.1875, 1.0, 2.1875)
    p = np.concatenate([np.column_stack([x, y, np.zeros_like(x)]), np.column_stack([tx, ty, np.full_like(tx, 0.75)])])
    return p[np.random.default_rng(5).permutation(p.shape[0])].astype(F32)


ON_T = 0.25                                                  # a power of two: s = +-z exactly under the planes z = const


def _on_threshold():
    """A floor z = 0 on multiples of 1/4 and, over it, points at z = +-t and the next float32 either side of each."""
    x, y = _grid(16, 16, 0.0, 3.75, 0.0, 3.75)
    t = F32(ON_T)
    zs = [t, np.nextafter(t, F32(0)), np.nextafter(t, F32(1)), -t, -np.nextafter(t, F32(0)), -np.nextafter(t, F32(1))]
    extra = np.array([[0.25 * i, 0.5 * j, z] for j, z in enumerate(zs) for i in range(8)], F64)
    p = np.concatenate([np.column_stack([x, y, np.zeros_like(x)]), extra])
    return p[np.random.default_rng(6).permutation(p.shape[0])].astype(F32)


TILT_LIMIT = 10.0


def _tilt_limit():
    """300 points on a plane 9.9 degrees from the hint and 500 on one 10.1 degrees from it, three units higher."""
    ax, ay = _grid(20, 15, -1.0, 1.0, -1.0, 1.0)
    bx, by = _grid(25, 20, -1.0, 1.0, -1.0, 1.0)
    a = np.column_stack([ax, ay, np.zeros_like(ax)]) @ _rot((1, 0, 0), TILT_LIMIT - 0.1).T
    b = np.column_stack([bx, by, np.zeros_like(bx)]) @ _rot((1, 0, 0), TILT_LIMIT + 0.1).T + np.array([0.0, 0.0, 3.0])
    p = np.concatenate([a, b])
    return p[np.random.default_rng(8).permutation(p.shape[0])].astype(F32)


UP = (0.0, 0.0, 1.0)


@functools.lru_cache(maxsize=None)
def cases():
    """name -> (xyz f32 [N, 3], threshold, fit_plane's keyword arguments without `hypotheses`)."""
    c = {}
    for n in (0, 1, 2):
        c["n%d" % n] = (_slab(8, 1)[:n], 0.02, {})
    c["n3"] = (np.array([[0, 0, 0], [1, 0, 0.25], [0, 1, 0.5]], F32), 0.02, {"seed": 5})
    for n in (SUM_BLOCK - 1, SUM_BLOCK, SUM_BLOCK + 1, SCORE_CHUNK - 1, SCORE_CHUNK, SCORE_CHUNK + 1):
        c["slab%d" % n] = (_slab(n, n), 0.02, {"seed": n})
    c["coincident"] = (np.full((100, 3), 1.5, F32), 0.02, {})
    c["collinear"] = ((np.arange(200, dtype=F64)[:, None] * np.array([0.25, 0.5, 0.75])).astype(F32), 0.02, {})
    c["two_slabs"] = (_two_slabs(), 0.02, {})
    c["two_slabs_up"] = (_two_slabs(), 0.02, {"up_hint": UP})
    c["two_slabs_down"] = (_two_slabs(), 0.02, {"up_hint": (0.0, 0.0, -2.0)})
    c["big_wall"] = (_big_wall(), 0.02, {})
    c["big_wall_up"] = (_big_wall(), 0.02, {"up_hint": UP})
    c["table"] = (_table(), 0.02, {"up_hint": UP})
    c["table_any"] = (_table(), 0.02, {"up_hint": UP, "below_frac": None})
    c["on_threshold"] = (_on_threshold(), ON_T, {"up_hint": UP, "max_tilt": 1.0, "below_frac": None})
    c["tilt_limit"] = (_tilt_limit(), 0.02, {"up_hint": UP, "max_tilt": TILT_LIMIT, "below_frac": None})
    c["room"] = (_room(), ROOM_T, {"up_hint": tuple(ROOM_UP), "seed": 11})
    c["room_no_hint"] = (_room(), ROOM_T, {"seed": 11})
    return c


def _kw(kw):
    full = dict(seed=0, up_hint=None, max_tilt=30.0, below_frac=0.01)
    full.update(kw)
    return full


@functools.lru_cache(maxsize=None)
def scored(name):
    """The first two stages at H = 4096, computed once per case: hypothesis h does not depend on H, so the stages at a
    smaller H are this result's first H rows."""
    xyz, t, kw = cases()[name]
    kw = _kw(kw)
    hint = None if kw["up_hint"] is None else unit_hint(kw["up_hint"])
    planes, live = hypotheses_ref(xyz, MAX_HYP, kw["seed"], hint, cos_tilt(kw["max_tilt"]))
    cin, cab, _ = score_ref(xyz, planes, live, t)
    return planes, live, cin, cab


@functools.lru_cache(maxsize=None)
def selected(name, n_hyp):
    xyz, t, kw = cases()[name]
    kw = _kw(kw)
    planes, live, cin, cab = (v[:n_hyp] for v in scored(name))
    return select_ref(planes, live, cin, cab, xyz.shape[0], kw["up_hint"] is not None,
                      max_below_of(kw["below_frac"], xyz.shape[0]))


@functools.lru_cache(maxsize=None)
def want(name, n_hyp):
    """The whole chain's result for a case at H = n_hyp; read-only, shared by the tests."""
    xyz, t, _ = cases()[name]
    return tail_ref(xyz, selected(name, n_hyp), t)


def angle_to(normal, up):
    """The angle in radians between two directions."""
    a, b = np.asarray(normal, F64), np.asarray(up, F64)
    return float(np.arctan2(np.linalg.norm(np.cross(a, b)), np.dot(a, b)))
