"""Designed inputs for the raw-scan tests (csrc/thin.hip), every one generated from a seed: nothing is committed as a
fixture.  THIN maps a name to (xyz f32 [N, 3], rgb f32 [N, 3] or None, pitch); THIN_RAISES to inputs mesh.thin_points must
refuse; OUTLIER to (d2 f32 [N, k], ratio); RAW to (inverse, keep, idx)."""
import functools

import numpy as np

import cloud_cases
import cloud_ref

F32 = np.float32
INF = F32(np.inf)


def _rgb(n, seed):
    return np.random.default_rng(700 + seed).integers(0, 256, (n, 3)).astype(F32)


def one_cell(n):
    """n points inside one cell of pitch 1: spread 0.9 from the minimum on every axis."""
    return (np.random.default_rng(100 + n).uniform(0.0, 0.9, (n, 3)) + np.array([3.0, -2.0, 0.5])).astype(F32)


def lattice(m=7):
    g = np.arange(m, dtype=F32)
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3).astype(F32)


def negative(n=400):
    return (np.random.default_rng(11).normal(size=(n, 3)) - 5.0).astype(F32)


BIG = F32(1.0e17)


def order_matters():
    """One cell of pitch 1e18 whose float64 sum depends on the order: (-1e17 + 1e17) + 3 = 3 but (3 + 1e17) - 1e17 = 0 (the
    spacing of float64 at 1e17 is 16).  The colours carry the same values."""
    x = np.array([-BIG, BIG, 3.0, 5.0], F32)
    p = np.stack([x, x[::-1], np.roll(x, 1)], axis=1).astype(F32)
    return p, p.copy()


def far(axis):
    """Two clusters 1.5 M cells of pitch 1 apart on `axis` (733 * 2048: the low 11 bits of the far cells are those of the
    near ones); the far one has the SMALLER x cells, so an order by the low 32 key bits alone (x, and the low 11 bits of y)
    lets it come first, while the full key puts it last."""
    rng = np.random.default_rng(300 + axis)
    near = rng.uniform(0.0, 4.0, (40, 3)) + np.array([5.0, 0.0, 0.0])
    away = rng.uniform(0.0, 4.0, (40, 3))
    away[:, axis] += 733 * 2048.0
    p = np.concatenate([near, away]).astype(F32)
    return p[rng.permutation(p.shape[0])]


def extent(cells):
    """Two points `cells` - 1 cells of pitch 1 apart on x: the far one lies in cell cells - 1."""
    return np.array([[0.0, 1.0, 2.0], [float(cells - 1), 1.5, 2.5]], F32)


def _thin():
    c = {"n0": (np.zeros((0, 3), F32), np.zeros((0, 3), F32), 0.02),
         "n1": (cloud_cases.gauss(1), _rgb(1, 1), 0.02), "n2": (cloud_cases.gauss(2), None, 0.02)}
    for n in (63, 64, 65, 255, 256, 257):
        c["cell%d" % n] = (one_cell(n), _rgb(n, n), 1.0)
    c["coincident"] = (cloud_cases.coincident(200), _rgb(200, 2), 0.02)
    c["lattice_1"] = (lattice(), _rgb(343, 3), 1.0)
    c["lattice_half"] = (lattice(), None, 0.5)
    c["negative"] = (negative(), _rgb(400, 4), 0.25)
    c["order"] = order_matters() + (1.0e18,)
    c["far_z"] = (far(2), _rgb(80, 5), 1.0)
    c["far_y"] = (far(1), _rgb(80, 6), 1.0)
    c["extent_max"] = (extent(1 << 21), None, 1.0)
    room = cloud_cases.room(1)
    c["room_2cm"] = (room, _rgb(room.shape[0], 7), 0.02)
    c["room_5cm"] = (room, _rgb(room.shape[0], 7), 0.05)
    return c


def _thin_raises():
    c = {"extent_over": (extent((1 << 21) + 1), 1.0)}
    for name, bad in (("nan", np.nan), ("inf", np.inf), ("ninf", -np.inf)):
        p = one_cell(257).copy()
        p[100, 1] = bad
        c[name] = (p, 1.0)
    return c


THIN = _thin()
THIN_RAISES = _thin_raises()


# ------------------------------------------------------------------------------------------------------------ outliers
def table(n, k, seed=0, short=0):
    """A d2 table as knn_graph writes one: rows ascending, non-negative; the last `short` entries of every third row +inf."""
    d = np.sort(np.random.default_rng(500 + seed + n + k).gamma(2.0, 0.01, (n, k)).astype(F32) ** 2, axis=1)
    if short:
        d[::3, k - short:] = INF
    return d


def exact_threshold():
    """m = 1, 1, 3, 3: mu = 2, sigma = 1 (population), every sum exact; at ratio 1 the threshold is exactly 3 = m of the
    last two points: `<=` keeps them, `<` does not."""
    return np.array([[1.0], [1.0], [9.0], [9.0]], F32), 1.0


def far_room():
    """cloud_cases.room(1) and 30 points scattered 10 to 30 m away from it."""
    far_pts = np.random.default_rng(77).uniform(10.0, 30.0, (30, 3))
    return np.concatenate([cloud_cases.room(1), far_pts]).astype(F32)


@functools.lru_cache(maxsize=None)
def far_room_graph(k=16):
    return cloud_ref.knn(far_room(), k)


def _outlier():
    c = {}
    for k in (1, 16):
        for n in (0, 1, 255, 256, 257, 513):
            c["n%d_k%d" % (n, k)] = (table(n, k), 2.0)
    c["short_rows"] = (table(300, 16, 1, short=5), 1.5)
    allinf = table(300, 16, 2, short=3)
    allinf[7] = INF
    allinf[256] = INF
    c["row_all_inf"] = (allinf, 2.0)
    c["only_inf"] = (np.full((3, 4), INF, F32), 2.0)
    c["exact_threshold"] = exact_threshold()
    c["ratio_zero"] = (table(257, 6, 3), 0.0)
    return c


OUTLIER = _outlier()


# ----------------------------------------------------------------------------------------------------------- raw index
def _raw():
    """Six thinned points, k = 3.  Point 2: an outlier with kept neighbours in rank order 3, then 0 (by rank 3, by index 0);
    point 4: an outlier whose neighbours are outliers or absent (-1); point 5: an outlier whose first-rank neighbour 4 is
    itself an outlier, the second (1) is kept."""
    keep = np.array([1, 1, 0, 1, 0, 0], bool)
    idx = np.array([[1, 3, 2], [0, 3, 5], [3, 0, 4], [1, 0, 2], [5, 2, -1], [4, 1, 3]], np.int32)
    inverse = np.array([0, 2, 2, 5, 4, 1, 3, 4, 5, 0, 2], np.int32)
    return {"designed": (inverse, keep, idx),
            "none_kept": (inverse, np.zeros(6, bool), idx),
            "all_kept": (inverse, np.ones(6, bool), idx),
            "empty": (np.zeros(0, np.int32), keep, idx)}


RAW = _raw()
