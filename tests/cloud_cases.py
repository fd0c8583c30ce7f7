"""Designed point clouds for the kNN / normals tests (csrc/cloud.hip), every one generated from a seed: nothing is
committed as a fixture.  Each generator returns float32 [N, 3]; CASES maps a name to (points, cell or None)."""
import numpy as np

F32 = np.float32
KS = (1, 6, 16, 32)
ROOM_CELLS = (None, 0.02, 0.5, 10.0)


def gauss(n, seed=0):
    return np.random.default_rng(1000 + seed + n).normal(size=(n, 3)).astype(F32)


def coincident(n=200):
    return np.tile(np.array([[0.25, -1.5, 3.0]], F32), (n, 1))


def lattice(m=12):
    """Integer lattice m^3; with cell = 1.0 every point lies exactly on a cell face, the 6 nearest neighbours of an inner
    point lie exactly at the first stopping bound (one cell), and distances tie by the thousand."""
    g = np.arange(m, dtype=F32)
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3).astype(F32)


def sheet(n=1500, seed=0):
    """A planar sheet: one axis of exactly zero extent."""
    p = np.random.default_rng(20 + seed).uniform(0, 1, (n, 3)).astype(F32)
    p[:, 2] = F32(0.375)
    return p


SHEET_VIEWPOINT = (0.5, 0.5, 3.0)       # off the plane: the cloud's own mean lies in it and orients nothing
BLOB_CELL = 0.25


def blob_and_outlier(n=500, seed=0):
    """A dense blob in [0, 1]^3 and one point 40 cells of BLOB_CELL away: its rings grow to the grid's edge."""
    p = np.random.default_rng(30 + seed).uniform(0, 1, (n, 3)).astype(F32)
    p[-1] = np.array([1.0 + 40 * BLOB_CELL, 0.5, 0.5], F32)
    return p


LINE_CELL = 0.01


def line(n=2000, seed=0):
    """A 1 x 1 x 1e4 box: with cell = 0.01 the long axis would need 1e6 cells, far past the 1024-cell clamp."""
    p = np.random.default_rng(40 + seed).uniform(0, 1, (n, 3))
    p[:, 2] *= 1.0e4
    return p.astype(F32)


def offset(n=700, seed=0):
    """Coordinates near +-1000 (float32 spacing 6e-5 there): large magnitudes, negative values."""
    p = np.random.default_rng(50 + seed).uniform(-1, 1, (n, 3)) * 2.0 + np.array([1000.0, -1000.0, -1003.0])
    return p.astype(F32)


def room(seed=1, n=3000):
    """A floor, two walls, a cylinder and one coincident pair, 1 mm of noise: the shape of an indoor scan."""
    rng = np.random.default_rng(seed)
    nf, nw, nc = 1400, 600, n - 1400 - 2 * 600 - 1
    floor = np.stack([rng.uniform(0, 4, nf), rng.uniform(0, 4, nf), np.zeros(nf)], 1)
    wall_a = np.stack([np.zeros(nw), rng.uniform(0, 4, nw), rng.uniform(0, 2.5, nw)], 1)
    wall_b = np.stack([rng.uniform(0, 4, nw), np.zeros(nw), rng.uniform(0, 2.5, nw)], 1)
    ang = rng.uniform(0, 2 * np.pi, nc)
    cyl = np.stack([2.0 + 0.3 * np.cos(ang), 2.0 + 0.3 * np.sin(ang), rng.uniform(0, 1, nc)], 1)
    p = np.concatenate([floor, wall_a, wall_b, cyl]) + rng.normal(scale=1e-3, size=(n - 1, 3))
    p = np.concatenate([p, p[777:778]])                     # the coincident pair: rows 777 and n - 1
    return p.astype(F32)


def collinear(n=300, seed=0):
    """Points on one line along x: two axes of zero extent, so two axes of one cell and shells that grow along x only."""
    p = np.zeros((n, 3))
    p[:, 0] = np.random.default_rng(60 + seed).uniform(0, 10, n)
    p[:, 1:] = (0.5, -2.0)
    return p.astype(F32)


FACE_TIE_CELL = 1.0


def face_tie():
    """Cells of 1.0 along x, origin 0.  Query 1 at x = 1.5 (cell 1) has point 2 at x = 1.0 (its own cell) and point 0 at
    x = 2.0 (cell 2, across the face) both at d2 = 0.25 exactly, and after shell 0 the bound to that face is 0.25 as well
    (the bound's slack of 2^-38 vanishes in the float32 rounding of 0.5).  For k = 1 the row is point 0, the lower index:
    the walk has to go on past a k-th d2 that EQUALS the bound.  Points 3 and 4 pin the grid's origin and its length."""
    x = np.array([2.0, 1.5, 1.0, 0.0, 4.0])
    return np.stack([x, np.full(5, 0.5), np.full(5, 0.5)], 1).astype(F32)


SPARSE_CELL = 0.05


def _cases():
    c = {"n0": (np.zeros((0, 3), F32), None), "n1": (gauss(1), None), "n2": (gauss(2), None)}
    for n in (63, 64, 65, 255, 256, 257):
        c["n%d" % n] = (gauss(n), None)
    for k in KS:                                             # N = k and N = k + 1: padded rows, then exactly full rows
        for n in (k, k + 1):
            c.setdefault("n%d" % n, (gauss(n), None))
    c["coincident"] = (coincident(), None)
    c["lattice"] = (lattice(), 1.0)
    c["sheet"] = (sheet(), None)
    c["blob"] = (blob_and_outlier(), BLOB_CELL)
    c["blob_auto"] = (blob_and_outlier(), None)
    c["line"] = (line(), LINE_CELL)
    c["offset"] = (offset(), None)
    for seed in (1, 2, 3):
        c["room%d" % seed] = (room(seed), None)
    c["collinear"] = (collinear(), None)
    c["face_tie"] = (face_tie(), FACE_TIE_CELL)
    # 300 points of a unit Gaussian under a cell of 0.05 (the table's cap widens it to ~0.4): the k-th neighbour of a point
    # in the tails lies several cells away, so its walk needs shells r >= 2
    c["sparse_small_cell"] = (gauss(300), SPARSE_CELL)
    # one cell for the whole grid: the block has no inner face, and the walk ends because it covers the grid
    c["n257_one_cell"] = (gauss(257), 1.0e3)
    return c


CASES = _cases()
