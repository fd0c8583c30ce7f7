"""Seeded, designed inputs for the grouping pipeline (csrc/cluster.hip), one family per cell-driven branch, shared by
tests/test_cluster_cases_cpu.py (the set is valid and sharp: preconditions, oracle == brute force, mutants die) and
tests/test_cluster_cases_gpu.py (HIP == brute force, bit for bit, in four call modes).  numpy only, no fixtures: the brute force
(tests/bruteforce_cluster.py) is the reference at test time.  Every case stays small enough for its O(n^2) reference.

A case is a dict: name, family, off f32[n,3], org f32[n,3], sem i32[n], seg i32[B], radius, min_pts, para_f, nv_flag, design (what
the builder intended, read by the precondition), precondition (None, or a function of the case that raises AssertionError when the
input no longer has the configuration it was designed for -- e.g. after a change of the cell size).

Cell membership is restated here in binary32, independently of the kernels: floor(f32(v) * f32(1 / f32(radius * 0.5625f))), clamped
to +-32764; a cell with an index AT the clamp is untrusted (it collects arbitrarily distant points)."""
import functools

import numpy as np

import bruteforce_cluster as brute

F4 = np.float32
CLAMP = 32764
PARA_SMALL = 0.0005          # thresholds 0.4725 (class 17), 0.5015 (class 10), 1.1515 (class 4)


def cell_size(radius):
    return F4(F4(radius) * F4(0.5625))


def cell_index(v, radius):
    """int64 cell indices of float32 coordinates (any shape)."""
    inv = F4(F4(1.0) / cell_size(radius))
    with np.errstate(over="ignore", invalid="ignore"):
        f = np.floor((np.asarray(v, F4) * inv).astype(F4))
    return np.clip(f, -CLAMP, CLAMP).astype(np.int64)


def clamped_points(off, radius):
    """True for points whose cell is untrusted (some axis index at the clamp)."""
    return (np.abs(cell_index(off, radius)) >= CLAMP).any(axis=1)


def d2(a, b):
    """Unfused binary32 squared distance of two points, as the specification computes it."""
    a, b = np.asarray(a, F4), np.asarray(b, F4)
    dx, dy, dz = F4(a[0] - b[0]), F4(a[1] - b[1]), F4(a[2] - b[2])
    return F4(F4(F4(dx * dx) + F4(dy * dy)) + F4(dz * dz))


def _case(name, family, off, org, sem, seg, radius, min_pts, para_f=PARA_SMALL, nv_flag=True, design=None, precondition=None):
    off = np.ascontiguousarray(off, F4).reshape(-1, 3)
    org = off.copy() if org is None else np.ascontiguousarray(org, F4).reshape(-1, 3)
    n = off.shape[0]
    sem = np.full(n, sem, np.int32) if np.isscalar(sem) else np.ascontiguousarray(sem, np.int32)
    seg = np.ascontiguousarray(seg, np.int32)
    assert int(seg.sum()) == n and sem.shape[0] == n and n <= 6000
    return dict(name=name, family=family, off=off, org=org, sem=sem, seg=seg, radius=float(radius), min_pts=int(min_pts),
                para_f=float(para_f), nv_flag=bool(nv_flag), design=design or {}, precondition=precondition)


def _rank_preserving_scatter(rng, groups):
    """groups: list of [m_g, 3] arrays whose ROW ORDER is designed.  Returns (points[n, 3], index lists per group): the groups are
    interleaved at random over 0..n-1, each group keeping its own row order in the global index order."""
    n = sum(g.shape[0] for g in groups)
    perm = rng.permutation(n)
    pts = np.empty((n, 3), np.float64)
    where, at = [], 0
    for g in groups:
        idx = np.sort(perm[at:at + g.shape[0]])
        pts[idx] = g
        where.append(idx)
        at += g.shape[0]
    return pts, where


# ---- A: components that hang on one edge between two non-representatives (k_union pass 1, rule (a)) ---------------------------
# local coordinates in cells; a name's first letter is its designed cell (A = +0, B = +2, C = +4 along x; P* = bridge, own cells)
_A_PTS = dict(A_far=(0.1, 0.1, 0.1), A_near=(0.9, 0.1, 0.1), B_far=(2.9, 0.1, 0.1), B_near=(2.1, 0.1, 0.1), B0=(2.5, 0.9, 0.9),
              B1=(2.1, 0.1, 0.1), B2=(2.9, 0.1, 0.1), C_near=(4.1, 0.1, 0.1), C_far=(4.9, 0.1, 0.1),
              P1=(0.1, 1.6, 0.1), P2=(0.1, 3.1, 0.1), P3=(1.6, 3.1, 0.1), P4=(3.1, 3.1, 0.1), P5=(4.6, 3.1, 0.1), P6=(4.9, 1.6, 0.1))
_A_CELL_X = dict(A=0, B=2, C=4)
_CHAIN = ("A_far", "A_near", "B0", "B1", "B2", "C_far", "C_near")
_BRIDGE = ("P1", "P2", "P3", "P4", "P5", "P6")
# kind -> (point names in designed index order, links).  A link is (cell X, cell Y, witness in X, witness in Y, cells whose
# representative -- the smallest index of the cell -- must be farther than r from EVERY point of the other cell)
_A_KINDS = {
    "dumbbell_ab": (("A_far", "A_near", "B_far", "B_near"), (("A", "B", "A_near", "B_near", "AB"),)),
    "dumbbell_ba": (("B_far", "B_near", "A_far", "A_near"), (("A", "B", "A_near", "B_near", "AB"),)),
    "dumbbell_ab_seen_from_b": (("A_far", "A_near", "B_near", "B_far"), (("A", "B", "A_near", "B_near", "A"),)),
    "dumbbell_ba_seen_from_b": (("B_near", "B_far", "A_far", "A_near"), (("A", "B", "A_near", "B_near", "A"),)),
    "chain_abc": (_CHAIN, (("A", "B", "A_near", "B1", "AB"), ("B", "C", "B2", "C_near", "BC"))),
    "chain_cba": (("C_far", "C_near", "B0", "B1", "B2", "A_far", "A_near"),
                  (("A", "B", "A_near", "B1", "AB"), ("B", "C", "B2", "C_near", "BC"))),
    # the ends A and C already share a root after pass 0 (bridge of single-point cells, each its own representative)
    "ring_bridge_first": (_BRIDGE + _CHAIN, (("A", "B", "A_near", "B1", "AB"), ("B", "C", "B2", "C_near", "BC"))),
    "ring_bridge_last": (_CHAIN + _BRIDGE, (("A", "B", "A_near", "B1", "AB"), ("B", "C", "B2", "C_near", "BC"))),
}


def _precondition_edges(case):
    off, radius, dz = case["off"], case["radius"], case["design"]
    r2 = F4(F4(radius) * F4(radius))
    cells = cell_index(off, radius)
    assert not clamped_points(off, radius).any()
    for s in dz["structures"]:
        at = s["index"]                                        # name -> global index
        origin = np.asarray(s["origin_cell"])
        members = {}
        for name, i in at.items():
            if name[0] in _A_CELL_X:
                want = origin + (_A_CELL_X[name[0]], 0, 0)
                assert tuple(cells[i]) == tuple(want), (s["kind"], name, cells[i], want)
                members.setdefault(name[0], []).append(i)
        occupied = [tuple(cells[i]) for i in at.values()]
        assert len(set(occupied)) == len(members) + sum(1 for k in at if k[0] == "P")    # bridge points sit alone in their cells
        for x, y, wx, wy, blind in s["links"]:
            assert d2(off[at[wx]], off[at[wy]]) <= r2, (s["kind"], wx, wy)
            for mine, other, witness in ((x, y, wx), (y, x, wy)):
                if mine in blind:
                    rep = min(members[mine])
                    assert rep != at[witness]                                            # the edge hangs on a NON-representative
                    assert all(d2(off[rep], off[j]) > r2 for j in members[other]), (s["kind"], mine, other)


def _family_a():
    rng = np.random.default_rng(4101)
    radius = 0.04
    c = float(cell_size(radius))
    kinds = list(_A_KINDS)
    slots = [(x, y, z) for x in range(7) for y in range(7) for z in range(7)]
    rng.shuffle(slots)
    groups, meta = [], []
    for k in range(320):
        kind = kinds[k % len(kinds)]
        names, links = _A_KINDS[kind]
        origin = (np.asarray(slots[k]) - 3) * 12                # > 5 cells between structures; negative coordinates too
        local = np.array([_A_PTS[nm] for nm in names]) + rng.uniform(-0.02, 0.02, (len(names), 3))
        groups.append((origin + local) * c)
        meta.append(dict(kind=kind, origin_cell=tuple(int(v) for v in origin), names=names, links=links))
    pts, where = _rank_preserving_scatter(rng, groups)
    for m, idx in zip(meta, where):
        m["index"] = {nm: int(i) for nm, i in zip(m["names"], idx)}
    n = pts.shape[0]
    return [_case("A_single_edges", "A", pts, None, 17, [n], radius, 1,
                  design=dict(structures=meta, expect_clusters=len(meta)), precondition=_precondition_edges)]


# ---- B: the trusted / untrusted seam (rule (b), the pairwise fallbacks of k_count, k_union, k_border) -------------------------
def _seam(radius, sign):
    """The clamped float32 coordinate nearest to zero on the given side."""
    inv = F4(F4(1.0) / cell_size(radius))
    raw = lambda v: np.floor(F4(F4(v) * inv))
    v = F4(sign * CLAMP * float(cell_size(radius)))
    toward0, away = F4(0.0), F4(sign * np.inf)
    while abs(raw(v)) < CLAMP:
        v = np.nextafter(v, away)
    while abs(raw(np.nextafter(v, toward0))) >= CLAMP:
        v = np.nextafter(v, toward0)
    return float(v)


# u = depth into the clamped region (negative: trusted side), then two small offsets on the other axes; designed index order
_B_MOTIFS = {
    # one HP-HP edge t0-k0 across the seam; every other pair across it is farther than r.  min_pts = 2: all six are HP
    "hp_edge_larger_index_trusted": (("k1", 0.040, 0, 0), ("k2", 0.040, 0.002, 0), ("k0", 0.002, 0, 0),
                                     ("t1", -0.040, 0, 0), ("t2", -0.040, 0.002, 0), ("t0", -0.002, 0, 0)),
    "hp_edge_larger_index_clamped": (("t1", -0.040, 0, 0), ("t2", -0.040, 0.002, 0), ("t0", -0.002, 0, 0),
                                     ("k1", 0.040, 0, 0), ("k2", 0.040, 0.002, 0), ("k0", 0.002, 0, 0)),
    # k0 is the only HP (neighbours l and k1); the LP l sits in a trusted cell, the LP k1 in the clamped cell of k0
    "lp_trusted_hp_clamped": (("l", -0.003, 0, 0), ("k1", 0.040, 0, 0), ("k0", 0.003, 0, 0)),
    "lp_clamped_hp_trusted": (("t0", -0.003, 0, 0), ("l", 0.003, 0, 0), ("t1", -0.040, 0, 0)),
}


def _precondition_seam(case):
    off, radius, dz = case["off"], case["radius"], case["design"]
    assert np.array_equal(clamped_points(off, radius), dz["clamped"]), "which points clamp"
    assert dz["clamped"].any() and not dz["clamped"].all()
    cells = cell_index(off, radius)
    r2 = F4(F4(radius) * F4(radius))
    for m in dz["motifs"]:
        at = m["index"]
        for i in at.values():                                   # the trusted side lies within two cells of the clamped key
            assert dz["clamped"][i] or CLAMP - 2 <= np.abs(cells[i]).max() < CLAMP
        cross = [(a, b) for a in at for b in at if a < b and dz["clamped"][at[a]] != dz["clamped"][at[b]]
                 and d2(off[at[a]], off[at[b]]) <= r2]
        assert len(cross) == 1, (m["kind"], cross)             # exactly one edge crosses the seam
    far = dz["far_groups"]
    assert len({tuple(cells[i]) for g in far for i in g}) == 1 and all(dz["clamped"][i] for g in far for i in g)
    a, b, loner = far
    assert all(d2(off[i], off[j]) > r2 for i in a for j in list(b) + list(loner))
    assert all(d2(off[i], off[j]) > r2 for i in b for j in loner)


def _family_b():
    rng = np.random.default_rng(4102)
    radius = 0.04
    groups, meta = [], []
    slot = 0
    for axis in range(3):
        for sign in (1, -1):
            s = _seam(radius, sign)
            for kind, rows in _B_MOTIFS.items():
                base = np.array([0.5 + 0.3 * (slot % 8), 0.5 + 0.3 * (slot // 8)])       # 13 cells between motifs
                slot += 1
                p = np.empty((len(rows), 3))
                for k, (_, u, v, w) in enumerate(rows):
                    p[k, axis] = s + sign * u
                    p[k, (axis + 1) % 3] = base[0] + v
                    p[k, (axis + 2) % 3] = base[1] + w
                groups.append(p)
                meta.append(dict(kind="%s_axis%d%s" % (kind, axis, "+" if sign > 0 else "-"), names=[r[0] for r in rows],
                                 clamped=[r[1] > 0 for r in rows]))
    # two groups and a loner that share ONE clamped cell and are far apart: no own-cell credit, no chaining, no free border
    yz = np.array([-2.0, -2.0]) + 0.001
    far_a = np.column_stack([800.0 + rng.uniform(0, 0.005, 5), yz[0] + rng.uniform(0, 0.005, 5), yz[1] + rng.uniform(0, 0.005, 5)])
    far_b = np.column_stack([900.0 + rng.uniform(0, 0.005, 5), yz[0] + rng.uniform(0, 0.005, 5), yz[1] + rng.uniform(0, 0.005, 5)])
    loner = np.array([[850.0, yz[0], yz[1]]])
    groups += [far_a, far_b, loner]
    pts, where = _rank_preserving_scatter(rng, groups)
    clamped = np.zeros(pts.shape[0], bool)
    for m, idx in zip(meta, where):
        m["index"] = {nm: int(i) for nm, i in zip(m["names"], idx)}
        clamped[idx] = m["clamped"]
    for idx in where[-3:]:
        clamped[idx] = True
    design = dict(motifs=meta, clamped=clamped, far_groups=[[int(i) for i in idx] for idx in where[-3:]])
    return [_case("B_seam", "B", pts, None, 17, [pts.shape[0]], radius, 2, nv_flag=False, design=design,
                  precondition=_precondition_seam)]


# ---- C: percolation clouds ---------------------------------------------------------------------------------------------------
def _family_c():
    out = []
    radius, n = 0.04, 4000
    ball = 4.0 / 3.0 * np.pi * radius ** 3
    for min_pts in (0, 1, 2, 3, 5):
        rng = np.random.default_rng(4300 + min_pts)
        mean = min_pts + (1.5 if min_pts == 0 else 1.0)       # mean neighbour count in the bulk (less at the faces)
        off = rng.uniform(0, (n * ball / mean) ** (1.0 / 3.0), (n, 3))
        org = off + rng.normal(0, 0.01, (n, 3))
        out.append(_case("C_cloud_m%d" % min_pts, "C", off, org, 17, [n], radius, min_pts))
        sem = rng.choice(np.array([17, 10, 4]), n)
        off = rng.uniform(0, (n / 2 * ball / mean) ** (1.0 / 3.0), (n, 3))     # two segments share the box: same density per segment
        org = off + rng.normal(0, 0.01, (n, 3))
        out.append(_case("C_cloud_m%d_classes" % min_pts, "C", off, org, sem, [1500, 0, 2500], radius, min_pts))
    return out


# ---- D: segment bookkeeping --------------------------------------------------------------------------------------------------
def _precondition_segments(case):
    seg, dz = case["seg"], case["design"]
    assert all(seg[z] == 0 for z in dz["empty"]) and len(seg) == dz["n_seg"]
    start = np.cumsum(seg)[:-1]
    assert (start[(seg[1:] > 0) & (start > 0)] % 64 != 0).mean() > 0.9      # boundaries inside waves


def _family_d():
    rng = np.random.default_rng(4401)
    radius = 0.04
    n_seg, n = 130, 3000
    empty = (0, 63, 64, 127, 129)
    full = [s for s in range(n_seg) if s not in empty]
    lens = np.zeros(n_seg, np.int64)
    lens[full] = 1 + rng.multinomial(n - len(full), np.ones(len(full)) / len(full))
    sem = np.concatenate([np.full(lens[s], 2 + (7 * s) % 18) for s in range(n_seg)])
    off = rng.uniform(0, 0.13, (n, 3)) + np.repeat(rng.uniform(-3, 3, (n_seg, 3)), lens, axis=0)
    org = off + rng.normal(0, 0.01, (n, 3))
    many = _case("D_130_segments", "D", off, org, sem, lens, radius, 2, design=dict(empty=empty, n_seg=n_seg),
                 precondition=_precondition_segments)
    n_seg = 40000
    lens = np.zeros(n_seg, np.int64)
    held = {32768: 40, 32770: 65, 36863: 130, 39999: 31}
    for s, k in held.items():
        lens[s] = k
    n = int(lens.sum())
    sem = np.concatenate([np.full(k, 2 + s % 18) for s, k in held.items()])
    off = rng.uniform(0, 0.1, (n, 3))                                       # the segments overlap in space: only the key separates them
    org = off + rng.normal(0, 0.01, (n, 3))
    high = _case("D_high_segments", "D", off, org, sem, lens, radius, 2, design=dict(empty=(0, 32767, 32769, 39998), n_seg=n_seg),
                 precondition=_precondition_segments)
    return [many, high]


# ---- E: centres and the member list ------------------------------------------------------------------------------------------
# per 256-point chunk of the segment: members of each cluster (cluster = its size; F = filler)
_E_CHUNKS = (
    {600: 255, 1: 1},
    {16: 16, 17: 17, 32: 32, 33: 33, 600: 31, 257: 15, 256: 1, "F": 111},
    {256: 255, 257: 1},
    {257: 241, 600: 15},
    {600: 256},
    {600: 43, "F": 17},
)
_E_FALLBACK = (600, 3)      # the 1e-25 coordinate: cluster 600, chunk 3


def _quotient_is_fast(p):
    a = np.abs(p.astype(F4))
    return bool(((a == 0) | ((a >= F4(1e-20)) & (a <= F4(1e20)))).all())


def _precondition_centres(case):
    dz, off = case["design"], case["off"]
    ref = reference(case["name"])
    cid = ref["cluster_id"]
    assert ref["cluster_num"].tolist() == [len(dz["label"])]
    slow = []
    for key, members in dz["members"].items():
        ids = np.unique(cid[members])
        assert len(ids) == 1 and (cid == ids[0]).sum() == len(members), key           # the designed sets ARE the clusters
        for ch, table in enumerate(_E_CHUNKS):
            inside = members[(members >= 256 * ch) & (members < 256 * (ch + 1))]
            assert len(inside) == table.get(key, 0), (key, ch)
            if len(inside) and not _quotient_is_fast(off[inside]):
                slow.append((key, ch))
    assert slow == [_E_FALLBACK], slow
    assert np.signbit(off[dz["members"][257], 1]).sum() == 1 and (off[dz["members"][256], 2] == 0).all()


def _precondition_scale(case):
    """Edges must not depend on a denormal-flush mode: flushing every sub-normal product or sum to zero keeps the graph."""
    off, radius = case["off"], case["radius"]
    r2 = F4(F4(radius) * F4(radius))
    tiny = np.finfo(F4).tiny
    assert np.isfinite(r2) and r2 >= tiny
    flush = lambda a: np.where(np.abs(a) < tiny, F4(0), a).astype(F4)
    with np.errstate(over="ignore"):
        d = [off[:, None, k] - off[None, :, k] for k in range(3)]
        sq = [(x * x).astype(F4) for x in d]
        plain = (sq[0] + sq[1]).astype(F4) + sq[2]
        fl = [flush(flush(x) * flush(x)) for x in d]
        flushed = flush(flush(fl[0] + fl[1]) + fl[2])
    assert np.array_equal(plain <= r2, flushed <= r2)
    if case["design"].get("overflow"):
        assert np.isinf(plain).any()
    assert not _quotient_is_fast(off)


def _family_e():
    rng = np.random.default_rng(4501)
    radius = 0.04
    keys = (1, 16, 17, 32, 33, 256, 257, 600, "F")
    n = sum(sum(t.values()) for t in _E_CHUNKS)
    members = {k: [] for k in keys}
    for ch, table in enumerate(_E_CHUNKS):
        size = sum(table.values())
        order = rng.permutation(np.concatenate([np.full(v, keys.index(k)) for k, v in table.items()]))
        for pos in range(size):
            members[keys[order[pos]]].append(256 * ch + pos)
    members = {k: np.array(v) for k, v in members.items()}
    centre = {1: (-31.0, 7.0, 2.0), 16: (3.0, -4.0, 5.0), 17: (55.5, 0.25, -9.0), 32: (-2.0, -2.0, -2.0), 33: (8.0, 8.0, 48.0),
              256: (12.0, -6.0, 0.0), 257: (-7.0, 0.0, 3.0), 600: (0.0, 21.0, -13.0), "F": (1.0, 1.0, 1.0)}
    off = np.empty((n, 3))
    for k, idx in members.items():
        off[idx] = np.asarray(centre[k]) + rng.uniform(0.001, 0.02, (len(idx), 3))    # inside one cell's reach: one component
    off = off.astype(F4)
    off[members[256], 2] = 0.0                                                        # a whole axis of zeros
    off[members[257][100], 1] = -0.0
    ch3 = members[600][(members[600] >= 768) & (members[600] < 1024)]
    off[ch3[7], 0] = 1e-25                                                            # leaves [1e-20, 1e20]: IEEE division
    # para_f puts the filter threshold of class 17 at exactly 1.0: the single-point cluster survives by the strict `<` alone
    mean17 = brute.MEAN_COUNT[17 - 2]
    para_f = F4(1.0) / mean17
    for _ in range(8):
        if F4(mean17 * para_f) >= F4(1.0):
            break
        para_f = np.nextafter(para_f, F4(1.0))
    assert F4(mean17 * para_f) == F4(1.0)
    design = dict(members=members, label=keys)
    out = [_case("E_interleaved_members", "E", off, None, 17, [n], radius, 0, para_f=float(para_f), design=design,
                 precondition=_precondition_centres)]
    rng = np.random.default_rng(4502)
    off = 1e20 + rng.uniform(0, 3e19, (300, 3))
    out.append(_case("E_huge", "E", off, None, 17, [300], 1e19, 40, design=dict(overflow=True), precondition=_precondition_scale))
    off = rng.uniform(0, 3e-17, (200, 3)) * (1.0, 1.0, 1e-6)
    out.append(_case("E_tiny", "E", off, None, 17, [200], 1e-17, 50, precondition=_precondition_scale))
    return out


# ---- F: noise assignment -----------------------------------------------------------------------------------------------------
def _precondition_noise(case):
    """The lattice gives exact ties of both kinds among the nearest candidates, a class without candidates, a silent segment."""
    ref = reference(case["name"])
    pre =brute.binary_cluster(case["off"], case["org"], case["sem"], case["seg"], case["radius"], case["min_pts"], case["para_f"], False)
    cid, sem, org, seg = pre["cluster_id"], case["sem"], case["org"], case["seg"]
    start = np.concatenate([[0], np.cumsum(seg)])
    same_lane = cross_lane = classless = 0
    for b in range(len(seg)):
        lo, hi = start[b], start[b + 1]
        assigned = lo + np.nonzero(cid[lo:hi] >= 0)[0]
        noise = lo + np.nonzero(cid[lo:hi] < 0)[0]
        if b == case["design"]["silent"]:
            assert len(assigned) == 0 and (ref["cluster_id"][lo:hi] == -1).all() and len(noise) > 0
            continue
        assert len(assigned) > 0
        if b == case["design"]["crowded"]:
            assert len(noise) > len(assigned)
        for i in noise:
            cand = assigned[sem[assigned] == sem[i]]
            if len(cand) == 0:
                classless += 1
                continue
            dd = np.array([d2(org[i], org[j]) for j in cand])
            best = cand[dd == dd.min()]
            if len(best) > 1:
                lanes = (best - lo) % 64
                same_lane += len(np.unique(lanes)) < len(lanes)
                cross_lane += len(np.unique(lanes)) > 1
    assert same_lane >= 5 and cross_lane >= 5 and classless >= 5, (same_lane, cross_lane, classless)
    assert (org == np.round(org)).all()


def _family_f():
    rng = np.random.default_rng(4601)
    radius, min_pts = 0.04, 3
    # per segment: (blob sizes with classes drawn from `blob_classes`, number of isolated points with classes from `noise_classes`)
    plan = [dict(blobs=(40, 30, 25, 20, 12, 9, 6, 5, 70, 64), blob_classes=(17, 10), noise=200, noise_classes=(17, 10)),
            dict(blobs=(50, 33, 17, 90), blob_classes=(17,), noise=120, noise_classes=(17, 4)),
            dict(blobs=(), blob_classes=(17,), noise=70, noise_classes=(17, 10)),
            dict(blobs=(20, 20), blob_classes=(10,), noise=300, noise_classes=(10,))]
    offs, sems, seg = [], [], []
    for s, p in enumerate(plan):
        pts, cls = [], []
        for b, size in enumerate(p["blobs"]):
            pts.append(np.array([2.0 * b, 5.0 * s, 0.0]) + rng.uniform(0, 0.01, (size, 3)))
            cls.append(rng.choice(np.array(p["blob_classes"]), size))
        k = p["noise"]
        pts.append(np.column_stack([100.0 + 1.0 * np.arange(k), np.full(k, 5.0 * s), np.zeros(k)]))   # alone: no neighbour
        cls.append(rng.choice(np.array(p["noise_classes"]), k))
        pts, cls = np.concatenate(pts), np.concatenate(cls)
        order = rng.permutation(len(pts))
        offs.append(pts[order])
        sems.append(cls[order])
        seg.append(len(pts))
    off, sem = np.concatenate(offs), np.concatenate(sems)
    org = rng.integers(0, 4, off.shape).astype(np.float64)                      # 64 lattice sites: exact ties everywhere
    design = dict(silent=2, crowded=3)
    return [_case("F_lattice_noise", "F", off, org, sem, seg, radius, min_pts, design=design, precondition=_precondition_noise),
            _case("F_lattice_noise_off", "F", off, org, sem, seg, radius, min_pts, nv_flag=False, design=design)]


# ---- G: count thresholds of the early exit -----------------------------------------------------------------------------------
_G_PILES = (64, 63, 65, 129)


def _precondition_piles(case):
    off, radius = case["off"], case["radius"]
    cells = cell_index(off, radius)
    assert not clamped_points(off, radius).any()
    for k, idx in zip(_G_PILES, case["design"]["piles"]):
        key = cells[idx[0]]
        assert (cells == key).all(axis=1).sum() == k and (cells[idx] == key).all()       # the cell holds exactly the pile
    i, j = case["design"]["at_r"]
    r = F4(radius)
    assert d2(off[i], off[j]) == F4(r * r)                                              # a neighbour at EXACTLY r


def _family_g():
    rng = np.random.default_rng(4701)
    radius = 0.04
    r = float(F4(radius))
    groups = []
    for k, size in enumerate(_G_PILES):
        base = np.array([0.5 * k, 0.0, 0.0])
        pile = np.zeros((size, 3))
        pile[size // 2:, 1:] = rng.uniform(1e-5, 1e-4, (size - size // 2, 2))            # half coincident, half near (x stays equal)
        # pile 0 sits at the origin, so its neighbour at (r, 0, 0) is at EXACTLY r from the coincident half and beyond r from the
        # near half; the other piles have one neighbour inside r of all their points.  Then a tail that no pile point reaches
        near = r if k == 0 else 0.039
        sparse = np.array([[near, 0, 0], [near + 0.03, 0, 0], [near + 0.03, 0.03, 0]])
        groups += [base + pile, base + sparse]
    pts, where = _rank_preserving_scatter(rng, groups)
    design = dict(piles=[where[2 * k] for k in range(len(_G_PILES))], at_r=(int(where[0][0]), int(where[1][0])))
    n = pts.shape[0]
    return [_case("G_piles_m%d" % m, "G", pts, None, 17, [n], radius, m, design=design, precondition=_precondition_piles)
            for m in (0, 1, 63, 64, 65)]


# ---- H: tiny sizes -----------------------------------------------------------------------------------------------------------
def _family_h():
    out = []
    radius = 0.04
    ball = 4.0 / 3.0 * np.pi * radius ** 3
    for n in (1, 2, 3, 4, 5, 6, 7, 8, 9, 63, 64, 65, 255, 256, 257):
        rng = np.random.default_rng(4800 + n)
        side = max(4 * float(cell_size(radius)), (n * ball / 3.0) ** (1.0 / 3.0))
        off = rng.uniform(-side / 2, side / 2, (n, 3))
        out.append(_case("H_n%d" % n, "H", off, off + rng.normal(0, 0.01, (n, 3)), 17, [n], radius, 2))
    return out


@functools.lru_cache(maxsize=None)
def cases():
    out = []
    for family in (_family_a, _family_b, _family_c, _family_d, _family_e, _family_f, _family_g, _family_h):
        out += family()
    assert len({c["name"] for c in out}) == len(out)
    return tuple(out)


NAMES = tuple(c["name"] for c in cases())
N_SEG_TOO_MANY = 65536       # the cell key keeps 16 bits for the segment: this count must be refused


def case(name):
    return next(c for c in cases() if c["name"] == name)


def run(fn, c):
    """fn(off, org, sem, seg, radius, min_pts, para_f, nv_flag) on a case."""
    return fn(c["off"], c["org"], c["sem"], c["seg"], c["radius"], c["min_pts"], c["para_f"], c["nv_flag"])


@functools.lru_cache(maxsize=None)
def reference(name):
    """The brute force on the case, computed once and shared (do not modify)."""
    out = run(brute.binary_cluster, case(name))
    for v in out.values():
        v.setflags(write=False)
    return out


def is_general(c):
    start = np.concatenate([[0], np.cumsum(c["seg"])])
    return any(len(np.unique(c["sem"][a:b])) > 1 for a, b in zip(start[:-1], start[1:]))
