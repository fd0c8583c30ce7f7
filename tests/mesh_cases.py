"""Designed inputs for the mesh decode (csrc/mesh.hip behind pbnet_amd.mesh: vertex normals, segmentator edge weights, the radix
sort of the edges, the host sweep, the relabel), shared by tests/test_mesh_cases_cpu.py (every precondition holds, the mutants of
tests/mesh_mutants.py die) and tests/test_mesh_cases_gpu.py (HIP == tests/mesh_ref.py, bit for bit).

A case is a dict: name, family, mode ("mesh": xyz + faces, "point": xyz + normals + edges), k_thresh, seg_min_verts, design (what
the builder intended) and precondition (a function of the case that raises AssertionError when the input no longer holds the
situation it was built for; it is evaluated with tests/mesh_ref.py on the CPU).  `only` narrows what the GPU tier runs ("normals":
vertex_normals alone), `large` marks the four launch-shape cases that are too big for the Python walk of the mutant harness.

Families
  N  incidence and vertex normals: fans whose hub has valence 1, 2, 65 and 300 (hub in slot 0, 1 or 2, faces shuffled), a face
     naming a vertex twice and three times, a triangle listed twice, unreferenced vertices at 0 / middle / V - 1, zero-area faces,
     V = 1 with F = 0, F = 1.
  W  edge weights, mostly in point mode where the normals are the case's own: dot2 == 0 with w != 0 on either side of k_thresh,
     one pair as (a, b) and as (b, a), coincident end points (NaN dot2), NaN normals, non-unit normals giving -3, -2^-23, +inf
     and -inf, and a tilted planar mesh whose lerped normals are a hair longer than 1 (a naturally negative weight).
     `1 - dot` is a multiple of 2^-23 when dot >= 1, so -2^-23 = -1.19e-7 stands for "about -1e-7": nothing closer to zero exists.
  O  sweep order: exactly tied weights whose ascending and descending order give different sup, negative weights of different
     size with +inf and NaN behind them, keys that differ only in the low / middle / top digit of the sort's three 11-bit digits,
     edge counts at the sort tile - 1, + 0, + 1 and twice the tile (built from a size; radix_sort_u32_tile() is asked of the library).
  S  sweep: a weight equal to both running thresholds bit for bit, a weight between the float32 and the float64 value of
     w + c / size, a threshold that needs the size after the join, components of exactly seg_min_verts and one fewer,
     seg_min_verts 0 and 1, a small component with two candidate neighbours, self loops and duplicate edges, and two inputs with
     one partition whose roots differ.
  L  launch shape, built from sizes: V and E at 255 / 256 / 257, V at the scan tile - 1, + 0, + 1 and twice the tile with the last
     vertex once a root and once not, and four large cases that take the second trip of the striding loops (below).

Not designed for: a weight of -0.  `1 - dot` and `w * w` never give -0 under round-to-nearest, so the `w == 0 -> +0` line of the
order key cannot be reached through the decode.

The second trips.  k_mesh_index, k_mesh_fill, k_face_normals, k_vertex_normals, k_edge_gather, k_root_flags and k_root_rank stride
over grids capped at MESH_GRID = 4096 workgroups x 256 lanes = 1 048 576 elements; k_edge_weights over 1024 x 256 = 262 144.
  L_grid420        420 x 420 height field, 2 x 419^2 = 351 122 faces = 1 053 366 indices > 1 048 576: second trip of k_mesh_index
                   and k_mesh_fill (normals only).                                      mesh_ref.decode_normals: 0.22 s
  L_v1048600       V = 1 048 600 > 1 048 576 with 300 faces on both sides of index 1 048 576: second trip of k_vertex_normals
                   (normals only).                                                     mesh_ref.decode_normals: 0.02 s
  L_point_v1048600 V = 1 048 600 with 400 edges on both sides of that index: second trip of k_root_flags and k_root_rank, and the
                   relabel scan over 513 tiles (segment_point).                         mesh_ref.segment_point: 0.21 s
  L_point_e262445  E = 262 144 + 1 + 300 = 262 445 edges on 3 000 vertices: second trip of k_edge_weights in point mode
                   (segment_point; 2 E = 524 890 indices stay inside one trip of k_mesh_index).   mesh_ref.segment_point: 0.22 s
k_face_normals (F > 1 048 576) and k_edge_gather (E > 1 048 576) stay on their first trip: a case that reached them would need more
than a million faces through the Python sweep of the reference.  The seconds are one measured run of the host reference
on a CPU; all four stay far below the 5 s a case may cost."""
import functools
import os
import re
import zlib

import numpy as np

import mesh_ref as MR

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN, INF = float("nan"), float("inf")


def _source_constants():
    csrc = os.path.join(ROOT, "pbnet_amd", "csrc")
    mesh = open(os.path.join(csrc, "mesh.hip")).read()
    common = open(os.path.join(csrc, "pbn_common.h")).read()
    grid = int(re.search(r"constexpr int MESH_GRID = (\d+);", mesh).group(1))
    tpb = int(re.search(r"constexpr int TPB = (\d+);", open(os.path.join(csrc, "coords_dev.h")).read()).group(1))
    weight_cap = int(re.search(r"inline int grid_for\(long long n, int cap = (\d+)\)", open(os.path.join(csrc, "scan_dev.h")).read()).group(1))
    scan = {k: int(v) for k, v in re.findall(r"constexpr int (SCAN_THREADS|SCAN_ITEMS) = (\d+);", common)}
    return grid, tpb, scan["SCAN_THREADS"] * scan["SCAN_ITEMS"], weight_cap


MESH_GRID, TPB, SCAN_TILE, WEIGHT_GRID = _source_constants()
STRIDE = MESH_GRID * TPB                    # elements of one trip of the striding kernels
WEIGHT_STRIDE = WEIGHT_GRID * TPB                # ... of k_edge_weights (grid_for's default cap)


@functools.lru_cache(maxsize=None)
def sort_tile():
    from pbnet_amd import selftest
    return selftest.sort_tile()


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def _freeze(c):
    for k in ("xyz", "faces", "normals", "edges"):
        if k in c:
            c[k].setflags(write=False)
    return c


def _mesh(name, xyz, faces, k=0.01, m=20, design="", pre=None, **more):
    return _freeze(dict(name=name, family=name[0], mode="mesh", xyz=np.ascontiguousarray(xyz, F32).reshape(-1, 3),
                        faces=np.ascontiguousarray(faces, np.int64).reshape(-1, 3), k_thresh=k, seg_min_verts=m, design=design,
                        precondition=pre or (lambda c: None), large=False, only=None, **more))


def _point(name, xyz, normals, edges, k=0.01, m=20, design="", pre=None, **more):
    return _freeze(dict(name=name, family=name[0], mode="point", xyz=np.ascontiguousarray(xyz, F32).reshape(-1, 3),
                        normals=np.ascontiguousarray(normals, F32).reshape(-1, 3),
                        edges=np.ascontiguousarray(edges, np.int64).reshape(-1, 2), k_thresh=k, seg_min_verts=m, design=design,
                        precondition=pre or (lambda c: None), large=False, only=None, **more))


# ---- what the preconditions look at ------------------------------------------------------------------------------------------------
def ends(c):
    if c["mode"] == "mesh":
        return MR.mesh_edges(c["faces"])
    return c["edges"][:, 0], c["edges"][:, 1]


def seg_normals(c):
    return MR.segmentator_normals(c["xyz"], c["faces"]) if c["mode"] == "mesh" else c["normals"]


def weights(c):
    ea, eb = ends(c)
    return MR.edge_weights(c["xyz"], seg_normals(c), ea, eb)


def sup_in_order(c, order):
    """sup of the reference's sweep over the edges taken in `order`."""
    ea, eb = ends(c)
    w = weights(c)
    return MR.relabel(MR.sweep(c["xyz"].shape[0], ea[order], eb[order], w[order], c["k_thresh"], c["seg_min_verts"]))


def sup_of(c, ties="asc"):
    return sup_in_order(c, MR.edge_order(weights(c), ties))


def trace(c):
    """The first phase of the reference's sweep with what it saw: per sorted edge (edge index, w, thr[a], thr[b], joined, size after,
    new threshold); float32 values.  Its roots after the second phase are checked against mesh_ref.sweep."""
    ea, eb = ends(c)
    w = weights(c)
    order = MR.edge_order(w, "asc")
    v = c["xyz"].shape[0]
    parent, rank, size = list(range(v)), [0] * v, [1] * v
    c32 = F32(c["k_thresh"])
    thr = [c32] * v

    def find(x):
        while x != parent[x]:
            x = parent[x]
        return x

    def join(x, y):
        if rank[x] > rank[y]:
            x, y = y, x
        elif rank[x] == rank[y]:
            rank[y] += 1
        parent[x] = y
        size[y] += size[x]

    events = []
    with np.errstate(all="ignore"):
        for e in order.tolist():
            a, b = find(int(ea[e])), find(int(eb[e]))
            if a == b:
                continue
            ta, tb = thr[a], thr[b]
            joined = bool(w[e] <= ta and w[e] <= tb)
            if joined:
                join(a, b)
                a = find(a)
                thr[a] = w[e] + c32 / F32(size[a])
            events.append(dict(edge=e, w=w[e], ta=ta, tb=tb, joined=joined, size=size[find(a)], thr=thr[find(a)]))
    for e in order.tolist():
        a, b = find(int(ea[e])), find(int(eb[e]))
        if a != b and (size[a] < c["seg_min_verts"] or size[b] < c["seg_min_verts"]):
            join(a, b)
    roots = np.array([find(q) for q in range(v)], np.int64)
    assert np.array_equal(roots, MR.sweep(v, ea[order], eb[order], w[order], c["k_thresh"], c["seg_min_verts"]))
    return events


def _bits(x):
    return np.asarray(x, F32).view(np.uint32)


def _expect_weights(c, want):
    got = weights(c)[:len(want)]
    want = np.asarray(want, F32)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan) and np.array_equal(_bits(got[~nan]), _bits(want[~nan])), (c["name"], got, want)


# ---- a forest with chosen edge weights (point mode) -------------------------------------------------------------------------------
def forest(parent, weight):
    """Point-mode arrays of a forest: parent[v] < v (-1: a root), weight[v] the weight of edge (parent[v], v).  A vertex at depth
    d has the normal c e_(d mod 3) + 1 e_(d+1 mod 3) with c = 1 - weight[v], so n_parent . n_v = c exactly and the weight is
    1 - (1 - weight[v]): exact for multiples of 2^-24 in [0, 1] and of 2^-23 in [-1, 0], for -3, and for +-inf / NaN on leaves.
    p_v = -depth (1, 1, 1): dot2 of an edge (parent, child) is negative (weights below 2), so no tree edge is squared.
    Returns xyz, normals and the tree edges in child order."""
    n = len(parent)
    depth = [0] * n
    xyz, nrm, edges = np.zeros((n, 3), F32), np.zeros((n, 3), F32), []
    for v in range(n):
        p = parent[v]
        assert p < v
        depth[v] = 0 if p < 0 else depth[p] + 1
        d = depth[v]
        nrm[v, d % 3] = F32(1) if p < 0 else F32(1) - F32(weight[v])
        nrm[v, (d + 1) % 3] = 1
        xyz[v] = -d
        if p >= 0:
            edges.append((p, v))
    return xyz, nrm, np.array(edges, np.int64).reshape(-1, 2)


def _forest_case(name, parent, weight, k, m, design, pre=None, extra_edges=(), edge_order=None):
    xyz, nrm, edges = forest(parent, weight)
    want = [weight[v] for v in range(len(parent)) if parent[v] >= 0]
    if edge_order is not None:
        edges, want = edges[list(edge_order)], [want[i] for i in edge_order]
    n_tree = len(edges)
    if len(extra_edges):
        edges = np.concatenate([edges, np.array(extra_edges, np.int64).reshape(-1, 2)])

    def precondition(c):
        _expect_weights(c, want[:n_tree])
        if pre:
            pre(c)

    return _point(name, xyz, nrm, edges, k, m, design, precondition)


def _chain(parent, weight, n, w_in=0.0, link=None, w_link=None):
    """Append a path of n vertices with inner weights w_in, hanging from vertex `link` by weight w_link (None: a new root)."""
    first = len(parent)
    for i in range(n):
        parent.append((link if link is not None else -1) if i == 0 else first + i - 1)
        weight.append((w_link if link is not None else 0.0) if i == 0 else w_in)
    return first, first + n - 1


# ---- N: incidence and vertex normals ------------------------------------------------------------------------------------------------
def _nfa(xyz, faces):
    p0, p1, p2 = xyz[faces[:, 0]], xyz[faces[:, 1]], xyz[faces[:, 2]]
    cx, cy, cz = MR._cross(p1 - p0, p2 - p0)
    ln = np.sqrt(MR._sum3(cx * cx, cy * cy, cz * cz)) + F32(1e-8)
    area = ln * F32(0.5)
    return np.stack([(cx / ln) * area, (cy / ln) * area, (cz / ln) * area], 1)


def _fan(name, valence):
    """An open fan: hub 0, rim 1 .. valence + 1 on a jittered cone, face i = (hub, r_i, r_i+1) rotated so that the hub sits in slot
    i mod 3, faces listed in shuffled order."""
    rng = _rng(name)
    ang = np.linspace(0.0, 1.7 * np.pi, valence + 1)
    rim = np.stack([np.cos(ang), np.sin(ang), 0.3 * np.sin(3 * ang)], 1) * rng.uniform(0.6, 1.4, (valence + 1, 1))
    xyz = np.concatenate([[[0.0, 0.0, 0.45]], rim + rng.normal(0, 0.02, rim.shape)]).astype(F32)
    faces = np.array([np.roll([0, 1 + i, 2 + i], i % 3) for i in range(valence)], np.int64)
    faces = faces[rng.permutation(valence)]

    def precondition(c):
        f = c["faces"]
        hub = np.sort(np.nonzero((f == 0).any(1))[0])
        assert len(hub) == valence and {int(np.nonzero(r == 0)[0][0]) for r in f[hub]} == set(range(min(3, valence)))
        assert valence < 3 or not np.array_equal(np.argsort(f.max(1), kind="stable"), np.arange(valence))       # shuffled
        if valence >= 3:                                     # a + b == b + a: order can show from three faces on
            a = _nfa(c["xyz"], f)[hub]
            fwd, rev = np.zeros(3, F32), np.zeros(3, F32)
            for r in a:
                fwd = fwd + r
            for r in a[::-1]:
                rev = rev + r
            unit = lambda s: s / (np.sqrt(MR._sum3(s[0] * s[0], s[1] * s[1], s[2] * s[2])) + F32(1e-8))
            assert not np.array_equal(_bits(unit(fwd)), _bits(unit(rev))), "reverse order gives the same nl bits"
            assert np.array_equal(_bits(unit(fwd)), _bits(MR.decode_normals(c["xyz"], f)[0]))

    return _mesh(name, xyz, faces, design="hub of valence %d in every slot, faces shuffled" % valence, pre=precondition)


def _sheet(name, nu, nv, amp=0.08):
    """nu x nv jittered height field, two triangles per cell."""
    rng = _rng(name)
    i, j = np.meshgrid(np.arange(nu), np.arange(nv), indexing="ij")
    z = amp * np.sin(i * 0.9) * np.cos(j * 0.7) + rng.normal(0, 0.004, i.shape)
    xyz = np.stack([i * 0.05, j * 0.05, z], -1).reshape(-1, 3).astype(F32)
    idx = np.arange(nu * nv).reshape(nu, nv)
    a, b, c, d = idx[:-1, :-1], idx[1:, :-1], idx[1:, 1:], idx[:-1, 1:]
    faces = np.concatenate([np.stack([a, b, c], -1).reshape(-1, 3), np.stack([a, c, d], -1).reshape(-1, 3)])
    return xyz, faces


def _family_n():
    out = [_fan("N_fan_%d" % k, k) for k in (1, 2, 65, 300)]

    xyz, faces = _sheet("N_repeat", 7, 8)
    rep = np.array([[17, 17, 18], [25, 30, 25], [12, 33, 33], [40, 40, 40]])
    faces = np.concatenate([faces[:20], rep[:2], faces[20:50], rep[2:], faces[50:]])

    def pre_repeat(c):
        f = c["faces"]
        twice = ((f[:, 0] == f[:, 1]) | (f[:, 1] == f[:, 2]) | (f[:, 0] == f[:, 2]))
        thrice = (f[:, 0] == f[:, 1]) & (f[:, 1] == f[:, 2])
        assert twice.sum() == 4 and thrice.sum() == 1
        assert np.all(_nfa(c["xyz"], f[twice]) == 0)                        # what such a face adds to nl: nothing
        sn = seg_normals(c)
        assert np.isnan(sn[[17, 25, 33, 40]]).all() and np.isfinite(sn[0]).all()
        assert np.isfinite(MR.decode_normals(c["xyz"], f)).all()

    out.append(_mesh("N_repeat", xyz, faces, design="faces naming a vertex twice (each slot pair) and three times", pre=pre_repeat))

    xyz, faces = _sheet("N_twin", 6, 6)
    faces = np.concatenate([faces[:31], faces[7:8], faces[31:], faces[7:8]])

    def pre_twin(c):
        f = c["faces"]
        assert (f == f[7]).all(1).sum() == 3
        once = np.concatenate([f[:31], f[32:-1]])
        assert not np.array_equal(_bits(MR.decode_normals(c["xyz"], f)), _bits(MR.decode_normals(c["xyz"], once)))
        assert not np.array_equal(_bits(seg_normals(c)), _bits(MR.segmentator_normals(c["xyz"], once)))

    out.append(_mesh("N_twin", xyz, faces, design="one triangle listed three times: distinct faces, all count", pre=pre_twin))

    xyz, faces = _sheet("N_unreferenced", 6, 7)
    extra = _rng("N_unreferenced/x").uniform(-1, 1, (4, 3)).astype(F32)
    xyz = np.concatenate([extra[:1], xyz[:20], extra[1:3], xyz[20:], extra[3:]])
    faces = np.where(faces >= 20, faces + 2, faces) + 1

    def pre_unref(c):
        free = np.setdiff1d(np.arange(c["xyz"].shape[0]), c["faces"])
        assert list(free) == [0, 21, 22, c["xyz"].shape[0] - 1]

    out.append(_mesh("N_unreferenced", xyz, faces, m=5, design="unreferenced vertices at 0, in the middle and at V - 1", pre=pre_unref))

    xyz, faces = _sheet("N_zero_area", 6, 6)
    xyz = np.concatenate([xyz, xyz[14:15], [[1.0, 1.0, 1.0], [1.5, 1.5, 1.5], [2.0, 2.0, 2.0]]]).astype(F32)
    flat = np.array([[36, 14, 20], [37, 38, 39], [14, 36, 15]])           # coincident coordinates; collinear corners
    faces = np.concatenate([faces[:9], flat[:2], faces[9:], flat[2:]])

    def pre_zero(c):
        f = c["faces"]
        cx, cy, cz = MR._cross(c["xyz"][f[:, 1]] - c["xyz"][f[:, 0]], c["xyz"][f[:, 2]] - c["xyz"][f[:, 0]])
        zero = (cx == 0) & (cy == 0) & (cz == 0)
        assert zero.sum() == 3 and not (f[zero, 0] == f[zero, 1]).any()    # zero area without a repeated index
        assert np.isnan(seg_normals(c)[[14, 36, 37]]).all() and np.isnan(weights(c)).any()
        assert np.isfinite(MR.decode_normals(c["xyz"], f)).all()

    out.append(_mesh("N_zero_area", xyz, faces, m=4, design="zero-area faces: the 1e-8 path of nl, NaN segmentator normals", pre=pre_zero))
    out.append(_mesh("N_v1_f0", [[0.25, -1.5, 3.0]], np.zeros((0, 3)), design="one vertex, no face"))
    out.append(_mesh("N_f1", [[0, 0, 0], [1, 0, 0.25], [0, 1, 0.5]], [[2, 0, 1]], m=0, design="one face"))
    return out


# ---- W: edge weights ------------------------------------------------------------------------------------------------------------------
def _family_w():
    out = []
    p01 = [[0, 0, 0], [1, 0, 0]]

    def pre_dot2(want_w, joins):
        def pre(c):
            e = c["edges"]
            n2, d = c["normals"][e[:, 1]], c["xyz"][e[:, 1]] - c["xyz"][e[:, 0]]
            assert np.all(MR._sum3(n2[:, 0] * d[:, 0], n2[:, 1] * d[:, 1], n2[:, 2] * d[:, 2]) == 0)
            _expect_weights(c, want_w)
            c32 = F32(c["k_thresh"])
            w, sq = F32(want_w[0]), F32(want_w[0]) * F32(want_w[0])
            assert (w <= c32) == joins and (sq <= c32) != joins
            assert (sup_of(c)[0] == sup_of(c)[1]) == joins
        return pre

    out.append(_point("W_dot2_zero_apart", p01, [[0, 0.5, 0], [0, 1, 0]], [[0, 1]], k=0.3, m=0,
                      design="dot2 == 0, w = 0.5 > k_thresh >= w^2 = 0.25: unsquared it stays apart", pre=pre_dot2([0.5], False)))
    out.append(_point("W_dot2_zero_joins", p01, [[0, 1.5, 0], [0, 1, 0]], [[0, 1]], k=0.2, m=0,
                      design="dot2 == 0, w = -0.5 <= k_thresh < w^2 = 0.25: unsquared it joins", pre=pre_dot2([-0.5], True)))

    def pre_both(c):
        _expect_weights(c, [0.5, 0.25, 0.25, 0.5])
        assert list(sup_of(c)) == [0, 0, 1, 1, 2, 3]

    # n_a = (0, .5, 0), n_b = (.5, 1, 0), b = a + x: (a, b) reads n_b . x = .5 > 0 -> squared; (b, a) reads n_a . -x = -0 -> not
    out.append(_point("W_both_directions", [[0, 0, 0], [1, 0, 0]] * 3, [[0, 0.5, 0], [0.5, 1, 0]] * 3,
                      [[1, 0], [0, 1], [2, 3], [5, 4]], k=0.3, m=0,
                      design="one pair as (b, a) and (a, b): dot2 reads n2, the weights are 0.5 and 0.25", pre=pre_both))

    def pre_coincident(c):
        assert np.array_equal(c["xyz"][0], c["xyz"][1])
        _expect_weights(c, [0.5, 0.25])
        assert list(sup_of(c)) == [0, 1, 2, 2]

    out.append(_point("W_coincident", [[2, 3, 4], [2, 3, 4], [0, 0, 0], [1, 0, 0]], [[0.5, 0.5, 0], [0.5, 0.5, 0]] * 2,
                      [[0, 1], [2, 3]], k=0.3, m=0,
                      design="coincident end points: dd = 0, dot2 NaN, w = 0.5 finite and not squared (its twin apart is: 0.25)",
                      pre=pre_coincident))

    def pre_nan(c):
        w = weights(c)
        assert np.isnan(w[[0, 1]]).all() and np.isfinite(w[2:]).all()
        assert list(sup_of(c)) == [0, 0, 1, 1, 2, 2]

    nrm = [[1, 0, 0], [NAN, 0, 0], [1, 0, 0], [1, 0, 0], [0, 1, 0], [0, 1, 0]]
    xyz = [[-i, -i, -i] for i in range(6)]
    out.append(_point("W_nan_normals", xyz, nrm, [[0, 1], [1, 2], [2, 3], [4, 5], [3, 4]], k=0.25, m=2,
                      design="a NaN normal: both its edges weigh NaN, sort last, join only as a small segment", pre=pre_nan))

    def pre_nonunit(c):
        assert list(sup_of(c)) == [0, 0, 1, 2, 2, 3, 3, 4, 5]
        assert np.isneginf(trace(c)[0]["thr"])

    # x -(-inf)- y, x -(0)- z: after the -inf join the threshold is -inf and 0 no longer joins; then pairs at -3, -2^-23, +inf
    out.append(_forest_case("W_nonunit", [-1, 0, 0, -1, 3, -1, 5, -1, 7], [0, -INF, 0.0, 0, -3.0, 0, -2.0 ** -23, 0, INF], 0.25, 0,
                            "non-unit normals: weights -inf, 0, -3, -2^-23 and +inf", pre_nonunit))

    for tilt in ((0.5, 0.25), (0.375, 0.625), (0.25, 0.75), (0.125, 0.875), (0.75, 0.5)):
        i, j = np.meshgrid(np.arange(9), np.arange(9), indexing="ij")
        xyz = np.stack([i * 0.125, j * 0.125, (i * tilt[0] + j * tilt[1]) * 0.125], -1).reshape(-1, 3).astype(F32)
        idx = np.arange(81).reshape(9, 9)
        a, b, c_, d = idx[:-1, :-1], idx[1:, :-1], idx[1:, 1:], idx[:-1, 1:]
        faces = np.concatenate([np.stack([a, b, c_], -1).reshape(-1, 3), np.stack([a, c_, d], -1).reshape(-1, 3)])
        w = MR.edge_weights(xyz, MR.segmentator_normals(xyz, faces), *MR.mesh_edges(faces))
        if (w < 0).any():
            break

    def pre_planar(c):
        p = c["xyz"].astype(np.float64)
        assert np.all(p[:, 2] == p[:, 0] * tilt[0] + p[:, 1] * tilt[1])     # exactly planar, in float32 coordinates
        w = weights(c)
        assert (w < 0).any() and (w >= 0).any() and np.isfinite(w).all()

    out.append(_mesh("W_planar_negative", xyz, faces, design="tilted exactly planar patch: lerped normals a hair longer than 1, "
                     "weights naturally below zero", pre=pre_planar))
    return out


# ---- O: sweep order -------------------------------------------------------------------------------------------------------------------
def _neighbour_gadget(parent, weight, w_first_listed, w_second_listed, n=3):
    """A (n vertices) - C (1 vertex) - B (n vertices): the edge A-C is listed before C-B.  With seg_min_verts = n the second pass
    joins C to whichever of the two edges it meets first."""
    _, a_end = _chain(parent, weight, n)
    c0, c1 = _chain(parent, weight, 1, link=a_end, w_link=w_first_listed)
    _chain(parent, weight, n, link=c1, w_link=w_second_listed)
    return c0


def _pre_order_matters(c, other_order, what):
    assert not np.array_equal(sup_of(c), sup_in_order(c, other_order)), "%s gives the same sup" % what


def _family_o():
    out = []
    parent, weight = [], []
    for _ in range(4):
        _neighbour_gadget(parent, weight, 0.5, 0.5)

    def pre_ties(c):
        w = weights(c)
        assert np.unique(_bits(w)).size == 2 and (w == 0.5).sum() == 8
        assert not np.array_equal(sup_of(c, "asc"), sup_of(c, "desc"))

    out.append(_forest_case("O_ties", parent, weight, 0.25, 3, "only two distinct weights; every small segment has two neighbours at "
                            "exactly 0.5, and ascending and descending edge index pick different ones", pre_ties))

    # path 0-1-2-3 at -1, -0.25, -0.5: ascending order joins {0, 1} and {2, 3}, and -0.25 lies above both new thresholds; taken by
    # magnitude (-0.25 first) everything joins.  Then -3 and +inf on one path, and a NaN edge (inf . 0) from a segment that a -inf
    # join has closed to a single vertex that also has an edge at 0.5: the second pass must meet 0.5 before NaN
    parent, weight = [-1, 0, 1, 2], [0, -1.0, -0.25, -0.5]
    a0, a1 = _chain(parent, weight, 2, w_in=-3.0)
    _chain(parent, weight, 1, link=a1, w_link=INF)
    xyz, nrm, edges = forest(parent, weight)
    n0 = len(parent)
    blk_n = [[1, 1, 0], [1, 1, 0], [1, INF, 0], [0, 0, 0.5], [0, 0, 1], [0, 0, 1], [0, 0, 1]]
    xyz = np.concatenate([xyz, [[0, 0, -i] for i in range(7)]])
    nrm = np.concatenate([nrm, blk_n])
    blk_e = np.array([[0, 1], [1, 2], [2, 3], [3, 4], [4, 5], [5, 6]]) + n0
    edges = np.concatenate([edges, blk_e])

    def pre_negative(c):
        _expect_weights(c, [-1.0, -0.25, -0.5, -3.0, INF, -1.0, -INF, NAN, 0.5, 0.0, 0.0])
        assert list(MR.edge_order(weights(c))) == [6, 3, 0, 5, 2, 1, 9, 10, 8, 4, 7]
        assert list(sup_of(c)) == [0, 0, 1, 1, 2, 2, 2, 3, 3, 3, 4, 4, 4, 4]

    out.append(_point("O_negative", xyz, nrm, edges, 0.25, 2, "negative weights of different size out of order in the input, then "
                      "+inf, then NaN last", pre_negative))

    base = 0.75
    for digit, (hi, lo) in {"low": (base + 1029 * 2.0 ** -24, base + 3 * 2.0 ** -24),
                            "mid": (base + (900 << 11) * 2.0 ** -24, base + (2 << 11) * 2.0 ** -24), "top": (0.75, 0.1875)}.items():
        parent, weight = [], []
        _neighbour_gadget(parent, weight, hi, lo)

        def pre_digit(c, digit=digit, hi=hi, lo=lo):
            k = MR.order_keys(np.array([hi, lo], F32)).astype(np.int64)
            x = int(k[0] ^ k[1])
            mask = {"low": 0x7ff, "mid": 0x7ff << 11, "top": 0x3ff << 22}[digit]
            assert x and x & ~mask == 0, hex(x)
            if digit == "top":                                # every key of the case: bits 0 .. 21 equal
                assert np.unique(MR.order_keys(weights(c)) & np.uint32(0x3fffff)).size == 1
            _pre_order_matters(c, np.arange(len(c["edges"])), "input order")

        out.append(_forest_case("O_digit_%s" % digit, parent, weight, 2.0 ** -6, 3, "the two edges of the small segment differ only in "
                                "the %s digit of their keys, the larger one listed first" % digit, pre_digit))
    t = sort_tile()
    for label, e in (("Tm1", t - 1), ("T", t), ("Tp1", t + 1), ("2T", 2 * t)):
        out.append(sort_size_case("O_sort_" + label, e))
    return out


PALETTE = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1], [0.75, 0.5, 0], [0, 0.875, 0.5], [0.5, 0.5, 0.75], [1, 0.25, 0], [0, 1, 0.125],
                    [0.625, 0, 0.75], [1.0625, 0, 0], [0, 0.9375, 0.375], [0.96875, 0.25, 0]], F32)


def random_graph(name, v, e, k=0.05, m=4, design="", pre=None):
    """Point mode: v points on a jittered lattice, normals from a small palette of exactly representable vectors (many tied
    weights, some negative), e edges between index neighbours (self loops and duplicates happen)."""
    rng = _rng(name)
    xyz = (rng.integers(-64, 64, (v, 3)) / 16.0).astype(F32)
    nrm = PALETTE[rng.integers(0, len(PALETTE), v) if v else np.zeros(0, np.int64)]
    a = rng.integers(0, max(v, 1), e)
    b = np.clip(a + rng.integers(-6, 7, e), 0, max(v - 1, 0))
    return _point(name, xyz, nrm, np.stack([a, b], 1), k, m, design, pre)


def sort_size_case(name, e):
    def pre(c):
        assert len(c["edges"]) == e
        k = MR.order_keys(weights(c)).astype(np.int64)
        assert all(np.unique((k >> (11 * p)) & 2047).size > 1 for p in range(3))
        w = weights(c)
        assert (w < 0).any() and np.unique(k).size < e // 8
        assert not np.array_equal(sup_of(c, "asc"), sup_of(c, "desc"))
    return random_graph(name, 700, e, design="%d edges: the sort's tile count changes here" % e, pre=pre)


# ---- S: sweep ---------------------------------------------------------------------------------------------------------------------------
def _family_s():
    out = []

    def pre_equal(c):
        ev = trace(c)
        hit = [x for x in ev if x["joined"] and _bits(x["w"]) == _bits(x["ta"]) == _bits(x["tb"])]
        assert {float(x["w"]) for x in hit} == {0.125, 0.25}            # a running threshold on both sides, and the initial one
        assert list(sup_of(c)) == [0, 0, 0, 0, 1, 1]

    out.append(_forest_case("S_equal_thresholds", [-1, 0, 1, 2, -1, 4], [0, 0.0, 0.125, 0.0, 0, 0.25], 0.25, 0,
                            "0.125 == 0 + 0.25 / 2 on both sides, and 0.25 == k_thresh between two single vertices", pre_equal))

    w2 = 13981014 * 2.0 ** -24                                            # 0.8333333730697632 = float32(0.5 + float32(1 / 3))

    def pre_f64(c):
        ev = trace(c)
        j = [x for x in ev if x["joined"]]
        assert len(j) == 3 and j[1]["size"] == 3 and float(j[1]["w"]) == 0.5
        thr32, thr64 = float(j[1]["thr"]), 0.5 + float(F32(c["k_thresh"])) / 3
        assert thr64 < w2 <= thr32 and _bits(j[2]["w"]) == _bits(thr32)
        assert list(sup_of(c)) == [0, 0, 0, 0]

    out.append(_forest_case("S_threshold_f32", [-1, 0, 1, 2], [0, 0.0, 0.5, w2], 1.0, 0,
                            "w = float32(0.5 + 1/3) lies above the float64 value of 0.5 + 1/3: joins only in float32", pre_f64))

    def pre_after(c):
        ev = trace(c)
        assert [x["joined"] for x in ev] == [True, True, False]
        c32 = F32(c["k_thresh"])
        after, before = F32(0.0625) + c32 / F32(3), F32(0.0625) + c32 / F32(2)
        assert _bits(ev[1]["thr"]) == _bits(after) and after < ev[2]["w"] <= before and ev[2]["w"] <= c32
        assert list(sup_of(c)) == [0, 0, 0, 1]

    out.append(_forest_case("S_size_after_join", [-1, 0, 1, 2], [0, 0.0, 0.0625, 0.15625], 0.25, 0,
                            "0.0625 + c/3 < 0.15625 <= 0.0625 + c/2: the threshold uses the size after the join", pre_after))

    def sized(m):
        parent, weight = [], []
        _, d1 = _chain(parent, weight, 4)                           # D: 4
        _, a1 = _chain(parent, weight, 4, link=d1, w_link=0.875)    # A: 4
        _, b1 = _chain(parent, weight, 3, link=a1, w_link=0.75)     # B: 3
        _, c1 = _chain(parent, weight, 4, link=b1, w_link=0.5)      # C: 4
        for _ in range(3):                                             # three single vertices
            _, c1 = _chain(parent, weight, 1, link=c1, w_link=0.625)
        return parent, weight

    def pre_sizes(want):
        def pre(c):
            assert list(np.bincount(sup_of(c))) == want
        return pre

    for m, want in ((4, [4, 4, 10]), (0, [4, 4, 3, 4, 1, 1, 1]), (1, [4, 4, 3, 4, 1, 1, 1])):
        parent, weight = sized(m)
        out.append(_forest_case("S_min_%d" % m, parent, weight, 0.25, m, "segments of 4, 4, 3, 4, 1, 1, 1 vertices after the first "
                                "phase; seg_min_verts = %d" % m, pre_sizes(want)))

    parent, weight = [], []
    _neighbour_gadget(parent, weight, 0.875, 0.5)

    def pre_two(c):
        assert list(sup_of(c)) == [0, 0, 0, 1, 1, 1, 1]
        assert list(sup_in_order(c, np.arange(len(c["edges"])))) == [0, 0, 0, 0, 1, 1, 1]

    out.append(_forest_case("S_two_neighbours", parent, weight, 0.25, 3, "a single vertex between two segments: the 0.875 edge comes "
                            "first in the input, the 0.5 edge first in sorted order", pre_two))

    parent, weight = [], []
    _neighbour_gadget(parent, weight, 0.875, 0.5)
    extra = [(1, 1), (3, 3), (0, 1), (1, 0), (3, 4), (4, 3), (3, 4), (6, 6), (2, 3)]

    def pre_loops(c):
        e = c["edges"]
        assert (e[:, 0] == e[:, 1]).sum() == 3 and np.unique(np.sort(e, 1), axis=0).shape[0] < len(e) - 4
        assert MR.same_partition(sup_of(c), [0, 0, 0, 1, 1, 1, 1])

    out.append(_forest_case("S_loops_duplicates", parent, weight, 0.25, 3, "self loops, duplicates and reversed duplicates around the "
                            "neighbour gadget: they change no join", pre_loops, extra_edges=extra))

    flat = np.zeros((6, 3), F32)
    flat[:, 0] = -np.arange(6)
    nrm = np.array([[1, 0, 0], [0, 1, 0], [0, 1, 0], [1, 0, 0], [0, 0, 1], [0, 0, 1]], F32)
    pairs = np.array([[0, 3], [1, 2], [4, 5]])

    def pre_rank(c):
        twin = case("S_rank_tie_b" if c["name"].endswith("_a") else "S_rank_tie_a")
        assert np.array_equal(np.sort(c["edges"], 1), np.sort(twin["edges"], 1))
        mine, other = sup_of(c), sup_of(twin)
        assert MR.same_partition(mine, other) and not np.array_equal(mine, other)
        assert list(mine) == ([1, 0, 0, 1, 2, 2] if c["name"].endswith("_a") else [0, 1, 1, 0, 2, 2])

    out.append(_point("S_rank_tie_a", flat, nrm, pairs, 0.25, 0, "equal ranks: the root is the edge's second end (3, 2, 5)", pre_rank))
    out.append(_point("S_rank_tie_b", flat, nrm, pairs[:, ::-1], 0.25, 0, "the same edges reversed: roots 0, 1, 4 -- the same "
                      "partition, other ids", pre_rank))
    return out


# ---- L: launch shape --------------------------------------------------------------------------------------------------------------------
def strip(name, v, m=20):
    """Mesh mode: a jittered zigzag triangle strip of v vertices, v - 2 faces."""
    rng = _rng(name)
    i = np.arange(v)
    xyz = np.stack([(i // 2) * 0.05, (i % 2) * 0.05, 0.05 * np.sin(i * 0.02) + rng.normal(0, 0.003, v)], 1).astype(F32)
    faces = np.stack([i[:-2], i[1:-1], i[2:]], 1)
    faces[1::2] = faces[1::2][:, [1, 0, 2]]

    def pre(c):
        assert c["xyz"].shape[0] == v and np.unique(c["faces"]).size == v

    return _mesh(name, xyz, faces, m=m, design="V = %d" % v, pre=pre)


def last_vertex_case(name, v, last_is_root):
    """Point mode: v vertices, a few hundred random edges among the others, and the last vertex either alone (its own root) or the
    first end of a zero-weight edge (the second end becomes the root on equal ranks)."""
    base = random_graph(name, v - 1, 300, m=0)
    rng = _rng(name + "/last")
    xyz = np.concatenate([base["xyz"], [[-9.0, -9.0, -9.0]]])
    nrm = np.concatenate([base["normals"], [[0, 0, 1]]])
    nrm[v - 2] = [0, 0, 1]
    edges = base["edges"][~(base["edges"] == v - 2).any(1)]
    if not last_is_root:
        edges = np.concatenate([edges, [[v - 1, v - 2]]])
        edges = edges[rng.permutation(len(edges))]

    def pre(c):
        ea, eb = ends(c)
        w = weights(c)
        o = MR.edge_order(w)
        roots = MR.sweep(v, ea[o], eb[o], w[o], c["k_thresh"], c["seg_min_verts"])
        assert c["xyz"].shape[0] == v and (roots[v - 1] == v - 1) == last_is_root
        assert np.unique(roots).size > 10

    return _point(name, xyz, nrm, edges, 0.05, 0, "V = %d, the last vertex %s a root" % (v, "is" if last_is_root else "is not"), pre)


def _pre_ve(n):
    def pre(c):
        assert (len(c["edges"]), len(c["xyz"])) == (n, n) and np.unique(sup_of(c)).size > 3
    return pre


def _family_l_small():
    out = []
    for n in (255, 256, 257):
        out.append(strip("L_strip_v%d" % n, n))
        out.append(random_graph("L_point_ve%d" % n, n, n, design="V = E = %d" % n, pre=_pre_ve(n)))
    t = SCAN_TILE
    for label, n, root in (("Tm1", t - 1, True), ("T", t, False), ("Tp1", t + 1, True), ("2T", 2 * t, False), ("T_root", t, True),
                           ("Tp1_noroot", t + 1, False)):
        out.append(last_vertex_case("L_scan_%s" % label, n, root))
    for label, n in (("Tm1", t - 1), ("T", t), ("Tp1", t + 1), ("2T", 2 * t)):
        out.append(strip("L_strip_scan_%s" % label, n))
    return out


def _height_field(n):
    rng = _rng("L_grid%d" % n)
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    z = 0.15 * np.sin(i * 0.06) * np.cos(j * 0.05) + rng.normal(0, 0.002, i.shape)
    xyz = np.stack([i * 0.02, j * 0.02, z], -1).reshape(-1, 3).astype(F32)
    idx = np.arange(n * n).reshape(n, n)
    a, b, c, d = idx[:-1, :-1], idx[1:, :-1], idx[1:, 1:], idx[:-1, 1:]
    return xyz, np.concatenate([np.stack([a, b, c], -1).reshape(-1, 3), np.stack([a, c, d], -1).reshape(-1, 3)])


def _large(name):
    if name == "L_grid420":
        xyz, faces = _height_field(420)

        def pre(c):
            assert c["faces"].shape[0] == 351122 and STRIDE < 3 * c["faces"].shape[0] < 2 * STRIDE
        return _mesh(name, xyz, faces, design="3 F = 1 053 366 > 4096 x 256", pre=pre)
    rng = _rng(name)
    v = STRIDE + 24
    lo, hi = STRIDE - 150, v
    if name == "L_v1048600":
        xyz = rng.normal(size=(v, 3)).astype(F32)
        faces = np.concatenate([rng.integers(lo, hi, (260, 3)), rng.integers(0, v, (40, 3))])

        def pre(c):
            f = c["faces"]
            assert c["xyz"].shape[0] == 1048600 == v and (f >= STRIDE).any(1).sum() > 30 and (f < STRIDE).any(1).sum() > 200
            assert ((f >= STRIDE).any(1) & (f < STRIDE).any(1)).sum() > 20        # faces that straddle the index
        return _mesh(name, xyz, faces, design="V = 1 048 600, 300 faces around index 4096 x 256", pre=pre)
    if name == "L_point_v1048600":
        xyz = (rng.integers(-64, 64, (v, 3)) / 16.0).astype(F32)
        nrm = PALETTE[rng.integers(0, len(PALETTE), v)]
        a = np.concatenate([rng.integers(lo, hi, 340), rng.integers(0, v, 60)])
        b = np.concatenate([np.clip(a[:340] + rng.integers(-20, 21, 340), 0, v - 1), rng.integers(lo, hi, 60)])

        def pre(c):
            e = c["edges"]
            assert c["xyz"].shape[0] == 1048600 and ((e >= STRIDE).any(1) & (e < STRIDE).any(1)).sum() > 10
            s = sup_of(c)
            assert np.unique(s[STRIDE:]).size > 3 and (np.bincount(s) > 1).sum() > 30
        return _point(name, xyz, nrm, np.stack([a, b], 1), 0.05, 2, "V = 1 048 600, 400 edges around index 4096 x 256", pre)
    assert name == "L_point_e262445"
    e = WEIGHT_STRIDE + 1 + 300

    def pre(c):
        assert len(c["edges"]) == 262445 == e > WEIGHT_STRIDE and 2 * e < STRIDE
        assert np.unique(sup_of(c)[c["edges"][WEIGHT_STRIDE:].reshape(-1)]).size > 3
    return random_graph(name, 3000, e, design="E = 1024 x 256 + 301 on 3000 vertices", pre=pre)


LARGE = ("L_grid420", "L_v1048600", "L_point_v1048600", "L_point_e262445")
ONLY = {"L_grid420": "normals", "L_v1048600": "normals", "L_point_v1048600": "segment", "L_point_e262445": "segment"}


@functools.lru_cache(maxsize=None)
def _small_cases():
    out = _family_n() + _family_w() + _family_o() + _family_s() + _family_l_small()
    names = [c["name"] for c in out]
    assert len(names) == len(set(names))
    for c in out:
        assert c["xyz"].shape[0] <= 5000
    return {c["name"]: c for c in out}


SMALL = tuple(_small_cases())
NAMES = SMALL + LARGE


@functools.lru_cache(maxsize=None)
def case(name):
    if name in LARGE:
        c = _large(name)
        c.update(large=True, only=ONLY[name])
        return c
    return _small_cases()[name]


@functools.lru_cache(maxsize=None)
def reference(name):
    """What the GPU tier compares against, computed once: nl (mesh cases) and sup with the library's tie order."""
    c = case(name)
    out = {}
    if c["mode"] == "mesh":
        out["nl"] = MR.decode_normals(c["xyz"], c["faces"])
    if c["only"] != "normals":
        out["sup"] = sup_of(c)
    for a in out.values():
        a.setflags(write=False)
    return out


def tie_free(name):
    """True when ascending and descending tie order give the same sup and no weight is NaN: what the compiled segmentator must
    reproduce whatever its std::sort does with ties (tests/golden/make_mesh_golden.py records these)."""
    c = case(name)
    return not np.isnan(weights(c)).any() and np.array_equal(sup_of(c, "asc"), sup_of(c, "desc"))


def designed_cases(g):
    """(name, mode, arrays, k_thresh, seg_min_verts, sup) of every case in mesh_designed.npz."""
    for name in g["names"].tolist():
        mode = "mesh" if name + ".faces" in g.files else "point"
        arrays = [g["%s.%s" % (name, k)] for k in (("xyz", "faces") if mode == "mesh" else ("xyz", "normals", "edges"))]
        yield name, mode, arrays, float(g[name + ".k_thresh"]), int(g[name + ".seg_min_verts"]), g[name + ".sup"]
