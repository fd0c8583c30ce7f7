"""CPU restatement of csrc/mesh.hip (pbnet_amd.mesh), written from the algorithms: decode_scannet.py's vertex normals and
lib/segmentator's Felzenszwalb segmentation, float32 operation by operation (numpy element-wise float32 arithmetic is
IEEE-rounded per operation and never fused).

The only freedom the reference leaves is the order of tied edge weights (its std::sort is unstable).  `ties` picks it:
"asc" = ascending edge index (the library's order), "desc" = descending.  NaN weights sort last in both.
"""
import numpy as np

F32 = np.float32


def _cross(v01, v02):
    """np.cross for float32 [n,3]: each product rounded, then subtracted."""
    a0, a1, a2 = v01[:, 0], v01[:, 1], v01[:, 2]
    b0, b1, b2 = v02[:, 0], v02[:, 1], v02[:, 2]
    return a1 * b2 - a2 * b1, a2 * b0 - a0 * b2, a0 * b1 - a1 * b0


def _sum3(x, y, z):
    return (x + y) + z


def _occurrences(faces, n_vertices):
    """Every (vertex, face) occurrence sorted by vertex, then face, then slot, with positions inside the vertex's list."""
    flat = faces.reshape(-1).astype(np.int64)
    order = np.lexsort((np.arange(flat.shape[0]), flat))
    sv = flat[order]
    sf = order // 3
    n = sv.shape[0]
    idx = np.arange(n)
    new_v = np.ones(n, bool)
    new_v[1:] = sv[1:] != sv[:-1]
    new_f = new_v.copy()
    new_f[1:] |= sf[1:] != sf[:-1]
    v_start = np.maximum.accumulate(np.where(new_v, idx, 0)) if n else idx
    f_start = np.maximum.accumulate(np.where(new_f, idx, 0)) if n else idx
    pos = idx - v_start                              # position of the occurrence in its vertex's list
    before = f_start - v_start                       # occurrences of earlier faces (segmentator's counts[i])
    dpos = np.cumsum(new_f) - 1 - (np.cumsum(new_f) - 1)[v_start] if n else idx   # rank among the vertex's distinct faces
    return sv, sf, pos, before, new_f, dpos


def decode_normals(xyz, faces):
    """decode_scannet.py vertex_normal: nf * area summed over each vertex's distinct faces in face order from 0, then
    divided by sqrt(sum of squares) + 1e-8."""
    xyz = np.asarray(xyz, F32)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    v = xyz.shape[0]
    nv = np.zeros((v, 3), F32)
    if faces.shape[0]:
        p0, p1, p2 = xyz[faces[:, 0]], xyz[faces[:, 1]], xyz[faces[:, 2]]
        cx, cy, cz = _cross(p1 - p0, p2 - p0)
        ln = np.sqrt(_sum3(cx * cx, cy * cy, cz * cz)) + F32(1e-8)
        area = ln * F32(0.5)
        nfa = np.stack([(cx / ln) * area, (cy / ln) * area, (cz / ln) * area], axis=1)
        sv, sf, _, _, new_f, dpos = _occurrences(faces, v)
        sv, sf, dpos = sv[new_f], sf[new_f], dpos[new_f]
        for k in range(int(dpos.max()) + 1 if dpos.size else 0):
            sel = dpos == k
            nv[sv[sel]] = nv[sv[sel]] + nfa[sf[sel]]
    ln = np.sqrt(_sum3(nv[:, 0] * nv[:, 0], nv[:, 1] * nv[:, 1], nv[:, 2] * nv[:, 2])) + F32(1e-8)
    return nv / ln[:, None]


def segmentator_normals(xyz, faces):
    """segmentator.cpp:170-202: normalised cross product per face, blended into each vertex by a running lerp with
    v = 1 / (count + 1), once per occurrence; count grows after all three of a face's lerps."""
    xyz = np.asarray(xyz, F32)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    v = xyz.shape[0]
    n = np.zeros((v, 3), F32)
    if faces.shape[0] == 0:
        return n
    p0, p1, p2 = xyz[faces[:, 0]], xyz[faces[:, 1]], xyz[faces[:, 2]]
    cx, cy, cz = _cross(p1 - p0, p2 - p0)
    with np.errstate(invalid="ignore", divide="ignore"):
        ln = np.sqrt(_sum3(cx * cx, cy * cy, cz * cz))
        snf = np.stack([cx / ln, cy / ln, cz / ln], axis=1)
    sv, sf, pos, before, _, _ = _occurrences(faces, v)
    with np.errstate(invalid="ignore"):
        for k in range(int(pos.max()) + 1):
            sel = pos == k
            vv = sv[sel]
            t = F32(1.0) / (before[sel].astype(F32) + F32(1.0))
            u = F32(1.0) - t
            n[vv] = t[:, None] * snf[sf[sel]] + u[:, None] * n[vv]
    return n


def mesh_edges(faces):
    """(i1,i2), (i1,i3), (i3,i2) per face, in face order (segmentator.cpp:186-192)."""
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    ea = np.stack([faces[:, 0], faces[:, 0], faces[:, 2]], axis=1).reshape(-1)
    eb = np.stack([faces[:, 1], faces[:, 2], faces[:, 1]], axis=1).reshape(-1)
    return ea, eb


def edge_weights(points, normals, ea, eb):
    """segmentator.cpp:204-229: w = 1 - n1.n2, squared where n2.(p2 - p1)/|p2 - p1| > 0 (NaN: not squared)."""
    p1, p2, n1, n2 = points[ea], points[eb], normals[ea], normals[eb]
    with np.errstate(invalid="ignore", divide="ignore"):
        d = p2 - p1
        dd = np.sqrt(_sum3(d[:, 0] * d[:, 0], d[:, 1] * d[:, 1], d[:, 2] * d[:, 2]))
        dx, dy, dz = d[:, 0] / dd, d[:, 1] / dd, d[:, 2] / dd
        dot = _sum3(n1[:, 0] * n2[:, 0], n1[:, 1] * n2[:, 1], n1[:, 2] * n2[:, 2])
        dot2 = _sum3(n2[:, 0] * dx, n2[:, 1] * dy, n2[:, 2] * dz)
        w = F32(1.0) - dot
        return np.where(dot2 > 0, w * w, w).astype(F32)


def order_keys(w):
    """Order-preserving uint32 of float32 weights: -0 ties with +0, NaN is largest."""
    w = np.asarray(w, F32)
    b = np.where(w == 0, F32(0), w).view(np.uint32)
    k = np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000)).astype(np.uint32)
    return np.where(np.isnan(w), np.uint32(0xffffffff), k)


def edge_order(w, ties="asc"):
    idx = np.arange(w.shape[0], dtype=np.int64)
    sec = {"asc": idx, "desc": -idx}[ties]
    return np.lexsort((sec, order_keys(w)))


def sweep(n_vertices, ea, eb, w, c=0.01, min_size=20):
    """segment_graph + the small-segment join over edges already in sweep order, with the reference's universe; returns
    every vertex's root (segmentator.cpp:245-250)."""
    parent = list(range(n_vertices))
    rank = [0] * n_vertices
    size = [1] * n_vertices
    c32 = F32(c)

    def find(x):
        y = x
        while y != parent[y]:
            y = parent[y]
        parent[x] = y
        return y

    def join(x, y):
        if rank[x] > rank[y]:
            parent[y] = x
            size[x] += size[y]
        else:
            parent[x] = y
            size[y] += size[x]
            if rank[x] == rank[y]:
                rank[y] += 1

    thr = [float(c32)] * n_vertices
    ea_l, eb_l, w_l = ea.tolist(), eb.tolist(), w.astype(np.float64).tolist()   # float32 -> float64 is exact
    for a0, b0, wi in zip(ea_l, eb_l, w_l):
        a, b = find(a0), find(b0)
        if a != b and wi <= thr[a] and wi <= thr[b]:
            join(a, b)
            a = find(a)
            thr[a] = float(F32(wi) + c32 / F32(size[a]))
    for a0, b0 in zip(ea_l, eb_l):
        a, b = find(a0), find(b0)
        if a != b and (size[a] < min_size or size[b] < min_size):
            join(a, b)
    return np.array([find(q) for q in range(n_vertices)], np.int64)


def relabel(roots):
    """main.py:17: torch.unique(index, return_inverse=True)[1]."""
    return np.unique(roots, return_inverse=True)[1].astype(np.int64).reshape(-1)


def _segment(points, normals, ea, eb, k, m, ties, return_roots):
    v = points.shape[0]
    w = edge_weights(points, normals, ea, eb)
    o = edge_order(w, ties)
    roots = sweep(v, ea[o], eb[o], w[o], k, m)
    sup = relabel(roots) if v else np.zeros(0, np.int64)
    return (sup, roots) if return_roots else sup


def segment_mesh(xyz, faces, kThresh=0.01, segMinVerts=20, ties="asc", return_roots=False):
    xyz = np.asarray(xyz, F32)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    ea, eb = mesh_edges(faces)
    return _segment(xyz, segmentator_normals(xyz, faces), ea, eb, kThresh, segMinVerts, ties, return_roots)


def segment_point(xyz, normals, edges, kThresh=0.01, segMinVerts=20, ties="asc", return_roots=False):
    edges = np.asarray(edges, np.int64).reshape(-1, 2)
    return _segment(np.asarray(xyz, F32), np.asarray(normals, F32), edges[:, 0], edges[:, 1], kThresh, segMinVerts, ties,
                    return_roots)


def same_partition(a, b):
    """True when two labelings group the vertices identically (ids may differ)."""
    a, b = np.asarray(a).reshape(-1), np.asarray(b).reshape(-1)
    if a.shape != b.shape:
        return False
    if a.size == 0:
        return True
    pairs = np.unique(np.stack([a, b], axis=1), axis=0)
    return pairs.shape[0] == np.unique(a).shape[0] == np.unique(b).shape[0]
