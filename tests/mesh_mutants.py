"""A second statement of the mesh decode, written the way csrc/mesh.hip works -- per-vertex incidence lists from count, exclusive
scan, fill and a per-vertex sort of the entries 3 * face + slot; the uint32 order key of a float32 weight; an LSD radix sort of
three 11-bit digits carrying the edge index; the host sweep with the reference's universe (union by rank, sizes, one-step path
compression); the relabel by the rank of a vertex's root among the roots -- with one switch per deliberate mistake.  With
mutant=None it must equal tests/mesh_ref.py on every designed case of tests/mesh_cases.py: nl bits, segmentator normals, weights,
sweep order, roots and sup (tests/test_mesh_cases_cpu.py).  A mutant that equals it on every case shows the set is too weak.

Not listed, because no input can tell them apart:
  * path compression (find's `parent[x] = y`): it shortens walks, never changes a root, a size, a rank or a threshold;
  * -0 tied with +0 in the order key: `1 - dot` and `w * w` never give -0 under round-to-nearest (x - x is +0, a square is >= +0),
    so no weight is ever -0.

EQUIVALENT holds three mistakes the issue of this case set asked for that CAN be written down but cannot change an output either.
All three differ from the kernel only at the second or third occurrence of one vertex in one face.  Such a face has two equal
corners, so one of its edge vectors is exactly (0, 0, 0) or both are equal: every product pair of the cross product cancels
exactly (or is NaN for non-finite coordinates).  Its nfa is therefore (+-0, +-0, +-0) or NaN -- adding it once or twice gives the
same bits -- and its segmentator normal is 0 / 0 = NaN, after which the vertex's running lerp is NaN whatever t and count are.
test_mesh_cases_cpu.py asserts that premise and that the three agree with the reference on every case."""
import numpy as np

import mesh_ref as MR

F32 = np.float32

MUTANTS = ("incidence_reversed", "third_edge_i2_i3", "dot2_from_n1", "dot2_ge", "nan_dot2_squared", "negative_keys_unflipped",
           "nan_first", "ties_desc", "sort_drops_top_digit", "strict_threshold", "threshold_f64", "threshold_size_before_join",
           "min_size_le", "second_pass_input_order", "rank_tie_other_side", "relabel_by_first_appearance")
EQUIVALENT = ("nl_once_per_occurrence", "lerp_count_per_occurrence", "lerp_t_from_position")
SWITCHES = MUTANTS + EQUIVALENT

RADIX_BITS, PASSES = 11, 3


def _incidence(idx, n_vertices, mutant):
    """off [V+1] and inc: per vertex the entries 3 * face + slot, as k_mesh_index / scan / k_mesh_fill / the insertion sort leave them."""
    cnt = np.zeros(n_vertices, np.int64)
    for v in idx.tolist():
        cnt[v] += 1
    off = np.zeros(n_vertices + 1, np.int64)
    off[1:] = np.cumsum(cnt)
    cur = np.zeros(n_vertices, np.int64)
    inc = np.zeros(idx.shape[0], np.int64)
    for i in range(idx.shape[0] - 1, -1, -1):              # some arrival order; the sort below must remove it
        v = int(idx[i])
        inc[off[v] + cur[v]] = i
        cur[v] += 1
    for v in range(n_vertices):
        part = np.sort(inc[off[v]:off[v + 1]])
        inc[off[v]:off[v + 1]] = part[::-1] if mutant == "incidence_reversed" else part
    return off, inc


def _face_normals(xyz, faces):
    p0, p1, p2 = xyz[faces[:, 0]], xyz[faces[:, 1]], xyz[faces[:, 2]]
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        a, b = p1 - p0, p2 - p0
        cx = a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1]
        cy = a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2]
        cz = a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]
        ss = (cx * cx + cy * cy) + cz * cz
        ln = np.sqrt(ss) + F32(1.0e-8)
        area = ln * F32(0.5)
        nfa = np.stack([(cx / ln) * area, (cy / ln) * area, (cz / ln) * area], 1).astype(F32)
        n = np.sqrt(ss)
        snf = np.stack([cx / n, cy / n, cz / n], 1).astype(F32)
    return nfa, snf


def _vertex_normals(off, inc, n_vertices, nfa, snf, mutant):
    nl = np.zeros((n_vertices, 3), F32)
    sn = np.zeros((n_vertices, 3), F32)
    one = F32(1.0)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for v in range(n_vertices):
            lst = inc[off[v]:off[v + 1]].tolist()
            s = np.zeros(3, F32)
            prev = -1
            for e in lst:
                f = e // 3
                if f == prev and mutant != "nl_once_per_occurrence":
                    continue
                prev = f
                s = s + nfa[f]
            ln = np.sqrt((s[0] * s[0] + s[1] * s[1]) + s[2] * s[2]) + F32(1.0e-8)
            nl[v] = s / ln
            n = np.zeros(3, F32)
            count = 0
            i = 0
            while i < len(lst):
                f = lst[i] // 3
                k = i
                while k < len(lst) and lst[k] // 3 == f:
                    c = count
                    if mutant == "lerp_count_per_occurrence":
                        c = count + (k - i)
                    elif mutant == "lerp_t_from_position":
                        c = k
                    t = one / (F32(c) + one)
                    u = one - t
                    n = t * snf[f] + u * n
                    k += 1
                count += k - i
                i = k
            sn[v] = n
    return nl, sn


def _edge_ends(idx, mode, mutant):
    if mode == "point":
        e = idx.reshape(-1, 2)
        return e[:, 0].copy(), e[:, 1].copy()
    f = idx.reshape(-1, 3)
    i1, i2, i3 = f[:, 0], f[:, 1], f[:, 2]
    if mutant == "third_edge_i2_i3":
        return np.stack([i1, i1, i2], 1).reshape(-1), np.stack([i2, i3, i3], 1).reshape(-1)
    return np.stack([i1, i1, i3], 1).reshape(-1), np.stack([i2, i3, i2], 1).reshape(-1)


def _weights(xyz, nrm, ea, eb, mutant):
    p1, p2, n1, n2 = xyz[ea], xyz[eb], nrm[ea], nrm[eb]
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        d = p2 - p1
        dd = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
        d = d / dd[:, None]
        dot = (n1[:, 0] * n2[:, 0] + n1[:, 1] * n2[:, 1]) + n1[:, 2] * n2[:, 2]
        q = n1 if mutant == "dot2_from_n1" else n2
        dot2 = (q[:, 0] * d[:, 0] + q[:, 1] * d[:, 1]) + q[:, 2] * d[:, 2]
        w = F32(1.0) - dot
        square = dot2 >= 0 if mutant == "dot2_ge" else dot2 > 0
        if mutant == "nan_dot2_squared":
            square = square | np.isnan(dot2)
        return np.where(square, w * w, w).astype(F32)


def _order_key(w, mutant):
    b = w.view(np.uint32).copy()
    b[w == 0] = 0
    top = np.uint32(0x80000000)
    flipped = b | top if mutant == "negative_keys_unflipped" else ~b
    k = np.where(b & top, flipped, b | top).astype(np.uint32)
    k[np.isnan(w)] = 0 if mutant == "nan_first" else 0xffffffff
    return k


def _radix_sort(keys, mutant):
    """Edge indices in sweep order: LSD passes, each a stable counting sort of one 11-bit digit."""
    n = keys.shape[0]
    vals = np.arange(n, dtype=np.int64)
    if mutant == "ties_desc":
        vals = vals[::-1].copy()
    k = keys[vals].astype(np.int64)
    for p in range(PASSES - 1 if mutant == "sort_drops_top_digit" else PASSES):
        digit = (k >> (RADIX_BITS * p)) & ((1 << RADIX_BITS) - 1)
        hist = np.bincount(digit, minlength=1 << RADIX_BITS)
        base = np.cumsum(hist) - hist
        pos = np.zeros(n, np.int64)
        seen = base.copy()
        for i, dg in enumerate(digit.tolist()):
            pos[i] = seen[dg]
            seen[dg] += 1
        k2, v2 = np.empty_like(k), np.empty_like(vals)
        k2[pos], v2[pos] = k, vals
        k, vals = k2, v2
    return vals


def _sweep(n_vertices, ea, eb, ew, ea_in, eb_in, c, min_size, mutant):
    rank = [0] * n_vertices
    parent = list(range(n_vertices))
    size = [1] * n_vertices
    c32 = F32(c)

    def find(x):
        y = x
        while y != parent[y]:
            y = parent[y]
        parent[x] = y
        return y

    def join(x, y):
        if rank[x] > rank[y] or (mutant == "rank_tie_other_side" and rank[x] == rank[y]):
            parent[y] = x
            size[x] += size[y]
            if rank[x] == rank[y]:
                rank[x] += 1
        else:
            parent[x] = y
            size[y] += size[x]
            if rank[x] == rank[y]:
                rank[y] += 1

    thr = [c32] * n_vertices
    with np.errstate(all="ignore"):
        for a0, b0, w in zip(ea.tolist(), eb.tolist(), list(ew)):
            a, b = find(a0), find(b0)
            if a == b:
                continue
            ok = (w < thr[a] and w < thr[b]) if mutant == "strict_threshold" else (w <= thr[a] and w <= thr[b])
            if ok:
                before = size[a]
                join(a, b)
                a = find(a)
                s = before if mutant == "threshold_size_before_join" else size[a]
                if mutant == "threshold_f64":
                    thr[a] = float(w) + float(c32) / s
                else:
                    thr[a] = w + c32 / F32(s)
    second = zip(ea_in.tolist(), eb_in.tolist()) if mutant == "second_pass_input_order" else zip(ea.tolist(), eb.tolist())
    for a0, b0 in second:
        a, b = find(a0), find(b0)
        small = (size[a] <= min_size or size[b] <= min_size) if mutant == "min_size_le" else (size[a] < min_size or size[b] < min_size)
        if a != b and small:
            join(a, b)
    return np.array([find(q) for q in range(n_vertices)], np.int64)


def _relabel(roots, mutant):
    n = roots.shape[0]
    if mutant == "relabel_by_first_appearance":
        ids, sup = {}, np.zeros(n, np.int64)
        for v, r in enumerate(roots.tolist()):
            sup[v] = ids.setdefault(r, len(ids))
        return sup
    flag = (roots == np.arange(n)).astype(np.int64)
    rank = np.cumsum(flag) - flag
    return rank[roots]


def decode(case, mutant=None):
    """Everything mesh.hip computes for a case of tests/mesh_cases.py: nl and sn (mesh mode), w, order, roots, sup."""
    assert mutant is None or mutant in SWITCHES, mutant
    xyz = np.asarray(case["xyz"], F32)
    v = xyz.shape[0]
    out = {}
    if case["mode"] == "mesh":
        faces = np.asarray(case["faces"], np.int64).reshape(-1, 3)
        idx = faces.reshape(-1)
        off, inc = _incidence(idx, v, mutant)
        nfa, snf = _face_normals(xyz, faces)
        out["nl"], out["sn"] = _vertex_normals(off, inc, v, nfa, snf, mutant)
        nrm = out["sn"]
    else:
        idx = np.asarray(case["edges"], np.int64).reshape(-1)
        nrm = np.asarray(case["normals"], F32)
    ea, eb = _edge_ends(idx, case["mode"], mutant)
    w = _weights(xyz, nrm, ea, eb, mutant)
    order = _radix_sort(_order_key(w, mutant), mutant)
    roots = _sweep(v, ea[order], eb[order], w[order], ea, eb, case["k_thresh"], case["seg_min_verts"], mutant)
    out.update(w=w, order=order, roots=roots, sup=_relabel(roots, mutant) if v else np.zeros(0, np.int64))
    return out


def reference(case, ties="asc"):
    """The same dict from tests/mesh_ref.py."""
    xyz = np.asarray(case["xyz"], F32)
    out = {}
    if case["mode"] == "mesh":
        faces = np.asarray(case["faces"], np.int64).reshape(-1, 3)
        out["nl"] = MR.decode_normals(xyz, faces)
        out["sn"] = nrm = MR.segmentator_normals(xyz, faces)
        ea, eb = MR.mesh_edges(faces)
    else:
        nrm = np.asarray(case["normals"], F32)
        e = np.asarray(case["edges"], np.int64).reshape(-1, 2)
        ea, eb = e[:, 0], e[:, 1]
    w = MR.edge_weights(xyz, nrm, ea, eb)
    order = MR.edge_order(w, ties)
    roots = MR.sweep(xyz.shape[0], ea[order], eb[order], w[order], case["k_thresh"], case["seg_min_verts"])
    out.update(w=w, order=order, roots=roots, sup=MR.relabel(roots) if xyz.shape[0] else np.zeros(0, np.int64))
    return out


def same(a, b):
    """Bit for bit: floats by their bits (NaN payloads included), integers by value."""
    if set(a) != set(b):
        return False
    for k in a:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        if x.shape != y.shape:
            return False
        if x.dtype == F32:
            if k in ("sn", "w"):                     # NaN sign and payload are not part of the contract: NaN == NaN here
                nx, ny = np.isnan(x), np.isnan(y)
                if not np.array_equal(nx, ny) or not np.array_equal(x.view(np.uint32)[~nx], y.view(np.uint32)[~ny]):
                    return False
            elif not np.array_equal(x.view(np.uint32), y.view(np.uint32)):
                return False
        elif not np.array_equal(x, y):
            return False
    return True
