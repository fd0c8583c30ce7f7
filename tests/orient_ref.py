"""numpy restatement of csrc/orient.hip's contract (include/pbnet_hip.h "Normal orientation"; pbnet_amd.mesh.orient_normals)
and the designed cases of its tests.

orient   float32 dots, one operation per line; np.argsort of the u64 keys (order_key(w) << 32 | slot); a sequential Kruskal
         over a union-find that carries every point's parity to its root; the majority rule per tree.  The keys are
         distinct, so the minimum spanning forest is unique and a parallel Boruvka must give the same bytes.
boruvka  a simulation of the rounds the device runs (minimum outgoing edge per component, offered to BOTH sides; hook;
         compress), for what Kruskal cannot show: the length of the hooking chains, and the `source_only` mistake.

`wrong=` names one deliberate mistake:
  signed_weight  w = 1 - d instead of 1 - |d|
  tie_any        the key without the slot id: equal weights come in some other order (here: descending slot)
  source_only    an edge is offered only to its source's component (the rounds then pick other edges)
  root_keeps     no majority vote: the tree's lowest-index point keeps its sign
  tie_flips      on a tie the tree's lowest-index point flips
  null_joins     null points take part like any other
  self_edge      the self slot is taken to be column 0, as searches that return the query itself have it, instead of being
                 tested by index (j != i).  A slot with j == i can never join two components, so that half of the mistake
                 is invisible in any output; the half that drops a real neighbour is what a case can catch
"""
import numpy as np

import cloud_ref

F32 = np.float32
WRONG = ("signed_weight", "tie_any", "source_only", "root_keeps", "tie_flips", "null_joins", "self_edge")


def order_key(w):
    """csrc/mesh.hip order_key: order-preserving bits of a float32, NaN last, -0 tied with +0."""
    w = np.ascontiguousarray(w, F32)
    b = w.view(np.uint32).copy()
    b[w == 0] = 0
    key = np.where((b & np.uint32(0x80000000)) != 0, ~b, b | np.uint32(0x80000000)).astype(np.uint32)
    key[np.isnan(w)] = np.uint32(0xffffffff)
    return key


def null_points(nl):
    nl = np.asarray(nl, F32)
    return ~np.isfinite(nl).all(1) | (nl == 0).all(1)


def edges(nl, idx, wrong=None):
    """Per slot e = i * k + r: (valid bool, i, j, key u64, f bool)."""
    nl = np.ascontiguousarray(nl, F32)
    idx = np.asarray(idx, np.int32)
    n, k = idx.shape
    null = null_points(nl) if wrong != "null_joins" else np.zeros(n, bool)
    i = np.repeat(np.arange(n, dtype=np.int64), k)
    j = idx.reshape(-1).astype(np.int64)
    in_range = (j >= 0) & (j < n)
    js = np.where(in_range, j, 0)
    if wrong == "self_edge":
        not_self = np.tile(np.arange(k) != 0, n)
    else:
        not_self = j != i
    valid = in_range & not_self & ~null[i] & ~null[js]
    with np.errstate(all="ignore"):
        xx = nl[i, 0] * nl[js, 0]
        yy = nl[i, 1] * nl[js, 1]
        xy = xx + yy
        zz = nl[i, 2] * nl[js, 2]
        d = xy + zz
        assert d.dtype == F32
        w = F32(1.0) - (d if wrong == "signed_weight" else np.abs(d))
    f = d < F32(0.0)
    e = np.arange(n * k, dtype=np.uint64)
    low = np.uint64(max(n * k - 1, 0)) - e if wrong == "tie_any" else e
    key = (order_key(w).astype(np.uint64) << np.uint64(32)) | low
    return valid, i, js, key, f


class ParityForest:
    """Union-find in which every point knows its parity to its root."""

    def __init__(self, n):
        self.parent = list(range(n))
        self.par = [0] * n

    def find(self, x):
        path = []
        while self.parent[x] != x:
            path.append(x)
            x = self.parent[x]
        p = 0
        for y in reversed(path):                                             # from the root's child down to the start
            p ^= self.par[y]
            self.parent[y], self.par[y] = x, p
        return x, p

    def union(self, a, b, f):
        """s_a ^ s_b = f; False when a and b are joined already."""
        ra, pa = self.find(a)
        rb, pb = self.find(b)
        if ra == rb:
            return False
        self.parent[ra], self.par[ra] = rb, pa ^ pb ^ f
        return True


def kruskal(n, slots, i, j, f):
    """The forest over the given slots in the given order: (ParityForest, accepted slots)."""
    uf = ParityForest(n)
    taken = []
    for e in slots.tolist():
        if uf.union(int(i[e]), int(j[e]), int(f[e])):
            taken.append(e)
    return uf, taken


def boruvka(nl, idx, wrong=None):
    """The rounds as the device runs them.  Returns (chosen slots of all rounds, the longest hooking chain per round)."""
    valid, i, j, key, f = edges(nl, idx, wrong)
    n = np.asarray(idx).shape[0]
    comp = np.arange(n, dtype=np.int64)
    empty = np.uint64(0xffffffffffffffff)
    chosen, chains = [], []
    slot_of = np.flatnonzero(valid)
    while True:
        out = slot_of[comp[i[slot_of]] != comp[j[slot_of]]]
        if out.size == 0:
            break
        best = np.full(n, empty, np.uint64)
        np.minimum.at(best, comp[i[out]], key[out])
        if wrong != "source_only":
            np.minimum.at(best, comp[j[out]], key[out])
        key_slot = dict(zip(key[out].tolist(), out.tolist()))
        link = np.arange(n, dtype=np.int64)
        for c in np.flatnonzero(best != empty).tolist():
            e = key_slot[int(best[c])]
            a, b = int(comp[i[e]]), int(comp[j[e]])
            o = b if a == c else a
            if best[o] == best[c] and c < o:
                continue
            link[c] = o
            chosen.append(e)
        hooked = np.flatnonzero(link != np.arange(n))
        if wrong is None:                                                    # a forest: the hops from every root to its new root
            hops = np.zeros(n, np.int64)
            cur = np.arange(n)
            for _ in range(n):
                nxt = link[cur]
                step = nxt != cur
                if not step.any():
                    break
                hops += step
                cur = nxt
            chains.append(int(hops.max()))
        else:                                                                # source_only can close a cycle: merge by union-find
            uf = ParityForest(n)
            for c in hooked.tolist():
                uf.union(c, int(link[c]), 0)
            cur = np.asarray([uf.find(c)[0] for c in range(n)], np.int64)
        comp = cur[comp]
    return np.asarray(sorted(set(chosen), key=lambda e: int(key[e])), np.int64), chains


def orient(nl, idx, wrong=None):
    """{"nl" f32 [N, 3], "flipped" bool [N], "tree" int32 [N], "stats" int32 [4]} as the header states them."""
    assert wrong is None or wrong in WRONG, wrong
    nl = np.ascontiguousarray(nl, F32).reshape(-1, 3)
    idx = np.asarray(idx, np.int32)
    n = nl.shape[0]
    valid, i, j, key, f = edges(nl, idx, wrong)
    if wrong == "source_only":
        slots = boruvka(nl, idx, wrong)[0]
    else:
        slots = np.flatnonzero(valid)
        slots = slots[np.argsort(key[slots], kind="stable")]
    uf, _ = kruskal(n, slots, i, j, f)
    null = null_points(nl) if wrong != "null_joins" else np.zeros(n, bool)
    root = np.zeros(n, np.int64)
    s = np.zeros(n, np.int64)
    for p in range(n):
        root[p], s[p] = uf.find(p)
    ones = np.bincount(root, weights=s, minlength=n).astype(np.int64)
    members = np.bincount(root, minlength=n)
    lowest = np.full(n, n, np.int64)
    np.minimum.at(lowest, root, np.arange(n))
    n1, n0, low = ones[root], (members - ones)[root], lowest[root]
    if wrong == "root_keeps":
        invert = s[low] == 1
    elif wrong == "tie_flips":
        invert = (n1 > n0) | ((n1 == n0) & (s[low] == 0))
    else:
        invert = (n1 > n0) | ((n1 == n0) & (s[low] == 1))
    flipped = ((s ^ invert.astype(np.int64)) == 1) & ~null
    out = nl.copy()
    out.view(np.uint32)[flipped] ^= np.uint32(0x80000000)                    # the sign bit: an exact negation, -0 and NaN included
    tree = np.where(null, np.arange(n), low).astype(np.int32)
    stats = np.array([np.unique(tree[~null]).size, int(flipped.sum()), int(null.sum()), 0], np.int32)
    return {"nl": out, "flipped": flipped, "tree": tree, "stats": stats}


# ------------------------------------------------------------------------------------------------------- designed cases
def _unit(rng, n):
    v = rng.standard_normal((n, 3))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(F32)


def _blob(seed, n, k):
    rng = np.random.default_rng(seed)
    xyz = rng.standard_normal((n, 3)).astype(F32)
    return _unit(rng, n), cloud_ref.knn(xyz, k)[0]


def _lattice(side=24, k=8):
    g = np.stack(np.meshgrid(np.arange(side), np.arange(side), indexing="ij"), -1).reshape(-1, 2)
    xyz = np.concatenate([g, np.zeros((g.shape[0], 1))], 1).astype(F32)
    return xyz, cloud_ref.knn(xyz, k)[0]


def _signed_z(neg):
    nl = np.zeros((neg.shape[0], 3), F32)
    nl[:, 2] = np.where(neg, -1.0, 1.0)
    return nl


def lattice_plane():
    xyz, idx = _lattice()
    rng = np.random.default_rng(11)
    neg = np.zeros(xyz.shape[0], bool)
    neg[rng.permutation(xyz.shape[0])[:int(0.3 * xyz.shape[0])]] = True      # exactly 30 % negative
    return _signed_z(neg), idx


def tie_half(point0_negative=False):
    xyz, idx = _lattice()
    n = xyz.shape[0]
    rng = np.random.default_rng(12)
    neg = np.zeros(n, bool)
    neg[1 + rng.permutation(n - 1)[:n // 2]] = True                          # exactly half, point 0 positive
    return _signed_z(neg ^ point0_negative), idx


def tie_triangle():
    """Three points, every |dot| exactly 1 (all weights 0) and an odd number of negative dots around the cycle: which two
    of the three edges make the tree decides the signs, and only the slot ids order them."""
    nl = np.array([[1, 0, 0], [1, 1, 0], [-1, 2, 0]], F32)
    return nl, np.array([[1, 2], [0, 2], [0, 1]], np.int32)


def short_rows():
    idx = np.full((5, 16), -1, np.int32)
    idx[0, :4] = [1, 2, 3, 4]
    idx[1, :3] = [0, 5, 2]                                                   # 5 = N: no neighbour
    idx[2, :3] = [-7, 1, 3]
    idx[3, :2] = [3, 4]                                                      # a self slot
    idx[4, :1] = [0]
    return _unit(np.random.default_rng(13), 5), idx


def null_mixed():
    nl, idx = _blob(14, 300, 8)
    nl[::7] = 0.0
    nl[3, 1] = -0.0
    nl[100, 0] = np.nan
    nl[200, 2] = np.inf
    return nl, idx


def coincident():
    rng = np.random.default_rng(15)
    return _unit(rng, 200), cloud_ref.knn(np.ones((200, 3), F32), 8)[0]


def chain(n=4096):
    """Points on a line, neighbours i - 1 and i + 1; the angle between consecutive normals grows strictly, so the weights
    do, and in the first round every point but the first hooks onto its left neighbour: one chain of n - 2 hops."""
    step = 0.01 + 2.0e-4 * np.arange(n - 1)
    theta = np.concatenate([[0.0], np.cumsum(step)])
    nl = np.stack([np.zeros(n), np.cos(theta), np.sin(theta)], 1).astype(F32)
    neg = np.random.default_rng(16).random(n) < 0.4
    nl[neg] = -nl[neg]
    idx = np.stack([np.arange(n) - 1, np.arange(n) + 1], 1).astype(np.int32)
    idx[-1, 1] = -1
    return nl, idx


ISLAND_SIZES = (40, 41, 300)


def islands():
    rng = np.random.default_rng(17)
    xyz = np.concatenate([rng.standard_normal((m, 3)) + [100.0 * b, 0, 0] for b, m in enumerate(ISLAND_SIZES)]).astype(F32)
    neg0 = np.zeros(40, bool)
    neg0[rng.permutation(40)[:16]] = True                                    # 60 % positive
    neg1 = np.zeros(41, bool)
    neg1[rng.permutation(41)[:20]] = True                                    # 21 positive, 20 negative
    nl = np.concatenate([_signed_z(neg0), _signed_z(neg1), _unit(rng, 300)])
    return nl, cloud_ref.knn(xyz, 8)[0]


def sphere_outside(n=2000):
    rng = np.random.default_rng(18)
    xyz = _unit(rng, n)
    nl = xyz.copy()
    away = np.einsum("ij,ij->i", nl.astype(np.float64), np.array([5.0, 0, 0]) - xyz) < 0
    nl[away] = -nl[away]
    return nl, cloud_ref.knn(xyz, 8)[0], xyz


SHEET_POINTS = 1600


def sheet_at_mean_points():
    """A 40 x 40 sheet at z = 0 with 1 mm of noise and two mirrored blobs, so that the mean lies in the sheet."""
    rng = np.random.default_rng(19)
    g = np.stack(np.meshgrid(np.arange(40), np.arange(40), indexing="ij"), -1).reshape(-1, 2) * 0.05 - 0.975
    sheet = np.concatenate([g, 0.001 * rng.standard_normal((SHEET_POINTS, 1))], 1)
    blob = 0.1 * rng.standard_normal((150, 3)) + [0.0, 0.0, 1.0]
    return np.concatenate([sheet, blob, blob * [1.0, 1.0, -1.0]]).astype(F32)


def sheet_at_mean(k=16):
    xyz = sheet_at_mean_points()
    idx = cloud_ref.knn(xyz, k)[0]
    return cloud_ref.normals(xyz, idx, None)[0].astype(F32), idx


def _build():
    cases = {
        "n0": (np.zeros((0, 3), F32), np.zeros((0, 4), np.int32)),
        "n1": (_unit(np.random.default_rng(1), 1), np.full((1, 3), -1, np.int32)),
        "n2": (_unit(np.random.default_rng(2), 1) * F32([[1.0], [-1.0]]), np.array([[1], [0]], np.int32)),   # n and -n
        "all_null": (np.zeros((20, 3), F32), cloud_ref.knn(np.random.default_rng(3).standard_normal((20, 3)), 4)[0]),
        "tie_triangle": tie_triangle(),
        "short_rows": short_rows(),
        "null_mixed": null_mixed(),
        "lattice_plane": lattice_plane(),
        "tie_half": tie_half(False),
        "tie_half_mirror": tie_half(True),
        "coincident": coincident(),
        "chain": chain(),
        "islands": islands(),
        "sphere_outside": sphere_outside()[:2],
        "sheet_at_mean": sheet_at_mean(),
    }
    for n in (63, 64, 65, 255, 256):
        cases["n%d" % n] = _blob(100 + n, n, 8)
    for k in (1, 6, 16, 32):
        cases["n257_k%d" % k] = _blob(357, 257, k)
    return cases


_CASES, _WANT = None, {}


def cases():
    global _CASES
    if _CASES is None:
        _CASES = _build()
    return _CASES


def want(name):
    """orient() of a designed case, computed once and shared."""
    if name not in _WANT:
        _WANT[name] = orient(*cases()[name])
    return _WANT[name]
