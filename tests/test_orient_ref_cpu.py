"""CPU tier for the normal orientation (csrc/orient.hip): the numpy restatement tests/orient_ref.py agrees with two
independent checks (brute force over ALL spanning forests on tiny graphs; scipy's minimum spanning tree after a tie-free
perturbation on the rest), every deliberate mistake shows on a named case, the designed cases have the properties they were
designed for, and the host argument checks raise before anything touches the library."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

import orient_ref as R
from pbnet_amd import _native as N
from pbnet_amd import mesh


# ---------------------------------------------------------------------------------------------- independent checks
def _outputs_from_forest(nl, null, forest):
    """The contract's signs, majority rule and outputs from a forest given as (a, b, f) triples, by a graph walk."""
    n = nl.shape[0]
    adj = [[] for _ in range(n)]
    for a, b, f in forest:
        adj[a].append((b, f))
        adj[b].append((a, f))
    s = np.zeros(n, np.int64)
    tree = np.arange(n)
    seen = np.zeros(n, bool)
    flipped = np.zeros(n, bool)
    for start in range(n):                                                   # ascending: a tree is met at its lowest point
        if seen[start] or null[start]:
            continue
        members, stack = [start], [start]
        seen[start] = True
        while stack:
            a = stack.pop()
            for b, f in adj[a]:
                if not seen[b]:
                    seen[b] = True
                    s[b] = s[a] ^ f
                    members.append(b)
                    stack.append(b)
        members = np.asarray(members)
        ones = int(s[members].sum())
        invert = ones > members.size - ones                                  # on a tie `start` (s = 0, the lowest) keeps its sign
        flipped[members] = (s[members] ^ int(invert)) == 1
        tree[members] = start
    out = nl.copy()
    out[flipped] = -out[flipped]
    return out, flipped, tree.astype(np.int32)


def _pairs(nl, idx):
    """Per unordered pair the smallest key among its slots, with that slot's f."""
    valid, i, j, key, f = R.edges(nl, idx)
    pairs = {}
    for e in np.flatnonzero(valid).tolist():
        p = (min(int(i[e]), int(j[e])), max(int(i[e]), int(j[e])))
        if p not in pairs or int(key[e]) < pairs[p][0]:
            pairs[p] = (int(key[e]), int(f[e]))
    return pairs


def _connected_components(n, pair_list):
    lab = list(range(n))

    def find(x):
        while lab[x] != x:
            x = lab[x]
        return x
    joins = 0
    for a, b in pair_list:
        ra, rb = find(a), find(b)
        if ra != rb:
            lab[ra] = rb
            joins += 1
    return joins


def _brute_forest(nl, idx):
    """Of all spanning forests the one whose ascending key sequence is lexicographically smallest."""
    n = nl.shape[0]
    pairs = _pairs(nl, idx)
    names = sorted(pairs, key=lambda p: pairs[p][0])
    size = _connected_components(n, names)                                   # edges of any spanning forest
    best = None
    for subset in itertools.combinations(names, size):                       # ascending key order within a subset
        if _connected_components(n, subset) != size:
            continue                                                         # a cycle, hence not spanning
        keys = [pairs[p][0] for p in subset]
        if best is None or keys < best[0]:
            best = (keys, subset)
    return [(a, b, pairs[(a, b)][1]) for a, b in (best[1] if best else ())]


def _scipy_forest(nl, idx):
    sp = pytest.importorskip("scipy.sparse")
    from scipy.sparse.csgraph import minimum_spanning_tree
    n = nl.shape[0]
    pairs = _pairs(nl, idx)
    names = sorted(pairs, key=lambda p: pairs[p][0])
    rank = np.arange(1, len(names) + 1, dtype=np.float64)                    # the tie-free perturbation: rank in the strict order
    rows, cols = np.array([p[0] for p in names], np.int64), np.array([p[1] for p in names], np.int64)
    mst = minimum_spanning_tree(sp.csr_matrix((rank, (rows, cols)), shape=(n, n))).tocoo()
    return [(int(a), int(b), pairs[(min(a, b), max(a, b))][1]) for a, b in zip(mst.row, mst.col)]


def _same(got, nl, forest):
    out, flipped, tree = _outputs_from_forest(np.ascontiguousarray(nl, np.float32), R.null_points(nl), forest)
    assert np.array_equal(got["flipped"], flipped)
    assert np.array_equal(got["tree"], tree)
    assert got["nl"].tobytes() == out.tobytes()
    null = R.null_points(nl)
    assert got["stats"].tolist() == [np.unique(tree[~null]).size, int(flipped.sum()), int(null.sum()), 0]


def _tiny_cases():
    out = {name: R.cases()[name] for name in ("n0", "n1", "n2", "tie_triangle", "short_rows")}
    rng = np.random.default_rng(5)
    for n, k, ties in ((6, 3, False), (7, 3, False), (7, 4, True), (6, 5, True), (7, 2, False)):
        xyz = rng.standard_normal((n, 3)).astype(np.float32)
        nl = R._signed_z(rng.random(n) < 0.5) if ties else R._unit(rng, n)
        if ties:
            nl[:, 0] = rng.integers(-1, 2, n)                                 # small integers: many equal |dots|, exact
        idx = R.cloud_ref.knn(xyz, k)[0]
        out["tiny_n%d_k%d_%s" % (n, k, "ties" if ties else "random")] = (nl, idx)
    nl, idx = out["tiny_n7_k4_ties"]
    nl = nl.copy()
    nl[2] = 0.0                                                              # a null point in the middle
    out["tiny_null"] = (nl, idx)
    return out


@pytest.mark.parametrize("name", sorted(_tiny_cases()))
def test_restatement_is_the_least_of_all_spanning_forests(name):
    nl, idx = _tiny_cases()[name]
    assert nl.shape[0] <= 7
    _same(R.orient(nl, idx), nl, _brute_forest(nl, idx))


@pytest.mark.parametrize("name", ["n63", "n257_k1", "n257_k6", "n257_k32", "null_mixed", "lattice_plane", "tie_half",
                                  "coincident", "chain", "islands", "sphere_outside", "sheet_at_mean", "all_null"])
def test_restatement_agrees_with_scipy_mst(name):
    nl, idx = R.cases()[name]
    _same(R.want(name), nl, _scipy_forest(nl, idx))


def test_boruvka_simulation_finds_kruskals_forest():
    for name in ("n257_k6", "islands", "null_mixed", "chain", "tie_triangle"):
        nl, idx = R.cases()[name]
        valid, i, j, key, f = R.edges(nl, idx)
        slots = np.flatnonzero(valid)
        _, taken = R.kruskal(nl.shape[0], slots[np.argsort(key[slots])], i, j, f)
        assert R.boruvka(nl, idx)[0].tolist() == taken, name


# ------------------------------------------------------------------------------------------------------ the mistakes
MISTAKE_SHOWS_ON = {
    "signed_weight": "coincident",
    "tie_any": "tie_triangle",
    "source_only": "islands",
    "root_keeps": "islands",
    "tie_flips": "tie_half",
    "null_joins": "all_null",
    "self_edge": "n2",
}


@pytest.mark.parametrize("wrong", R.WRONG)
def test_every_mistake_changes_a_named_case(wrong):
    name = MISTAKE_SHOWS_ON[wrong]
    got, want = R.orient(*R.cases()[name], wrong=wrong), R.want(name)
    assert any(got[k].tobytes() != want[k].tobytes() for k in ("nl", "flipped", "tree", "stats")), (wrong, name)


def test_mistake_table_is_complete():
    assert sorted(MISTAKE_SHOWS_ON) == sorted(R.WRONG)


# ---------------------------------------------------------------------------------------------------- the properties
def test_empty_single_and_null_clouds():
    assert R.want("n0")["stats"].tolist() == [0, 0, 0, 0] and R.want("n0")["nl"].shape == (0, 3)
    assert R.want("n1")["stats"].tolist() == [1, 0, 0, 0] and R.want("n1")["tree"].tolist() == [0]
    w = R.want("n2")                                                         # opposite normals: a tie, point 0 keeps its sign
    assert w["flipped"].tolist() == [False, True] and w["tree"].tolist() == [0, 0]
    w = R.want("all_null")
    assert w["stats"].tolist() == [0, 0, 20, 0] and w["tree"].tolist() == list(range(20)) and not w["flipped"].any()


def test_null_points_stay_as_they_are():
    nl, _ = R.cases()["null_mixed"]
    w = R.want("null_mixed")
    null = R.null_points(nl)
    assert null.sum() == 45 and np.isnan(nl[100, 0]) and np.isinf(nl[200, 2])
    assert w["nl"][null].tobytes() == nl[null].tobytes() and not w["flipped"][null].any()
    assert np.array_equal(w["tree"][null], np.flatnonzero(null))
    assert w["stats"][2] == 45 and np.signbit(w["nl"][3, 1]) != w["flipped"][3]   # -0 flips like any number


def test_short_rows_ignore_what_is_no_neighbour():
    nl, idx = R.cases()["short_rows"]
    assert idx.shape == (5, 16) and (idx == 5).sum() == 1 and (idx == -7).sum() == 1 and (idx[3] == 3).sum() == 1
    cleaned = np.where((idx < 0) | (idx >= 5) | (idx == np.arange(5)[:, None]), -1, idx)
    for k in ("nl", "flipped", "tree", "stats"):
        assert R.orient(nl, cleaned)[k].tobytes() == R.want("short_rows")[k].tobytes()


def test_lattice_only_slot_ids_order_the_edges():
    nl, idx = R.cases()["lattice_plane"]
    _, _, _, key, _ = R.edges(nl, idx)
    assert np.all(key >> np.uint64(32) == np.uint64(0x80000000))             # every weight is exactly 0
    w = R.want("lattice_plane")
    assert (nl[:, 2] < 0).sum() == int(0.3 * 576) and np.all(w["nl"][:, 2] == 1.0) and w["stats"].tolist() == [1, 172, 0, 0]
    assert np.array_equal(w["flipped"], nl[:, 2] < 0)


def test_a_tie_keeps_the_lowest_point():
    for name, sign in (("tie_half", 1.0), ("tie_half_mirror", -1.0)):
        nl, _ = R.cases()[name]
        assert (nl[:, 2] > 0).sum() == 288 and nl[0, 2] == sign
        assert np.all(R.want(name)["nl"][:, 2] == sign) and R.want(name)["stats"].tolist() == [1, 288, 0, 0]
    w = R.want("tie_triangle")
    assert w["flipped"].tolist() == [False, False, True]


def test_coincident_points_orient_like_any_others():
    w = R.want("coincident")
    assert w["stats"][0] == 1 and w["stats"][1] == w["flipped"].sum() <= 100


def test_chain_is_the_longest_hooking_chain():
    nl, idx = R.cases()["chain"]
    valid, i, j, key, _ = R.edges(nl, idx)
    fwd = key[np.arange(4095) * 2 + 1] >> np.uint64(32)                      # slot (i, i + 1)
    assert np.all(np.diff(fwd.astype(np.int64)) > 0)                         # weights grow strictly along the line
    chains = R.boruvka(nl, idx)[1]
    assert max(chains) >= 64 and chains[0] == 4095
    w = R.want("chain")
    assert w["stats"][0] == 1 and np.all(w["tree"] == 0)
    d = np.einsum("ij,ij->i", w["nl"][:-1].astype(np.float64), w["nl"][1:].astype(np.float64))
    assert np.all(d > 0)                                                     # consecutive normals agree after orientation
    assert w["flipped"].sum() <= 2048                                        # the majority kept its sign


def test_islands_are_three_trees_with_their_own_majorities():
    nl, _ = R.cases()["islands"]
    w = R.want("islands")
    a, b, _ = R.ISLAND_SIZES
    assert w["stats"][0] == 3 and np.unique(w["tree"]).tolist() == [0, a, a + b]
    assert np.all(w["nl"][:a, 2] == 1.0) and w["flipped"][:a].sum() == 16     # 24 against 16
    assert np.all(w["nl"][a:a + b, 2] == 1.0) and w["flipped"][a:a + b].sum() == 20   # 21 against 20
    assert w["flipped"][a + b:].sum() <= 150


def test_sphere_gets_one_side():
    nl, idx, xyz = R.sphere_outside()
    inward = np.einsum("ij,ij->i", nl, xyz) < 0
    assert 0.3 < inward.mean() < 0.7
    w = R.want("sphere_outside")
    side = np.sign(np.einsum("ij,ij->i", w["nl"], xyz))
    assert w["stats"][0] == 1 and np.all(side == side[0]) and side[0] != 0


def test_sheet_at_the_mean_has_noise_for_signs_before_and_one_sign_after():
    nl, _ = R.cases()["sheet_at_mean"]
    sheet = slice(0, R.SHEET_POINTS)
    up = (nl[sheet, 2] > 0).mean()
    assert 0.1 <= up <= 0.9 and np.all(np.abs(nl[sheet, 2]) > 0.9)
    w = R.want("sheet_at_mean")
    assert np.unique(np.sign(w["nl"][sheet, 2])).size == 1 and np.unique(w["tree"][sheet]).size == 1


# ------------------------------------------------------------------------------------------------ host argument checks
def _pointer(addr, typ):
    return ctypes.cast(ctypes.c_void_p(addr), typ) if addr else None


def test_orient_normals_checks_its_arguments_before_the_library(monkeypatch):
    def no_library():
        raise AssertionError("the library was reached")
    monkeypatch.setattr(N, "lib", no_library)
    nl, idx = torch.zeros(4, 3), torch.zeros(4, 2, dtype=torch.int32)
    with pytest.raises(TypeError):
        mesh.orient_normals(nl.numpy(), idx)
    with pytest.raises(TypeError):
        mesh.orient_normals(nl.double(), idx)
    with pytest.raises(TypeError):
        mesh.orient_normals(torch.zeros(4, 4), idx)
    with pytest.raises(TypeError):
        mesh.orient_normals(nl, idx.long())
    with pytest.raises(TypeError):
        mesh.orient_normals(nl, torch.zeros(5, 2, dtype=torch.int32))
    with pytest.raises(TypeError):
        mesh.orient_normals(nl, torch.zeros(8, dtype=torch.int32))
    with pytest.raises(ValueError):
        mesh.orient_normals(nl, torch.zeros(4, 0, dtype=torch.int32))
    with pytest.raises(ValueError):
        mesh.orient_normals(nl, torch.zeros(4, 33, dtype=torch.int32))
    with pytest.raises(RuntimeError):                                        # valid, but on the host: there is no CPU path
        mesh.orient_normals(nl, idx)
    with pytest.raises(ValueError):
        mesh.decode_points((np.zeros((4, 3), np.float32), np.zeros((4, 3), np.float32)), orient="viewpoint")


def test_library_checks_sizes_on_the_host():
    """The pointers below are never dereferenced."""
    lib = N.lib()
    vp, fake = N.c_vp, 1 << 20
    assert lib.pbn_cloud_orient_workspace_bytes(-1, 16) == 0
    assert lib.pbn_cloud_orient_workspace_bytes(100, 0) == 0 and lib.pbn_cloud_orient_workspace_bytes(100, 33) == 0
    assert lib.pbn_cloud_orient_workspace_bytes(1 << 27, 16) == 0            # n * k = 2^31
    assert lib.pbn_cloud_orient_workspace_bytes((1 << 27) - 1, 16) > 0
    small, big = lib.pbn_cloud_orient_workspace_bytes(100, 16), lib.pbn_cloud_orient_workspace_bytes(200000, 16)
    assert 0 < lib.pbn_cloud_orient_workspace_bytes(0, 1) <= small < big

    def call(n, k, ws_bytes=big, stats=fake):
        f32, i32 = _pointer(fake, N.c_f32p), _pointer(fake, N.c_i32p)
        return lib.pbn_cloud_orient(f32, n, i32, k, f32, vp(fake), i32, _pointer(stats, N.c_i32p), i32, vp(fake), ws_bytes, None)
    assert call(-1, 16) == N.PBN_ERR_ARG
    assert call(100, 0) == N.PBN_ERR_ARG and call(100, 33) == N.PBN_ERR_ARG
    assert call(1 << 27, 16) == N.PBN_ERR_ARG
    assert call(100, 16, stats=0) == N.PBN_ERR_ARG
    assert call(200000, 16, ws_bytes=small) == N.PBN_ERR_WORKSPACE


def test_bookkeeping_keys_are_never_scene_files():
    assert "flipped" in mesh.SCENE_BOOKKEEPING and "tree" in mesh.SCENE_BOOKKEEPING
