"""Seeded, designed inputs for the coordinate pyramid (csrc/pyramid.hip behind pbn_coords_prepare / _dev, the hash-table pipeline
behind pbn_coords_prepare_hash, pbn_coords_build), shared by tests/test_pyramid_cases_cpu.py (every precondition holds, the mutants
of tests/pyramid_mutants.py die) and tests/test_pyramid_cases_gpu.py (HIP == tests/pyramid_ref.reference, element for element).

A case is a dict: name, family, coords int32[n,4] (batch, x, y, z), n_valid (None, or the device-side row count of the capacity
form: rows beyond it are garbage), x_fastest, want_k5, design (what the builder intended) and precondition (a function of the case
that raises AssertionError when the input no longer exercises what it was built for).  Rows are clustered: blobs of about 50 %
occupancy, some pinned to the box corners so that the extent (and with it the digit plan of the sort) is designed.

The tile constants of pyramid.hip and sort.hip the designs depend on are restated here; a precondition evaluated under other constants fails."""
import functools

import numpy as np

import pyramid_ref as PR

TILES = dict(sort=2048, pyr=1024, wave=64, round=256)        # SORT_TILE, PYR_TILE, wave width, rows of one striped round
LOOKBACK = {8: 32, 9: 32, 10: 16, 11: 8}                       # digit bits -> predecessors per look-back batch (LB)
TINY = 16                 # below this many unique rows no input can have siblings on four levels: structure checks do not apply


def _rng(name):
    return np.random.default_rng(int.from_bytes(name.encode(), "little") % (1 << 63))


def blob(rng, lo, size, count=None, occ=0.5):
    """`count` (default occ * volume) distinct lattice points of the box lo .. lo + size - 1, as int64 [count, 3]."""
    size = np.broadcast_to(np.asarray(size, np.int64), (3,))
    vol = int(size.prod())
    count = int(vol * occ) if count is None else int(count)
    assert count <= vol
    j = np.sort(rng.choice(vol, count, replace=False))
    return np.stack([j % size[0], (j // size[0]) % size[1], j // (size[0] * size[1])], 1) + np.asarray(lo, np.int64)


def rows(b, xyz):
    return np.concatenate([np.full((len(xyz), 1), b, np.int64), np.asarray(xyz, np.int64).reshape(-1, 3)], 1)


def curve_point(j):
    """Cell j of the Z-order curve through the non-negative octant: bit 3i of j is bit i of x, 3i + 1 of y, 3i + 2 of z."""
    j = np.asarray(j, np.int64)
    out = np.zeros(j.shape + (3,), np.int64)
    for i in range(16):
        for a in range(3):
            out[..., a] |= ((j >> (3 * i + a)) & 1) << i
    return out


def _case(name, family, coords, n_valid=None, x_fastest=1, want_k5=1, design=None, precondition=None, shuffle=True):
    coords = np.asarray(coords, np.int64).reshape(-1, 4)
    if shuffle and n_valid is None:
        coords = coords[_rng(name + "/order").permutation(len(coords))]
    return dict(name=name, family=family, coords=np.ascontiguousarray(coords, np.int32), n_valid=n_valid, x_fastest=x_fastest,
                want_k5=want_k5, design=design or {}, precondition=precondition)


@functools.lru_cache(maxsize=None)
def reference(name):
    c = case(name)
    return PR.reference(c["coords"], c["n_valid"], c["x_fastest"], c["want_k5"])


def ref_of(c):
    """Reference of a case dict (cached for the registered ones; a modified copy is recomputed)."""
    if c["name"] in NAMES and case(c["name"]) is c:
        return reference(c["name"])
    return PR.reference(c["coords"], c["n_valid"], c["x_fastest"], c["want_k5"])


# ---- what every precondition includes --------------------------------------------------------------------------------------------
def structure(c, ref=None, sibling_levels=(1, 2, 3, 4)):
    """A quarter of the level-0 rows have a face neighbour, every coarser level has a voxel with two children, every level's k = 3
    map has an absent entry.  Not applicable below TINY unique rows (nothing can hold there)."""
    ref = ref or ref_of(c)
    if int(ref["n_unique"][0]) < TINY:
        return
    k3 = ref["k3_0"]
    assert ((k3[:, [4, 10, 12, 14, 16, 22]] >= 0).any(1)).mean() >= 0.25, "face neighbours"        # centre 13 +- 1, 3, 9
    for l in sibling_levels:
        assert ((ref["nbr_down%d" % (l - 1)] >= 0).sum(1) >= 2).any(), "siblings below level %d" % l
    for l in range(5):
        assert (ref["k3_%d" % l] == -1).any(), "absent neighbour at level %d" % l


def _pre_plan(c, tiles=TILES):
    ref, d = ref_of(c), c["design"]
    assert ref["nbits"] == d["nbits"] and ref["plan"] == d["plan"], (ref["nbits"], ref["plan"])
    n1 = int(ref["n_unique"][0])
    assert -(-n1 // tiles["sort"]) > d.get("sort_tiles_over", 0), "sort tiles"
    assert -(-n1 // tiles["pyr"]) > d.get("pyr_tiles_over", 0), "pyramid tiles"
    structure(c, ref, d.get("sibling_levels", (1, 2, 3, 4)))


def _pre_structure(c, tiles=TILES):
    structure(c)


# ---- D: one case per digit plan ----------------------------------------------------------------------------------------------------
def _two_corner_scene(name, e, batches, n_rows):
    """Exactly n_rows unique rows in blobs of about half occupancy inside a box of extent 2^e - 1 from the curve origin (-48 on
    every axis, so the box straddles 0): one blob pinned near the origin corner (box minimum origin + 5: not a multiple of 16), one
    to the far corner, the rest anywhere inside; blob i lies in batches[i % len(batches)]."""
    rng = _rng(name)
    x0, far = -48, (1 << e) - 1
    need = int(n_rows * 1.06) + 8
    side = min(32, far + 1)
    while side > 8 and side < far + 1 and need / (side ** 3 // 2) < 3:
        side //= 2
    n_blobs = max(2, -(-need // (side ** 3 // 2)))
    per = -(-need // n_blobs)
    assert n_blobs >= len(batches) and (side <= far - 5 or n_blobs <= len(batches))
    pinned = []
    parts = []
    for i in range(n_blobs):
        if side == far + 1:
            lo = np.zeros(3, np.int64)
        elif i == 0:
            lo = np.full(3, 5)
        elif i == 1:
            lo = np.full(3, far - side + 1)
        else:
            lo = rng.integers(0, far - side + 2, 3)
        parts.append(rows(batches[i % len(batches)], blob(rng, lo + x0, side, count=per)))
        if i < 2:
            pinned.append(rows(batches[i], [lo + x0 + (0 if i == 0 else side - 1)]))
    pinned = np.concatenate(pinned)
    body = np.unique(np.concatenate(parts), axis=0)
    body = body[~((body[:, None, :] == pinned[None]).all(2).any(1))]
    assert len(body) + len(pinned) >= n_rows, (name, len(body))
    body = body[np.sort(rng.choice(len(body), n_rows - len(pinned), replace=False))]
    return np.concatenate([pinned, body])


def _plan_case(name, e, batches, nbits, plan, n_rows, **design):
    design.update(nbits=nbits, plan=plan)
    return _case(name, "D", _two_corner_scene(name, e, batches, n_rows), design=design, precondition=_pre_plan)


def _family_d():
    out = []
    # (1, 8): 3 * 2 + 2 = 8 bits, at most 256 keys; a box of 4 cells per axis lies inside one level-2 voxel, so siblings exist on
    # levels 1 and 2 only
    rng = _rng("D_1x8")
    out.append(_case("D_1x8", "D", np.concatenate([rows(b, blob(rng, (16, -16, 32), 4, count=40)) for b in (2, 3, 4, 5)]),
                     design=dict(nbits=8, plan=(1, 8), sort_tiles_over=0, sibling_levels=(1, 2)), precondition=_pre_plan))
    out.append(_plan_case("D_2x8", 4, (0, 3, 9, 15, 6, 12), 16, (2, 8), 10000, sort_tiles_over=1))
    out.append(_plan_case("D_3x8", 6, (1, 16, 5), 22, (3, 8), 9000, sort_tiles_over=1))
    out.append(_plan_case("D_3x9_68k", 8, (0, 3, 1, 2), 26, (3, 9), 68000, sort_tiles_over=32, pyr_tiles_over=65))
    out.append(_plan_case("D_3x10", 9, (4, 7), 29, (3, 10), 34000, sort_tiles_over=16))
    out.append(_plan_case("D_3x11", 10, (0, 2), 32, (3, 11), 17500, sort_tiles_over=8))
    out.append(_plan_case("D_4x9", 11, (10, 13), 35, (4, 9), 5000, sort_tiles_over=1))
    out.append(_plan_case("D_4x10", 12, (0, 3), 38, (4, 10), 34000, sort_tiles_over=16))
    out.append(_plan_case("D_4x11", 13, (0, 7, 4), 42, (4, 11), 17500, sort_tiles_over=8))
    out.append(_plan_case("D_44_bits", 14, (20, 23), 44, (4, 11), 5000, sort_tiles_over=1))
    out.append(_plan_case("D_45_bits", 14, (20, 27, 24), 45, None, 5000, sort_tiles_over=1))
    return out


# ---- S: seams of the level pass ------------------------------------------------------------------------------------------------------
S_SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 4097)
_S_START = 512 - 20         # the walk starts 20 cells before the end of level-3 voxel 0: level 4 has two children from the start


@functools.lru_cache(maxsize=None)
def _seam_walk(tiles=tuple(sorted(TILES.items()))):
    """Curve cells of 4097 rows, in curve order: every second cell on average, except that around sorted rows 64, 256 and 1024
    (wave, striped round, workgroup of the level pass) a whole level-1 voxel is taken so that rows s - 1 and s are siblings."""
    t = dict(tiles)
    seams = sorted((t["wave"], t["round"], t["pyr"]))
    rng = _rng("S_walk")
    cells, j = [], _S_START
    while len(cells) < max(S_SIZES):
        s = next((s for s in seams if s - 6 <= len(cells) <= s - 1), None)
        if s is not None:
            j = -(-j // 8) * 8
            cells.extend(range(j, j + 8))
            j += 8
        else:
            if rng.random() < 0.5:
                cells.append(j)
            j += 1
    return np.array(cells[:max(S_SIZES)], np.int64)


def _pre_seams(c, tiles=TILES):
    ref = ref_of(c)
    n1 = int(ref["n_unique"][0])
    assert n1 == c["design"]["n"]
    anc = [np.arange(n1)]
    for l in range(4):
        anc.append(ref["parent_row%d" % l][anc[-1]])
    for s in (tiles["wave"], tiles["round"], tiles["pyr"]):
        if s < n1:
            if c["design"]["kind"] == "siblings":       # rows s - 1 and s share every ancestor: a level-1 voxel taken whole
                assert all(anc[l][s - 1] == anc[l][s] for l in (1, 2, 3, 4)), "seam %d" % s
                assert s + 1 >= n1 or (ref["nbr_down0"][anc[1][s]] >= 0).all(), "seam %d: the designed voxel" % s
            else:                                        # ... or none
                assert all(anc[l][s - 1] != anc[l][s] for l in (1, 2, 3, 4)), "seam %d" % s
    structure(c, ref)


def _family_s():
    out = []
    base = np.array([-16, 32, -32])                       # multiples of 16: the curve through the box is the curve of curve_point
    cells = _seam_walk()
    for n in S_SIZES:
        out.append(_case("S_n%d" % n, "S", rows(3, curve_point(cells[:n]) + base), design=dict(n=n, kind="siblings"),
                         precondition=_pre_seams))
    rng = _rng("S_level4_seams")
    per_voxel = (64, 192, 768, 2048, 1025)                # level-4 voxels 0..4 end at sorted rows 64, 256, 1024, 3072
    cells = np.concatenate([4096 * v + np.sort(rng.choice(min(4096, 2 * m), m, replace=False)) for v, m in enumerate(per_voxel)])
    out.append(_case("S_level4_seams", "S", rows(3, curve_point(cells) + base), design=dict(n=4097, kind="level4"),
                     precondition=_pre_seams))
    return out


# ---- B: batch seams --------------------------------------------------------------------------------------------------------------------
def _pre_batch(c, tiles=TILES):
    ref = ref_of(c)
    c0 = ref["coords0"]
    seam = np.nonzero(c0[1:, 0] != c0[:-1, 0])[0] + 1
    same = [s for s in seam if (c0[s, 1:] == c0[s - 1, 1:]).all()]
    assert len(same) >= 2, "adjacent sorted rows of two batches on the same voxel"
    batches = sorted(set(c0[:, 0].tolist()))
    assert batches[0] > 0 and np.any(np.diff(batches) > 1)
    # a neighbour that exists, but only in another batch
    offs = PR.kernel_offsets(3, c["x_fastest"])
    spatial = {tuple(r) for r in c0[:, 1:].tolist()}
    miss = np.argwhere(ref["k3_0"] == -1)[:20000]
    assert any(tuple((c0[r, 1:] + offs[k]).tolist()) in spatial for r, k in miss), "target only in another batch"
    structure(c, ref)


def _family_b():
    rng = _rng("B_seams")
    v, w = np.array([[8, 8, 8]]), np.array([[15, 15, 15]])
    lowc = blob(rng, (0, 0, 0), 8)
    parts = [rows(3, lowc), rows(3, v),                                  # batch 3 ends with the voxel batch 7 starts with
             rows(7, v), rows(7, blob(rng, (8, 8, 8), 8)), rows(7, w),    # ... and batch 7 ends with the one batch 8 starts with
             rows(8, w), rows(8, blob(rng, (16, 16, 16), 16)),
             rows(20, blob(rng, (0, 0, 0), 8)), rows(20, blob(rng, (20, 4, 9), 10))]
    # shifted by multiples of 16 only: the curve through the box stays the one the blocks were laid out on
    return [_case("B_seams", "B", np.concatenate(parts) + np.array([0, -16, 16, 0]), precondition=_pre_batch)]


# ---- N: negative and edge coordinates ----------------------------------------------------------------------------------------------------
def _pre_n(c, tiles=TILES):
    ref, d = ref_of(c), c["design"]
    uc = ref["ucoords"].astype(np.int64)
    if "straddle" in d:
        assert (uc[:, 1:].min(0) < 0).all() and (uc[:, 1:].max(0) > 0).all()
    if "minimum" in d:
        assert uc[:, 1:].min(0).tolist() == list(d["minimum"]) and ref["origin"].tolist() == list(d["origin"])
    if "corner" in d:
        assert (uc[:, 1:] == d["corner"]).all(1).any()
        for l in range(5):                       # the neighbours beyond the range are absent at every level
            cl, offs = ref["coords%d" % l].astype(np.int64), PR.kernel_offsets(3, c["x_fastest"]) << l
            t = cl[:, None, 1:] + offs[None]
            outside = ((t < PR.LO) | (t > PR.HI)).any(2)
            assert outside.any() and (ref["k3_%d" % l][outside] == -1).all()
    if "sortable" in d:
        assert (ref["plan"] is not None) == d["sortable"]
    if "wrap" in d:
        e, org = ref["e"], ref["origin"]
        assert int((uc[:, 1:].max(0) - org).max()) == (1 << e) - 1
        far = uc[uc[:, 1] - org[0] == (1 << e) - 1]
        keys = {tuple(r) for r in uc.tolist()}
        assert any((b + 1, int(org[0]), y, z) in keys for b, _, y, z in far.tolist()), "the next batch's voxel at x0"
        for l in (2, 3, 4):                      # ... and likewise on the levels whose maps are searched by key
            cl = ref["coords%d" % l].astype(np.int64)
            kl = {tuple(r) for r in cl.tolist()}
            hit = [r for r in cl.tolist() if r[1] + (1 << l) - org[0] == (1 << e) and (r[0] + 1, int(org[0]), r[2], r[3]) in kl]
            assert hit, "wrap partner at level %d" % l
    structure(c, ref)


def _family_n():
    out = []
    rng = _rng("N")
    out.append(_case("N_straddle_zero", "N", np.concatenate([rows(0, blob(rng, (-8, -8, -8), 16)), rows(1, blob(rng, (-20, -3, -9), 12)),
                                                             rows(1, blob(rng, (2, 6, -1), 9))]),
                     design=dict(straddle=True), precondition=_pre_n))
    out.append(_case("N_minimum_unaligned", "N", np.concatenate([rows(0, blob(rng, (5, 21, 37), 14, occ=0.6)), rows(0, [[5, 21, 37]]),
                                                                 rows(2, blob(rng, (9, 30, 40), 12))]),
                     design=dict(minimum=(5, 21, 37), origin=(0, 16, 32)), precondition=_pre_n))
    out.append(_case("N_minimum_minus_one", "N", np.concatenate([rows(4, blob(rng, (-1, -1, -1), 13, occ=0.6)), rows(4, [[-1, -1, -1]]),
                                                                 rows(5, blob(rng, (3, 0, 2), 12))]),
                     design=dict(minimum=(-1, -1, -1), origin=(-16, -16, -16)), precondition=_pre_n))
    lo_c, hi_c = np.full(3, PR.LO), np.full(3, PR.HI)
    low = np.concatenate([rows(0, blob(rng, lo_c, 12, occ=0.6)), rows(0, [lo_c]), rows(1, blob(rng, lo_c + (0, 3, 1), 10))])
    high = np.concatenate([rows(0, blob(rng, hi_c - 11, 12, occ=0.6)), rows(0, [hi_c]), rows(1, blob(rng, hi_c - (9, 12, 10), 10))])
    out.append(_case("N_low_corner", "N", low, design=dict(corner=tuple(lo_c), sortable=True), precondition=_pre_n))
    out.append(_case("N_high_corner", "N", high, design=dict(corner=tuple(hi_c), sortable=True), precondition=_pre_n))
    out.append(_case("N_both_corners", "N", np.concatenate([low, high]), design=dict(corner=tuple(hi_c), sortable=False),
                     precondition=_pre_n))
    box = blob(rng, (0, 0, 0), 16, occ=0.5)
    face = np.array([[x, y, z] for x in (0, 15) for y in range(0, 16, 3) for z in range(0, 16, 5)])
    wrap = np.concatenate([rows(b, np.concatenate([box[rng.random(len(box)) < 0.8], face])) for b in (5, 6, 7)])
    out.append(_case("N_box_edge_wrap", "N", wrap + np.array([0, 32, -16, 0]), design=dict(wrap=True), precondition=_pre_n))
    return out


# ---- U: duplicates ------------------------------------------------------------------------------------------------------------------------
def _pre_u(c, tiles=TILES):
    ref, d = ref_of(c), c["design"]
    n, n1 = len(c["coords"]), int(ref["n_unique"][0])
    mult = np.bincount(ref["inverse"], minlength=n1)
    if d["kind"] == "twice":
        assert (mult == 2).all()
    elif d["kind"] == "around":                 # duplicates in front of the first occurrence block and behind it
        assert n1 < n and (ref["unique_index"] < d["front"]).sum() > d["front"] // 3 and ref["unique_index"].max() < n - d["back"]
    elif d["kind"] == "identical":
        assert n1 == 1 and n > 100 and ref["e"] == 1 and ref["nbits"] == 3 and ref["unique_index"].tolist() == [0]
    elif d["kind"] == "last":
        assert ref["unique_index"][-1] == n - 1 and (mult > 1).any()
    structure(c, ref)


def _family_u():
    rng = _rng("U")
    base = np.concatenate([rows(1, blob(rng, (-6, 3, 10), 12)), rows(2, blob(rng, (0, 0, 0), 9))])
    base = base[rng.permutation(len(base))]
    front, back = base[rng.integers(0, len(base), 300)], base[rng.integers(0, len(base), 400)]
    lone = rows(2, [[9, 4, 4]])
    assert not (base == lone).all(1).any()
    return [_case("U_every_row_twice", "U", np.concatenate([base, base]), design=dict(kind="twice"), precondition=_pre_u),
            _case("U_duplicates_around", "U", np.concatenate([front, base, back]), shuffle=False,
                  design=dict(kind="around", front=300, back=400), precondition=_pre_u),
            _case("U_all_identical", "U", np.repeat(rows(9, [[-16, 128, 32]]), 500, 0), design=dict(kind="identical"), precondition=_pre_u),
            _case("U_first_in_last_position", "U", np.concatenate([base, back, lone]), shuffle=False, design=dict(kind="last"),
                  precondition=_pre_u)]


# ---- C: capacity form ---------------------------------------------------------------------------------------------------------------------
C_CAP = 1500


def _pre_c(c, tiles=TILES):
    ref = ref_of(c)
    tail = c["coords"][c["n_valid"]:].astype(np.int64)
    assert len(c["coords"]) == C_CAP and len(tail) >= 1
    if len(tail) > 1:
        assert ((tail[:, 1:] > PR.HI) | (tail[:, 1:] < PR.LO) | (tail[:, :1] < 0)).any(), "garbage outside the range"
    assert int(ref["n_unique"][0]) <= c["n_valid"]
    structure(c, ref)


def _family_c():
    rng = _rng("C")
    good = np.concatenate([rows(0, blob(rng, (3, -9, 0), 11)), rows(1, blob(rng, (0, 0, 0), 12)), rows(1, blob(rng, (8, 2, 3), 6))])
    good = np.concatenate([good, good[:300]])
    good = good[rng.permutation(len(good))][:C_CAP]
    assert len(good) == C_CAP
    out = []
    for nv in (0, 1, 1024, 1025, C_CAP - 1):
        coords = good.copy()
        junk = rng.integers(-200000, 200000, (C_CAP - nv, 4))
        junk[::3] = good[rng.integers(0, C_CAP, len(junk[::3]))]          # some garbage looks like real rows
        junk[-1] = (-1, 40000, -40000, 70000)
        coords[nv:] = junk
        out.append(_case("C_valid_%d" % nv, "C", coords, n_valid=nv, precondition=_pre_c))
    out.append(_case("C_host_n0", "C", np.zeros((0, 4)), precondition=_pre_structure))
    return out


# ---- O: options ------------------------------------------------------------------------------------------------------------------------------
def _pre_option(c, tiles=TILES):
    base = reference(c["design"]["base"])
    ref = ref_of(c)
    if c["x_fastest"] == 0:
        assert not np.array_equal(ref["k3_0"], base["k3_0"]) and np.array_equal(ref["k3_0"][:, 13], base["k3_0"][:, 13])
    if c["want_k5"] == 0:
        assert "k5" not in ref and all(np.array_equal(ref[k], base[k]) for k in PR.ARRAYS if k != "k5")
    structure(c, ref)


def _family_o(by_name):
    out = []
    for base, xf, k5 in (("B_seams", 0, 1), ("N_box_edge_wrap", 0, 1), ("D_3x8", 0, 1), ("N_minimum_minus_one", 1, 0), ("S_n1025", 1, 0)):
        b = by_name[base]
        name = "O_%s_%s" % ("z_fastest" if xf == 0 else "no_k5", base)
        out.append(dict(b, name=name, family="O", x_fastest=xf, want_k5=k5, design=dict(base=base), precondition=_pre_option))
    return out


@functools.lru_cache(maxsize=None)
def cases():
    out = _family_d() + _family_s() + _family_b() + _family_n() + _family_u() + _family_c()
    out += _family_o({c["name"]: c for c in out})
    return tuple(out)


_BY_NAME = {}


def case(name):
    if not _BY_NAME:
        _BY_NAME.update({c["name"]: c for c in cases()})
    return _BY_NAME[name]


NAMES = tuple(c["name"] for c in cases())
FAMILY_D = tuple(c["name"] for c in cases() if c["family"] == "D")
