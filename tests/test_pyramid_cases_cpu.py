"""CPU tier: the designed coordinate inputs of tests/pyramid_cases.py are valid (every precondition holds, and fails loudly under
other tile constants), the specification tests/pyramid_ref.py agrees with the CPU oracle's coordinate manager, and the set is sharp:
each deliberately wrong variant in tests/pyramid_mutants.py differs from the specification on at least one case.  The kill matrix is
printed (pytest -s shows it)."""
import functools

import numpy as np
import pytest

from oracle import sparse_ref as R
import pyramid_cases as PC
import pyramid_mutants as PM
import pyramid_ref as PR


def _same(a, b):
    return set(a) == set(b) and all(a[k].shape == b[k].shape and np.array_equal(a[k], b[k]) for k in a)


@pytest.mark.parametrize("name", PC.NAMES)
def test_precondition_holds(name):
    c = PC.case(name)
    c["precondition"](c)
    ref = PC.reference(name)
    print("\nPRE %-30s rows %6d unique %6d key bits %2d plan %s" % (name, len(c["coords"]), ref["n_unique"][0], ref["nbits"], ref["plan"]))


def test_family_d_reaches_every_plan_and_both_sides_of_the_key_limit():
    plans = {PC.reference(n)["plan"] for n in PC.FAMILY_D}
    assert plans == {(1, 8), (2, 8), (3, 8), (3, 9), (3, 10), (3, 11), (4, 9), (4, 10), (4, 11), None}
    assert PC.reference("D_44_bits")["nbits"] == 44 and PC.reference("D_45_bits")["nbits"] == 45
    for n in PC.FAMILY_D:                    # the look-back of the sort needs a second batch of predecessors where one was asked for
        ref, d = PC.reference(n), PC.case(n)["design"]
        if d.get("sort_tiles_over", 0) > 1:
            assert d["sort_tiles_over"] == PC.LOOKBACK[ref["plan"][1]] and -(-int(ref["n_unique"][0]) // PC.TILES["sort"]) > d["sort_tiles_over"]


def test_preconditions_fail_loudly_under_other_tile_constants():
    """The seam cases read as if the workgroup tile of the level pass were 512 rows, the large digit-plan cases as if a sort tile
    held 4096 keys: the designed seams and tile counts are not there."""
    for name in ("S_n1025", "S_n4097", "S_level4_seams"):
        c = PC.case(name)
        with pytest.raises(AssertionError):
            c["precondition"](c, tiles=dict(PC.TILES, pyr=512))
    for name in ("D_3x9_68k", "D_3x11", "D_4x10"):
        c = PC.case(name)
        with pytest.raises(AssertionError):
            c["precondition"](c, tiles=dict(PC.TILES, sort=4096))
    c = PC.case("D_3x9_68k")
    with pytest.raises(AssertionError):
        c["precondition"](c, tiles=dict(PC.TILES, pyr=2048))


def test_plan_definition():
    assert [PR.sort_plan(b) for b in (1, 8, 9, 16, 17, 24, 25, 27, 28, 30, 31, 33, 34, 36, 37, 40, 41, 44, 45)] == \
        [(1, 8), (1, 8), (2, 8), (2, 8), (3, 8), (3, 8), (3, 9), (3, 9), (3, 10), (3, 10), (3, 11), (3, 11), (4, 9), (4, 9), (4, 10),
         (4, 10), (4, 11), (4, 11), None]
    for b in range(1, 45):
        p, d = PR.sort_plan(b)
        assert p * d >= b and 8 <= d <= 11 and p <= 4


@pytest.mark.parametrize("name", ["B_seams", "N_straddle_zero", "U_duplicates_around"])
def test_reference_agrees_with_the_oracle_coordinate_manager(name):
    c = PC.case(name)
    ref = PC.reference(name)
    first, inverse = R.unique_first(c["coords"])
    assert np.array_equal(ref["unique_index"], first) and np.array_equal(ref["inverse"], inverse)
    cm = R.CoordinateManager(ref["ucoords"])
    rows_of = lambda l: [tuple(r) for r in ref["coords%d" % l].tolist()]
    for l, s in enumerate((1, 2, 4, 8, 16)):
        want = cm.get_coords(s)
        assert len(want) == len(rows_of(l)) and set(map(tuple, want.tolist())) == set(rows_of(l)), "level %d" % l

    def pairs(maps, in_coords, out_coords):
        return {(k, tuple(in_coords[i]), tuple(out_coords[o])) for k, (ins, outs) in enumerate(maps) for i, o in zip(ins.tolist(), outs.tolist())}

    for l, s in enumerate((1, 2, 4, 8, 16)):
        for ksize, key in ((3, "k3_%d" % l),) + (((5, "k5"),) if l == 0 else ()):
            nbr, cl = ref[key], rows_of(l)
            got = {(k, cl[nbr[r, k]], cl[r]) for r, k in np.argwhere(nbr >= 0).tolist()}
            oc = cm.get_coords(s).tolist()
            assert got == pairs(cm.get_map(s, s, ksize), oc, oc), key
    for l, s in enumerate((1, 2, 4, 8)):                     # 2x2x2 stride-2 maps: offset k = child_k (C1, C2: offsets 0..1, x fastest)
        fine, coarse = rows_of(l), rows_of(l + 1)
        nd, par, ck, up = ref["nbr_down%d" % l], ref["parent_row%d" % l], ref["child_k%d" % l], ref["up%d" % l]
        got = {(k, fine[nd[r, k]], coarse[r]) for r, k in np.argwhere(nd >= 0).tolist()}
        assert got == pairs(cm.get_map(s, 2 * s, 2), cm.get_coords(s).tolist(), cm.get_coords(2 * s).tolist()), "down %d" % l
        assert got == {(int(ck[r]), fine[r], coarse[par[r]]) for r in range(len(fine))}
        assert ((up >= 0).sum(1) == 1).all() and np.array_equal(up[np.arange(len(fine)), ck], par)


def _restated(name, mutant=None):
    c = PC.case(name)
    return PM.reference(c["coords"], c["n_valid"], c["x_fastest"], c["want_k5"], mutant=mutant)


@pytest.mark.parametrize("name", PC.NAMES)
def test_mutant_harness_restates_the_specification(name):
    assert _same(_restated(name), PR.contract(PC.reference(name)))


MUTANT_CASES = tuple(n for n in PC.NAMES if len(PC.case(n)["coords"]) <= 10000)        # the large cases add time, not kills


@functools.lru_cache(maxsize=None)
def _kills(mutant):
    return tuple(n for n in MUTANT_CASES if not _same(_restated(n, mutant), PR.contract(PC.reference(n))))


@pytest.mark.parametrize("mutant", PM.MUTANTS)
def test_mutant_is_killed(mutant):
    killed_by = _kills(mutant)
    print("\nKILL %-22s %2d/%d cases: %s" % (mutant, len(killed_by), len(MUTANT_CASES), " ".join(killed_by)))
    assert killed_by, "mutant %s survives the whole case set: the set is too weak" % mutant


def test_designed_kills():
    """The mistakes a family was built for die on that family."""
    assert "B_seams" in _kills("flag_ignores_batch") and "B_seams" in _kills("lookup_ignores_batch")
    assert "N_box_edge_wrap" in _kills("no_box_limit")
    assert {"U_every_row_twice", "U_duplicates_around"} <= set(_kills("last_occurrence"))
    assert "N_minimum_unaligned" in _kills("raw_origin") and "N_straddle_zero" in _kills("trunc_div")
    assert "D_1x8" in _kills("level_key_drops_batch")          # a box narrower than a level-3 voxel, several batches
    for name in ("D_3x8", "D_4x9"):                            # key bits that are no multiple of the digit width
        assert name in _kills("plan_drops_top_digit")
