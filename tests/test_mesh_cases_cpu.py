"""CPU tier: the designed mesh inputs of tests/mesh_cases.py are valid (every precondition holds), the kernel-shaped statement
tests/mesh_mutants.py equals tests/mesh_ref.py on every case (nl bits, segmentator normals, weights, sweep order, roots, sup), and the
set is sharp: each deliberate mistake of mesh_mutants.MUTANTS differs from the reference on at least one small case, and on the case
that was built for it.  The kill matrix is printed (pytest -s shows it).

Three mistakes the case set was asked to kill cannot be killed by any input (mesh_mutants.EQUIVALENT: nl once per occurrence, the
lerp's count per occurrence, the lerp's t from the list position).  They differ from the kernel only on a face that names a vertex
twice, and such a face adds exactly zero to nl and NaN to the lerp.  test_equivalent_mistakes_change_nothing asserts both halves:
the premise on adversarial coordinates, and that the three agree with the reference on every case."""
import functools
import os

import numpy as np
import pytest

import mesh_cases as MC
import mesh_mutants as MM
import mesh_ref as MR
from pbnet_amd import _native as N
from pbnet_amd import selftest as S

HERE = os.path.dirname(os.path.abspath(__file__))


def test_constants_are_the_kernels():
    """The sizes the O and L cases are built from are the library's: the sort tile is asked of it, the scan tile and the grid cap
    are read from the sources the library is built from."""
    assert MC.sort_tile() == N.lib().pbn_selftest_sort_tile() > 0
    assert MC.SCAN_TILE == S.SCAN_TILE and (MC.MESH_GRID, MC.TPB) == (4096, 256)
    assert MC.STRIDE == 4096 * 256 == 1048576 and MC.WEIGHT_STRIDE == 1024 * 256 == 262144
    t = MC.sort_tile()
    assert [len(MC.case("O_sort_" + k)["edges"]) for k in ("Tm1", "T", "Tp1", "2T")] == [t - 1, t, t + 1, 2 * t]
    t = MC.SCAN_TILE
    assert [len(MC.case("L_scan_" + k)["xyz"]) for k in ("Tm1", "T", "Tp1", "2T")] == [t - 1, t, t + 1, 2 * t]
    assert [len(MC.case("L_strip_scan_" + k)["xyz"]) for k in ("Tm1", "T", "Tp1", "2T")] == [t - 1, t, t + 1, 2 * t]


@pytest.mark.parametrize("name", MC.NAMES)
def test_precondition_holds(name):
    c = MC.case(name)
    c["precondition"](c)
    n = len(c["faces"]) if c["mode"] == "mesh" else len(c["edges"])
    print("\nPRE %-22s %-5s V %7d %s %7d  %s" % (name, c["mode"], len(c["xyz"]), "F" if c["mode"] == "mesh" else "E", n, c["design"]))
    if not c["large"]:
        assert len(c["xyz"]) <= 5000


def test_large_cases_take_the_second_trip():
    """The arithmetic of the module docstring, on the arrays."""
    assert 3 * len(MC.case("L_grid420")["faces"]) == 1053366 > MC.STRIDE
    assert len(MC.case("L_v1048600")["xyz"]) == len(MC.case("L_point_v1048600")["xyz"]) == 1048600 > MC.STRIDE
    assert len(MC.case("L_point_e262445")["edges"]) == 262445 > MC.WEIGHT_STRIDE
    for name in MC.LARGE:
        assert MC.case(name)["large"] and MC.case(name)["only"] == MC.ONLY[name]


@pytest.mark.parametrize("name", MC.SMALL)
def test_mutant_harness_restates_the_reference(name):
    c = MC.case(name)
    assert MM.same(MM.decode(c), MM.reference(c))


MUTANT_CASES = tuple(n for n in MC.SMALL if len(MC.case(n)["xyz"]) <= 800)        # the larger cases add time, not kills


@functools.lru_cache(maxsize=None)
def _kills(mutant):
    return tuple(n for n in MUTANT_CASES if not MM.same(MM.decode(MC.case(n), mutant), MM.reference(MC.case(n))))


@pytest.mark.parametrize("mutant", MM.MUTANTS)
def test_mutant_is_killed(mutant):
    killed_by = _kills(mutant)
    print("\nKILL %-28s %2d/%d cases: %s" % (mutant, len(killed_by), len(MUTANT_CASES), " ".join(killed_by)))
    assert killed_by, "mutant %s survives the whole case set: the set is too weak" % mutant


def _sup_differs(mutant, name):
    c = MC.case(name)
    return not np.array_equal(MM.decode(c, mutant)["sup"], MC.reference(name)["sup"])


def test_designed_kills():
    """Each mistake dies on the case that was built for it; where the mistake lies behind the normals, by sup alone (what the GPU
    tier can see)."""
    designed = {
        "incidence_reversed": ("N_fan_65", "N_fan_300"),
        "third_edge_i2_i3": ("W_planar_negative", "N_fan_65"),
        "dot2_from_n1": ("W_both_directions",),
        "dot2_ge": ("W_dot2_zero_apart", "W_dot2_zero_joins"),
        "nan_dot2_squared": ("W_coincident",),
        "negative_keys_unflipped": ("O_negative",),
        "nan_first": ("O_negative",),
        "ties_desc": ("O_ties",),
        "sort_drops_top_digit": ("O_digit_top",),
        "strict_threshold": ("S_equal_thresholds",),
        "threshold_f64": ("S_threshold_f32",),
        "threshold_size_before_join": ("S_size_after_join",),
        "min_size_le": ("S_min_4", "S_min_1"),
        "second_pass_input_order": ("S_two_neighbours",),
        "rank_tie_other_side": ("S_rank_tie_a", "S_rank_tie_b"),
        "relabel_by_first_appearance": ("S_rank_tie_a",),
    }
    assert set(designed) == set(MM.MUTANTS)
    for mutant, names in designed.items():
        for name in names:
            assert name in _kills(mutant), (mutant, name)
    by_sup = {m: n for m, n in designed.items() if m not in ("incidence_reversed", "third_edge_i2_i3")}
    for mutant, names in by_sup.items():
        for name in names:
            assert _sup_differs(mutant, name), (mutant, name)
    assert not np.array_equal(MM.decode(MC.case("N_fan_65"), "incidence_reversed")["nl"].view(np.uint32),
                              MC.reference("N_fan_65")["nl"].view(np.uint32))
    assert "S_min_0" not in _kills("min_size_le")             # size <= 0 holds for no segment either


def test_what_the_recorded_fixtures_missed():
    """Seven mistakes changed sup on none of the four recorded fixtures.  Six are reachable and die here on cases the fixtures did
    not have: a join at w == threshold, the float32 threshold, the small-segment bound, dot2 == 0, a NaN dot2 between unequal
    normals, and a negative weight.  (The seventh, -0 against +0, is not reachable.)"""
    for mutant, name in (("strict_threshold", "S_equal_thresholds"), ("threshold_f64", "S_threshold_f32"), ("min_size_le", "S_min_4"),
                         ("dot2_ge", "W_dot2_zero_apart"), ("nan_dot2_squared", "W_coincident"),
                         ("negative_keys_unflipped", "O_negative")):
        assert _sup_differs(mutant, name), (mutant, name)
    assert "W_planar_negative" in _kills("negative_keys_unflipped")          # mesh mode: the sweep order changes
    for path in ("mesh_flat", "mesh_oddities", "mesh_room"):
        g = np.load(os.path.join(HERE, "golden", path + ".npz"))
        w = MR.edge_weights(g["xyz"], MR.segmentator_normals(g["xyz"], g["faces"]), *MR.mesh_edges(g["faces"]))
        assert not (w < 0).any()                               # the fixtures hold no negative weight; W_planar_negative does
    g = np.load(os.path.join(HERE, "golden", "mesh_point.npz"))
    e = g["edges"]
    assert not (MR.edge_weights(g["points"], g["normals"], e[:, 0], e[:, 1]) < 0).any()


def test_equivalent_mistakes_change_nothing():
    rng = np.random.default_rng(5)
    for scale in (1.0, 1e-20, 1e19, 3e38):                     # ordinary, underflowing, overflowing products, overflowing differences
        with np.errstate(over="ignore"):
            xyz = (rng.normal(size=(40, 3)) * scale).astype(np.float32)
        a, b = rng.integers(0, 40, 200), rng.integers(0, 40, 200)
        faces = np.concatenate([np.stack([a, a, b], 1), np.stack([a, b, a], 1), np.stack([b, a, a], 1), np.stack([a, a, a], 1)])
        nfa, snf = MM._face_normals(xyz, faces)
        assert np.all((nfa == 0) | np.isnan(nfa))              # adds nothing, or poisons the sum either way
        assert np.isnan(snf).all()                             # 0 / 0: the running lerp is NaN whatever t and count are
    for name in MC.SMALL:
        c = MC.case(name)
        if c["mode"] == "mesh":
            ref = MM.reference(c)
            for mutant in MM.EQUIVALENT:
                assert MM.same(MM.decode(c, mutant), ref), (mutant, name)


def test_cases_of_the_designed_fixture():
    """tests/golden/mesh_designed.npz (the compiled segmentator's own sup) holds exactly the S and W cases whose result does not
    depend on the order of tied weights, with the arrays of this file."""
    g = np.load(os.path.join(HERE, "golden", "mesh_designed.npz"))
    want = [n for n in MC.SMALL if n[0] in "SW" and MC.tie_free(n)]
    assert list(g["names"]) == want and len(want) >= 12
    for name in want:
        c = MC.case(name)
        for k in ("xyz", "faces") if c["mode"] == "mesh" else ("xyz", "normals", "edges"):
            a = g["%s.%s" % (name, k)]
            assert a.dtype == c[k].dtype and np.array_equal(a.view(np.uint8), c[k].view(np.uint8)), (name, k)
        assert float(g[name + ".k_thresh"]) == float(np.float32(c["k_thresh"])) and int(g[name + ".seg_min_verts"]) == c["seg_min_verts"]
