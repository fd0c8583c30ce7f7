"""CPU tier: the designed inputs of tests/select_cases.py are valid (every precondition holds), the kernel-shaped statement
tests/select_mutants.py equals tests/select_ref.py on every case (all four outputs bit for bit, and the sentinel wherever nothing is
written), and the set is sharp: each deliberate mistake of select_mutants.MUTANTS differs from the reference on at least one case, and
on the case that was built for it.  The kill matrix is printed (pytest -s shows it).

One mistake the case set was asked to kill cannot be killed by any legal input (select_mutants.EQUIVALENT: a tail lane counted).
test_equivalent_mistake_changes_nothing asserts both halves: the premise -- the kernel walks the points in index order, so a tail lane
is in front of nobody -- and that the mistake agrees with the reference on every case."""
import functools
import os
import re

import numpy as np
import pytest

import select_cases as SC
import select_mutants as SM
import select_ref as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_constants_are_the_kernels():
    src = open(os.path.join(ROOT, "pbnet_amd", "csrc", "front.hip")).read()
    common = open(os.path.join(ROOT, "pbnet_amd", "csrc", "pbn_common.h")).read()
    assert int(re.search(r"constexpr int SEL_BLOCK = (\d+);", src).group(1)) == SC.BLOCK == SM.BLOCK == 1024
    assert int(re.search(r"constexpr int SEL_MAX_CLASSES = (\d+);", common).group(1)) == 32 == max(SC.case(n)["n_cls"] for n in SC.NAMES)
    assert "const int wbase = blockIdx.x * SEL_BLOCK + wave * (SEL_BLOCK / 4);" in src and "const int i = wbase + k * 64 + lane;" in src
    assert (SC.WAVE, SC.ROUND) == (SM.BLOCK // SM.WAVES, SM.LANES) == (256, 64) and SM.ROUNDS * SM.LANES == SC.WAVE
    assert tuple(len(SC.case("N_n%d" % n)["sem_pred"]) for n in SC.N_VALUES) == (1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049, 3073)
    assert {SC.case(n)["n_cls"] for n in SC.NAMES} >= {1, 2, 20, 32}
    assert {(SC.case(n)["dtype"], SC.case(n)["ld_off"]) for n in SC.NAMES} == {(d, l) for d in SC.DTYPES for l in (3, 8)}


@pytest.mark.parametrize("name", SC.NAMES)
def test_precondition_holds(name):
    c = SC.case(name)
    c["precondition"](c)
    lab = c["sem_pred"]
    assert (lab < c["n_cls"]).all(), "labels >= n_cls are outside the contract and are not fed to the kernel"
    assert np.array_equal(SC._as(c["offset"], c["dtype"]), c["offset"]) and len(lab) <= 5 * SC.BLOCK + 1
    print("\nPRE %-20s n %5d classes %2d %s ld %d  %s" % (name, len(lab), c["n_cls"], c["dtype"], c["ld_off"], c["design"]))


@pytest.mark.parametrize("name", SC.NAMES)
def test_reference_is_a_stable_argsort(name):
    """The anchor: a stable sort by the rank of the class's range (dropped classes and negative labels last), cut at the total."""
    c = SC.case(name)
    lab, base = c["sem_pred"], c["class_base"].astype(np.int64)
    ref = SC.reference(c)
    big = np.iinfo(np.int64).max
    key = np.where(lab >= 0, np.where(base[np.maximum(lab, 0)] >= 0, base[np.maximum(lab, 0)], big), big)
    order = np.argsort(key, kind="stable")[:ref["total"]]
    assert ref["written"].all() and len(ref["written"]) == ref["total"]                # every case packs its ranges densely
    assert np.array_equal(ref["ins_ind"], order) and np.array_equal(ref["ins_sem"], lab[order])
    assert np.array_equal(ref["ins_orig"].view(np.uint32), c["xyz"][order].view(np.uint32))
    assert np.array_equal(ref["ins_off"].view(np.uint32), (c["xyz"][order] + c["offset"][order]).view(np.uint32))
    hist = SR.block_hist(lab, c["n_cls"], SC.BLOCK)
    assert np.array_equal(hist.sum(0), np.bincount(lab[lab >= 0], minlength=c["n_cls"]))
    assert all(np.array_equal(hist[b], np.bincount(lab[b * 1024:(b + 1) * 1024][lab[b * 1024:(b + 1) * 1024] >= 0], minlength=c["n_cls"]))
               for b in range(hist.shape[0]))


@functools.lru_cache(maxsize=None)
def _reference(name):
    ref = SC.reference(SC.case(name))
    cap = len(ref["written"]) + SM.SLACK
    return SM.reference(ref, cap), cap


def _differs(name, mutant=None):
    c = SC.case(name)
    want, cap = _reference(name)
    hist = SR.block_hist(c["sem_pred"], c["n_cls"], SC.BLOCK)
    got = SM.select(c["sem_pred"], c["class_base"], hist, c["xyz"], SC.offset_buffer(c).reshape(-1), c["ld_off"], c["dtype"], cap, mutant)
    return not SM.same(got, want)


@pytest.mark.parametrize("name", SC.NAMES)
def test_restatement_equals_the_reference(name):
    assert not _differs(name)


@functools.lru_cache(maxsize=None)
def _kills(mutant):
    return tuple(n for n in SC.NAMES if _differs(n, mutant))


@pytest.mark.parametrize("mutant", SM.MUTANTS)
def test_mutant_is_killed(mutant):
    killed_by = _kills(mutant)
    print("\nKILL %-22s %2d/%d cases: %s" % (mutant, len(killed_by), len(SC.NAMES), " ".join(killed_by)))
    assert killed_by, "mutant %s survives the whole case set: the set is too weak" % mutant


DESIGNED = {
    "blocks_inclusive": ("N_n1", "L_only_b2w3r3"),
    "waves_omitted": ("N_n257", "L_one_class"),
    "run_not_advanced": ("N_n65", "L_runs64"),
    "lanes_le": ("N_n63", "L_one_class"),
    "dropped_contributes": ("L_all_dropped", "L_alternating_drop", "L_highest_only"),
    "off_in_16bit": ("O_rounding_bf16", "O_rounding_fp16"),
    "sem_of_leader": ("N_n63", "L_cls32_all"),
    "ld_ignored": ("O_rounding_fp32", "L_cls32_all"),
}


def test_designed_kills():
    """Each term of the position dies alone where only it is at work, and the neighbours that must not see a mistake do not."""
    assert set(DESIGNED) == set(SM.MUTANTS)
    for mutant, names in DESIGNED.items():
        for name in names:
            assert name in _kills(mutant), (mutant, name)
    assert not {"N_n1", "N_n63", "N_n64", "N_n65", "N_n255", "N_n256"} & set(_kills("waves_omitted"))     # one wave
    assert "L_runs256" not in _kills("waves_omitted")          # a class per wave: no wave in front holds the class
    assert not {"N_n1", "N_n63", "N_n64"} & set(_kills("run_not_advanced"))                                # one round
    assert not {"L_one_class", "L_runs64", "L_runs256"} & set(_kills("sem_of_leader"))                     # one class per round
    assert all(SC.case(n)["dtype"] != "fp32" for n in _kills("off_in_16bit"))
    assert all(SC.case(n)["ld_off"] == 8 for n in _kills("ld_ignored"))
    assert "L_one_class" not in _kills("dropped_contributes")  # nothing is dropped there


def test_only_b2w3r3_isolates_the_terms():
    """Class 7 of L_only_b2w3r3 has no block, wave or round in front that holds it: its points sit at class_base[7] + lane, and the
    mistakes about blocks, waves and rounds leave class 7's rows alone while `lanes_le` moves them."""
    c = SC.case("L_only_b2w3r3")
    ref = SC.reference(c)
    rows = np.nonzero(ref["ins_sem"] == 7)[0]
    assert c["class_base"][7] == 0 and np.array_equal(rows, np.arange(64)) and np.array_equal(ref["ins_ind"][:64], np.arange(3008, 3072))


def test_equivalent_mistake_changes_nothing():
    for n in SC.N_VALUES + (5 * SC.BLOCK + 1,):
        order = SM.walk_order(n)
        real = np.nonzero(order >= 0)[0]
        assert np.array_equal(order[real], np.arange(n)) and np.array_equal(real, np.arange(n))   # walk order = index order; tail lanes last
        assert (order[n:] == -1).all() and len(order) % SC.BLOCK == 0
    for name in SC.NAMES:
        for mutant in SM.EQUIVALENT:
            assert not _differs(name, mutant), (mutant, name)
    assert any(len(SC.case(n)["sem_pred"]) % 64 and SC.case(n)["class_base"][0] >= 0 for n in SC.NAMES)    # tail lanes of a KEPT class 0


def test_no_case_is_redundant():
    """Every case kills a mistake that some other case lets through, or says which shape it is there for."""
    everywhere = {m for m in SM.MUTANTS if len(_kills(m)) == len(SC.NAMES)}
    for name in SC.NAMES:
        kills = [m for m in SM.MUTANTS if m not in everywhere and name in _kills(m)]
        assert kills or SC.case(name)["reason"], name


def test_kill_matrix():
    print("\n%-20s %s" % ("", " ".join("%2d" % i for i in range(len(SM.SWITCHES)))))
    for name in SC.NAMES:
        print("%-20s %s" % (name, " ".join(" x" if _differs(name, m) else " ." for m in SM.SWITCHES)))
    for i, m in enumerate(SM.SWITCHES):
        print("%2d %s%s" % (i, m, "  (EQUIVALENT)" if m in SM.EQUIVALENT else ""))
