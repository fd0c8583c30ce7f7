"""CPU tier: the designed maps of tests/pairs_cases.py are valid (every precondition holds), the kernel-shaped statement
tests/pairs_mutants.py equals tests/pairs_ref.py on every case (totals, post-scan table, seg_begin, in_idx, out_idx, seg_offset and
what stays unwritten, in the device form, the host form with two surplus segments, and the job tables), and the set is sharp: each
deliberate mistake of pairs_mutants.MUTANTS differs from the reference on at least one case, and on the case that was built for it.
The kill matrix is printed (pytest -s shows it).  pairs_mutants.EQUIVALENT is empty: every mistake asked for can be told apart."""
import functools
import os
import re

import numpy as np
import pytest

import pairs_cases as PC
import pairs_mutants as PM
import pairs_ref as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SURPLUS = 2                                   # segments the host form is given beyond what the map needs


def test_constants_are_the_kernels():
    """The sizes the cases are built from, and the ones the restatement walks in, are those of the source the library is built from."""
    src = open(os.path.join(ROOT, "pbnet_amd", "csrc", "pairs.hip")).read()
    c = {k: int(v) for k, v in re.findall(r"constexpr int (TPB|PAIR_KC|PAIR_MAX_K|PAIR_MAX_JOBS) = (\d+);", src)}
    assert "constexpr int PAIR_ROWS = 256;" in src and c["TPB"] == 256
    assert (c["PAIR_KC"], c["PAIR_MAX_K"], c["PAIR_MAX_JOBS"]) == (PC.TILE_K, PC.MAX_K, PC.MAX_JOBS) == (PM.KC, PM.MAX_K, PM.MAX_JOBS)
    assert "for (int b0 = 0; b0 < n_blocks; b0 += 64)" in src and "for (int k0 = 0; k0 < K; k0 += 64)" in src
    assert (PC.BLOCK_ROWS, PC.SCAN_BLOCKS, PC.SEG_CHUNK) == (PM.ROWS, PM.SCAN_CHUNK, PM.SEG_CHUNK) == (256, 64, 64)
    assert tuple(PC.case(n)["nbr"].shape[0] for n in PC.NAMES if n[0] == "R") == (0, 1, 255, 256, 257, 16383, 16384, 16385)
    assert tuple(PC.case("K_k%d" % k)["nbr"].shape[1] for k in PC.OFFSETS_K) == (1, 2, 3, 31, 32, 33, 63, 64, 65, 125, 129, 512)


@pytest.mark.parametrize("name", PC.NAMES)
def test_precondition_holds(name):
    c = PC.case(name)
    c["precondition"](c)
    shape = "%d maps" % len(c["maps"]) if c["kind"] == "multi" else "%d x %d" % c["nbr"].shape
    print("\nPRE %-16s %-7s %-11s seg %4d  %s" % (name, c["kind"], shape, c["seg"], c["design"]))
    for m in (c["maps"] if c["kind"] == "multi" else [c["nbr"]]):
        assert m.size <= 300 * 512 and m.dtype == np.int32


@pytest.mark.parametrize("name", PC.SINGLE + PC.REFUSED)
def test_reference_is_nonzero_of_the_transposed_mask(name):
    """The anchor: an independent statement of the same lists.  np.nonzero of the transposed mask walks offset-major, rows ascending."""
    c = PC.case(name)
    nbr, seg = c["nbr"], c["seg"]
    ref = PR.pair_lists(nbr, seg)
    kk, oo = np.nonzero((nbr >= 0).T)
    assert np.array_equal(ref["totals"], np.bincount(kk, minlength=nbr.shape[1]))
    flat = np.concatenate(ref["pairs"]) if len(kk) else np.zeros((0, 2), np.int64)
    assert np.array_equal(flat[:, 1], oo) and np.array_equal(flat[:, 0], nbr[oo, kk])
    segs = -(-ref["totals"] // seg)
    assert np.array_equal(ref["seg_begin"], np.concatenate([[0], np.cumsum(segs)]))
    in_idx, out_idx, seg_offset = PR.host_layout(ref, int(segs.sum()) + SURPLUS)
    valid = in_idx >= 0
    assert np.array_equal(valid, out_idx >= 0) and np.array_equal(in_idx[valid], nbr[oo, kk]) and np.array_equal(out_idx[valid], oo)
    assert np.array_equal(seg_offset[:int(segs.sum())], np.repeat(np.arange(nbr.shape[1]), segs)) and not seg_offset[int(segs.sum()):].any()
    assert np.array_equal(np.nonzero(valid)[0], np.concatenate([b * seg + np.arange(t) for b, t in zip(ref["seg_begin"], ref["totals"])]))
    assert int(segs.sum()) <= PR.worst_case_segments(nbr.shape[0], nbr.shape[1], seg)
    assert np.array_equal(PR.block_prefix(nbr, 256), np.concatenate(
        [np.zeros((1, nbr.shape[1]), np.int64)] + [(nbr[:b] >= 0).sum(0, keepdims=True) for b in range(256, nbr.shape[0], 256)]))


@functools.lru_cache(maxsize=None)
def _references(name):
    c = PC.case(name)
    if c["kind"] == "multi":
        return [PM.reference_multi(m, c["seg"]) for m in c["maps"]]
    return PM.reference_dev(c["nbr"], c["seg"]), PM.reference_host(c["nbr"], c["seg"], SURPLUS)


def _differs(name, mutant=None):
    """Does the restatement (with the mistake) leave anything but the reference's words in any buffer?"""
    c = PC.case(name)
    if c["kind"] == "multi":
        got = PM.build_groups(c["maps"], c["seg"], mutant)
        return not all(PM.same(g, r) for g, r in zip(got, _references(name)))
    dev, (host, seg_start, n_seg) = _references(name)
    return not (PM.same(PM.build_dev(c["nbr"], c["seg"], mutant), dev) and
                PM.same(PM.build_host(c["nbr"], c["seg"], seg_start, n_seg, mutant), host))


@pytest.mark.parametrize("name", PC.NAMES)
def test_restatement_equals_the_reference(name):
    assert not _differs(name)


def test_refused_map_leaves_the_lists_alone():
    """K = 513 in the restatement: totals and table as for any map, every list word still the sentinel, in both forms."""
    c = PC.case("K_k513")
    dev, (host, _, _) = _references("K_k513")
    for r in (dev, host):
        assert (r["in_idx"] == PM.SENT32).all() and (r["out_idx"] == PM.SENT32).all() and (r["seg_offset"] == PM.SENT64).all()
        assert np.array_equal(r["totals"], PR.pair_lists(c["nbr"], c["seg"])["totals"]) and r["totals"].sum() > 0


MUTANT_CASES = tuple(n for n in PC.SINGLE + PC.MULTI if n != "K_k512")           # 300 x 512 adds time, not kills


@functools.lru_cache(maxsize=None)
def _kills(mutant):
    return tuple(n for n in MUTANT_CASES if _differs(n, mutant))


@pytest.mark.parametrize("mutant", PM.MUTANTS)
def test_mutant_is_killed(mutant):
    killed_by = _kills(mutant)
    print("\nKILL %-28s %2d/%d cases: %s" % (mutant, len(killed_by), len(MUTANT_CASES), " ".join(killed_by)))
    assert killed_by, "mutant %s survives the whole case set: the set is too weak" % mutant


DESIGNED = {
    "scan_carry_dropped": ("R_n16385",),
    "scan_inclusive": ("R_n1", "R_n257"),
    "seg_begin_carry_dropped": ("K_k65", "K_k125", "K_k129"),
    "segments_floor": ("S_seg7_counts", "S_seg1000"),
    "slot_wrong_base": ("C_columns", "S_seg7_counts"),
    "seg_offset_prev_at_multiple": ("S_seg1", "S_seg7_counts"),
    "tail_rows_counted": ("R_n0", "R_n1", "R_n255", "R_n257", "R_n16385"),
    "src_gt_zero": ("R_n1", "C_columns"),
    "seg_begin_end_unpublished": ("R_n0", "K_k1"),
    "multi_empty_zero_blocks": ("M_empty_first", "M_empty_middle", "M_empty_last"),
    "multi_job_gt": ("M_16_mixed", "M_empty_first"),
    "subrounds_reversed": ("R_n255", "C_columns"),
}


def test_designed_kills():
    """Each mistake dies on the case built for it -- and the neighbours that must NOT see it do not: a dropped scan carry needs a 65th
    block, a dropped seg_begin carry a 65th offset, a counted tail a partial last block, a one-job table has no job to mistake."""
    assert set(DESIGNED) == set(PM.MUTANTS)
    for mutant, names in DESIGNED.items():
        for name in names:
            assert name in _kills(mutant), (mutant, name)
    assert _kills("scan_carry_dropped") == ("R_n16385",)
    assert not {"K_k63", "K_k64"} & set(_kills("seg_begin_carry_dropped"))
    assert not {"R_n256", "R_n16384"} & set(_kills("tail_rows_counted"))
    assert "M_one" not in _kills("multi_job_gt") and "S_seg1" not in _kills("segments_floor")
    assert set(_kills("multi_empty_zero_blocks")) == {"M_empty_first", "M_empty_middle", "M_empty_last"}


def test_no_case_is_redundant():
    """Every case kills a mistake that some other case lets through, or says which shape it is there for."""
    everywhere = {m for m in PM.MUTANTS if len(_kills(m)) == len(MUTANT_CASES)}
    assert everywhere == {"seg_begin_end_unpublished"}
    for name in PC.NAMES:
        c = PC.case(name)
        kills = [m for m in PM.MUTANTS if m not in everywhere and name in _kills(m)]
        assert kills or c["reason"], name


def test_kill_matrix():
    print("\n%-16s %s" % ("", " ".join("%2d" % i for i in range(len(PM.MUTANTS)))))
    for name in MUTANT_CASES:
        print("%-16s %s" % (name, " ".join(" x" if name in _kills(m) else " ." for m in PM.MUTANTS)))
    for i, m in enumerate(PM.MUTANTS):
        print("%2d %s" % (i, m))
    assert PM.EQUIVALENT == ()
