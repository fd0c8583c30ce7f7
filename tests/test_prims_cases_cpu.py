"""CPU tier: the designed inputs of tests/prims_cases.py sit where they were meant to (tile and window edges, both flush
triggers of the fill), the kernel-shaped statement tests/prims_mutants.py equals the plain one (tests/prims_ref.py) on every
case, and the set is sharp: each deliberate mistake differs from it on at least one case.  The kill list is printed
(pytest -s).  Last, the argument checks of the self-test entry points, which run on the host before any launch."""
import functools

import numpy as np
import pytest

import prims_cases as PC
import prims_mutants as PM
import prims_ref as PR
from pbnet_amd import _native as N
from pbnet_amd import selftest as S


# ---- the cases are where they were designed to be ------------------------------------------------------------------------------
def test_tile_constants():
    assert (PC.SCAN_TILE, PC.SCAN_THREADS) == (S.SCAN_TILE, S.SCAN_THREADS) == (2048, 256)
    assert PC.sort_tile() == N.lib().pbn_selftest_sort_tile() > 0 and PC.sort_tile() % 64 == 0


def test_scan_sizes_cross_every_edge():
    tiles = {name: -(-n // PC.SCAN_TILE) for name, n in PC.SCAN_SIZES.items()}
    w, th = PC.SCAN_WINDOW, PC.SCAN_THREADS
    assert {tiles[k] for k in ("n0", "n1", "n2048", "n2049")} == {0, 1, 2}
    # the chained walk: exactly one window, one window and the prefix holder just outside it, two windows and one beyond
    assert [tiles[k] for k in ("t64", "t64p1", "t65", "t65p1", "t66", "t66p1", "t129", "t129p1")] == \
        [w, w + 1, w + 1, w + 2, w + 2, w + 3, 2 * w + 1, 2 * w + 2]
    # k_scan_sums: its loop runs once up to SCAN_THREADS tiles and carries from there on
    assert [tiles[k] for k in ("t256m1", "t256", "t256p1", "t257p5", "t600p1")] == [th, th, th + 1, th + 2, 601]
    assert max(PC.SCAN_SIZES.values()) == 600 * PC.SCAN_TILE + 1 < 1.3e6
    for n in PC.SCAN_SIZES.values():
        assert 0 < S.N.lib().pbn_selftest_workspace_bytes(S.SCAN, n) and 0 < S.N.lib().pbn_selftest_workspace_bytes(S.SCAN_CHAINED, n)


def test_scan_values():
    for size in ("n2049", "t257p5"):
        c = {v: PC.scan_case("three-%s-%s-plain" % (size, v)) for v in PC.SCAN_VALUES}
        n = c["ones"]["n"]
        assert c["ones"]["total"] == n and c["zeros"]["total"] == 0 and c["last1"]["total"] == 1 and c["last1"]["in"][-1] == 1
        assert c["maxint"]["total"] == PR.INT32_MAX
        assert set(np.unique(c["flags7"]["in"])) == {0, 1} and abs(c["flags7"]["total"] / n - 1 / 7) < 0.03
        assert -3 <= c["random"]["in"].min() < 0 and 990 < c["random"]["in"].max() <= 1000
    big = PC.scan_case("three-t600p1-random-plain")["in"]
    assert big.min() == -3 and big.max() == 1000
    assert len(PC.SCAN_NAMES) == len(set(PC.SCAN_NAMES))


def test_sort_key_sets():
    t = PC.sort_tile()
    s = PC.sort_sizes()
    assert [s[k] for k in PC.SORT_SIZE_NAMES] == [0, 1, 2, 63, 64, 65, t - 1, t, t + 1, 3 * t + 17, 64 * t, 65 * t + 1, 66 * t, 130 * t + 3]
    name = "T3p17-%s"
    digits = lambda k: [np.unique((k >> (11 * p)) & 2047).size for p in range(3)]
    assert [d > 1 for d in digits(PC.sort_case(name % "digit0")["keys"])] == [True, False, False]
    assert [d > 1 for d in digits(PC.sort_case(name % "digit1")["keys"])] == [False, True, False]
    assert [d > 1 for d in digits(PC.sort_case(name % "digit2")["keys"])] == [False, False, True]
    assert np.unique(PC.sort_case(name % "digit2")["keys"] >> 22).size > 512         # both values of bit 31, many of the others
    assert np.unique(PC.sort_case(name % "equal")["keys"]).size == 1 and np.unique(PC.sort_case(name % "two")["keys"]).size == 2
    assert (np.diff(PC.sort_case("T130p3-descending")["keys"].astype(np.int64)) < 0).all()
    assert min(digits(PC.sort_case("T130p3-descending")["keys"])) > 1
    assert {0, 0xffffffff} <= set(PC.sort_case(name % "extremes")["keys"].tolist())
    f = PC.sort_case(name % "floats")["keys"]
    assert {0xffffffff, 0x80000000, int(PR.order_key([np.inf])[0]), int(PR.order_key([-np.inf])[0])} <= set(f.tolist())
    assert PR.order_key([-0.0])[0] == PR.order_key([0.0])[0] == 0x80000000
    w = np.array([-np.inf, -2.0, -1e-45, 0.0, 1e-45, 1.0, np.inf, np.nan], np.float32)
    assert (np.diff(PR.order_key(w).astype(np.int64)) > 0).all()
    for nm in PC.SORT_NAMES:                                     # values are a permutation, and not the identity
        c = PC.sort_case(nm)
        assert np.array_equal(np.sort(c["vals"]), np.arange(c["n"]))
        assert c["n"] < 64 or not np.array_equal(c["vals"], np.arange(c["n"]))


def test_fill_cases_reach_both_flushes():
    def tables(ranges):                                          # vector ranges and byte ranges the call collects in all
        nv = nb = 0
        for off, length, _ in ranges:
            if off is None or length == 0:
                continue
            if length < PC.FILL_SMALL:
                nb += 1
                continue
            head = (16 - off % 16) % 16
            nv, nb = nv + 1, nb + (head > 0) + ((length - head) % 16 > 0)
        return nv, nb
    assert tables(PC.FILL_CASES["nine_1k_aligned"]) == (PC.FILL_VEC_SLOTS + 1, 0)
    nv, nb = tables(PC.FILL_CASES["nine_1k_unaligned"])
    assert nv == PC.FILL_VEC_SLOTS + 1 and nb > 0
    assert tables(PC.FILL_CASES["twenty_5b"]) == (0, 20) and 20 > PC.FILL_BYTE_SLOTS
    assert tables(PC.FILL_CASES["nine_1k_tails"]) == (PC.FILL_VEC_SLOTS + 1, 9)      # eight tails pending at the ninth vector range
    nv, nb = tables(PC.FILL_CASES["mix"])
    assert nv > PC.FILL_VEC_SLOTS and nb > PC.FILL_BYTE_SLOTS
    for length in PC.FILL_LENGTHS:                               # every value at every length, every alignment at every length
        rs = [PC.FILL_CASES["len%d_align%d" % (length, a)][0] for a in range(16)]
        assert {r[2] for r in rs} == set(PC.FILL_VALUES) and {r[0] % 16 for r in rs} == set(range(16))
    for name in PC.FILL_NAMES:                                   # ranges stay inside the buffer
        assert all(o is None or 0 <= o and o + b <= PC.FILL_BYTES for o, b, _ in PC.FILL_CASES[name])


# ---- the kernel-shaped statement equals the plain one; every mistake shows ---------------------------------------------------------
def _scan_differs(name, mutant):
    c = PC.scan_case(name)
    out, total = PM.scan(c["in"], c["chained"], c["alias"], mutant)
    return not np.array_equal(out, c["out"]) or (not c["nototal"] and total != c["total"])


def _sort_differs(name, mutant):
    c = PC.sort_case(name)
    k, v = PM.sort(c["keys"], c["vals"], mutant)
    return not (k.dtype == np.uint64 and np.array_equal(k, c["keys_out"]) and np.array_equal(v, c["vals_out"]))


def _fill_differs(name, mutant):
    return not np.array_equal(PM.fill(PC.fill_preset(), PC.FILL_CASES[name], mutant), PC.fill_reference(name))


FAMILIES = ((PM.SCAN_MUTANTS, PC.SCAN_NAMES, _scan_differs), (PM.FILL_MUTANTS, PC.FILL_NAMES, _fill_differs),
            (PM.SORT_MUTANTS, PC.SORT_NAMES, _sort_differs))


@pytest.mark.parametrize("family", range(3), ids=("scan", "fill", "sort"))
def test_statement_equals_reference(family):
    _, names, differs = FAMILIES[family]
    wrong = [n for n in names if differs(n, None)]
    assert not wrong, wrong


@functools.lru_cache(maxsize=None)
def _kills(mutant):
    for mutants, names, differs in FAMILIES:
        if mutant in mutants:
            return tuple(n for n in names if differs(n, mutant))
    raise KeyError(mutant)


@pytest.mark.parametrize("mutant", PM.MUTANTS)
def test_mutant_is_killed(mutant):
    killed_by = _kills(mutant)
    print("\nKILL %-26s %3d cases, e.g. %s" % (mutant, len(killed_by), " ".join(killed_by[:4])))
    assert killed_by, "mutant %s survives the whole case set: a case is missing" % mutant


def test_designed_kills():
    """The mistakes a case was built for die on that case, and not on its neighbour below the edge."""
    k = _kills("sums_carry_dropped")
    assert "three-t257p5-ones-plain" in k and "three-t256p1-random-plain" in k and not [n for n in k if "-t256-" in n or "chained" in n]
    k = _kills("total_from_tile_of_n")
    assert "chained-t64-ones-plain" in k and "chained-n2048-random-plain" in k and "chained-t64p1-ones-plain" not in k
    k = _kills("inplace_reads_written")
    assert {"three-n2049-random-alias", "chained-t257p5-random-alias"} <= set(k) and all(n.endswith("-alias") for n in k)
    k = _kills("lookback_stops_early")
    assert "chained-t66-ones-plain" in k and "chained-t129p1-random-plain" in k
    assert not [n for n in k if "-t64-" in n or "-t65-" in n or n.startswith("three")]
    assert "len79_align0" in _kills("fill_tail_skipped") and "len64_align0" not in _kills("fill_tail_skipped")
    k = _kills("fill_head_p_and_15")
    assert "len80_align3" in k and "len80_align8" not in k and "len63_align3" not in k
    assert set(_kills("fill_flush_forgets_bytes")) == {"nine_1k_tails", "mix"}
    assert "T3p17-mod7" in _kills("ties_reversed") and "n2-equal" in _kills("ties_reversed")
    k = _kills("top_digit_wrong_shift")
    assert "n65-digit2" in k and not [n for n in k if n.endswith("digit0")]
    k = _kills("hist_not_cleared")
    assert "Tp1-random" in k and not [n for n in k if n.endswith("-equal")]


# ---- argument checks of the entry points: host only -------------------------------------------------------------------------
FAKE = N.c_vp(1 << 20)                                           # aligned, never dereferenced: the checks come before any launch


def test_workspace_query_refuses_bad_arguments():
    q = N.lib().pbn_selftest_workspace_bytes
    assert q(S.SCAN, -1) == 0 and q(S.SORT, -1) == 0 and q(3, 10) == 0 and q(-1, 10) == 0 and q(S.SORT, (1 << 28) + 1) == 0
    assert 0 < q(S.SCAN, 0) <= q(S.SCAN, 5000) < q(S.SCAN, 10 ** 6) and 0 < q(S.SCAN_CHAINED, 0) < q(S.SCAN_CHAINED, 10 ** 6)
    assert 0 < q(S.SORT, 0) == q(S.SORT, 1) < q(S.SORT, 10 ** 6)


@pytest.mark.parametrize("chained", (0, 1))
def test_scan_argument_checks(chained):
    lib = N.lib()
    n = 5000
    need = lib.pbn_selftest_workspace_bytes(chained, n)

    def call(inp=FAKE, out=FAKE, n=n, chained=chained, total=FAKE, status=FAKE, ws=FAKE, ws_bytes=need):
        return lib.pbn_selftest_scan(inp, out, n, chained, total, status, ws, ws_bytes, None)
    assert call(n=-1) == N.PBN_ERR_ARG
    assert call(inp=None) == N.PBN_ERR_ARG and call(out=None) == N.PBN_ERR_ARG and call(ws=None) == N.PBN_ERR_ARG
    assert call(chained=2) == N.PBN_ERR_ARG
    if chained:
        assert call(status=None) == N.PBN_ERR_ARG
    assert call(ws_bytes=need - 1) == N.PBN_ERR_WORKSPACE and call(ws_bytes=0) == N.PBN_ERR_WORKSPACE


def test_sort_argument_checks():
    lib = N.lib()
    n = 5000
    need = lib.pbn_selftest_workspace_bytes(S.SORT, n)

    def call(keys=FAKE, vals=FAKE, n=n, keys_out=FAKE, vals_out=FAKE, status=FAKE, ws=FAKE, ws_bytes=need):
        return lib.pbn_selftest_sort_u32(keys, vals, n, keys_out, vals_out, status, ws, ws_bytes, None)
    assert call(n=-1) == N.PBN_ERR_ARG
    for missing in ("keys", "vals", "keys_out", "vals_out", "status", "ws"):
        assert call(**{missing: None}) == N.PBN_ERR_ARG, missing
    assert call(ws_bytes=need - 1) == N.PBN_ERR_WORKSPACE


def test_fill_argument_checks():
    import ctypes
    lib = N.lib()
    off, cnt, val = (N.c_i64 * 2)(0, 16), (N.c_i64 * 2)(8, 8), (ctypes.c_uint8 * 2)(1, 2)
    assert lib.pbn_selftest_fill(FAKE, off, cnt, val, -1, None) == N.PBN_ERR_ARG
    assert lib.pbn_selftest_fill(FAKE, off, cnt, val, S.MAX_RANGES + 1, None) == N.PBN_ERR_ARG
    assert lib.pbn_selftest_fill(None, off, cnt, val, 2, None) == N.PBN_ERR_ARG
    assert lib.pbn_selftest_fill(FAKE, None, cnt, val, 2, None) == N.PBN_ERR_ARG
    assert lib.pbn_selftest_fill(FAKE, off, (N.c_i64 * 2)(8, -8), val, 2, None) == N.PBN_ERR_ARG
    assert lib.pbn_selftest_fill(FAKE, (N.c_i64 * 2)(0, -2), cnt, val, 2, None) == N.PBN_ERR_ARG


def test_wrappers_refuse_host_tensors_and_bad_shapes():
    import torch
    z = torch.zeros(8, dtype=torch.int32)
    with pytest.raises(RuntimeError):
        S.scan(z, z, 8)
    with pytest.raises(RuntimeError):
        S.sort_u32(z, z)
    with pytest.raises(RuntimeError):
        S.fill(torch.zeros(8, dtype=torch.uint8), [(0, 8, 1)])
    with pytest.raises(ValueError):
        S.scan(z, z, -1)
    with pytest.raises(ValueError):
        S.workspace(S.SORT, -1, "cpu")
    with pytest.raises(ValueError):
        S.workspace(7, 10, "cpu")
