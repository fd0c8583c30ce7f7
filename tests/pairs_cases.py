"""Designed inputs for the rule-pair lists (csrc/pairs.hip), shared by tests/test_pairs_cases_cpu.py (every precondition holds,
the mutants of tests/pairs_mutants.py die) and tests/test_pairs_cases_gpu.py (HIP == tests/pairs_ref.py, word for word, inside
sentinel-filled buffers).

A case is a dict: name, kind ("single": one map nbr int32 [n, K]; "multi": a job table `maps`; "refused": a map the fills must
refuse), seg, design (what the builder intended), precondition (a function of the case that raises AssertionError when the input no
longer holds the situation it was built for; evaluated with tests/pairs_ref.py) and, where the case is there for a shape and not for
a kill, `reason`.

Families
  R  rows 0, 1, 255, 256, 257 (one block of 256 rows -1, +0, +1) and 16383, 16384, 16385 (64 blocks -1, +0, +1: the block scan
     walks 64 blocks per trip) with K = 3: a full column, every third row, and the last row alone.
  K  offsets 1, 2, 3 (fewer columns than the 4 waves of a block), 31, 32, 33 (the 32-offset LDS tile), 63, 64, 65, 125, 129 (the
     64-offset chunk of the in-kernel seg_begin scan) and 512 (the most the fill takes) on 300 rows = one whole and one partial block;
     the columns cycle through the eight kinds below.  513 offsets: the counts succeed, both fills refuse.
  C  the eight column kinds side by side: full, empty, row 0 alone, the last row of the partial block alone, lanes 63 / 64 of the
     ballots alone (rows 63, 64, 127, 128, ...), one pair in five with -1, -2 and INT_MIN in between, every third row, seg + 1 pairs.
  S  segment 1; segment 7 with columns of exactly 6, 7, 8 and 21 pairs (seg - 1, seg, seg + 1, 3 seg), an empty and a full one;
     a segment larger than every count.
  M  job tables of the multi launch: one job; 16 jobs of K = 1, 8, 27, 125; an empty map first, in the middle and last; 17 maps
     (two launches of conv.rulebook_pairs_dev_multi).
The production segment on a real k = 3 map with its down / up maps, and a map whose lists are cached, need the device: they are built
in the GPU tier.  Input rows are (31 o + 17 k) mod n: row 0 is named by the first pair of the first column, so `src > 0` shows."""
import functools

import numpy as np

import pairs_ref as PR

INT_MIN = -2 ** 31
BLOCK_ROWS, SCAN_BLOCKS, TILE_K, SEG_CHUNK, MAX_K, MAX_JOBS = 256, 64, 32, 64, 512, 16        # asserted against pairs.hip (CPU tier)
KINDS = ("full", "empty", "row0", "last", "lanes6364", "mixneg", "third", "segp1")


def _column(n, kind, seg):
    """bool [n] rows with a pair, and the no-pair value per row."""
    rows, hole = np.zeros(n, bool), np.full(n, -1, np.int64)
    r = np.arange(n)
    if kind == "full":
        rows[:] = True
    elif kind == "row0":
        rows[:1] = True
    elif kind == "last":
        rows[n - 1:] = True
    elif kind == "lanes6364":
        rows[(r % 64 == 63) | ((r % 64 == 0) & (r > 0))] = True
    elif kind == "mixneg":
        rows[r % 5 == 2] = True
        hole = np.array([-1, -2, INT_MIN], np.int64)[r % 3]
    elif kind == "third":
        rows[r % 3 == 0] = True
    elif kind == "segp1":
        rows[_spread(n, seg + 1)] = True
    elif isinstance(kind, int):
        rows[_spread(n, kind)] = True
    else:
        assert kind == "empty"
    return rows, hole


def _spread(n, count):
    count = min(count, n)
    return (np.arange(count) * n) // max(count, 1)


def make_map(n, kinds, seg):
    """nbr int32 [n, len(kinds)]: column k of kind kinds[k], input rows (31 o + 17 k) mod n."""
    nbr = np.full((n, len(kinds)), -1, np.int64)
    o = np.arange(n)
    for k, kind in enumerate(kinds):
        rows, hole = _column(n, kind, seg)
        nbr[:, k] = np.where(rows, (31 * o + 17 * k) % max(n, 1), hole)
    nbr = nbr.astype(np.int32)
    nbr.setflags(write=False)
    return nbr


def cycle_map(n, n_off, seg):
    return make_map(n, [KINDS[k % len(KINDS)] for k in range(n_off)], seg)


def _case(name, kind, seg, design, pre, reason=None, **more):
    return dict(name=name, kind=kind, seg=seg, design=design, precondition=pre, reason=reason, **more)


def totals(c):
    return PR.pair_lists(c["nbr"], c["seg"])["totals"]


def blocks(n):
    return -(-n // BLOCK_ROWS)


# ---- R: rows ---------------------------------------------------------------------------------------------------------------------
def _rows_case(n):
    def pre(c):
        t = totals(c)
        assert c["nbr"].shape == (n, 3) and list(t) == [n, -(-n // 3), min(n, 1)]
        if n:
            assert c["nbr"][n - 1, 2] >= 0 and (c["nbr"][:n - 1, 2] < 0).all()        # the last row alone
        want = {0: 0, 1: 1, 255: 1, 256: 1, 257: 2, 16383: 64, 16384: 64, 16385: 65}[n]
        assert blocks(n) == want
        assert (blocks(n) > SCAN_BLOCKS) == (n == 16385)                                # the second trip of the block scan
    design = {0: "no rows: totals zero, seg_begin all zero, the device form's one empty block publishes it",
              1: "one row, one lane of one ballot", 255: "one block, last lane idle", 256: "one block exactly",
              257: "second block holds one row", 16383: "64 blocks, the last partial: one trip of the block scan, all lanes busy",
              16384: "64 blocks exactly: one trip of the block scan", 16385: "65 blocks: block 64 takes the carry of the second trip"}[n]
    reason = {255: "block edge - 1", 256: "block edge", 16383: "scan chunk edge - 1", 16384: "scan chunk edge"}.get(n)
    return _case("R_n%d" % n, "single", 64, design, pre, reason, nbr=make_map(n, ("full", "third", "last"), 64))


# ---- K: offsets --------------------------------------------------------------------------------------------------------------------
def _offsets_case(n_off):
    n, seg = 300, 16

    def pre(c):
        assert c["nbr"].shape == (n, n_off) and blocks(n) == 2 and n % BLOCK_ROWS != 0
        t = totals(c)
        want = dict(full=n, empty=0, row0=1, last=1, lanes6364=8, mixneg=60, third=100, segp1=seg + 1)
        assert list(t) == [want[KINDS[k % 8]] for k in range(n_off)]
        assert n_off <= MAX_K
        if n_off > SEG_CHUNK:
            assert t[:SEG_CHUNK].sum() > 0 and t[SEG_CHUNK:].sum() > 0        # a carry to drop, and someone to miss it
    edge = ("fewer columns than waves" if n_off < 4 else "LDS tile of 32 offsets" if n_off < 40 else
            "64-offset chunk of the seg_begin scan" if n_off < 200 else "the most offsets the fill takes")
    reason = "%s: %d" % (edge, n_off)
    return _case("K_k%d" % n_off, "single", seg, reason, pre, reason, nbr=cycle_map(n, n_off, seg))


def _refused_case():
    def pre(c):
        assert c["nbr"].shape[1] == MAX_K + 1 and totals(c).sum() > 0
    return _case("K_k513", "refused", 16, "one offset more than the fill's LDS table: counts succeed, fills refuse", pre,
                 "the limit + 1", nbr=cycle_map(10, MAX_K + 1, 16))


# ---- C: columns ------------------------------------------------------------------------------------------------------------------
def _columns_case():
    n, seg = 300, 16

    def pre(c):
        nbr = c["nbr"]
        has = nbr >= 0
        assert list(totals(c)) == [300, 0, 1, 1, 8, 60, 100, 17]
        assert has[0, 2] and has[299, 3] and 299 % BLOCK_ROWS not in (0, 255)            # last row of a PARTIAL block
        assert list(np.nonzero(has[:, 4])[0]) == [63, 64, 127, 128, 191, 192, 255, 256]     # last lane of a ballot, first of the next
        assert (nbr[:, 5] == -2).any() and (nbr[:, 5] == INT_MIN).any() and (nbr[:, 5] == -1).any()
        assert (nbr[has] == 0).any()                                                      # input row 0 is a pair
        assert 100 - 86 == 14 and has[:256, 6].sum() == 86 and 86 % seg != 0              # block 1 starts inside a segment
    return _case("C_columns", "single", seg, "the eight column kinds side by side", pre, nbr=make_map(n, KINDS, seg))


# ---- S: segments -----------------------------------------------------------------------------------------------------------------
def _segment_cases():
    def pre1(c):
        assert c["seg"] == 1 and totals(c).max() > 1

    def pre7(c):
        assert c["seg"] == 7 and list(totals(c)) == [6, 7, 8, 21, 0, 300]               # seg - 1, seg, seg + 1, 3 seg, none, all
        sb = PR.pair_lists(c["nbr"], 7)["seg_begin"]
        assert list(np.diff(sb)) == [1, 1, 2, 3, 0, 43]

    def pre_big(c):
        assert c["seg"] > totals(c).max() > 0
        assert list(np.diff(PR.pair_lists(c["nbr"], c["seg"])["seg_begin"])) == [1, 0, 1, 1, 1, 1, 1, 1]
    return [_case("S_seg1", "single", 1, "segment 1: every pair heads a segment", pre1, nbr=make_map(300, KINDS, 1)),
            _case("S_seg7_counts", "single", 7, "counts of seg - 1, seg, seg + 1 and 3 seg next to an empty and a full column", pre7,
                  nbr=make_map(300, (6, 7, 8, 21, "empty", "full"), 7)),
            _case("S_seg1000", "single", 1000, "a segment larger than every count: one segment per non-empty offset", pre_big,
                  "segment above every count", nbr=make_map(300, KINDS, 1000))]


# ---- M: job tables -----------------------------------------------------------------------------------------------------------------
MULTI_SEG = 16
_MIXED = tuple(zip((300, 1, 257, 70, 513, 256, 33, 600, 255, 64, 2, 129, 300, 17, 100, 511), (1, 8, 27, 125) * 4))


def _multi_case(name, shapes, design, grouped=False):
    def pre(c):
        assert [m.shape for m in c["maps"]] == [tuple(s) for s in shapes]
        assert grouped == (len(shapes) > MAX_JOBS)
        if "empty" in name:
            where = [i for i, s in enumerate(shapes) if s[0] == 0]
            assert where == [dict(first=0, middle=1, last=len(shapes) - 1)[name.split("_")[-1]]]
            assert sum(PR.pair_lists(m, MULTI_SEG)["totals"].sum() for m in c["maps"]) > 0
    return _case(name, "multi", MULTI_SEG, design, pre, maps=[cycle_map(n, k, MULTI_SEG) for n, k in shapes], grouped=grouped)


def _multi_cases():
    def pre16(c):
        assert len(c["maps"]) == MAX_JOBS and sorted(set(m.shape[1] for m in c["maps"])) == [1, 8, 27, 125]
    c16 = _multi_case("M_16_mixed", _MIXED, "a full job table, K = 1, 8, 27, 125 by turns, one to three blocks per job")
    c16["precondition"] = pre16
    one = _multi_case("M_one", ((300, 27),), "a job table of one")
    one["reason"] = "the smallest job table"
    return [one, c16,
            _multi_case("M_empty_first", ((0, 8), (300, 27), (70, 1)), "an empty map opens the table: its one block publishes seg_begin"),
            _multi_case("M_empty_middle", ((300, 27), (0, 125), (70, 8)), "an empty map between two others"),
            _multi_case("M_empty_last", ((70, 8), (300, 1), (0, 27)), "an empty map closes the table"),
            _multi_case("M_17_groups", _MIXED + ((90, 8),), "17 maps: conv.rulebook_pairs_dev_multi launches 16 + 1", grouped=True)]


ROWS_N = (0, 1, 255, 256, 257, 16383, 16384, 16385)
OFFSETS_K = (1, 2, 3, 31, 32, 33, 63, 64, 65, 125, 129, 512)


@functools.lru_cache(maxsize=None)
def _all():
    cases = [_rows_case(n) for n in ROWS_N] + [_offsets_case(k) for k in OFFSETS_K] + [_refused_case(), _columns_case()]
    cases += _segment_cases() + _multi_cases()
    return {c["name"]: c for c in cases}


def case(name):
    return _all()[name]


NAMES = tuple(_all())
SINGLE = tuple(n for n in NAMES if case(n)["kind"] == "single")
MULTI = tuple(n for n in NAMES if case(n)["kind"] == "multi")
REFUSED = tuple(n for n in NAMES if case(n)["kind"] == "refused")
