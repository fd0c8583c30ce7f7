"""Designed inputs for the shared device primitives: every size at which fill_ranges, the two exclusive scans and
radix_sort_u32 take another path.  A case is built from its name alone (seeded by it), once per process, and never changed;
tests/prims_ref.py states what must come out.  Sizes are written in tiles of the kernels, read from csrc/pbn_common.h (scans)
and asked of the library (sort), so a change of tile moves the cases with it."""
import functools
import os
import re
import zlib

import numpy as np

import prims_ref as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header_constants():
    text = open(os.path.join(ROOT, "pbnet_amd", "csrc", "pbn_common.h")).read()
    c = {k: int(v) for k, v in re.findall(r"constexpr int (SCAN_THREADS|SCAN_ITEMS) = (\d+);", text)}
    assert re.search(r"SCAN_TILE = SCAN_THREADS \* SCAN_ITEMS;\s*// 2048 elements per block", text)
    return c["SCAN_THREADS"], c["SCAN_THREADS"] * c["SCAN_ITEMS"]


SCAN_THREADS, SCAN_TILE = _header_constants()
SCAN_WINDOW = 64                 # predecessors per poll of k_scan_chained (one per lane)
FILL_VEC_SLOTS, FILL_BYTE_SLOTS, FILL_SMALL = 8, 16, 64       # FillArgs: vector ranges, byte ranges; ranges below 64 bytes go bytewise


@functools.lru_cache(maxsize=None)
def sort_tile():
    from pbnet_amd import selftest
    return selftest.sort_tile()


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


# ---- scan ------------------------------------------------------------------------------------------------------------------
def _scan_sizes():
    t, th = SCAN_TILE, SCAN_THREADS
    s = {"n0": 0, "n1": 1, "n63": 63, "n64": 64, "n65": 65, "n2047": t - 1, "n2048": t, "n2049": t + 1}
    for k in (64, 65, 66, 129):                       # around one and two look-back windows of the chained form
        s["t%d" % k] = k * t
        s["t%dp1" % k] = k * t + 1
    s.update({"t256m1": th * t - 1, "t256": th * t, "t256p1": th * t + 1,      # k_scan_sums: one trip of its loop, then a second
              "t257p5": (th + 1) * t + 5, "t600p1": 600 * t + 1})
    return s


SCAN_SIZES = _scan_sizes()
SCAN_FORMS = ("three", "chained")
SCAN_VALUES = ("ones", "random", "flags7", "zeros", "last1", "maxint")
SCAN_VARIANTS = ("plain", "alias", "adjacent", "nototal")
_SCAN_FEW = ("n65", "n2049", "t65p1", "t257p5")       # sizes of the value sets that say little about position
_SCAN_VARIANT_SIZES = ("n2049", "t257p5")


def _scan_names():
    names = []
    for form in SCAN_FORMS:
        for size in SCAN_SIZES:
            for values in SCAN_VALUES:
                if values in ("ones", "random") or (size in _SCAN_FEW and SCAN_SIZES[size] > 0):
                    names.append("%s-%s-%s-plain" % (form, size, values))
        for size in _SCAN_VARIANT_SIZES:
            for variant in SCAN_VARIANTS[1:]:
                names.append("%s-%s-random-%s" % (form, size, variant))
    return tuple(names)


SCAN_NAMES = _scan_names()


@functools.lru_cache(maxsize=None)
def _scan_input(size, values):
    n, rng = SCAN_SIZES[size], _rng("scan-%s-%s" % (size, values))
    if values == "ones":
        x = np.ones(n, np.int32)
    elif values == "random":
        x = rng.integers(-3, 1001, n).astype(np.int32)
    elif values == "flags7":
        x = (rng.random(n) < 1.0 / 7.0).astype(np.int32)
    elif values == "zeros":
        x = np.zeros(n, np.int32)
    elif values == "last1":
        x = np.zeros(n, np.int32)
        x[-1:] = 1
    else:                                            # the total is exactly 2^31 - 1, reached by the last element
        assert n > 0
        x = np.full(n, PR.INT32_MAX // n, np.int64)
        x[-1] += PR.INT32_MAX - int(x.sum())
        x = x.astype(np.int32)
    out, total = PR.scan(x)                          # asserts that every running sum stays inside int32
    if values == "maxint":
        assert total == PR.INT32_MAX
    x.setflags(write=False)
    out.setflags(write=False)
    return x, out, total


def scan_case(name):
    form, size, values, variant = name.split("-")
    x, out, total = _scan_input(size, values)
    return {"name": name, "chained": form == "chained", "n": len(x), "tiles": -(-len(x) // SCAN_TILE), "in": x, "out": out,
            "total": total, "alias": variant == "alias", "adjacent": variant == "adjacent", "nototal": variant == "nototal"}


# ---- sort ------------------------------------------------------------------------------------------------------------------
def sort_sizes():
    t = sort_tile()
    return {"n0": 0, "n1": 1, "n2": 2, "n63": 63, "n64": 64, "n65": 65, "Tm1": t - 1, "T": t, "Tp1": t + 1, "T3p17": 3 * t + 17,
            "T64": 64 * t, "T65p1": 65 * t + 1, "T66": 66 * t, "T130p3": 130 * t + 3}


SORT_SIZE_NAMES = ("n0", "n1", "n2", "n63", "n64", "n65", "Tm1", "T", "Tp1", "T3p17", "T64", "T65p1", "T66", "T130p3")
SORT_KEYS = ("random", "equal", "two", "mod7", "descending", "digit0", "digit1", "digit2", "extremes", "floats")
SORT_NAMES = tuple("%s-%s" % (s, k) for s in SORT_SIZE_NAMES for k in SORT_KEYS)


@functools.lru_cache(maxsize=None)
def sort_case(name):
    size, kind = name.split("-")
    n, rng = sort_sizes()[size], _rng("sort-" + name)
    i = np.arange(n, dtype=np.uint64)
    base = np.uint64(0x5a5a5a5a)
    if kind == "random":
        keys = rng.integers(0, 1 << 32, n, dtype=np.uint64)
    elif kind == "equal":
        keys = np.full(n, 0x9e3779b9, np.uint64)
    elif kind == "two":
        keys = np.where(rng.random(n) < 0.5, 0x80000401, 0x00200400).astype(np.uint64)
    elif kind == "mod7":
        keys = i % np.uint64(7)
    elif kind == "descending":                       # strictly descending, all three digits in use at the larger sizes
        keys = (np.uint64(n) - np.uint64(1) - i) * np.uint64(8191) if n else i
        assert n == 0 or int(keys.max()) < 1 << 32
    elif kind == "digit0":
        keys = (base & ~np.uint64(0x7ff)) | rng.integers(0, 1 << 11, n, dtype=np.uint64)
    elif kind == "digit1":
        keys = (base & ~np.uint64(0x7ff << 11)) | (rng.integers(0, 1 << 11, n, dtype=np.uint64) << np.uint64(11))
    elif kind == "digit2":                           # bits 22..31: the top digit has 10 significant bits
        keys = (base & np.uint64(0x3fffff)) | (rng.integers(0, 1 << 10, n, dtype=np.uint64) << np.uint64(22))
    elif kind == "extremes":
        keys = rng.choice(np.array([0, 0xffffffff, 1, 0xfffffffe, 0x80000000, 0x7fffffff], np.uint64), n)
    else:                                            # weights as mesh and orient feed them: order_key of float32
        special = np.array([0.0, -0.0, np.nan, np.inf, -np.inf, 1e-45, -1e-45, 1.0, -1.0, 2.0, 0.5], np.float32)
        w = np.where(rng.random(n) < 0.3, rng.choice(special, n), (rng.standard_normal(n) ** 2).astype(np.float32)).astype(np.float32)
        keys = PR.order_key(w).astype(np.uint64)
    keys = keys.astype(np.uint32)
    vals = rng.permutation(n).astype(np.int32)       # not iota: a carried value cannot be mistaken for a recomputed position
    keys_out, vals_out = PR.sort(keys, vals)
    for a in (keys, vals, keys_out, vals_out):
        a.setflags(write=False)
    return {"name": name, "n": n, "keys": keys, "vals": vals, "keys_out": keys_out, "vals_out": vals_out}


# ---- fill ------------------------------------------------------------------------------------------------------------------
FILL_BYTES, FILL_PRESET = 64 * 1024, 0xA5
FILL_LENGTHS = (0, 1, 15, 16, 17, 63, 64, 65, 79, 80, 4101)
FILL_VALUES = (0, 1, 0x7f, 0xff)


def _fill_cases():
    c = {}
    for li, length in enumerate(FILL_LENGTHS):        # every length at every start alignment; every value at every length
        for a in range(16):
            c["len%d_align%d" % (length, a)] = [(1024 + a, length, FILL_VALUES[(li + a) % 4])]
    c["adjacent"] = [(1003, 101, 0x11), (1104, 203, 0xee)]
    c["adjacent_small"] = [(77, 9, 0), (86, 40, 0xff), (126, 3, 1)]
    c["whole_buffer"] = [(3, FILL_BYTES - 7, 0x5c)]                                         # more than one workgroup of vectors
    c["nine_1k_aligned"] = [(i * 2048, 1024, 0x10 + i) for i in range(9)]                   # the ninth vector range: a flush mid-call
    c["nine_1k_unaligned"] = [(i * 2048 + 1 + i, 1024, 0x20 + i) for i in range(9)]         # ... with heads and tails pending
    c["twenty_5b"] = [(500 + 11 * i, 5, 0x30 + i) for i in range(20)]                       # the seventeenth byte range: a flush
    c["nine_1k_tails"] = [(i * 2048, 1024 + 1 + i, 0x70 + i) for i in range(9)]             # ... with eight tails pending, no more
    # both triggers in one call: the ninth vector range arrives with eight tails pending, then the seventeenth byte range with
    # a vector range pending, then an unaligned range after both
    c["mix"] = [(i * 2048 + 16, 1024 + 3, 0x40 + i) for i in range(9)] + [(20000 + 11 * i, 5, 0x50 + i) for i in range(18)] + \
        [(40007, 2000, 0x6f)]
    c["null_and_empty"] = [(100, 70, 1), (None, 50, 2), (300, 0, 3), (405, 33, 4), (None, 0, 5), (600, 100, 0x7f)]
    c["no_ranges"] = []
    return c


FILL_CASES = _fill_cases()
FILL_NAMES = tuple(FILL_CASES)


def fill_preset():
    return np.full(FILL_BYTES, FILL_PRESET, np.uint8)


@functools.lru_cache(maxsize=None)
def fill_reference(name):
    out = PR.fill(fill_preset(), FILL_CASES[name])
    out.setflags(write=False)
    return out
