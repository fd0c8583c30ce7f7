"""Designed inputs for the class-major selection (k_select_points in csrc/front.hip), shared by tests/test_select_cases_cpu.py
(every precondition holds, the mutants of tests/select_mutants.py die) and tests/test_select_cases_gpu.py (HIP == tests/select_ref.py,
bit for bit, inside sentinel-filled buffers).

A case is a dict: name, sem_pred int64 [n], n_cls, class_base int32 [n_cls], xyz float32 [n, 3], offset float32 [n, 3] (already
representable in `dtype`), dtype ("fp32", "bf16", "fp16"), ld_off (3 or 8), design, precondition (raises AssertionError when the input
no longer holds the situation it was built for; evaluated with tests/select_ref.py) and `reason` where the case stands for a shape.

A block is 1024 points, a wave 256 consecutive points of it, a round 64 consecutive points of a wave.
Families
  N  n = 1, 63, 64, 65 (a round -1, +0, +1), 255, 256, 257 (a wave), 1023, 1024, 1025 (a block), 2049, 3073 (two and three blocks
     in front) with label = (i + 2) mod 20 -- every ballot round splits into 20 groups --, classes 0 and 1 dropped as the network drops
     them; the offsets' type and ld_off take turns.
  L  labels: one class only (n_cls = 1); two classes in runs of 64 that align with the rounds; runs of 256 that align with the
     waves; a class seen only in block 2, wave 3, round 3; kept and dropped classes by turns; every class dropped (nothing is
     written); only the highest of 32 classes kept; negative labels (-1, -5) among valid ones; class_base NOT ascending in class
     (disjoint ranges in a permuted class order); 32 classes all kept.
  O  offsets: x + o rounds in float32 (x large, o tiny) and o = -x exactly, per type; ld_off 8 with the padding columns poisoned.
Labels >= n_cls are outside the contract -- the kernel indexes its n_cls-word tables with the label -- and are NOT fed to it; the
reference asserts their absence."""
import functools
import zlib

import numpy as np

import heads_ref as HR
import select_ref as SR

BLOCK, WAVE, ROUND = 1024, 256, 64            # asserted against front.hip (CPU tier)
DTYPES = ("fp32", "bf16", "fp16")
POISON = 1024.0                              # what the padding columns of a wide offset buffer hold (representable in every type)


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def _as(v, dtype):
    return HR.round_to(np.asarray(v, np.float64), dtype).astype(np.float32)


def bases(sem_pred, n_cls, keep, order=None):
    """class_base: the kept classes packed in `order` (default ascending), -1 for the others."""
    pop = np.bincount(sem_pred[sem_pred >= 0], minlength=n_cls)
    base, run = np.full(n_cls, -1, np.int32), 0
    for c in (order if order is not None else range(n_cls)):
        if c in keep:
            base[c] = run
            run += int(pop[c])
    return base


def _case(name, sem_pred, n_cls, class_base, dtype, ld_off, design, pre, reason=None, xyz=None, offset=None):
    rng = _rng(name)
    n = len(sem_pred)
    if xyz is None:
        xyz = (rng.normal(size=(n, 3)) * 3).astype(np.float32)
        offset = _as(rng.normal(size=(n, 3)) * 0.7, dtype)
    c = dict(name=name, sem_pred=np.asarray(sem_pred, np.int64), n_cls=n_cls, class_base=np.asarray(class_base, np.int32),
             xyz=np.ascontiguousarray(xyz, np.float32), offset=np.ascontiguousarray(offset, np.float32), dtype=dtype, ld_off=ld_off,
             design=design, precondition=pre, reason=reason)
    for k in ("sem_pred", "class_base", "xyz", "offset"):
        c[k].setflags(write=False)
    return c


def offset_buffer(c):
    """float32 [n, ld_off]: the offsets in the first three columns, POISON behind them."""
    buf = np.full((len(c["sem_pred"]), c["ld_off"]), POISON, np.float32)
    buf[:, :3] = c["offset"]
    return buf


def reference(c):
    return SR.select_points(c["sem_pred"], c["class_base"], c["xyz"], c["offset"])


def slot(i):
    """(block, wave, round, lane) of point i."""
    return i // BLOCK, i % BLOCK // WAVE, i % WAVE // ROUND, i % ROUND


# ---- N -----------------------------------------------------------------------------------------------------------------------------
N_VALUES = (1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049, 3073)


def _n_case(j, n):
    lab = (np.arange(n) + 2) % 20                 # point 0 is of a kept class
    keep = set(range(2, 20))

    def pre(c):
        assert len(c["sem_pred"]) == n and c["n_cls"] == 20
        r = reference(c)
        assert r["total"] == int((lab >= 2).sum()) == len(r["written"]) and r["written"].all() and r["total"] >= 1
        assert len(set(lab[:ROUND].tolist())) == min(n, 20)                        # a round splits into 20 groups
        assert slot(n - 1) == {1: (0, 0, 0, 0), 63: (0, 0, 0, 62), 64: (0, 0, 0, 63), 65: (0, 0, 1, 0), 255: (0, 0, 3, 62),
                               256: (0, 0, 3, 63), 257: (0, 1, 0, 0), 1023: (0, 3, 3, 62), 1024: (0, 3, 3, 63), 1025: (1, 0, 0, 0),
                               2049: (2, 0, 0, 0), 3073: (3, 0, 0, 0)}[n]
    edge = "round" if n < 100 else "wave" if n < 300 else "block" if n < 1100 else "blocks in front"
    why = "n = %d: %s edge, last point in (block, wave, round, lane) = %s" % (n, edge, (slot(n - 1),))
    return _case("N_n%d" % n, lab, 20, bases(lab, 20, keep), DTYPES[j % 3], (3, 8)[j % 2], why, pre, why)


# ---- L -----------------------------------------------------------------------------------------------------------------------------
def _label_cases():
    out = []

    def add(name, lab, n_cls, base, dtype, ld, design, pre, reason=None):
        out.append(_case(name, lab, n_cls, base, dtype, ld, design, pre, reason))

    def pre_one(c):
        r = reference(c)
        assert c["n_cls"] == 1 and (c["sem_pred"] == 0).all() and np.array_equal(r["ins_ind"], np.arange(1025))
    lab = np.zeros(1025, np.int64)
    add("L_one_class", lab, 1, [0], "fp32", 3, "n_cls = 1, every point of the one class: the output is the input", pre_one)

    def pre_64(c):
        lab = c["sem_pred"]
        for r0 in range(0, len(lab), ROUND):
            assert len(set(lab[r0:r0 + ROUND].tolist())) == 1                      # a round holds one class: one ballot
        assert set(lab[:WAVE].tolist()) == {0, 1}                                   # a wave holds both: run must advance
    lab = (np.arange(1025) // ROUND) % 2
    add("L_runs64", lab, 2, bases(lab, 2, {0, 1}), "bf16", 3, "two classes in runs of 64 = the rounds", pre_64)

    def pre_256(c):
        lab = c["sem_pred"]
        for w0 in range(0, len(lab), WAVE):
            assert len(set(lab[w0:w0 + WAVE].tolist())) == 1                       # a wave holds one class
        assert len(lab) == 5 * BLOCK + 1 and lab[5 * BLOCK] == lab[0] == 0 and (lab[WAVE:5 * BLOCK] != 0).all()
    lab = (np.arange(5 * BLOCK + 1) // WAVE) % 20
    add("L_runs256", lab, 20, bases(lab, 20, set(range(20))), "fp16", 8,
        "20 classes in runs of 256 = the waves; class 0 comes back in block 5 with only blocks in front", pre_256)

    def pre_only(c):
        rows = np.nonzero(c["sem_pred"] == 7)[0]
        assert len(rows) == ROUND and {slot(int(i))[:3] for i in rows} == {(2, 3, 3)} and len(c["sem_pred"]) == 3073
        assert c["class_base"][7] >= 0
    lab = np.arange(3073) % 5
    lab[2 * BLOCK + 3 * WAVE + 3 * ROUND:3 * BLOCK] = 7
    add("L_only_b2w3r3", lab, 20, bases(lab, 20, {1, 3, 7}, order=(7, 3, 1)), "fp32", 8,
        "class 7 lives in block 2, wave 3, round 3 alone: its base is class_base and nothing else", pre_only)

    def pre_alt(c):
        b = c["class_base"]
        assert (b[0::2] >= 0).all() and (b[1::2] < 0).all() and reference(c)["total"] == int((c["sem_pred"] % 2 == 0).sum())
    lab = np.arange(1025) % 20
    add("L_alternating_drop", lab, 20, bases(lab, 20, set(range(0, 20, 2))), "bf16", 8, "kept and dropped classes by turns", pre_alt)

    def pre_none(c):
        r = reference(c)
        assert (c["class_base"] < 0).all() and r["total"] == 0 and len(r["written"]) == 0
    lab = np.arange(257) % 20
    add("L_all_dropped", lab, 20, np.full(20, -1), "fp32", 3, "every class dropped: total 0, no output word is written", pre_none,
        "total 0")

    def pre_high(c):
        assert c["n_cls"] == 32 and (c["class_base"][:31] < 0).all() and c["class_base"][31] == 0
        assert np.array_equal(reference(c)["ins_ind"], np.arange(31, 1025, 32))
    lab = np.arange(1025) % 32
    add("L_highest_only", lab, 32, bases(lab, 32, {31}), "fp16", 3, "32 classes, only class 31 kept: lane 31 carries the one run", pre_high)

    def pre_neg(c):
        lab = c["sem_pred"]
        assert (lab == -1).sum() > 100 and (lab == -5).sum() > 10 and (lab[:ROUND] < 0).any() and lab[0] < 0
        assert reference(c)["total"] == int((lab >= 2).sum())
    lab = np.arange(1025) % 20
    lab[::7] = -1
    lab[3::91] = -5
    add("L_negative_labels", lab, 20, bases(lab, 20, set(range(2, 20))), "fp32", 3, "negative labels among valid ones take no position",
        pre_neg)

    order = (11, 3, 19, 7, 2, 16, 5, 13)

    def pre_perm(c):
        b = c["class_base"]
        kept = [k for k in range(20) if b[k] >= 0]
        assert sorted(kept) == sorted(order) and [int(b[k]) for k in order] == sorted(int(b[k]) for k in order)
        assert any(b[kept[i]] > b[kept[i + 1]] for i in range(len(kept) - 1))       # not ascending in class
        assert reference(c)["written"].all()                                        # disjoint and dense
    lab = np.arange(1025) % 20
    add("L_permuted_base", lab, 20, bases(lab, 20, set(order), order=order), "fp32", 3,
        "class_base not ascending in class: disjoint ranges in a permuted class order", pre_perm)

    def pre_32(c):
        assert c["n_cls"] == 32 and (c["class_base"] >= 0).all() and len(set(c["sem_pred"][:ROUND].tolist())) == 32
    lab = (np.arange(257) * 5) % 32
    add("L_cls32_all", lab, 32, bases(lab, 32, set(range(32))), "bf16", 8, "32 classes, all kept: every lane below 32 carries a run", pre_32)
    return out


# ---- O -----------------------------------------------------------------------------------------------------------------------------
def _offset_cases():
    out = []
    for dtype, ld, tiny in (("fp32", 8, 2.0 ** -20), ("bf16", 3, 2.0 ** -12), ("fp16", 8, 2.0 ** -12)):
        n = 65
        name = "O_rounding_" + dtype
        rng = _rng(name)
        lab = np.arange(n) % 3
        xyz = _as(rng.uniform(900, 1100, (n, 3)), dtype)                             # representable: -x is an offset of the type
        xyz[1::2] += np.float32(0.37)                                                # ... and rows whose x is float32 only
        off = np.empty((n, 3), np.float32)
        off[0::2] = -xyz[0::2]
        off[1::2] = tiny * (1 + (2 * rng.integers(0, 64, (n // 2, 3)) + 1) / 128.0)     # odd 7-bit fractions: exact in every type

        def pre(c, tiny=tiny, dtype=dtype):
            x, o = c["xyz"].astype(np.float64), c["offset"].astype(np.float64)
            assert np.array_equal(_as(c["offset"], dtype), c["offset"])
            assert ((x + o)[0::2] == 0).all()
            s32 = (c["xyz"] + c["offset"]).astype(np.float64)
            assert (s32[1::2] != (x + o)[1::2]).all()                                # the float32 addition rounds
            r = reference(c)
            assert np.array_equal(r["ins_off"].view(np.uint32), (c["xyz"] + c["offset"])[r["ins_ind"]].view(np.uint32))
            if dtype != "fp32":
                assert (_as(s32[1::2], dtype) != s32[1::2]).all()                    # and is not a value of the 16-bit type
        out.append(_case(name, lab, 3, bases(lab, 3, {0, 1, 2}), dtype, ld, "x + o rounds in float32 (odd rows), o = -x (even rows)",
                         pre, "offset arithmetic in " + dtype, xyz=xyz, offset=off))
    return out


@functools.lru_cache(maxsize=None)
def _all():
    cases = [_n_case(j, n) for j, n in enumerate(N_VALUES)] + _label_cases() + _offset_cases()
    return {c["name"]: c for c in cases}


def case(name):
    return _all()[name]


NAMES = tuple(_all())
CHAINED = ("N_n1025", "L_runs256", "L_cls32_all")            # also run behind pbn_sem_argmax_table and stage_ops.select_points
