"""A second statement of the shared device primitives, written the way the kernels work -- tiles of SCAN_TILE with per-tile
sums and a carried prefix (k_scan_block_sums / k_scan_sums / k_scan_apply), a walk back over windows of 64 predecessors
(k_scan_chained), head / 16-byte body / tail with two tables that flush when full (fill_ranges), three counting passes over
11-bit digits with per-tile counts, a prefix over the tiles and the caller's histogram (radix_sort_u32) -- with one switch per
deliberate mistake.  With mutant=None it must equal tests/prims_ref.py on every designed case; a mutant that equals it on every
case shows that a case is missing (tests/test_prims_cases_cpu.py).

What the model assumes about the machine, where a mistake would otherwise have no effect in numpy: a 16-byte vector store
to an address that is not a multiple of 16 lands on the multiple below it."""
import numpy as np

import prims_cases as PC

SCAN_MUTANTS = ("sums_carry_dropped", "total_from_tile_of_n", "inplace_reads_written", "lookback_stops_early")
FILL_MUTANTS = ("fill_tail_skipped", "fill_head_p_and_15", "fill_flush_forgets_bytes")
SORT_MUTANTS = ("ties_reversed", "top_digit_wrong_shift", "hist_not_cleared")
MUTANTS = SCAN_MUTANTS + FILL_MUTANTS + SORT_MUTANTS


def _wrap32(a):
    return np.asarray(a, np.int64).astype(np.int32)      # two's complement, as the device's int


def _excl(a, axis=-1):
    return np.cumsum(a, axis=axis) - a


# ---- scans -----------------------------------------------------------------------------------------------------------------
def scan(x, chained, alias=False, mutant=None):
    """(out int32 [n], total int): `total` is what a non-null total pointer holds afterwards (zero before the launch in the
    chained form, written by the n <= 0 path's fill in the other)."""
    assert mutant is None or mutant in SCAN_MUTANTS
    tile, threads, items = PC.SCAN_TILE, PC.SCAN_THREADS, PC.SCAN_TILE // PC.SCAN_THREADS
    x = np.asarray(x, np.int64)
    n = len(x)
    if n == 0:
        return np.zeros(0, np.int32), 0
    nb = -(-n // tile)
    tiles = np.zeros(nb * tile, np.int64)
    tiles[:n] = x
    tiles = tiles.reshape(nb, tile)
    seen = tiles                                         # what the pass that writes `out` loads
    if alias and mutant == "inplace_reads_written":      # the items after a thread's first are loaded when out already holds
        right = (_excl(tiles, 1) + _excl(tiles.sum(1))[:, None]).reshape(-1)              # ... the prefix, not the input
        k = np.arange(nb * tile)
        seen = np.where((k % items != 0) & (k < n), right, tiles.reshape(-1)).reshape(nb, tile)
    if not chained:
        sums = tiles.sum(1)                              # k_scan_block_sums reads the input before anything is written
        pref = np.zeros(nb, np.int64)
        carry = 0
        for base in range(0, nb, threads):               # k_scan_sums: one workgroup, SCAN_THREADS sums per trip
            chunk = sums[base:base + threads]
            pref[base:base + threads] = _excl(chunk) + (0 if mutant == "sums_carry_dropped" and base else carry)
            carry += int(chunk.sum())
        total = carry
    else:
        tot = seen.sum(1)                                # the one pass loads once: sums and outputs see the same values
        incl = np.cumsum(tot)
        pref = incl - tot                                # every window of 64 back to workgroup 0, whose word is a prefix at once
        if mutant == "lookback_stops_early":             # the last window a walk needs is not read (walks of two and more)
            b = np.arange(nb)
            windows = (b + PC.SCAN_WINDOW - 1) // PC.SCAN_WINDOW
            last_end = b - 1 - PC.SCAN_WINDOW * (windows - 1)          # workgroups 0..last_end make up that window
            pref = pref - np.where(windows >= 2, incl[np.clip(last_end, 0, nb - 1)], 0)
        writer = n // tile if mutant == "total_from_tile_of_n" else nb - 1      # the workgroup that holds element n, were the grid
        total = int(pref[writer] + tot[writer]) if writer < nb else 0           # ... one longer: not launched at whole tiles
    out = (_excl(seen, 1) + pref[:, None]).reshape(-1)[:n]
    return _wrap32(out), int(_wrap32(total))


# ---- fill ------------------------------------------------------------------------------------------------------------------
def fill(buf, ranges, mutant=None):
    assert mutant is None or mutant in FILL_MUTANTS
    out = np.array(buf, np.uint8, copy=True)
    vec, byt = [], []                                    # the two tables of one launch

    def launch(forget_bytes=False):
        if not forget_bytes:
            for p, length, v in byt:
                out[p:p + length] = v
        for p, nvec, v in vec:
            p &= ~15                                     # a vector store ignores the low address bits
            out[p:p + 16 * nvec] = v
        del vec[:], byt[:]

    def add_bytes(p, length, v):
        if length:
            if len(byt) == PC.FILL_BYTE_SLOTS:
                launch()
            byt.append((p, length, v))

    for off, length, v in ranges:
        if off is None or length == 0:
            continue
        p = off                                          # the buffer itself is 16-byte aligned (the GPU test asserts it)
        if length < PC.FILL_SMALL:
            add_bytes(p, length, v)
            continue
        head = (p & 15) if mutant == "fill_head_p_and_15" else (16 - (p & 15)) & 15
        if head:
            add_bytes(p, head, v)
            p += head
            length -= head
        tail = length & 15
        if length >= 16:
            if len(vec) == PC.FILL_VEC_SLOTS:
                launch(forget_bytes=mutant == "fill_flush_forgets_bytes")
            vec.append((p, length // 16, v))
        if tail and mutant != "fill_tail_skipped":
            add_bytes(p + (length - tail), tail, v)
    launch()
    return out


# ---- sort ------------------------------------------------------------------------------------------------------------------
DIGIT_BITS, PASSES = 11, 3
RADIX = 1 << DIGIT_BITS
KEY_CANARY, VAL_CANARY = np.uint64(0xdeadbeefdeadbeef), np.int32(-77)


def _digit(keys, p, mutant):
    if p == 2 and mutant == "top_digit_wrong_shift":     # ten bits, taken one position too low
        return ((keys >> np.uint64(21)) & np.uint64(1023)).astype(np.int64)
    return ((keys >> np.uint64(DIGIT_BITS * p)) & np.uint64(RADIX - 1)).astype(np.int64)


def sort(keys, vals, mutant=None):
    """(keys_out uint64 [n], vals_out int32 [n]) of the SECOND call into one workspace; with a histogram that every call
    clears it is the first call's."""
    assert mutant is None or mutant in SORT_MUTANTS
    tile = PC.sort_tile()
    keys = np.asarray(keys, np.uint32).astype(np.uint64)
    vals = np.asarray(vals, np.int32)
    n = len(keys)
    if n == 0:
        return keys, vals
    ghist = np.zeros((PASSES, RADIX), np.int64)
    key_b, val_b = np.full(n, KEY_CANARY), np.full(n, VAL_CANARY)
    for call in range(2):
        if call == 0 or mutant != "hist_not_cleared":
            ghist[:] = 0
        for p in range(PASSES):                          # the keys kernel: every key into the three histograms
            ghist[p] += np.bincount(_digit(keys, p, mutant), minlength=RADIX)
        bufs = [(keys.copy(), vals.copy()), (key_b, val_b)]
        for p in range(PASSES):
            (kin, vin), (kout, vout) = bufs[p & 1], bufs[1 - (p & 1)]
            d = _digit(kin, p, mutant)
            blk = np.arange(n) // tile
            nb = int(blk[-1]) + 1
            cell = blk * RADIX + d                       # (workgroup, bin)
            cnt = np.bincount(cell, minlength=nb * RADIX).reshape(nb, RADIX)
            order = np.argsort(cell, kind="stable")      # rank of a key among its workgroup's keys of the same bin, in input order
            rank = np.empty(n, np.int64)
            rank[order] = np.arange(n) - _excl(cnt.reshape(-1))[cell[order]]
            if mutant == "ties_reversed":
                rank = cnt[blk, d] - 1 - rank
            pos = _excl(ghist[p])[d] + _excl(cnt, 0)[blk, d] + rank     # bin start + the workgroups in front + own rank
            ok = pos < n                                 # (a position outside the buffers is not modelled)
            kout[pos[ok]] = kin[ok]
            vout[pos[ok]] = vin[ok]
        key_b, val_b = bufs[1]
    return key_b, val_b
