"""Host reference of the offset-major rule-pair lists (csrc/pairs.hip: pbn_rulebook_pair_counts, _pair_fill, _pair_fill_dev,
pbn_rulebook_pairs_multi), written from the contract in include/pbnet_hip.h and the header comment of pairs.hip.  Numpy, explicit
loops, no knowledge of blocks, waves, tiles or chunks.

The contract as this file reads it
  * nbr int32 [n, K] is an output-stationary map: nbr[o, k] >= 0 names the input row that reaches output row o through offset k.
    EVERY negative value is "no pair" (-1 is what the map kernels write; -2 or INT_MIN mean the same).
  * The pairs of offset k are (nbr[o, k], o) for the rows o with a pair, output rows ascending.  totals[k] is their number.
  * Offset k owns ceil(totals[k] / seg) consecutive segments of `seg` slots; seg_begin[k] is its first segment, seg_begin[K] the
    number of segments.  Pair p of offset k sits in slot seg_begin[k] * seg + p.  seg_offset[s] = the offset segment s belongs to.
  * Host fill (pbn_rulebook_pair_fill): the caller passes seg_begin[:K] and n_segments >= seg_begin[K]; all n_segments * seg slots
    are written, -1 where no pair sits; seg_offset of a segment no offset owns (a surplus segment) is 0.
  * Device fill (pbn_rulebook_pair_fill_dev, pbn_rulebook_pairs_multi): seg_begin [K + 1] is an output; the slots behind an offset's
    count, and everything from segment seg_begin[K] on, are NOT written.
The per-block table that pbn_rulebook_pair_counts leaves for the fill is part of the ABI (the caller carries it from one call to
the next): block_prefix() states it as "pairs of column k in the rows in front of the block", for whatever block height."""
import numpy as np

I32 = np.int32


def pair_lists(nbr, seg):
    """totals int64 [K], seg_begin int64 [K + 1], pairs: per offset an int64 [totals[k], 2] array of (in, out) rows."""
    nbr = np.asarray(nbr)
    n, n_off = nbr.shape
    assert seg >= 1
    pairs, totals = [], np.zeros(n_off, np.int64)
    for k in range(n_off):
        col = nbr[:, k].tolist()
        lst = []
        for o in range(n):
            if col[o] >= 0:
                lst.append((col[o], o))
        pairs.append(np.array(lst, np.int64).reshape(-1, 2))
        totals[k] = len(lst)
    seg_begin = np.zeros(n_off + 1, np.int64)
    for k in range(n_off):
        seg_begin[k + 1] = seg_begin[k] + (totals[k] + seg - 1) // seg            # ceil
    return dict(totals=totals, seg_begin=seg_begin, pairs=pairs, seg=seg, n=n, n_offsets=n_off)


def host_layout(ref, n_segments=None):
    """in_idx, out_idx int32 [n_segments * seg] and seg_offset int64 [n_segments] as pbn_rulebook_pair_fill leaves them."""
    seg, n_off = ref["seg"], ref["n_offsets"]
    used = int(ref["seg_begin"][n_off])
    n_segments = used if n_segments is None else n_segments
    assert n_segments >= used
    in_idx = np.full(n_segments * seg, -1, I32)
    out_idx = np.full(n_segments * seg, -1, I32)
    seg_offset = np.zeros(n_segments, np.int64)
    for k in range(n_off):
        base = int(ref["seg_begin"][k]) * seg
        for p, (i, o) in enumerate(ref["pairs"][k].tolist()):
            in_idx[base + p], out_idx[base + p] = i, o
        for s in range(int(ref["seg_begin"][k]), int(ref["seg_begin"][k + 1])):
            seg_offset[s] = k
    return in_idx, out_idx, seg_offset


def device_layout(ref, capacity_segments, fill32, fill64):
    """The same three arrays at the caller's capacity as pbn_rulebook_pair_fill_dev leaves them when they held fill32 / fill64
    before: only the slots below each offset's count and the segments below seg_begin[K] are written."""
    seg, n_off = ref["seg"], ref["n_offsets"]
    assert capacity_segments >= int(ref["seg_begin"][n_off])
    in_idx = np.full(capacity_segments * seg, fill32, I32)
    out_idx = np.full(capacity_segments * seg, fill32, I32)
    seg_offset = np.full(capacity_segments, fill64, np.int64)
    for k in range(n_off):
        base = int(ref["seg_begin"][k]) * seg
        for p, (i, o) in enumerate(ref["pairs"][k].tolist()):
            in_idx[base + p], out_idx[base + p] = i, o
        for s in range(int(ref["seg_begin"][k]), int(ref["seg_begin"][k + 1])):
            seg_offset[s] = k
    return in_idx, out_idx, seg_offset


def worst_case_segments(n, n_offsets, seg):
    """What the device form's lists must hold (include/pbnet_hip.h): n * K / seg + K segments.  It bounds every map:
    sum ceil(t_k / seg) <= sum floor(t_k / seg) + K <= floor(sum t_k / seg) + K <= n * K // seg + K."""
    return (n * n_offsets) // seg + n_offsets


def block_prefix(nbr, rows_per_block):
    """table int64 [max(blocks, 1), K]: the pairs of column k in the rows before the block's first row.  An empty map keeps one
    (zero) row: the multi launch gives it one block."""
    nbr = np.asarray(nbr)
    n, n_off = nbr.shape
    blocks = -(-n // rows_per_block)
    table = np.zeros((max(blocks, 1), n_off), np.int64)
    for k in range(n_off):
        col = nbr[:, k].tolist()
        seen = 0
        for o in range(n):
            if o % rows_per_block == 0:
                table[o // rows_per_block, k] = seen
            if col[o] >= 0:
                seen += 1
    return table
