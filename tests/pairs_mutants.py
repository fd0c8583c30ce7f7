"""A second statement of the rule-pair lists, written the way csrc/pairs.hip works -- a block of 256 rows, the [256 x 32-offset]
tile of the map, per column four ballots of 64 rows; a column-wise exclusive scan over the blocks in chunks of 64 blocks with a
running carry; seg_begin from the totals in chunks of 64 offsets with a running carry; the fill's slot (first + q) * seg + (pos -
q * seg); and for several maps the job table with its block and column prefixes -- with one switch per deliberate mistake.
With mutant=None it must equal tests/pairs_ref.py on every designed case of tests/pairs_cases.py: totals, the post-scan table,
seg_begin, in_idx, out_idx and seg_offset INCLUDING what stays unwritten (tests/test_pairs_cases_cpu.py).

Every buffer starts as a sentinel (SENT32 / SENT64) at the size the callers allocate (conv._pair_buffers); a write outside a buffer
is not made but sets `oob`, and a result with `oob` equals nothing.

How the twelve mistakes are stated
  scan_carry_dropped        run = chunk total instead of run += chunk total between 64-block chunks (prefixes and totals)
  scan_inclusive            table[b] <- pairs up to and including block b
  seg_begin_carry_dropped   the same slip between the 64-offset chunks of the seg_begin scan
  segments_floor            total / seg segments per offset instead of ceil
  slot_wrong_base           slot inside the segment taken as (pos - block's first position) % seg instead of pos % seg
  seg_offset_prev_at_multiple  every pair writes seg_offset of its segment, but the pair at an exact multiple of seg writes the
                            PREVIOUS offset (k - 1); in order of position the last writer wins, so a segment holding one pair is wrong
  tail_rows_counted         rows >= n of the last block read as input row 0 instead of -1
  src_gt_zero               pair test src > 0
  seg_begin_end_unpublished seg_begin[K] is not written (device forms)
  multi_empty_zero_blocks   an empty map gets zero blocks in the job table: no block publishes its seg_begin
  multi_job_gt              job of a block / column looked up with > instead of >=
  subrounds_reversed        the four ballots of a column walked 3, 2, 1, 0 in the fill
The host form (seg_start given) has no seg_begin scan: seg_begin_carry_dropped, segments_floor and seg_begin_end_unpublished
cannot touch it, the multi mistakes touch only the job table.  Nothing here turned out equivalent."""
import numpy as np

ROWS, KC, SCAN_CHUNK, SEG_CHUNK, MAX_K, MAX_JOBS = 256, 32, 64, 64, 512, 16
SENT32, SENT64 = 0x5A5A5A5A, 0x5A5A5A5A5A5A5A5A

MUTANTS = ("scan_carry_dropped", "scan_inclusive", "seg_begin_carry_dropped", "segments_floor", "slot_wrong_base",
           "seg_offset_prev_at_multiple", "tail_rows_counted", "src_gt_zero", "seg_begin_end_unpublished", "multi_empty_zero_blocks",
           "multi_job_gt", "subrounds_reversed")
EQUIVALENT = ()


def blocks_of(n):
    return -(-n // ROWS) if n > 0 else 0


class Job(object):
    """One map and the buffers of its lists, all sentinel."""

    def __init__(self, nbr, seg, n_segments=None):
        self.nbr = np.asarray(nbr, np.int64)
        self.n, self.K = self.nbr.shape
        self.seg = seg
        cap = (self.n * self.K) // seg + self.K if n_segments is None else n_segments
        self.table = np.full((max(blocks_of(self.n), 1), self.K), SENT32, np.int64)
        self.totals = np.full(self.K, SENT32, np.int64)
        self.seg_begin = np.full(self.K + 1, SENT32, np.int64)
        self.in_idx = np.full(cap * seg, SENT32, np.int64)
        self.out_idx = np.full(cap * seg, SENT32, np.int64)
        self.seg_offset = np.full(cap, SENT64, np.int64)
        self.oob = False

    def put(self, arr, idx, val):
        idx, val = np.atleast_1d(idx), np.atleast_1d(val)
        ok = (idx >= 0) & (idx < arr.shape[0])
        if not ok.all():
            self.oob = True
        arr[idx[ok]] = val[ok] if val.shape == idx.shape else val

    def result(self):
        return dict(totals=self.totals, table=self.table, seg_begin=self.seg_begin, in_idx=self.in_idx, out_idx=self.out_idx,
                    seg_offset=self.seg_offset, oob=self.oob)


def _tile(job, blk, mutant):
    """The block's 256 rows of the map; rows past the map read as -1."""
    t = np.full((ROWS, job.K), 0 if mutant == "tail_rows_counted" else -1, np.int64)
    lo = blk * ROWS
    if lo < job.n:
        hi = min(lo + ROWS, job.n)
        t[:hi - lo] = job.nbr[lo:hi]
    return t


def _is_pair(src, mutant):
    return src > 0 if mutant == "src_gt_zero" else src >= 0


def count_body(job, blk, mutant):
    if blk >= job.table.shape[0]:
        job.oob = True
        return
    tile = _tile(job, blk, mutant)
    for k0 in range(0, job.K, KC):                              # the LDS tile
        for k in range(k0, min(k0 + KC, job.K)):
            cnt = 0
            for sub in range(ROWS // 64):                       # one ballot each
                cnt += int(_is_pair(tile[sub * 64:sub * 64 + 64, k], mutant).sum())
            job.table[blk, k] = cnt


def scan_body(job, k, n_blocks, mutant):
    if k >= job.K:
        job.oob = True
        return
    run = 0
    for b0 in range(0, n_blocks, SCAN_CHUNK):
        v = job.table[b0:min(b0 + SCAN_CHUNK, n_blocks), k].copy()
        inc = np.cumsum(v)
        job.table[b0:b0 + len(v), k] = run + inc - (0 if mutant == "scan_inclusive" else v)
        run = int(inc[-1]) if mutant == "scan_carry_dropped" else run + int(inc[-1])
    job.totals[k] = run


def _seg_begin(job, mutant):
    """What wave 0 of every fill block derives from the totals."""
    first = np.zeros(job.K, np.int64)
    run = 0
    for k0 in range(0, job.K, SEG_CHUNK):
        t = job.totals[k0:min(k0 + SEG_CHUNK, job.K)]
        v = t // job.seg if mutant == "segments_floor" else (t + job.seg - 1) // job.seg
        inc = np.cumsum(v)
        first[k0:k0 + len(v)] = run + inc - v
        run = int(inc[-1]) if mutant == "seg_begin_carry_dropped" else run + int(inc[-1])
    return first, run


def fill_body(job, blk, seg_start, mutant):
    seg = job.seg
    if seg_start is not None:
        first = np.asarray(seg_start, np.int64)
    else:
        first, end = _seg_begin(job, mutant)
        if blk == 0:
            job.seg_begin[:job.K] = first
            if mutant != "seg_begin_end_unpublished":
                job.seg_begin[job.K] = end
    if blk >= job.table.shape[0]:
        job.oob = True
        return
    tile = _tile(job, blk, mutant)
    subs = range(ROWS // 64)
    for k in range(job.K):
        block_first = pos0 = int(job.table[blk, k])
        for sub in (reversed(subs) if mutant == "subrounds_reversed" else subs):
            src = tile[sub * 64:sub * 64 + 64, k]
            m = _is_pair(src, mutant)
            lanes = np.nonzero(m)[0]
            if len(lanes):
                pos = pos0 + np.arange(len(lanes))               # lanes in front
                q = pos // seg
                within = (pos - block_first) % seg if mutant == "slot_wrong_base" else pos - q * seg
                slot = (first[k] + q) * seg + within
                job.put(job.in_idx, slot, src[lanes])
                job.put(job.out_idx, slot, blk * ROWS + sub * 64 + lanes)
                if mutant == "seg_offset_prev_at_multiple":
                    for p, s in zip(pos.tolist(), (first[k] + q).tolist()):
                        job.put(job.seg_offset, s, k - 1 if p % seg == 0 else k)
                else:
                    head = pos == q * seg
                    job.put(job.seg_offset, (first[k] + q)[head], k)
            pos0 += len(lanes)


# ---- one map: pbn_rulebook_pair_counts, then one of the fills -----------------------------------------------------------------
def counts(job, mutant=None):
    if job.n == 0:
        job.totals[:] = 0
        return
    nb = blocks_of(job.n)
    for blk in range(nb):
        count_body(job, blk, mutant)
    for k in range(job.K):
        scan_body(job, k, nb, mutant)


def build_dev(nbr, seg, mutant=None):
    """pbn_rulebook_pair_counts + pbn_rulebook_pair_fill_dev; K > 512: the fill refuses, only the counts are there."""
    job = Job(nbr, seg)
    counts(job, mutant)
    if job.K <= MAX_K:
        for blk in range(max(blocks_of(job.n), 1)):
            fill_body(job, blk, None, mutant)
    return job.result()


def build_host(nbr, seg, seg_start, n_segments, mutant=None):
    """pbn_rulebook_pair_counts + pbn_rulebook_pair_fill with the caller's seg_start [K] and n_segments."""
    job = Job(nbr, seg, n_segments)
    counts(job, mutant)
    if job.K <= MAX_K:                                           # beyond: refused before anything is written
        job.in_idx[:] = -1
        job.out_idx[:] = -1
        job.seg_offset[:] = 0
        for blk in range(blocks_of(job.n)):
            fill_body(job, blk, seg_start, mutant)
    return job.result()


# ---- several maps: the job table ------------------------------------------------------------------------------------------------
def _job_of(begin, n_jobs, b, mutant):
    j = 0
    while j + 1 < n_jobs and (b > begin[j + 1] if mutant == "multi_job_gt" else b >= begin[j + 1]):
        j += 1
    return j


def build_multi(maps, seg, mutant=None):
    """pbn_rulebook_pairs_multi of up to 16 maps: three launches over the blocks, the columns and the blocks again."""
    assert 1 <= len(maps) <= MAX_JOBS
    jobs = [Job(m, seg) for m in maps]
    block_begin, col_begin = [0], [0]
    for j in jobs:
        nb = blocks_of(j.n)
        block_begin.append(block_begin[-1] + (nb if mutant == "multi_empty_zero_blocks" else max(nb, 1)))
        col_begin.append(col_begin[-1] + j.K)
    nj = len(jobs)
    for b in range(block_begin[-1]):
        j = _job_of(block_begin, nj, b, mutant)
        count_body(jobs[j], b - block_begin[j], mutant)
    for c in range(col_begin[-1]):
        j = _job_of(col_begin, nj, c, mutant)
        scan_body(jobs[j], c - col_begin[j], block_begin[j + 1] - block_begin[j], mutant)
    for b in range(block_begin[-1]):
        j = _job_of(block_begin, nj, b, mutant)
        fill_body(jobs[j], b - block_begin[j], None, mutant)
    return [j.result() for j in jobs]


def build_groups(maps, seg, mutant=None):
    """conv.rulebook_pairs_dev_multi: groups of 16 maps, one pbn_rulebook_pairs_multi each."""
    out = []
    for i in range(0, len(maps), MAX_JOBS):
        out += build_multi(maps[i:i + MAX_JOBS], seg, mutant)
    return out


# ---- the reference in the same shape ------------------------------------------------------------------------------------------
def reference_dev(nbr, seg):
    import pairs_ref as PR
    nbr = np.asarray(nbr)
    n, k = nbr.shape
    ref = PR.pair_lists(nbr, seg)
    table = PR.block_prefix(nbr, ROWS)
    if n == 0:
        table = np.full((1, k), SENT32, np.int64)            # pbn_rulebook_pair_counts of an empty map zeroes the totals only
    if k > MAX_K:
        cap = PR.worst_case_segments(n, k, seg)
        return dict(totals=ref["totals"], table=table, seg_begin=np.full(k + 1, SENT32, np.int64),
                    in_idx=np.full(cap * seg, SENT32, np.int64), out_idx=np.full(cap * seg, SENT32, np.int64),
                    seg_offset=np.full(cap, SENT64, np.int64), oob=False)
    i, o, s = PR.device_layout(ref, PR.worst_case_segments(n, k, seg), SENT32, SENT64)
    return dict(totals=ref["totals"], table=table, seg_begin=ref["seg_begin"], in_idx=i.astype(np.int64), out_idx=o.astype(np.int64),
                seg_offset=s, oob=False)


def reference_multi(nbr, seg):
    """As reference_dev, but an empty map's one block went through the count and the scan: its table row is zero."""
    r = reference_dev(nbr, seg)
    if np.asarray(nbr).shape[0] == 0:
        r["table"] = np.zeros_like(r["table"])
    return r


def reference_host(nbr, seg, surplus=0):
    """-> (result, seg_start [K], n_segments) with `surplus` segments more than the map needs."""
    import pairs_ref as PR
    nbr = np.asarray(nbr)
    n, k = nbr.shape
    ref = PR.pair_lists(nbr, seg)
    n_seg = int(ref["seg_begin"][k]) + surplus
    table = PR.block_prefix(nbr, ROWS) if n else np.full((1, k), SENT32, np.int64)
    if k > MAX_K:
        i, o, s = (np.full(n_seg * seg, SENT32, np.int64), np.full(n_seg * seg, SENT32, np.int64), np.full(n_seg, SENT64, np.int64))
    else:
        i, o, s = PR.host_layout(ref, n_seg)
    return (dict(totals=ref["totals"], table=table, seg_begin=np.full(k + 1, SENT32, np.int64), in_idx=np.asarray(i, np.int64),
                 out_idx=np.asarray(o, np.int64), seg_offset=np.asarray(s, np.int64), oob=False), ref["seg_begin"][:k], n_seg)


KEYS = ("totals", "table", "seg_begin", "in_idx", "out_idx", "seg_offset")


def same(a, b):
    return not a["oob"] and not b["oob"] and all(a[k].shape == b[k].shape and np.array_equal(a[k], b[k]) for k in KEYS)
