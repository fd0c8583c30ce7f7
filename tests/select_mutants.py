"""A second statement of the class-major selection, written the way k_select_points (csrc/front.hip) works -- a block of 1024
points whose base per class is class_base plus the block histograms in front; four waves of 256 consecutive points each, with a
per-wave class histogram; per wave four rounds of 64 lanes; per round one ballot per class present, the running position of class c
carried by lane c between the rounds -- with one switch per deliberate mistake.  With mutant=None it must equal tests/select_ref.py
on every designed case of tests/select_cases.py, written positions and unwritten ones (tests/test_select_cases_cpu.py).

Position of a point = class_base + blocks in front + waves in front + rounds in front (`run`) + lanes in front: five terms, and
  blocks_inclusive      the block's own histogram is added to its base
  waves_omitted         the waves in front are not added
  run_not_advanced      `run` stays where it was after a round
  lanes_le              lanes in front counted with <= (the lane counts itself)
  dropped_contributes   a dropped class keeps class_base + counts as its base (its points are written once that is >= 0)
  off_in_16bit          ins_off formed in the offsets' 16-bit type: T(x) + o rounded to T
  sem_of_leader         ins_sem takes the class of the round's first leader (its lowest valid lane)
  ld_ignored            offsets read with a leading dimension of 3
each miss one of them or one of the payloads.

EQUIVALENT
  tail_lane_counted     lanes with i >= n count as class 0 in the wave histogram, the ballots and `run`; they still write nothing.
A position is made of what lies IN FRONT of a point in (block, wave, round, lane) order, that order is the order of i, and every
tail lane lies behind every point: nobody's position reads what a tail lane added.  test_select_cases_cpu.py asserts the premise
(the walk order is the index order at every designed n) and that the mistake agrees with the reference on every case.  Had the tail
lane also WRITTEN, it would have read xyz past its end: that is no legal input to state."""
import numpy as np

import heads_ref as HR

F32 = np.float32
BLOCK, WAVES, ROUNDS, LANES = 1024, 4, 4, 64
SENT_I, SENT_BITS = -0x5A5A5A5B, 0x5A5A5A5A

MUTANTS = ("blocks_inclusive", "waves_omitted", "run_not_advanced", "lanes_le", "dropped_contributes", "off_in_16bit",
           "sem_of_leader", "ld_ignored")
EQUIVALENT = ("tail_lane_counted",)
SWITCHES = MUTANTS + EQUIVALENT
SLACK = 70                      # positions kept behind the reference's last one: a shift by a lane, a round's run or a class shows


def walk_order(n):
    """Index of the point each (block, wave, round, lane) slot reads, in walk order, -1 for a tail lane."""
    blocks = max(-(-n // BLOCK), 1)
    i = np.arange(blocks * BLOCK)
    return np.where(i < n, i, -1)                          # slot s reads point s: wave w of block b starts at 1024 b + 256 w


def select(sem_pred, class_base, hist, xyz, off_flat, ld_off, dtype, capacity, mutant=None):
    """off_flat float32 [n * ld_off]: the offsets' buffer as the kernel sees it, padding columns included."""
    sem_pred = np.asarray(sem_pred, np.int64)
    n, n_cls = sem_pred.shape[0], len(class_base)
    out = dict(ins_ind=np.full(capacity, SENT_I, np.int64), ins_sem=np.full(capacity, SENT_I, np.int64),
               ins_orig=np.full((capacity, 3), SENT_BITS, np.uint32), ins_off=np.full((capacity, 3), SENT_BITS, np.uint32), oob=False)
    ld = 3 if mutant == "ld_ignored" else ld_off
    for blk in range(-(-n // BLOCK)):
        s_base = np.zeros(n_cls, np.int64)
        for c in range(n_cls):
            t = int(class_base[c])
            if t >= 0 or mutant == "dropped_contributes":
                for b in range(blk + 1 if mutant == "blocks_inclusive" else blk):
                    t += int(hist[b][c])
            else:
                t = -(1 << 30)
            s_base[c] = t
        cls = np.full((WAVES, ROUNDS, LANES), -1, np.int64)
        s_wave = np.zeros((WAVES, n_cls), np.int64)
        for w in range(WAVES):
            for k in range(ROUNDS):
                for lane in range(LANES):
                    i = blk * BLOCK + w * (BLOCK // WAVES) + k * LANES + lane
                    c = int(sem_pred[i]) if i < n else (0 if mutant == "tail_lane_counted" else -1)
                    cls[w, k, lane] = c
                    if c >= 0:
                        s_wave[w, c] += 1
        for w in range(WAVES):
            run = s_base.copy()                                 # lane c owns class c
            if mutant != "waves_omitted":
                for w2 in range(w):
                    run += s_wave[w2]
            for k in range(ROUNDS):
                c = cls[w, k]
                pos = np.full(LANES, -1, np.int64)
                todo = c >= 0
                first_leader = int(c[np.argmax(todo)]) if todo.any() else -1
                while todo.any():
                    lc = int(c[np.argmax(todo)])                # the lowest lane still to do leads
                    m = c == lc
                    start = int(run[lc])
                    rank = np.cumsum(m) - (0 if mutant == "lanes_le" else m)
                    if start >= 0:
                        pos[m] = start + rank[m]
                    if run[lc] >= 0 and mutant != "run_not_advanced":
                        run[lc] += int(m.sum())
                    todo &= ~m
                for lane in np.nonzero(pos >= 0)[0].tolist():
                    i = blk * BLOCK + w * (BLOCK // WAVES) + k * LANES + lane
                    if i >= n:
                        continue                                # only tail_lane_counted gets here: counted, never written
                    p = int(pos[lane])
                    if p >= capacity:
                        out["oob"] = True
                        continue
                    x = xyz[i].astype(F32)
                    o = off_flat[i * ld:i * ld + 3].astype(F32)
                    if mutant == "off_in_16bit" and dtype != "fp32":
                        s = HR.round_to(HR.round_to(x.astype(np.float64), dtype) + o.astype(np.float64), dtype).astype(F32)
                    else:
                        s = x + o
                    out["ins_ind"][p] = i
                    out["ins_sem"][p] = first_leader if mutant == "sem_of_leader" else int(c[lane])
                    out["ins_orig"][p] = x.view(np.uint32)
                    out["ins_off"][p] = s.view(np.uint32)
    return out


def reference(ref, capacity):
    """select_ref.select_points' result in the same shape: the sentinel wherever nothing is written."""
    out = dict(ins_ind=np.full(capacity, SENT_I, np.int64), ins_sem=np.full(capacity, SENT_I, np.int64),
               ins_orig=np.full((capacity, 3), SENT_BITS, np.uint32), ins_off=np.full((capacity, 3), SENT_BITS, np.uint32), oob=False)
    w = ref["written"]
    m = len(w)
    assert capacity >= m
    out["ins_ind"][:m][w] = ref["ins_ind"][w]
    out["ins_sem"][:m][w] = ref["ins_sem"][w]
    out["ins_orig"][:m][w] = ref["ins_orig"].view(np.uint32)[w]
    out["ins_off"][:m][w] = ref["ins_off"].view(np.uint32)[w]
    return out


KEYS = ("ins_ind", "ins_sem", "ins_orig", "ins_off")


def same(a, b):
    return not a["oob"] and not b["oob"] and all(np.array_equal(a[k], b[k]) for k in KEYS)
