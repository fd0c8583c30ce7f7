"""Designed inputs for the label vote (csrc/vote.hip), every one generated from a seed: nothing is committed as a fixture.
VOTE maps a name to (rows int32 [N], sem int32 [N], ins int32 [N] or None, m, n_classes); VOTE_RAISES to inputs
mesh.vote_labels must refuse; room_scan() is the annotated raw scan of the GPU tier."""
import functools

import numpy as np

import cloud_cases

I32 = np.int32
INS_TOP = (1 << 21) - 2                  # the largest instance id


def _case(rows, sem, ins, m, n_classes=20, seed=None):
    rows, sem = np.asarray(rows, I32), np.asarray(sem, I32)
    ins = None if ins is None else np.asarray(ins, I32)
    if seed is not None:                                     # a sensor does not deliver row by row
        p = np.random.default_rng(seed).permutation(rows.shape[0])
        rows, sem, ins = rows[p], sem[p], None if ins is None else ins[p]
    return rows, sem, ins, int(m), n_classes


def _pairs(groups):
    """[(row, sem, ins, count), ...] -> rows, sem, ins."""
    r = np.concatenate([np.full(c, g, I32) for g, _, _, c in groups])
    s = np.concatenate([np.full(c, v, I32) for _, v, _, c in groups])
    q = np.concatenate([np.full(c, v, I32) for _, _, v, c in groups])
    return r, s, q


def one_row(n):
    """n members in one row: four pairs in uneven shares, one unannotated."""
    rng = np.random.default_rng(900 + n)
    pick = rng.choice(4, n, p=[0.4, 0.3, 0.2, 0.1])
    sem = np.array([3, 3, 7, -100], I32)[pick]
    ins = np.array([12, 5, 40, -100], I32)[pick]
    return _case(np.zeros(n, I32), sem, ins, 1)


def walk300():
    """Row 1 holds 300 distinct pairs: 299 once or twice and one three times (the winner sits in the middle of the walk);
    rows 0 and 2 around it hold one pair each."""
    rng = np.random.default_rng(31)
    sem = rng.integers(0, 20, 300)
    ins = rng.permutation(5000)[:300]
    cnt = rng.integers(1, 3, 300)
    order = np.lexsort((ins, sem))
    cnt[order[150]] = 3
    groups = [(1, int(s), int(q), int(c)) for s, q, c in zip(sem, ins, cnt)] + [(0, 2, 9000, 4), (2, 19, 0, 5)]
    return _case(*_pairs(groups), 3, seed=32)


def border():
    """A cell on the border of three objects: (1, 5) x 3, (2, 6) x 2, (2, 7) x 2.  Jointly (1, 5) wins; separately the
    semantic vote goes to 2 (4 against 3) and the instance vote to 5: a pair that no raw point carries."""
    return _case(*_pairs([(0, 1, 5, 3), (0, 2, 6, 2), (0, 2, 7, 2), (1, 4, 8, 2)]), 2, seed=33)


def _vote():
    c = {"n0": _case(np.zeros(0), np.zeros(0), np.zeros(0), 5),
         "n1": _case([0], [4], [17], 1),
         "m0": _case([-1] * 4, [1, 2, 3, -100], [0, 1, 2, -100], 0)}
    for n in (63, 64, 65, 255, 256, 257):
        c["row%d" % n] = one_row(n)
    c["walk300"] = walk300()
    # ties: the lowest key wins; in tie3 the lowest key is neither the first nor the last met in index order
    c["tie2"] = _case(*_pairs([(0, 5, 9, 2), (0, 5, 3, 2), (0, 1, 1, 1), (1, 2, 2, 1)]), 2)
    c["tie3"] = _case(*_pairs([(0, 6, 1, 3), (0, 4, 8, 3), (0, 4, 2, 3), (0, 9, 9, 2), (1, 3, 3, 2), (1, 3, 4, 2)]), 2, seed=34)
    c["all_unannotated"] = _case(np.arange(40) % 3, np.full(40, -100), np.full(40, -1), 3)
    c["all_minus1"] = _case(np.full(30, -1), np.arange(30) % 20, np.arange(30), 4)
    c["gaps"] = _case(*_pairs([(1, 3, 4, 5), (1, 3, 6, 2), (4, 0, 0, 3), (7, 19, 11, 1)]), 10, seed=35)      # 8, 9: the last rows
    c["no_ins"] = _case(np.arange(50) % 4, (np.arange(50) * 7) % 5 - 1, None, 5, seed=36)
    c["extremes"] = _case(*_pairs([(0, 1022, INS_TOP, 3), (0, 1022, 0, 2), (1, 0, INS_TOP, 1), (1, -100, INS_TOP - 1, 1)]), 2, 1023,
                          seed=37)
    c["vanish"] = _case(*_pairs([(0, 0, -100, 3), (0, 2, 5, 2), (1, 1, -100, 4), (1, 3, 6, 3), (2, -100, -100, 2), (2, 2, 7, 1)]),
                        3, seed=38)
    # a tie between an annotated pair and the unannotated one: unannotated orders LAST, so the annotated pair wins
    c["unannotated_tie"] = _case(*_pairs([(0, -100, -100, 2), (0, 7, 3, 2), (1, 7, -100, 2), (1, 7, 4, 2)]), 2, seed=39)
    # the unannotated pair has the majority: it is a label like any other and wins
    c["unannotated_majority"] = _case(*_pairs([(0, -100, -100, 3), (0, 7, 3, 2), (1, 1, 1, 1)]), 2, seed=40)
    c["border"] = border()
    # five points routed nowhere carry (9, 9); counted into row 0 they would outvote its (2, 1) x 3
    c["minus1"] = _case(*_pairs([(-1, 9, 9, 5), (0, 2, 1, 3), (0, 9, 9, 1), (1, 4, 4, 2)]), 2, seed=41)
    # the winners' ids descend with the row: ascending-id compaction and first-appearance compaction disagree
    c["descending_ids"] = _case(*_pairs([(0, 3, 90, 2), (1, 3, 30, 2), (2, 5, 60, 2), (3, 5, -100, 1), (4, 3, 30, 1)]), 5, seed=42)
    return c


def _vote_raises():
    rows, sem, ins = np.arange(300, dtype=I32) % 4, np.arange(300, dtype=I32) % 20, np.arange(300, dtype=I32) % 9
    c = {}
    for name, which, value in (("sem_range", 1, 20), ("ins_range", 2, (1 << 21) - 1), ("row_high", 0, 4), ("row_low", 0, -2)):
        a = [rows.copy(), sem.copy(), ins.copy()]
        a[which][257] = value
        c[name] = (a[0], a[1], a[2], 4, 20)
    return c


VOTE = _vote()
VOTE_RAISES = _vote_raises()


@functools.lru_cache(maxsize=None)
def room_scan(copies=6, jitter=0.004, far=0.01):
    """cloud_cases.room(1) `copies` times over with `jitter` m of noise plus `far` x as many points scattered 10 to 30 m
    away, shuffled.  Labels follow the room's construction: floor (0, unannotated instance), the two walls (1, instances
    0 and 1), the cylinder (5, instance 7), the coincident extra point as its partner (floor); the far points are
    unannotated.  Returns xyz f32 [N, 3], sem int32 [N], ins int32 [N]."""
    base = cloud_cases.room(1).astype(np.float64)
    n = base.shape[0]
    sem = np.concatenate([np.full(1400, 0), np.full(1200, 1), np.full(n - 2601, 5), [0]]).astype(I32)
    ins = np.concatenate([np.full(1400, -100), np.full(600, 0), np.full(600, 1), np.full(n - 2601, 7), [-100]]).astype(I32)
    rng = np.random.default_rng(50)
    xyz = np.concatenate([base + rng.normal(scale=jitter, size=base.shape) for _ in range(copies)])
    n_far = int(far * xyz.shape[0])
    xyz = np.concatenate([xyz, rng.uniform(10.0, 30.0, (n_far, 3))]).astype(np.float32)
    sem = np.concatenate([np.tile(sem, copies), np.full(n_far, -100, I32)])
    ins = np.concatenate([np.tile(ins, copies), np.full(n_far, -100, I32)])
    p = rng.permutation(xyz.shape[0])
    return xyz[p], sem[p], ins[p]
