"""numpy restatement of csrc/vote.hip: an annotated raw scan's labels voted down to the kept points, in the terms of the
contract (include/pbnet_hip.h).  `vote` takes a `wrong` keyword naming ONE deliberate mistake; tests/test_vote_ref_cpu.py
shows which designed case tells each mistake from the contract.  `vote_loop` is the same by a Counter per row."""
import collections

import numpy as np

INS_BITS = 21
INS_NONE = (1 << INS_BITS) - 1           # the code of an unannotated instance; ids are 0 .. 2^21 - 2
MAX_CLASSES = 1023
NONE = -100
WRONG = ("ties_high", "unannotated_first", "unannotated_out", "separate", "minus_one_row0", "first_appearance", "ge")


def _check(rows, sem, ins, m, n_classes):
    if not 1 <= n_classes <= MAX_CLASSES:
        raise ValueError("n_classes must lie in 1..%d" % MAX_CLASSES)
    if sem.shape != rows.shape or (ins is not None and ins.shape != rows.shape):
        raise ValueError("rows, sem and ins must have one length")
    if sem.size and sem.max() >= n_classes:
        raise ValueError("a semantic label is n_classes or more")
    if ins is not None and ins.size and ins.max() >= INS_NONE:
        raise ValueError("an instance label is 2^21 - 1 or more")
    if rows.size and (rows.min() < -1 or rows.max() >= m):
        raise ValueError("a row lies outside [-1, m)")


def _winners(urow, ukey, cnt, m, wrong):
    """Per row the (key, count) of the winner among its distinct keys: the largest count, ties to the lowest key.  The
    input is in ascending (row, key) order.  Returns key int64 [m] (-1 = no voter) and votes int32 [m]."""
    key, votes = np.full(m, -1, np.int64), np.zeros(m, np.int32)
    if wrong == "ge":                                        # the device's walk over a row's runs, with >= for >
        best = {}
        for r, k, c in zip(urow.tolist(), ukey.tolist(), cnt.tolist()):
            if r not in best or c >= best[r][1]:
                best[r] = (k, c)
        for r, (k, c) in best.items():
            key[r], votes[r] = k, c
        return key, votes
    order = np.lexsort((-ukey if wrong == "ties_high" else ukey, -cnt, urow))
    first = np.ones(order.shape[0], bool)
    first[1:] = urow[order][1:] != urow[order][:-1]
    w = order[first]
    key[urow[w]], votes[urow[w]] = ukey[w], cnt[w]
    return key, votes


def _runs(rows, key):
    u, cnt = np.unique((rows << 31) | key, return_counts=True)
    return u >> 31, u & ((1 << 31) - 1), cnt


def compact_ids(ins_label, wrong=None):
    """The ids >= 0 renumbered 0..I'-1 in ascending old-id order: (renumbered int64 [m], old_id int64 [I'])."""
    ids = ins_label[ins_label >= 0]
    if wrong == "first_appearance":
        _, at = np.unique(ids, return_index=True)
        old = ids[np.sort(at)]
    else:
        old = np.unique(ids)
    new = np.full(int(old.max()) + 1 if old.size else 0, -1, np.int64)
    new[old] = np.arange(old.shape[0])
    out = ins_label.copy()
    out[ins_label >= 0] = new[ids]
    return out, old.astype(np.int64)


def vote(rows, sem, ins=None, m=None, n_classes=20, compact=True, wrong=None):
    """mesh.vote_labels on the host: dict of sem_label, ins_label (int64 [m]), votes, members (int32 [m]), old_id."""
    rows, sem = np.asarray(rows, np.int64).reshape(-1), np.asarray(sem, np.int64).reshape(-1)
    ins = None if ins is None else np.asarray(ins, np.int64).reshape(-1)
    m = int(m) if m is not None else (int(rows.max()) + 1 if rows.size else 0)
    _check(rows, sem, ins, m, n_classes)
    if wrong == "minus_one_row0" and m > 0:
        rows = np.maximum(rows, 0)
    q_raw = np.zeros_like(sem) if ins is None else ins
    if wrong == "unannotated_first":                         # the unannotated code below every label
        s, q = np.where(sem < 0, 0, sem + 1), np.where(q_raw < 0, 0, q_raw + 1)
    else:
        s, q = np.where(sem < 0, n_classes, sem), np.where(q_raw < 0, INS_NONE, q_raw)
    voter = rows >= 0
    members = np.bincount(rows[voter], minlength=m).astype(np.int32)[:m] if m else np.zeros(0, np.int32)
    if wrong == "unannotated_out":
        voter = voter & (sem >= 0) & (q_raw >= 0)
    r, s, q = rows[voter], s[voter], q[voter]
    if wrong == "separate":
        ks, votes = _winners(*_runs(r, s), m, None)
        kq, _ = _winners(*_runs(r, q), m, None)
        key = np.where(ks >= 0, (ks << INS_BITS) | kq, -1)
    else:
        key, votes = _winners(*_runs(r, (s << INS_BITS) | q), m, wrong)
    ws, wq = key >> INS_BITS, key & INS_NONE
    if wrong == "unannotated_first":
        sem_label, ins_label = np.where(ws == 0, NONE, ws - 1), np.where(wq == 0, NONE, wq - 1)
    else:
        sem_label, ins_label = np.where(ws == n_classes, NONE, ws), np.where(wq == INS_NONE, NONE, wq)
    sem_label, ins_label = np.where(key < 0, NONE, sem_label), np.where(key < 0, NONE, ins_label)
    old = np.zeros(0, np.int64)
    if compact:
        ins_label, old = compact_ids(ins_label, wrong)
    return {"sem_label": sem_label.astype(np.int64), "ins_label": ins_label.astype(np.int64), "votes": votes,
            "members": members, "old_id": old}


def vote_loop(rows, sem, ins=None, m=None, n_classes=20, compact=True):
    """The same with a Counter per row and plain Python integers."""
    rows, sem = [int(v) for v in rows], [int(v) for v in sem]
    ins = [0] * len(rows) if ins is None else [int(v) for v in ins]
    m = int(m) if m is not None else (max(rows) + 1 if rows else 0)
    counters = [collections.Counter() for _ in range(m)]
    for r, s, q in zip(rows, sem, ins):
        if r >= 0:
            counters[r][(n_classes if s < 0 else s, INS_NONE if q < 0 else q)] += 1
    out = {"sem_label": np.full(m, NONE, np.int64), "ins_label": np.full(m, NONE, np.int64), "votes": np.zeros(m, np.int32),
           "members": np.zeros(m, np.int32)}
    for t, c in enumerate(counters):
        if not c:
            continue
        top = max(c.values())
        s, q = min(pair for pair, v in c.items() if v == top)
        out["sem_label"][t] = NONE if s == n_classes else s
        out["ins_label"][t] = NONE if q == INS_NONE else q
        out["votes"][t], out["members"][t] = top, sum(c.values())
    old = sorted(set(int(v) for v in out["ins_label"] if v >= 0)) if compact else []
    if compact:
        new = {v: i for i, v in enumerate(old)}
        out["ins_label"] = np.array([new[int(v)] if v >= 0 else NONE for v in out["ins_label"]], np.int64).reshape(m)
    out["old_id"] = np.array(old, np.int64).reshape(-1)
    return out
