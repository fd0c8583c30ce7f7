"""A plain numpy restatement of pbn_scene_summary's contract (include/pbnet_hip.h): float32 additions in copy order,
first-maximum argmax, np.rint fixed point, float64 division.  No test logic here; tests/test_scene_summary_ref_cpu.py checks it
against a brute-force loop, the GPU tests compare the kernels with it."""
import numpy as np

NO_LABEL = -100
STATUS_CLASS, STATUS_COORD, STATUS_INSTANCE = 2, 4, 8


def first_max(s):
    """Per row the first k with s[k] > everything before it, starting from -inf: a NaN never wins, an all-NaN row gives 0."""
    n, k = s.shape
    best = np.full(n, -np.inf, dtype=np.float32)
    arg = np.zeros(n, dtype=np.int32)
    for c in range(k):
        v = s[:, c]
        with np.errstate(invalid="ignore"):
            m = v > best
        arg[m] = c
        best[m] = v[m]
    return arg


def fold_labels(scores, point_starts, copies):
    """scores float32 [copies * N, K] (already widened) -> int32 [N].  Scene j's copies lie at rows copies * start[j] + c * n_j + i."""
    scores = np.asarray(scores, dtype=np.float32)
    out = np.zeros(int(point_starts[-1]), dtype=np.int32)
    for j in range(len(point_starts) - 1):
        p0, p1 = int(point_starts[j]), int(point_starts[j + 1])
        n = p1 - p0
        if n == 0:
            continue
        blk = scores[copies * p0:copies * p1].reshape(copies, n, -1)
        s = blk[0].copy()
        with np.errstate(invalid="ignore", over="ignore"):
            for c in range(1, copies):
                s = (s + blk[c]).astype(np.float32)
        out[p0:p1] = first_max(s)
    return out


def kept_counts(n_keep, n_prop):
    """The clamp of the kernels: the scenes' counts are cut so that they sum to at most P."""
    out, total = [], 0
    for k in n_keep:
        k = max(0, min(int(k), n_prop - total))
        out.append(k)
        total += k
    return out


def summarize(scores, point_starts, copies, point_instance, n_keep, n_prop, xyz, label_table):
    """dict(sem_fold i32[N], class_vote i64[B, P], class_points i32[B, P], box f32[B, P, 6] | None, centroid f32[B, P, 3] | None,
    status i32[B])."""
    b, p = len(point_starts) - 1, int(n_prop)
    n_cls = int(np.asarray(scores).shape[1])
    sem_fold = fold_labels(scores, point_starts, copies)
    label_table = np.asarray(label_table, dtype=np.int64)
    vote = np.full((b, p), -1, dtype=np.int64)
    points = np.zeros((b, p), dtype=np.int32)
    status = np.zeros(b, dtype=np.int32)
    box = cen = None
    if xyz is not None:
        xyz = np.asarray(xyz, dtype=np.float32)
        box, cen = np.zeros((b, p, 6), dtype=np.float32), np.zeros((b, p, 3), dtype=np.float32)
    kept = kept_counts(n_keep, p) if p > 0 else [0] * b
    for j in range(b):
        p0, p1 = int(point_starts[j]), int(point_starts[j + 1])
        nk = kept[j]
        inst = (np.asarray(point_instance[p0:p1], dtype=np.int64) if p > 0 else np.full(p1 - p0, NO_LABEL, dtype=np.int64))
        ok = np.ones(p1 - p0, dtype=bool)
        if xyz is not None:
            with np.errstate(invalid="ignore"):
                ok = (np.abs(xyz[p0:p1]) < np.float32(32768.0)).all(1)
            if not ok.all():
                status[j] |= STATUS_COORD
        bad = (inst != NO_LABEL) & ((inst < 0) | (inst >= nk))
        if bad.any():
            status[j] |= STATUS_INSTANCE
        member = (inst >= 0) & (inst < nk)
        if nk == 0:
            continue
        hist = np.bincount(inst[member] * n_cls + sem_fold[p0:p1][member], minlength=nk * n_cls).reshape(nk, n_cls)
        c_star = hist.argmax(1)                                         # first maximum: the lower class on a tie
        points[j, :nk] = hist[np.arange(nk), c_star]
        inside = c_star < label_table.shape[0]
        vote[j, :nk][inside] = label_table[c_star[inside]]
        if not inside.all():
            status[j] |= STATUS_CLASS
        if xyz is None:
            continue
        use = member & ok
        ids, pts = inst[use], xyz[p0:p1][use]
        lo = np.full((nk, 3), np.inf, dtype=np.float32)
        hi = np.full((nk, 3), -np.inf, dtype=np.float32)
        np.minimum.at(lo, ids, pts)
        np.maximum.at(hi, ids, pts)
        q = np.rint(pts * np.float32(65536.0)).astype(np.int64)
        total = np.zeros((nk, 3), dtype=np.int64)
        np.add.at(total, ids, q)
        count = np.bincount(ids, minlength=nk)
        with np.errstate(invalid="ignore", divide="ignore"):
            centre = (total.astype(np.float64) / count.astype(np.float64)[:, None] / 65536.0).astype(np.float32)
        empty = count == 0
        lo[empty] = hi[empty] = centre[empty] = np.nan
        box[j, :nk, :3], box[j, :nk, 3:], cen[j, :nk] = lo, hi, centre
    return dict(sem_fold=sem_fold, class_vote=vote, class_points=points, box=box, centroid=cen, status=status)
