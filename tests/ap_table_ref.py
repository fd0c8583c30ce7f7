"""numpy restatement of the device AP table (include/pbnet_hip.h, pbn_ap_table_*), written from that contract and from
tools/eval.py:27-190, working on the int32 words of association logs directly -- no SceneMatches, none of pbnet_amd.evaluate's
functions.  `evaluate_logs` returns what the device leaves: the entry multiset of every cell, the cell counts, the classes'
flags, the directory and the AP cells."""
import numpy as np

MAGIC, HEADER = 0x41504c47, 8
CLASS_IDS = (3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 14, 16, 24, 28, 33, 34, 36, 39)
OVERLAPS = np.append(np.arange(0.5, 0.95, 0.05), 0.25)          # the doubles themselves: 0.6000000000000001 is one of them
MIN_REGION = 100


def walk(words):
    """[(offset, tag, status, n_keep, n_gt)] of the whole records in order, and the word at which the walk stopped (None = at the
    end of the log)."""
    words = np.asarray(words, np.int32).reshape(-1)
    pos, end, out = 0, int(words.shape[0]), []
    while pos < end:
        if end - pos < HEADER or int(words[pos]) != MAGIC:
            return out, pos
        tag, nk, ng, _, status, size = (int(v) for v in words[pos + 1:pos + 7])
        if nk < 0 or ng < 0 or size != HEADER + (2 * ng + 2 * nk + nk * ng if nk else 0) or pos + size > end:
            return out, pos
        out.append((pos, tag, status, nk, ng))
        pos += size
    return out, None


def class_index(value, class_ids):
    return class_ids.index(int(value)) if int(value) in class_ids else -1


def match_record(words, pos, nk, ng, class_ids, overlaps, min_region, entries, cells, flags):
    """One usable record into `entries[cell]` (lists of (score, true)), `cells[:, :, 2]` (hard_fn) and `flags`."""
    body = np.asarray(words[pos + HEADER:], np.int64)
    uid, gt_vert = body[:ng], body[ng:2 * ng]
    label = body[2 * ng:2 * ng + nk]
    conf = np.asarray(words[pos + HEADER + 2 * ng + nk:pos + HEADER + 2 * ng + 2 * nk], np.int32).view(np.float32)
    inter = body[2 * ng + 2 * nk:2 * ng + 2 * nk + nk * ng].reshape(nk, ng)
    col_class = [class_index(u // 1000, class_ids) if u >= 0 else -1 for u in uid]
    instance = [c >= 0 and u != 0 for c, u in zip(col_class, uid)]
    counts = [inst and u >= 1000 and v >= min_region for inst, u, v in zip(instance, uid, gt_vert)]
    vert = inter.sum(1)
    pred_class = [class_index(l, class_ids) for l in label]
    pred_class = [c if c >= 0 and vert[q] >= min_region else -1 for q, c in enumerate(pred_class)]
    for g in range(ng):
        if counts[g]:
            flags[0, col_class[g]] = 1
    for q in range(nk):
        if pred_class[q] >= 0:
            flags[1, pred_class[q]] = 1

    same = np.array([[instance[g] and pred_class[q] >= 0 and col_class[g] == pred_class[q] for g in range(ng)]
                     for q in range(nk)], bool).reshape(nk, ng)
    union = np.maximum(vert[:, None] + gt_vert[None, :] - inter, 1)
    iou = inter.astype(np.float64) / union.astype(np.float64)           # one IEEE division per pair

    for o, th in enumerate(overlaps):
        over = (same & (inter > 0) & (iou > th)).tolist()
        visited = [False] * nk
        for g in range(ng):
            if not counts[g]:
                continue
            best = None
            for q in range(nk):
                if visited[q] or not over[q][g]:
                    continue
                if best is None:
                    best, visited[q] = conf[q], True
                else:
                    entries[col_class[g]][o].append((min(best, conf[q]), 0))
                    best = max(best, conf[q])
            if best is None:
                cells[col_class[g], o, 2] += 1
            else:
                entries[col_class[g]][o].append((best, 1))
        for q in range(nk):
            c = pred_class[q]
            if c < 0 or any(over[q]):
                continue
            ignore = sum(int(inter[q, g]) for g in range(ng)
                         if col_class[g] < 0 or (instance[g] and col_class[g] == c and not counts[g]))
            if np.float64(ignore) / np.float64(int(vert[q])) <= th:
                entries[c][o].append((conf[q], 0))


def average_precision(cell_entries, hard_fn):
    """tools/eval.py:131-176 term by term; (area float64, distinct scores)."""
    order = sorted(cell_entries, key=lambda e: (np.float64(e[0]), e[1]))
    n, n_true = len(order), sum(t for _, t in order)
    first, below, seen = [], [], 0
    for p, (s, t) in enumerate(order):
        if p == 0 or s != order[p - 1][0]:
            first.append(p)
            below.append(seen)
        seen += t
    d = len(first)
    precision = np.ones(d + 1, np.float64)
    recall = np.zeros(d + 2, np.float64)                          # [d] = the artificial last point, [d + 1] the padding
    with np.errstate(invalid="ignore"):                           # a cell without ground truth divides 0 by 0; it is not used
        for k in range(d):
            tp = np.float64(n_true - below[k])
            fp = np.float64(n - first[k]) - tp
            fn = np.float64(below[k] + hard_fn)
            precision[k] = tp / (tp + fp)
            recall[k] = tp / (tp + fn)
    width = np.array([0.5 * recall[max(k - 1, 0)] + -0.5 * recall[k + 1] for k in range(d + 1)], np.float64)
    return np.dot(precision, width), d


def evaluate_logs(logs, class_ids=CLASS_IDS, overlaps=OVERLAPS, min_region=MIN_REGION):
    """`logs`: int32 word arrays, added in turn.  Returns dict(entries, cells, flags, directory, ap, malformed): entries[class]
    [overlap] = sorted (score bits, true) pairs, cells int32 [C, O, 4], flags int32 [2, C], directory int32 [R, 4] with offsets
    counted over the concatenation and tags shifted by the records before the log, ap float32 [1, C, O], malformed = the word
    of the first log that is not a sequence of whole records, or None."""
    class_ids = tuple(int(c) for c in class_ids)
    n_c, n_o = len(class_ids), len(overlaps)
    entries = [[[] for _ in range(n_o)] for _ in range(n_c)]
    cells, flags = np.zeros((n_c, n_o, 4), np.int32), np.zeros((2, n_c), np.int32)
    directory, malformed, words_before = [], None, 0
    for words in logs:
        words = np.asarray(words, np.int32).reshape(-1)
        records, stop = walk(words)
        tag_base = len(directory)
        for pos, tag, status, nk, ng in records:
            directory.append((words_before + pos, tag + tag_base, status, nk))
            if status == 0 and nk > 0:
                match_record(words, pos, nk, ng, class_ids, overlaps, min_region, entries, cells, flags)
        if stop is not None and malformed is None:
            malformed = stop
        words_before += int(words.shape[0])
    ap = np.zeros((1, n_c, n_o), np.float32)
    for c in range(n_c):
        for o in range(n_o):
            e = entries[c][o]
            cells[c, o, 0], cells[c, o, 1] = len(e), sum(t for _, t in e)
            area, cells[c, o, 3] = average_precision(e, int(cells[c, o, 2])) if e else (0.0, 0)
            ap[0, c, o] = area if flags[0, c] and flags[1, c] else (0.0 if flags[0, c] else np.nan)
            entries[c][o] = sorted((int(np.float32(s).view(np.int32)), t) for s, t in e)
    return dict(entries=entries, cells=cells, flags=flags, directory=np.array(directory, np.int32).reshape(-1, 4), ap=ap,
                malformed=malformed)
