"""Plain-numpy restatement of the evaluation-time post-processing (eval_map.py:55-123, tools/mIOU.py:77-87,
tools/getins.py:72-98) under the DEVICE tie rule of the greedy NMS: survivors are ordered by score descending and, among
equal scores, the lower survivor index goes first.  numpy's `scores.argsort()[::-1]` leaves the order of ties to the sort of
the numpy build; this rule is the one csrc/post.hip's k_post_nms implements, and the yardstick of tests/test_post_device_gpu.py
wherever a recorded golden depends on the other order."""
import numpy as np

SEMANTIC_LABEL_IDX = np.array([1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 14, 16, 24, 28, 33, 34, 36, 39], np.int64)
STATUS_SUPERPOINT_RANGE = 1


def rank_by_counting(scores):
    """rank[i] = #{j : s[j] > s[i] or (s[j] == s[i] and j < i)}: position of survivor i in the walk order."""
    s = np.asarray(scores)
    idx = np.arange(s.shape[0])
    before = (s[None, :] > s[:, None]) | ((s[None, :] == s[:, None]) & (idx[None, :] < idx[:, None]))
    return before.sum(1).astype(np.int64)


def order_from_rank(rank):
    order = np.empty(rank.shape[0], np.int64)
    order[rank] = np.arange(rank.shape[0])
    return order


def select(clt, counts, score_t, npoint_t):
    """eval_map.py:74-84: ascending proposal indices with score > float32(score_t) and count > npoint_t."""
    clt = np.asarray(clt, np.float32).reshape(-1)
    return np.nonzero((clt > np.float32(score_t)) & (np.asarray(counts, np.int64) > int(npoint_t)))[0].astype(np.int32)


def fold_masks(proposals_idx, n_prop, n_fold):
    masks = np.zeros((n_prop, n_fold), bool)
    p, pt = proposals_idx[:, 0], proposals_idx[:, 1] % n_fold
    ok = (p >= 0) & (p < n_prop)
    masks[p[ok], pt[ok]] = True
    return masks


def mask_iou(masks, counts):
    """|Mi & Mj| / ((|Mi| + |Mj|) - |Mi & Mj|), every operation in float32 (k_mask_iou)."""
    m = masks.astype(np.int64)
    inter = (m @ m.T).astype(np.float32)
    c = counts.astype(np.float32)
    with np.errstate(invalid="ignore", divide="ignore"):
        return (inter / ((c[:, None] + c[None, :]) - inter)).astype(np.float32)


def greedy_nms(ious, scores, threshold):
    """tools/mIOU.py:77-87 walked in the order of rank_by_counting; `iou > threshold` compares in float32."""
    thr = np.float32(threshold)
    order = order_from_rank(rank_by_counting(scores))
    suppressed = np.zeros(order.shape[0], bool)
    pick = []
    for it in order:
        if suppressed[it]:
            continue
        pick.append(it)
        suppressed |= ious[it] > thr
    return np.array(pick, np.int32)


def superpoint_vote(seg, superpoint, n_label, n_sp):
    """tools/getins.py:72-98: first arg-max label per superpoint; negative labels vote in bucket n_label -> -100.  Ids outside
    [0, n_sp) take no part and keep -100; ids >= n_sp are reported in the returned status."""
    sp = np.asarray(superpoint, np.int64)
    ok = (sp >= 0) & (sp < n_sp)
    lab = np.where(seg < 0, n_label, seg)
    hist = np.zeros((n_sp, n_label + 1), np.int64)
    np.add.at(hist, (sp[ok], lab[ok]), 1)
    sp_label = hist.argmax(1).astype(np.int64)
    sp_label[sp_label == n_label] = -100
    seg2 = np.full(seg.shape[0], -100, np.int64)
    seg2[ok] = sp_label[sp[ok]]
    return seg2, (STATUS_SUPERPOINT_RANGE if (sp >= n_sp).any() else 0)


def refine(pred_sem, proposals_idx, proposals_offset, clt, point_num, superpoint, score_t, npoint_t, nms_t, n_superpoints=None):
    """The whole per-scene unit; every intermediate under the name the device form's result uses."""
    pred_sem, proposals_idx = np.asarray(pred_sem), np.asarray(proposals_idx, np.int64)
    off = np.asarray(proposals_offset, np.int64)
    clt = np.asarray(clt, np.float32).reshape(-1)
    n_fold, n_prop = int(point_num) // 3, off.shape[0] - 1
    n_sp = n_fold if n_superpoints is None else int(n_superpoints)
    masks = fold_masks(proposals_idx, n_prop, n_fold)
    counts = masks.sum(1).astype(np.int32)
    rows = select(clt, counts, score_t, npoint_t)
    ious = mask_iou(masks[rows], counts[rows])
    pick = greedy_nms(ious, clt[rows], nms_t)
    pick_rows = rows[pick]
    seg = np.full(n_fold, -100, np.int64)
    for c, r in enumerate(pick_rows):
        seg[masks[r]] = c
    seg2, status = superpoint_vote(seg, superpoint, pick.shape[0], n_sp)
    clusters_all = (seg2[None, :] == np.arange(pick.shape[0])[:, None])
    counts2 = clusters_all.sum(1).astype(np.int32)
    keep = np.nonzero(counts2 > 0)[0].astype(np.int32)
    sel = pick_rows[keep]
    first = proposals_idx[off[:-1], 1] if n_prop else np.zeros(0, np.int64)
    semantic_id = SEMANTIC_LABEL_IDX[pred_sem[first]]
    return dict(pointnum=counts, rows=rows, cross_ious=ious, pick=pick, pick_rows=pick_rows.astype(np.int32), seg=seg,
                seg_refined=seg2, counts2=counts2, keep=keep, clusters=clusters_all[keep].astype(np.int32),
                scores=clt[sel], semantic_id=semantic_id[sel].astype(np.int64), status=status)


def refine_golden(g, **kw):
    return refine(g["in_pred_sem"], g["in_proposals_idx"], g["in_proposals_offset"], g["in_clt"], int(g["in_point_num"]),
                  g["in_superpoint"], float(g["score_t"]), int(g["npoint_t"]), float(g["nms_t"]), **kw)


# golden key -> key of refine()'s dict
GOLDEN_KEYS = dict(out_pointnum="pointnum", out_cross_ious="cross_ious", out_pick="pick", out_seg="seg",
                   out_seg_refined="seg_refined", out_clusters="clusters", out_cluster_scores="scores",
                   out_cluster_semantic_id="semantic_id")
