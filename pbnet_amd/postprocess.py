"""Evaluation-time post-processing after PBNet.forward -- the MI355X form of /root/reference/eval_map.py:55-123
(TTA fold, score / point-count thresholds, mask-IoU NMS, superpoint alignment), SURVEY.md 8(f) rank 1.

`refine_instances` takes exactly what eval_map.py has in hand at line 55 (the `pred` dict of model_fn_eval, the number of
points of the 3-copy batch and the scene's superpoint ids) and returns what it holds at line 118:
(clusters i32[C, N/3], cluster_scores [C], cluster_semantic_id i64[C]) on the device.  Masks are bitsets on the device
(csrc/post.hip); the greedy NMS runs on the host on a [P, P] matrix with the reference's own numpy statements.

`refine_instances_device` is the same step without the five host stops of `refine_instances` (the threshold read-back, the IoU
read-back, `sp.max().item()`, the vanished-cluster read-back and the index uploads): every count stays in a device scalar until
the caller asks for `.sliced()`.

`refine_batch_device` is the device-resident form for ALL scenes of one merged forward (pbnet_amd/serving.py), without the TTA
fold: one pass with a scene axis (csrc/post_batch.hip), the masks as one label per point, one read-back of n_keep[B] / status[B].

`refine_tta_merged_device` is that pass WITH the fold, for a merged forward that holds `copies` rotated copies of every scene (the
reference's evaluation unit, eval_map.py:48-70): the proposals of all copies of a scene are refined together over the scene's own
points (pbn_post_batch_tta).  Scene table, working tables and results are over folded points.

`summarize_merged_device` runs behind either merged pass (csrc/summary.hip): the folded semantic label per point and, per kept
instance, the class its points vote for (eval_map.py:142-155), its box and its centre -- three launches, no read-back."""
import numpy as np
import torch

from . import _native as N

SEMANTIC_LABEL_IDX = [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 14, 16, 24, 28, 33, 34, 36, 39]   # eval_map.py:32


def non_max_suppression(ious, scores, threshold):
    """tools/mIOU.py:77-87 (host, numpy): greedy NMS over a few hundred proposals."""
    ixs = scores.argsort()[::-1]
    pick = []
    while len(ixs) > 0:
        i = ixs[0]
        pick.append(i)
        iou = ious[i, ixs[1:]]
        remove_ixs = np.where(iou > threshold)[0] + 1
        ixs = np.delete(ixs, remove_ixs)
        ixs = np.delete(ixs, 0)
    return np.array(pick, dtype=np.int32)


def refine_instances(pred_sem, proposals, clt_scores, point_num, superpoint, cfg, return_debug=False):
    proposals_idx, proposals_offset = proposals[0], proposals[1]
    N.require_cuda(proposals_idx, proposals_offset, pred_sem)
    dev = proposals_idx.device
    lib = N.lib()
    st = N.current_stream()
    n_fold = int(point_num) // 3
    n_prop = int(proposals_offset.shape[0]) - 1
    words = lib.pbn_post_words(n_fold)
    clt_score = clt_scores.view(-1).float()
    empty = (torch.zeros(0, n_fold, dtype=torch.int32, device=dev), clt_score[:0], torch.zeros(0, dtype=torch.int64, device=dev))
    if n_prop <= 0:
        return empty
    # eval_map.py:63-65: class of a proposal = class of its first member
    label_idx = torch.tensor(SEMANTIC_LABEL_IDX, device=dev)
    semantic_id = label_idx[pred_sem[proposals_idx[:, 1][proposals_offset[:-1].long()].long()]]
    # :67-70 + :80: folded bitsets and their sizes
    pidx = proposals_idx.contiguous()
    masks = torch.empty(n_prop, words, dtype=torch.int32, device=dev)
    counts = torch.empty(n_prop, dtype=torch.int32, device=dev)
    N.check(lib.pbn_proposal_bitmask(N.ptr(pidx), int(pidx.shape[0]), n_fold, n_prop, N.ptr(masks), N.ptr(counts), st),
            "pbn_proposal_bitmask")
    # :74-84 thresholds (host: P scalars)
    host = torch.cat([clt_score, counts.float()]).cpu().numpy()
    score_h, count_h = host[:n_prop], host[n_prop:].astype(np.int64)
    rows = np.nonzero(score_h > np.float32(cfg.TEST_SCORE_THRESH))[0]
    rows = rows[count_h[rows] > cfg.TEST_NPOINT_THRESH]
    if rows.shape[0] == 0:
        return empty
    # :90-98 mask IoU of the survivors + greedy NMS
    rows_d = torch.from_numpy(rows.astype(np.int32)).to(dev)
    r = int(rows.shape[0])
    iou = torch.empty(r, r, dtype=torch.float32, device=dev)
    N.check(lib.pbn_mask_iou(N.ptr(masks), N.ptr(rows_d), r, n_fold, N.ptr(counts), N.ptr(iou), st), "pbn_mask_iou")
    pick = non_max_suppression(iou.cpu().numpy(), score_h[rows], cfg.TEST_NMS_THRESH)
    pick_rows = rows[pick]
    n_pick = int(pick_rows.shape[0])
    # :104-116 superpoint alignment and rebuilt clusters
    sp = torch.as_tensor(superpoint).to(dev).long().contiguous()
    n_sp = int(sp.max().item()) + 1
    pick_d = torch.from_numpy(pick_rows.astype(np.int32)).to(dev)
    seg = torch.empty(n_fold, dtype=torch.int64, device=dev)
    seg2 = torch.empty(n_fold, dtype=torch.int64, device=dev)
    hist = torch.empty(n_sp, n_pick + 1, dtype=torch.int32, device=dev)
    sp_label = torch.empty(n_sp, dtype=torch.int64, device=dev)
    masks2 = torch.empty(n_pick, words, dtype=torch.int32, device=dev)
    counts2 = torch.empty(n_pick, dtype=torch.int32, device=dev)
    N.check(lib.pbn_superpoint_refine(N.ptr(masks), N.ptr(pick_d), n_pick, n_fold, N.ptr(sp), n_sp, N.ptr(seg), N.ptr(hist),
                                      N.ptr(sp_label), N.ptr(seg2), N.ptr(masks2), N.ptr(counts2), st),
            "pbn_superpoint_refine")
    keep = np.nonzero(counts2.cpu().numpy() > 0)[0]                                   # :113-118 drop vanished clusters
    keep_d = torch.from_numpy(keep.astype(np.int32)).to(dev)
    clusters = torch.empty(int(keep.shape[0]), n_fold, dtype=torch.int32, device=dev)
    N.check(lib.pbn_bitmask_to_dense(N.ptr(masks2), N.ptr(keep_d), int(keep.shape[0]), n_fold, N.ptr(clusters), st),
            "pbn_bitmask_to_dense")
    sel = torch.from_numpy(pick_rows[keep].astype(np.int64)).to(dev)
    out = (clusters, clt_score[sel], semantic_id[sel])
    if return_debug:
        return out + (dict(pointnum=counts, cross_ious=iou, pick=pick, seg=seg, seg_refined=seg2),)
    return out


# ---- the device-resident form -------------------------------------------------------------------------------------------
STATUS_SUPERPOINT_RANGE, STATUS_CLASS_RANGE = 1, 2          # bits of RefinedInstances.status (csrc/post.hip)


class PostWorkspace(object):
    """Every buffer `refine_instances_device` touches, outputs included, sized from capacities (P, n_fold, n_superpoints).

    A call with sizes that fit (`fits`) allocates nothing: it works on leading views of the flat buffers.  The results of a
    call ALIAS these buffers, so the next call on the same workspace overwrites them.  One workspace per stream."""

    def __init__(self, n_prop, n_fold, n_superpoints, device):
        p, f, s = max(int(n_prop), 1), max(int(n_fold), 1), max(int(n_superpoints), 1)
        if p > N.lib().pbn_post_max_proposals():
            raise ValueError("the device form takes at most %d proposals, got %d" % (N.lib().pbn_post_max_proposals(), p))
        self.n_prop, self.n_fold, self.n_superpoints = p, f, s
        self.device = torch.device(device)
        w = N.lib().pbn_post_words(f)
        i32 = lambda n: torch.zeros(n, dtype=torch.int32, device=self.device)
        i64 = lambda n: torch.zeros(n, dtype=torch.int64, device=self.device)
        self.masks, self.masks2 = i32(p * w), i32(p * w)
        self.counts, self.counts2, self.rows, self.pick, self.pick_rows, self.keep = (i32(p) for _ in range(6))
        self.iou = torch.zeros(p * p, dtype=torch.float32, device=self.device)
        self.seg, self.seg_refined, self.sp_label = i64(f), i64(f), i64(s)
        self.hist = i32(s * (p + 1))
        self.scores = torch.zeros(p, dtype=torch.float32, device=self.device)
        self.semantic_id = i64(p)
        self.clusters = i32(p * f)
        self.scalars = i32(4)                                   # n_rows, n_pick, n_keep, status
        self.label_table = torch.tensor(SEMANTIC_LABEL_IDX, dtype=torch.int64, device=self.device)

    def fits(self, n_prop, n_fold, n_superpoints):
        return n_prop <= self.n_prop and n_fold <= self.n_fold and n_superpoints <= self.n_superpoints


class RefinedInstances(object):
    """What `refine_instances_device` leaves on the device.  Capacity-sized tensors (P = number of proposals): clusters
    i32[P, n_fold] (rows from n_keep on are zero), scores f32[P], semantic_id i64[P], pick i32[P] (survivor positions in pick
    order, tail -1), seg / seg_refined i64[n_fold]; the debug tables pointnum i32[P], rows i32[P], cross_ious f32[P, P] (live in
    [:n_rows, :n_rows]), pick_rows, keep; the device scalars n_rows, n_pick, n_keep, status (views of `scalars` i32[4]).
    Nothing here has been read back; `sliced()` is the one method that synchronises -- unless the caller has already read
    `scalars` back together with other values (ValidationEpoch does) and hands the four integers in: then it only slices."""

    def __init__(self, ws, n_prop, n_fold, views):
        self.workspace, self.n_prop, self.n_fold = ws, n_prop, n_fold
        self.clusters, self.scores, self.semantic_id = views["clusters"], views["scores"], views["semantic_id"]
        self.pick, self.seg, self.seg_refined = views["pick"], views["seg"], views["seg_refined"]
        self.pointnum, self.rows, self.cross_ious = views["pointnum"], views["rows"], views["cross_ious"]
        self.pick_rows, self.keep = views["pick_rows"], views["keep"]
        self.scalars = ws.scalars
        self.n_rows, self.n_pick, self.n_keep, self.status = (ws.scalars[i] for i in range(4))

    def sliced(self, scalars=None):
        """(clusters i32[n_keep, n_fold], scores [n_keep], semantic_id i64[n_keep]): exactly what `refine_instances` returns.
        One read-back of the four scalars, unless the caller has made it already and passes the four values.  ValueError when
        the status word is set (a superpoint id >= n_superpoints, or a proposal whose class cannot be looked up)."""
        n_rows, n_pick, n_keep, status = (int(v) for v in (self.scalars.tolist() if scalars is None else scalars))
        if status & STATUS_SUPERPOINT_RANGE:
            raise ValueError("a superpoint id is >= n_superpoints: pass the scene's real superpoint count (or leave the default)")
        if status & STATUS_CLASS_RANGE:
            raise ValueError("a kept proposal has no first member, or its predicted class is outside the label table")
        return self.clusters[:n_keep], self.scores[:n_keep], self.semantic_id[:n_keep]


def refine_instances_device(pred_sem, proposals, clt_scores, point_num, superpoint, cfg, n_superpoints=None, workspace=None):
    """`refine_instances` without a host read-back, a host-computed launch argument or an allocation sized from device data
    between its first and its last launch: thresholds, mask IoU, greedy NMS, superpoint vote and compaction are fourteen launches
    whose counts (n_rows, n_pick, n_keep) stay in device scalars.  Returns a `RefinedInstances`; `.sliced()` gives the host
    form's triple.  The call can be captured in a graph and enqueued ahead of the previous scene's read-back.

    Tie rule of the NMS: score descending, among equal scores the lower survivor index first.  The host form inherits the tie
    order of numpy's (unstable) argsort; the two agree whenever the surviving scores are distinct.

    `superpoint` must be a device int64 tensor of n_fold ids (a numpy array is uploaded once by the caller, not here).
    `n_superpoints` bounds the ids from above and sizes the vote table [n_superpoints, P + 1] int32; the default n_fold is always
    enough (an id can never exceed the number of points) but makes that table n_fold x (P + 1): a loader that knows the scene's
    superpoint count should pass it.  An id >= n_superpoints sets bit 1 of `status` (and `.sliced()` raises); nothing is written
    out of bounds.  `workspace`: a `PostWorkspace` that fits (P, n_fold, n_superpoints) -- a call with one allocates nothing
    (given float32 scores and contiguous inputs); None allocates a fresh one.  At most 4096 proposals."""
    proposals_idx, proposals_offset = proposals[0], proposals[1]
    N.require_cuda(proposals_idx, proposals_offset, pred_sem, clt_scores, superpoint)
    if superpoint.dtype != torch.int64:
        raise TypeError("superpoint must be an int64 device tensor, got %s" % superpoint.dtype)
    for name, t in (("proposals_offset", proposals_offset), ("pred_sem", pred_sem)):
        if t.dtype not in (torch.int32, torch.int64):
            raise TypeError("%s must be int32 or int64, got %s" % (name, t.dtype))
    dev = proposals_idx.device
    lib = N.lib()
    st = N.current_stream()
    n_fold = int(point_num) // 3
    n_prop = int(proposals_offset.shape[0]) - 1
    if n_fold < 1 or int(superpoint.numel()) < n_fold:
        raise ValueError("superpoint holds %d ids for %d folded points" % (superpoint.numel(), n_fold))
    n_sp = n_fold if n_superpoints is None else int(n_superpoints)
    if n_sp < 1:
        raise ValueError("n_superpoints must be positive, got %d" % n_sp)
    ws = workspace
    if ws is None:
        ws = PostWorkspace(n_prop, n_fold, n_sp, dev)
    elif not ws.fits(n_prop, n_fold, n_sp):
        raise ValueError("workspace (%d, %d, %d) does not fit (%d, %d, %d)" % (ws.n_prop, ws.n_fold, ws.n_superpoints, n_prop,
                                                                              n_fold, n_sp))
    p = max(n_prop, 0)
    words = lib.pbn_post_words(n_fold)
    views = dict(clusters=ws.clusters[:p * n_fold].view(p, n_fold), scores=ws.scores[:p], semantic_id=ws.semantic_id[:p],
                 pick=ws.pick[:p], pick_rows=ws.pick_rows[:p], keep=ws.keep[:p], rows=ws.rows[:p], pointnum=ws.counts[:p],
                 cross_ious=ws.iou[:p * p].view(p, p), seg=ws.seg[:n_fold], seg_refined=ws.seg_refined[:n_fold])
    res = RefinedInstances(ws, p, n_fold, views)
    if p == 0:
        ws.scalars.zero_()
        return res
    clt_score = clt_scores.view(-1)
    clt_score = clt_score if clt_score.dtype == torch.float32 else clt_score.float()
    pidx = proposals_idx.contiguous()
    off, sem, sp = proposals_offset.contiguous(), pred_sem.contiguous(), superpoint.contiguous()
    n_rows, n_pick, n_keep, status = (_elem_ptr(ws.scalars, i) for i in range(4))
    N.check(lib.pbn_proposal_bitmask(N.ptr(pidx), int(pidx.shape[0]), n_fold, p, N.ptr(ws.masks), N.ptr(ws.counts), st),
            "pbn_proposal_bitmask")
    N.check(lib.pbn_post_select(N.ptr(clt_score), N.ptr(ws.counts), p, float(cfg.TEST_SCORE_THRESH), int(cfg.TEST_NPOINT_THRESH),
                                N.ptr(ws.rows), n_rows, status, st), "pbn_post_select")
    N.check(lib.pbn_mask_iou_dev(N.ptr(ws.masks), N.ptr(ws.rows), n_rows, p, n_fold, N.ptr(ws.counts), N.ptr(ws.iou), st),
            "pbn_mask_iou_dev")
    N.check(lib.pbn_post_nms(N.ptr(clt_score), N.ptr(ws.rows), n_rows, p, N.ptr(ws.iou), float(cfg.TEST_NMS_THRESH),
                             N.ptr(ws.pick), N.ptr(ws.pick_rows), n_pick, st), "pbn_post_nms")
    N.check(lib.pbn_superpoint_refine_dev(N.ptr(ws.masks), N.ptr(ws.pick_rows), n_pick, p, n_fold, N.ptr(sp), n_sp, N.ptr(ws.seg),
                                          N.ptr(ws.hist), N.ptr(ws.sp_label), N.ptr(ws.seg_refined), N.ptr(ws.masks2),
                                          N.ptr(ws.counts2), status, st), "pbn_superpoint_refine_dev")
    N.check(lib.pbn_post_compact(N.ptr(ws.counts2), N.ptr(ws.pick_rows), n_pick, p, n_fold, N.ptr(clt_score), N.ptr(pidx),
                                 int(pidx.shape[0]), N.ptr(off), int(off.dtype == torch.int64), N.ptr(sem),
                                 int(sem.dtype == torch.int64), int(sem.numel()), N.ptr(ws.label_table),
                                 int(ws.label_table.numel()), N.ptr(ws.masks2), N.ptr(ws.keep), N.ptr(ws.scores),
                                 N.ptr(ws.semantic_id), N.ptr(ws.clusters), n_keep, status, st), "pbn_post_compact")
    return res


def _elem_ptr(t, i):
    """Address of element i of a contiguous tensor."""
    return N.c_vp(t.data_ptr() + i * t.element_size())


# ---- the batched form: all scenes of one merged forward (csrc/post_batch.hip) ------------------------------------------------
MAX_SCENES = N.MAX_SCENES


def scene_table(point_starts, sp_starts):
    """The by-value launch argument of pbn_post_batch from two host lists of B + 1 ascending starts (host data, no tensor)."""
    b = len(point_starts) - 1
    if not 1 <= b <= MAX_SCENES or len(sp_starts) != b + 1:
        raise ValueError("a merged forward holds 1..%d scenes, got %d (and %d superpoint starts)" % (MAX_SCENES, b, len(sp_starts)))
    t = N.SceneTable()
    t.n_scenes = b
    for j in range(b + 1):
        t.point_start[j], t.sp_start[j] = int(point_starts[j]), int(sp_starts[j])
    return t


class PostBatchWorkspace(object):
    """Every buffer `refine_batch_device` touches, outputs included, sized from capacities: proposals of the merged forward,
    its points, its scenes and the sum of the scenes' superpoint capacities.  A call that fits allocates nothing; its results
    ALIAS these buffers, so the next call on the same workspace overwrites them.  One workspace per stream."""

    def __init__(self, n_prop, n_points_total, n_scenes, n_superpoints_total, device):
        p, n, b, s = max(int(n_prop), 1), max(int(n_points_total), 1), int(n_scenes), max(int(n_superpoints_total), 0)
        lib = N.lib()
        if p > lib.pbn_post_max_proposals():
            raise ValueError("the device form takes at most %d proposals, got %d" % (lib.pbn_post_max_proposals(), p))
        if not 1 <= b <= MAX_SCENES:
            raise ValueError("a merged forward holds 1..%d scenes, got %d" % (MAX_SCENES, b))
        self.n_prop, self.n_points_total, self.n_scenes, self.n_superpoints_total = p, n, b, s
        self.device = torch.device(device)
        self.nbytes = int(lib.pbn_post_batch_workspace_bytes(p, n, b, s, None))
        mk = lambda k, dt: torch.zeros(k, dtype=dt, device=self.device)
        self.buffer = mk(self.nbytes, torch.uint8)
        self.point_instance, self.superpoint = mk(n, torch.int32), mk(n, torch.int64)
        self.scores, self.semantic_id, self.npoints = mk(b * p, torch.float32), mk(b * p, torch.int64), mk(b * p, torch.int32)
        self.scalars = mk(2 * MAX_SCENES, torch.int32)
        self.label_table = torch.tensor(SEMANTIC_LABEL_IDX, dtype=torch.int64, device=self.device)

    def fits(self, n_prop, n_points_total, n_scenes, n_superpoints_total):
        return (n_prop <= self.n_prop and n_points_total <= self.n_points_total and n_scenes <= self.n_scenes
                and n_superpoints_total <= self.n_superpoints_total)

    def grown_for(self, n_prop, n_points_total, n_scenes, n_superpoints_total):
        """A workspace that fits both this one's capacities and the given sizes (this one when it already does)."""
        if self.fits(n_prop, n_points_total, n_scenes, n_superpoints_total):
            return self
        return PostBatchWorkspace(max(n_prop, self.n_prop), max(n_points_total, self.n_points_total), max(n_scenes, self.n_scenes),
                                  max(n_superpoints_total, self.n_superpoints_total), self.device)


class RefinedBatch(object):
    """What `refine_batch_device` leaves on the device for the B scenes of a merged forward with P proposals:
    point_instance i32[N_total] (scene-local kept-instance number or -100), scores f32[B, P], semantic_id i64[B, P],
    npoints i32[B, P] (row j: scene j's kept instances in pick order, then 0 / -1 / 0), scalars i32[2 B] = n_keep[B], status[B].
    Nothing has been read back; `scene` / `dense` synchronise only when the caller does not hand the scalars in."""

    def __init__(self, ws, n_prop, point_starts, sp_starts):
        self.workspace, self.n_prop, self.point_starts, self.sp_starts = ws, n_prop, list(point_starts), list(sp_starts)
        self.n_scenes = b = len(point_starts) - 1
        n = self.point_starts[-1]
        self.point_instance = ws.point_instance[:n]
        self.scores, self.semantic_id, self.npoints = (t[:b * n_prop].view(b, n_prop) for t in (ws.scores, ws.semantic_id, ws.npoints))
        self.scalars = ws.scalars[:2 * b]

    def table(self, name):
        """Debug view of one internal table of the last call (names and shapes: pbn_post_batch_layout); float32 for `iou`."""
        lay = N.PostBatchLayout()
        N.lib().pbn_post_batch_workspace_bytes(max(self.n_prop, 1), self.point_starts[-1], self.n_scenes, self.sp_starts[-1], lay)
        names = [f[0] for f in N.PostBatchLayout._fields_]
        lo, hi = getattr(lay, name), getattr(lay, names[names.index(name) + 1])
        return self.workspace.buffer[lo:hi].view(torch.float32 if name == "iou" else torch.int32)

    def _counts(self, j, scalars):
        sc = [int(v) for v in (self.scalars.tolist() if scalars is None else scalars)]
        n_keep, status = sc[j], sc[self.n_scenes + j]
        if status & STATUS_SUPERPOINT_RANGE:
            raise ValueError("scene %d: a superpoint id is >= the scene's n_superpoints" % j)
        if status & STATUS_CLASS_RANGE:
            raise ValueError("scene %d: a kept proposal's predicted class is outside the label table" % j)
        return n_keep

    def scene(self, j, scalars=None):
        """Scene j's instances: dict(point_instance i32[n_j], scores [k_j], semantic_id i64[k_j], npoints i32[k_j]).  ValueError
        when scene j's status word is set.  `scalars`: the 2 B integers of `.scalars` if the caller has read them back already."""
        k = self._counts(j, scalars)
        return dict(point_instance=self.point_instance[self.point_starts[j]:self.point_starts[j + 1]], scores=self.scores[j, :k],
                    semantic_id=self.semantic_id[j, :k], npoints=self.npoints[j, :k])

    def dense(self, j, scalars=None):
        """The reference's cluster table of scene j, int32[k_j, n_j], materialised on request."""
        k = self._counts(j, scalars)
        pi = self.point_instance[self.point_starts[j]:self.point_starts[j + 1]]
        return (pi[None, :] == torch.arange(k, dtype=torch.int32, device=pi.device)[:, None]).to(torch.int32)


def tta_table(point_starts, sp_starts, copies):
    """The by-value launch argument of pbn_post_batch_tta from two host lists of B + 1 ascending starts over FOLDED points and the
    number of copies of every scene in the merged forward (B * copies batch elements, at most MAX_SCENES)."""
    b, copies = len(point_starts) - 1, int(copies)
    if copies < 1:
        raise ValueError("copies must be at least 1, got %d" % copies)
    if len(sp_starts) != b + 1:
        raise ValueError("%d point starts, %d superpoint starts" % (len(point_starts), len(sp_starts)))
    if b < 1 or b * copies > MAX_SCENES:
        raise ValueError("a merged forward holds 1..%d batch elements, got %d scenes x %d copies" % (MAX_SCENES, b, copies))
    t = N.TtaTable()
    t.n_scenes, t.copies = b, copies
    for j in range(b + 1):
        t.point_start[j], t.sp_start[j] = int(point_starts[j]), int(sp_starts[j])
    return t


def _check_merged_inputs(proposals_idx, proposals_offset, sem_pred_p, clt_scores):
    """The dtype checks both merged entries make."""
    if proposals_idx.dtype != torch.int64:
        raise TypeError("proposals_idx must be int64, got %s" % proposals_idx.dtype)
    for name, t in (("proposals_offset", proposals_offset), ("sem_pred_p", sem_pred_p)):
        if t.dtype not in (torch.int32, torch.int64):
            raise TypeError("%s must be int32 or int64, got %s" % (name, t.dtype))
    if clt_scores.dtype not in N.DT:
        raise TypeError("clt_scores must be float32, bfloat16 or float16, got %s" % clt_scores.dtype)


def _refine_merged(sem_pred_p, proposals, clt_scores, point_starts, sp_starts, superpoint, cfg, copies, workspace):
    """Both merged entries: the checks, the workspace fit, the `RefinedBatch` and the call.  copies None: pbn_post_batch on a scene
    table; an integer: pbn_post_batch_tta on a TTA table over folded points."""
    proposals_idx, proposals_offset = proposals[0], proposals[1]
    N.require_cuda(proposals_idx, proposals_offset, sem_pred_p, clt_scores, superpoint)
    _check_merged_inputs(proposals_idx, proposals_offset, sem_pred_p, clt_scores)
    if copies is None:
        entry, table, n_copies = "pbn_post_batch", scene_table(point_starts, sp_starts), 1
    else:
        entry, table = "pbn_post_batch_tta", tta_table(point_starts, sp_starts, copies)
        n_copies = table.copies
    b, n_total, n_sp_total = table.n_scenes, int(point_starts[-1]), int(sp_starts[-1])
    n_merged = n_copies * n_total
    if int(sem_pred_p.numel()) != n_merged:
        raise ValueError("sem_pred_p holds %d points, the scene table %d" % (sem_pred_p.numel(), n_total) if copies is None else
                         "sem_pred_p holds %d points, the table %d x %d" % (sem_pred_p.numel(), n_copies, n_total))
    if n_sp_total > 0:
        if superpoint is None or superpoint.dtype != torch.int64 or int(superpoint.numel()) < n_total:
            raise ValueError("superpoint must be an int64 device tensor of %d ids" % n_total)
    n_prop = max(int(proposals_offset.shape[0]) - 1, 0)
    lib = N.lib()
    if n_prop > lib.pbn_post_max_proposals():
        raise ValueError("the device form takes at most %d proposals, got %d" % (lib.pbn_post_max_proposals(), n_prop))
    ws = workspace
    if ws is None:
        ws = PostBatchWorkspace(n_prop, n_total, b, n_sp_total, proposals_idx.device)
    elif not ws.fits(n_prop, n_total, b, n_sp_total):
        raise ValueError("workspace (%d, %d, %d, %d) does not fit (%d, %d, %d, %d)" % (
            ws.n_prop, ws.n_points_total, ws.n_scenes, ws.n_superpoints_total, n_prop, n_total, b, n_sp_total))
    res = RefinedBatch(ws, n_prop, point_starts, sp_starts)
    pidx, off, sem, clt = proposals_idx.contiguous(), proposals_offset.contiguous(), sem_pred_p.contiguous(), clt_scores.contiguous()
    sp = None if n_sp_total == 0 else superpoint.contiguous()
    N.check(getattr(lib, entry)(N.ptr(pidx), int(pidx.shape[0]), N.ptr(off), int(off.dtype == torch.int64), n_prop, N.ptr(clt),
                                N.DT[clt.dtype], N.ptr(sem), int(sem.dtype == torch.int64), n_merged, table, N.ptr(sp),
                                float(cfg.TEST_SCORE_THRESH), int(cfg.TEST_NPOINT_THRESH), float(cfg.TEST_NMS_THRESH),
                                N.ptr(ws.label_table), int(ws.label_table.numel()), N.ptr(ws.point_instance), N.ptr(ws.scores),
                                N.ptr(ws.semantic_id), N.ptr(ws.npoints), N.ptr(ws.scalars), N.ptr(ws.buffer), ws.nbytes,
                                N.current_stream()), entry)
    return res


def refine_merged_device(sem_pred_p, proposals, clt_scores, point_starts, sp_starts, superpoint, cfg, workspace=None):
    """`refine_batch_device` on ids that are already merged: `superpoint` int64[N_total] (scene-local ids; rows of scenes with
    sp_starts[j + 1] == sp_starts[j] are never read; None when no scene has superpoints)."""
    return _refine_merged(sem_pred_p, proposals, clt_scores, point_starts, sp_starts, superpoint, cfg, None, workspace)


def refine_tta_merged_device(sem_pred_p, proposals, clt_scores, point_starts, sp_starts, superpoint, cfg, copies=3, workspace=None):
    """`refine_merged_device` with the TTA fold (pbn_post_batch_tta): the merged forward holds `copies` copies of each of its B
    scenes (B * copies <= MAX_SCENES batch elements, scene j's copies one after the other).  `point_starts` / `sp_starts`: B + 1
    host integers over FOLDED points; sem_pred_p holds copies * point_starts[-1] labels (the class of an instance is read at its
    unfolded first member, eval_map.py:64); `superpoint` int64[point_starts[-1]], one scene-local id per folded point (None when no
    scene has any).  Returns a `RefinedBatch` over folded points: scene j's point_instance has n_j entries.  Thirteen launches for
    all scenes, no host stop; `workspace`: a `PostBatchWorkspace` sized by folded points."""
    return _refine_merged(sem_pred_p, proposals, clt_scores, point_starts, sp_starts, superpoint, cfg, copies, workspace)


def superpoint_starts(point_starts, has_superpoints, n_superpoints=None):
    """sp_start of the scene table: scene j's vote slice holds n_superpoints[j] rows (default: its point count), 0 without ids."""
    starts = [0]
    for j, has in enumerate(has_superpoints):
        cap = 0
        if has:
            cap = int(point_starts[j + 1] - point_starts[j]) if n_superpoints is None or n_superpoints[j] is None else int(n_superpoints[j])
            if cap < 1:
                raise ValueError("scene %d: n_superpoints must be positive, got %d" % (j, cap))
        starts.append(starts[-1] + cap)
    return starts


def refine_batch_device(sem_pred_p, proposals, clt_scores, point_starts, superpoints, cfg, n_superpoints=None, workspace=None):
    """The post-processing of eval_map.py:55-123 for every scene of ONE merged forward (pbnet_amd/serving.py), without the TTA
    fold: thirteen launches for all scenes, every count in a device scalar, no host stop.  Returns a `RefinedBatch`.

    sem_pred_p [N_total], proposals (idx int64[M, 2], offset [P + 1]) and clt_scores [P] are the merged forward's own results;
    point_starts: the B + 1 host integers `merge_scenes` returns.  `superpoints`: B entries, each an int64 device tensor of the
    scene's ids or None (that scene is refined as if every point were its own superpoint; the vote is skipped).  `n_superpoints`:
    per-scene upper bounds of the ids (default: the scene's point count); an id at or above its scene's bound sets that scene's
    status and `.scene(j)` raises for that scene alone.  Same tie rule and limits as `refine_instances_device`."""
    b = len(point_starts) - 1
    superpoints = [None] * b if superpoints is None else list(superpoints)
    if len(superpoints) != b:
        raise ValueError("%d superpoint entries for %d scenes" % (len(superpoints), b))
    sp_starts = superpoint_starts(point_starts, [s is not None for s in superpoints], n_superpoints)
    n_total, n_prop = int(point_starts[-1]), max(int(proposals[1].shape[0]) - 1, 0)
    ws = workspace
    if ws is None:
        ws = PostBatchWorkspace(n_prop, n_total, b, sp_starts[-1], proposals[0].device)
    merged = None
    if sp_starts[-1] > 0:
        if n_total > ws.n_points_total:
            raise ValueError("workspace holds %d points, the batch %d" % (ws.n_points_total, n_total))
        merged = ws.superpoint
        for j, s in enumerate(superpoints):
            if s is None:
                continue
            N.require_cuda(s)
            if s.dtype != torch.int64 or int(s.numel()) != point_starts[j + 1] - point_starts[j]:
                raise ValueError("scene %d: superpoints must be %d int64 ids" % (j, point_starts[j + 1] - point_starts[j]))
            merged[point_starts[j]:point_starts[j + 1]].copy_(s.view(-1))
    return refine_merged_device(sem_pred_p, proposals, clt_scores, point_starts, sp_starts, merged, cfg, workspace=ws)


# ---- the scene summary: folded semantics, class vote and boxes per kept instance (csrc/summary.hip) ---------------------------------
STATUS_SUMMARY_CLASS, STATUS_SUMMARY_COORD, STATUS_SUMMARY_INSTANCE = 2, 4, 8       # bits of SceneSummary.status
MAX_CLASSES = 32                                                                    # SEL_MAX_CLASSES (csrc/pbn_common.h)


class SummaryWorkspace(object):
    """Every buffer `summarize_merged_device` touches, outputs included, sized from capacities: proposals of the merged forward,
    its FOLDED points, its scenes and the classes of the semantic head.  A call that fits allocates nothing; its results ALIAS
    these buffers, so the next call on the same workspace overwrites them.  One workspace per stream."""

    def __init__(self, n_prop, n_points_total, n_scenes, n_cls, device):
        p, n, b, k = max(int(n_prop), 1), max(int(n_points_total), 1), int(n_scenes), int(n_cls)
        lib = N.lib()
        if p > lib.pbn_post_max_proposals():
            raise ValueError("the device form takes at most %d proposals, got %d" % (lib.pbn_post_max_proposals(), p))
        if not 1 <= b <= MAX_SCENES:
            raise ValueError("a merged forward holds 1..%d scenes, got %d" % (MAX_SCENES, b))
        if not 1 <= k <= MAX_CLASSES:
            raise ValueError("the semantic head has 1..%d classes, got %d" % (MAX_CLASSES, k))
        self.n_prop, self.n_points_total, self.n_scenes, self.n_cls = p, n, b, k
        self.device = torch.device(device)
        self.nbytes = int(lib.pbn_scene_summary_workspace_bytes(p, k))
        mk = lambda m, dt: torch.zeros(m, dtype=dt, device=self.device)
        self.buffer = mk(self.nbytes, torch.uint8)
        self.sem_fold = mk(n, torch.int32)
        self.class_vote, self.class_points = mk(b * p, torch.int64), mk(b * p, torch.int32)
        self.box, self.centroid = mk(b * p * 6, torch.float32), mk(b * p * 3, torch.float32)
        self.status = mk(MAX_SCENES, torch.int32)
        self.label_table = torch.tensor(SEMANTIC_LABEL_IDX, dtype=torch.int64, device=self.device)

    def fits(self, n_prop, n_points_total, n_scenes, n_cls):
        return (n_prop <= self.n_prop and n_points_total <= self.n_points_total and n_scenes <= self.n_scenes
                and n_cls <= self.n_cls)

    def grown_for(self, n_prop, n_points_total, n_scenes, n_cls):
        """A workspace that fits both this one's capacities and the given sizes (this one when it already does)."""
        if self.fits(n_prop, n_points_total, n_scenes, n_cls):
            return self
        return SummaryWorkspace(max(n_prop, self.n_prop), max(n_points_total, self.n_points_total), max(n_scenes, self.n_scenes),
                                max(n_cls, self.n_cls), self.device)


class SceneSummary(object):
    """What `summarize_merged_device` leaves on the device for the B scenes of a merged forward with P proposals: sem_fold
    i32[N] over folded points, class_vote i64[B, P], class_points i32[B, P], box f32[B, P, 6] and centroid f32[B, P, 3] (None
    without coordinates), status i32[B].  Nothing has been read back; `scene` synchronises only when the caller does not hand
    the scalars in."""

    def __init__(self, ws, refined, point_starts, with_xyz):
        self.workspace, self.refined, self.point_starts = ws, refined, list(point_starts)
        self.n_scenes = b = len(point_starts) - 1
        self.n_prop = p = refined.n_prop
        self.sem_fold = ws.sem_fold[:self.point_starts[-1]]
        self.class_vote, self.class_points = ws.class_vote[:b * p].view(b, p), ws.class_points[:b * p].view(b, p)
        self.box = ws.box[:b * p * 6].view(b, p, 6) if with_xyz else None
        self.centroid = ws.centroid[:b * p * 3].view(b, p, 3) if with_xyz else None
        self.status = ws.status[:b]

    def readback(self):
        """The 3 B integers `scene` reads: the post-processing's n_keep[B] and status[B], then the summary's status[B] -- one
        read-back for both passes."""
        return torch.cat([self.refined.scalars, self.status]).tolist()

    def scene(self, j, scalars=None):
        """Scene j's summary: dict(sem_fold i32[n_j], class_vote i64[k_j], class_points i32[k_j], box f32[k_j, 6] or None,
        centroid f32[k_j, 3] or None).  ValueError when scene j's summary status is set (the post-processing's own status is
        `RefinedBatch.scene`'s to report).  `scalars`: the 3 B integers of `readback()` if the caller has them already."""
        sc = [int(v) for v in (self.readback() if scalars is None else scalars)]
        b = self.n_scenes
        k, status = max(0, min(sc[j], self.n_prop)), sc[2 * b + j]
        if status & STATUS_SUMMARY_CLASS:
            raise ValueError("scene %d: the class an instance's points vote for is outside the label table" % j)
        if status & STATUS_SUMMARY_COORD:
            raise ValueError("scene %d: a coordinate is NaN or not inside (-32768, 32768)" % j)
        if status & STATUS_SUMMARY_INSTANCE:
            raise ValueError("scene %d: a point_instance value is neither -100 nor a kept instance" % j)
        return dict(sem_fold=self.sem_fold[self.point_starts[j]:self.point_starts[j + 1]], class_vote=self.class_vote[j, :k],
                    class_points=self.class_points[j, :k], box=None if self.box is None else self.box[j, :k],
                    centroid=None if self.centroid is None else self.centroid[j, :k])


def summarize_merged_device(sem_score, refined_batch, point_starts, copies=1, xyz=None, cfg_labels=None, workspace=None):
    """The scene summary behind `refine_merged_device` / `refine_tta_merged_device` (pbn_scene_summary): three launches on the
    current stream, no read-back.  sem_score: the merged forward's `sem_pred_score_p` [copies * N, K] (float32 / bfloat16 /
    float16, any row stride); refined_batch: the `RefinedBatch` of the same forward (its point_instance and n_keep are read on the
    device); point_starts: its B + 1 starts over FOLDED points; xyz: float32 [N, 3] in the scenes' own frames, or None (no box, no
    centre); cfg_labels: the label table as a list, default the one `refine_*_device` uses (the refined batch's own tensor).
    Returns a `SceneSummary`."""
    N.require_cuda(sem_score, refined_batch.point_instance, xyz)
    if sem_score.dim() != 2 or sem_score.dtype not in N.DT or sem_score.stride(1) != 1:
        raise TypeError("sem_score must be a [rows, classes] float32, bfloat16 or float16 tensor with unit column stride")
    b, n_total, copies = len(point_starts) - 1, int(point_starts[-1]), int(copies)
    table = tta_table(point_starts, [0] * (b + 1), copies)
    n_merged, n_cls = copies * n_total, int(sem_score.shape[1])
    if int(sem_score.shape[0]) != n_merged:
        raise ValueError("sem_score holds %d rows, the table %d x %d" % (sem_score.shape[0], copies, n_total))
    if list(refined_batch.point_starts) != [int(v) for v in point_starts]:
        raise ValueError("the refined batch was made for another scene table")
    if xyz is not None and (xyz.dtype != torch.float32 or tuple(xyz.shape) != (n_total, 3)):
        raise ValueError("xyz must be float32 [%d, 3]" % n_total)
    n_prop = refined_batch.n_prop
    ws = workspace
    if ws is None:
        ws = SummaryWorkspace(n_prop, n_total, b, n_cls, sem_score.device)
    elif not ws.fits(n_prop, n_total, b, n_cls):
        raise ValueError("workspace (%d, %d, %d, %d) does not fit (%d, %d, %d, %d)" % (ws.n_prop, ws.n_points_total, ws.n_scenes,
                                                                                      ws.n_cls, n_prop, n_total, b, n_cls))
    if cfg_labels is None:
        labels = refined_batch.workspace.label_table
    else:
        labels = torch.tensor([int(v) for v in cfg_labels], dtype=torch.int64, device=sem_score.device)
    xyz_c = None if xyz is None else xyz.contiguous()
    res = SceneSummary(ws, refined_batch, point_starts, xyz is not None)
    rc = N.lib().pbn_scene_summary(N.c_vp(sem_score.data_ptr()), int(sem_score.stride(0)), n_cls, N.DT[sem_score.dtype], n_merged,
                                   table, N.ptr(refined_batch.point_instance), N.ptr(refined_batch.scalars), n_prop, N.ptr(xyz_c),
                                   N.ptr(labels), int(labels.numel()), N.ptr(ws.sem_fold), N.ptr(ws.class_vote),
                                   N.ptr(ws.class_points), N.ptr(ws.box), N.ptr(ws.centroid), N.ptr(ws.status), N.ptr(ws.buffer),
                                   ws.nbytes, N.current_stream())
    N.check(rc, "pbn_scene_summary")
    return res
