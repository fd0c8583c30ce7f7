"""ScanNet instance-segmentation AP -- the evaluator behind eval_map.py:126-151, i.e.
/root/reference/tools/eval.py (`assign_instances_for_scan` :205-250, `evaluate_matches` :27-190, `compute_averages`
:193-210) and the ground-truth id encoding of datasets/scannetv2/get_val_gt.py:26-39.

What changes against the reference is the data model, not the numbers:

* association: the reference walks the scene once per (prediction, ground-truth instance) pair.  Here the scene's ids are
  turned into indices into their sorted unique list once, and ONE device pass per prediction fills a row of the
  [predictions, unique ids] overlap table (`pbn_instance_overlap`, csrc/apassoc.hip).  Vertex counts, void overlap and every
  `intersection` field are sums / entries of that integer table.
* a scene's matches are a `SceneMatches` record of flat arrays instead of dicts of dicts of copies;
  `to_reference()` / `from_reference()` convert to and from the reference's layout so either evaluator accepts either.
* matching is the reference's greedy rule run on arrays; the precision/recall integration is vectorised.
* `AssociationLog` is the association without a host stop (csrc/apassoc.hip): ids numbered and tables filled on the device, one
  compact record per scene in an epoch log that `collect()` reads back once and `decode_association_log` turns into the same
  `SceneMatches`.
* `APTable` is `evaluate_matches` without reading the log back (csrc/apeval.hip): the records are matched and the curves
  integrated on the device, and what comes back is the AP table.  Off unless asked for; the host functions are the default.

Everything else here except the overlap table is host bookkeeping on a few hundred integers, as in the reference."""
import numpy as np
import torch

from . import _native as N

# tools/eval.py:8-24
CLASS_LABELS = ['cabinet', 'bed', 'chair', 'sofa', 'table', 'door', 'window', 'bookshelf', 'picture', 'counter', 'desk',
                'curtain', 'refrigerator', 'shower curtain', 'toilet', 'sink', 'bathtub', 'otherfurniture']
VALID_CLASS_IDS = np.array([3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 14, 16, 24, 28, 33, 34, 36, 39])
OVERLAPS = np.append(np.arange(0.5, 0.95, 0.05), 0.25)
MIN_REGION_SIZE = 100
_CLASS_OF_ID = {int(c): i for i, c in enumerate(VALID_CLASS_IDS)}
# datasets/scannetv2/get_val_gt.py:8 (20 training classes -> NYU40 ids; 0/1 = wall/floor)
SEMANTIC_LABEL_IDX = np.array([1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 14, 16, 24, 28, 33, 34, 36, 39])


# ---------------------------------------------------------------------------------------------- ground-truth formats
def encode_gt_ids(sem_label, ins_label):
    """get_val_gt.py:26-37: per point `NYU40 id * 1000 + instance + 1`, 0 where the point has no instance.  The class of
    an instance is the class of its lowest-index point (`instance_mask[0]`); semantic label -100 counts as class 0."""
    sem = np.asarray(sem_label).astype(np.int64)
    ins = np.asarray(ins_label).astype(np.int64)
    out = np.zeros(ins.shape, np.int32)
    has = ins >= 0
    if not has.any():
        return out
    n_inst = int(ins.max()) + 1
    first = np.full(n_inst, ins.shape[0], np.int64)
    np.minimum.at(first, ins[has], np.nonzero(has)[0])
    present = first < ins.shape[0]                       # the reference raises on an id without points; skipped here
    sem_of = np.zeros(n_inst, np.int64)
    sem_of[present] = sem[first[present]]
    sem_of[sem_of == -100] = 0
    code = SEMANTIC_LABEL_IDX[sem_of] * 1000 + np.arange(n_inst) + 1
    out[has] = code[ins[has]]
    return out


def save_gt_ids(path, ids):
    """get_val_gt.py:39: one decimal id per line."""
    np.savetxt(path, np.asarray(ids), fmt="%d")


def load_gt_ids(path):
    """tools/getins.py:7-10."""
    with open(path) as f:
        return np.array(f.read().split(), dtype=np.int64)


# ------------------------------------------------------------------------------------------------------ association
class SceneMatches:
    """One scene's association tables.  Ground-truth rows are in ascending id order, prediction rows in input order
    (the orders the reference's lists have); `inter[q, g]` is zero where the classes differ."""

    __slots__ = ("scene", "gt_class", "gt_id", "gt_vert", "pred_class", "pred_id", "pred_label_id", "pred_vert", "pred_void",
                 "pred_conf", "inter")

    def __init__(self, scene, gt_class, gt_id, gt_vert, pred_class, pred_id, pred_label_id, pred_vert, pred_void, pred_conf,
                 inter):
        self.scene = scene
        self.gt_class, self.gt_id, self.gt_vert = gt_class, gt_id, gt_vert
        self.pred_class, self.pred_id, self.pred_label_id = pred_class, pred_id, pred_label_id
        self.pred_vert, self.pred_void, self.pred_conf = pred_vert, pred_void, pred_conf
        self.inter = inter

    def to_reference(self):
        """(gt2pred, pred2gt) exactly as tools/eval.py:205-250 returns them."""
        gt2pred = {name: [] for name in CLASS_LABELS}
        pred2gt = {name: [] for name in CLASS_LABELS}

        def gt_dict(g):
            return dict(instance_id=int(self.gt_id[g]), label_id=int(self.gt_id[g] // 1000), vert_count=int(self.gt_vert[g]),
                        med_dist=-1, dist_conf=0.0)

        def pred_dict(q):
            return dict(filename="%s_%03d" % (self.scene, int(self.pred_id[q])), pred_id=int(self.pred_id[q]),
                        label_id=int(self.pred_label_id[q]), vert_count=int(self.pred_vert[q]),
                        confidence=self.pred_conf[q], void_intersection=int(self.pred_void[q]))

        for g in range(self.gt_id.shape[0]):
            d = gt_dict(g)
            d["matched_pred"] = [dict(pred_dict(q), intersection=int(self.inter[q, g]))
                                 for q in np.nonzero(self.inter[:, g])[0]]
            gt2pred[CLASS_LABELS[self.gt_class[g]]].append(d)
        for q in range(self.pred_id.shape[0]):
            d = pred_dict(q)
            d["matched_gt"] = [dict(gt_dict(g), intersection=int(self.inter[q, g]), matched_pred=[])
                               for g in np.nonzero(self.inter[q])[0]]
            pred2gt[CLASS_LABELS[self.pred_class[q]]].append(d)
        return gt2pred, pred2gt

    @classmethod
    def from_reference(cls, scene, gt2pred, pred2gt):
        """Flatten the reference's dicts (e.g. matches produced by tools/eval.py itself)."""
        gts = [(li, g) for li, name in enumerate(CLASS_LABELS) for g in gt2pred[name]]
        gts.sort(key=lambda t: t[1]["instance_id"])
        preds = [(li, p) for li, name in enumerate(CLASS_LABELS) for p in pred2gt[name]]
        preds.sort(key=lambda t: t[1]["pred_id"])
        col = {g["instance_id"]: j for j, (_, g) in enumerate(gts)}
        inter = np.zeros((len(preds), len(gts)), np.int64)
        for q, (_, p) in enumerate(preds):
            for g in p["matched_gt"]:
                inter[q, col[g["instance_id"]]] = g["intersection"]
        i64 = lambda v: np.array(v, np.int64)                                                        # noqa: E731
        return cls(scene, i64([li for li, _ in gts]), i64([g["instance_id"] for _, g in gts]),
                   i64([g["vert_count"] for _, g in gts]), i64([li for li, _ in preds]), i64([p["pred_id"] for _, p in preds]),
                   i64([p["label_id"] for _, p in preds]), i64([p["vert_count"] for _, p in preds]),
                   i64([p["void_intersection"] for _, p in preds]),
                   np.array([p["confidence"] for _, p in preds], np.float32), inter)


def overlap_table(masks, gt_ids, device=None):
    """[predictions, unique ids] overlap counts on the device.  `masks`: [P, N] tensor or array (non-zero = inside);
    `gt_ids`: int[N].  Returns (inter int64[P, U] on the host, unique ids int64[U])."""
    gt_ids = np.asarray(gt_ids.cpu() if torch.is_tensor(gt_ids) else gt_ids).astype(np.int64).reshape(-1)
    uid, index = np.unique(gt_ids, return_inverse=True)
    if torch.is_tensor(masks):
        dev = masks.device if device is None else torch.device(device)
        m = masks.to(dev)
    else:
        dev = torch.device("cuda" if device is None else device)
        m = torch.from_numpy(np.ascontiguousarray(masks)).to(dev)
    if m.dim() != 2 or m.shape[1] != gt_ids.shape[0]:
        # tools/eval.py:222-224 only logs this; counting over mismatched lengths has no meaning, so it is an error here
        raise ValueError("prediction masks are %s but the scene has %d vertices" % (tuple(m.shape), gt_ids.shape[0]))
    n_pred, n_pts, n_gt = int(m.shape[0]), int(m.shape[1]), max(1, int(uid.shape[0]))
    if n_pred == 0 or n_pts == 0:
        return np.zeros((n_pred, int(uid.shape[0])), np.int64), uid
    m = (m if m.dtype == torch.int32 else (m != 0).to(torch.int32)).contiguous()
    N.require_cuda(m)
    idx = torch.from_numpy(index.astype(np.int32).reshape(-1)).to(dev)
    inter = torch.empty(n_pred, n_gt, dtype=torch.int32, device=dev)
    N.check(N.lib().pbn_instance_overlap(N.ptr(m), n_pred, n_pts, N.ptr(idx), n_gt, N.ptr(inter), N.current_stream()),
            "pbn_instance_overlap")
    return inter.cpu().numpy().astype(np.int64), uid


def assign_instances_for_scan(scene_name, pred_info, gt, device=None):
    """tools/eval.py:205-250.  `pred_info` = {'conf' [P], 'label_id' [P], 'mask' [P, N]} (eval_map.py:128-131; the mask may
    stay a device tensor), `gt` = the scene's id vector or the path of its val_gt file.  Returns a SceneMatches."""
    gt_ids = load_gt_ids(gt) if isinstance(gt, (str, bytes)) or hasattr(gt, "__fspath__") else gt
    inter_all, uid = overlap_table(pred_info["mask"], gt_ids, device)
    label_id = np.asarray(pred_info["label_id"].cpu() if torch.is_tensor(pred_info["label_id"]) else pred_info["label_id"])
    conf = np.asarray(pred_info["conf"].cpu() if torch.is_tensor(pred_info["conf"]) else pred_info["conf"])
    counts_all = np.bincount(np.searchsorted(uid, np.asarray(gt_ids).astype(np.int64).reshape(-1)), minlength=uid.shape[0])
    return matches_from_table(scene_name, inter_all, uid, counts_all, label_id, conf)


def matches_from_table(scene_name, inter_all, uid, counts_all, label_id, conf):
    """The host tail of tools/eval.py:205-250 on a scene's integer tables: `inter_all` int[P, U] overlap counts against the
    ascending unique ids `uid` [U] with their vertex counts `counts_all` [U]; `label_id` / `conf` [P].  Returns a SceneMatches."""
    # ground-truth instances: ids of benchmark classes (getins.py:59-70; 0 = unannotated never qualifies)
    uid_class = np.array([_CLASS_OF_ID.get(int(u // 1000), -1) for u in uid], np.int64)
    g_cols = np.nonzero((uid != 0) & (uid_class >= 0))[0]
    void_cols = uid_class < 0                                                     # :217 (id 0 included: 0 // 1000 = 0)
    # predictions: benchmark label and at least MIN_REGION_SIZE vertices (:219-229), numbered in input order
    vert_all = inter_all.sum(1)
    pred_class_all = np.array([_CLASS_OF_ID.get(int(l), -1) for l in label_id], np.int64)
    keep = np.nonzero((pred_class_all >= 0) & (vert_all >= MIN_REGION_SIZE))[0]
    inter = inter_all[np.ix_(keep, g_cols)]
    inter = inter * (pred_class_all[keep][:, None] == uid_class[g_cols][None, :])  # :238 same-class instances only
    return SceneMatches(scene_name, uid_class[g_cols], uid[g_cols], counts_all[g_cols].astype(np.int64), pred_class_all[keep],
                        np.arange(keep.shape[0], dtype=np.int64), label_id[keep].astype(np.int64), vert_all[keep],
                        inter_all[keep][:, void_cols].sum(1), conf[keep], inter)


# ------------------------------------------------------------------------------- association without a host stop
# One record per scene in an int32 log (include/pbnet_hip.h, pbn_ap_record_append): header[8] = magic | scene tag | n_keep |
# n_gt | n_pts | status | record words | 0, then uid[n_gt] | gt_vert[n_gt] | label_id[n_keep] | conf[n_keep] (float32 bits) |
# inter[n_keep, n_gt]; a scene without clusters is its header alone.
AP_RECORD_MAGIC, AP_RECORD_HEADER = 0x41504c47, 8
AP_STATUS = ((1, "a superpoint id is >= n_superpoints"),
             (2, "a kept proposal has no first member, or its predicted class is outside the label table"),
             (4, "a ground-truth id is negative or >= id_cap"),
             (8, "the scene has more than u_cap distinct ground-truth ids"),
             (16, "a prediction's label id does not fit 32 bits"),
             (32, "an instance label is >= n_inst_cap"),
             (64, "a semantic label other than -100 is outside the label table"))
AP_STATUS_ID_RANGE, AP_STATUS_ID_COUNT, AP_STATUS_LABEL_RANGE, AP_STATUS_INSTANCE_CAP, AP_STATUS_SEMANTIC_RANGE = 4, 8, 16, 32, 64


def _status_reasons(status):
    """The texts of a record's status bits, empty for a clean record."""
    reasons = [text for bit, text in AP_STATUS if status & bit]
    if status & ~sum(bit for bit, _ in AP_STATUS):
        reasons.append("unknown status bits 0x%x" % status)
    return reasons


def _walk_association_log(words, names):
    """Generator over the records of an association log in log order: (tag, scene name, reasons of its status bits, SceneMatches
    or None for a header-only record).  ValueError for a log that is not a sequence of whole records."""
    words = np.ascontiguousarray(words, dtype=np.int32).reshape(-1)
    pos, end = 0, int(words.shape[0])
    while pos < end:
        if end - pos < AP_RECORD_HEADER or int(words[pos]) != AP_RECORD_MAGIC:
            raise ValueError("the association log has no record header at word %d" % pos)
        tag, n_keep, n_gt, n_pts, status, size = (int(v) for v in words[pos + 1:pos + 7])
        scene = names[tag] if 0 <= tag < len(names) else "<scene tag %d>" % tag
        want = AP_RECORD_HEADER + (2 * n_gt + 2 * n_keep + n_keep * n_gt if n_keep else 0)
        if n_keep < 0 or n_gt < 0 or size != want or pos + size > end:
            raise ValueError("%s: the record at word %d is malformed (n_keep %d, n_gt %d, %d words, %d left)"
                             % (scene, pos, n_keep, n_gt, size, end - pos))
        reasons = _status_reasons(status)
        rec = None
        if n_keep and not reasons:
            body = words[pos + AP_RECORD_HEADER:pos + size]
            uid, vert = body[:n_gt].astype(np.int64), body[n_gt:2 * n_gt].astype(np.int64)
            label_id = body[2 * n_gt:2 * n_gt + n_keep].astype(np.int64)
            conf = body[2 * n_gt + n_keep:2 * n_gt + 2 * n_keep].copy().view(np.float32)
            inter_all = body[2 * n_gt + 2 * n_keep:].astype(np.int64).reshape(n_keep, n_gt)
            rec = matches_from_table(scene, inter_all, uid, vert, label_id, conf)
        yield tag, scene, reasons, rec
        pos += size


def _sort_records(records, on_status):
    """(matches, dropped[, failed]) from walked records, in the order given."""
    if on_status not in ("raise", "skip"):
        raise ValueError("on_status must be 'raise' or 'skip', got %r" % (on_status,))
    matches, dropped, failed = {}, [], []
    for _, scene, reasons, rec in records:
        if reasons:
            if on_status == "raise":
                raise ValueError("%s: %s" % (scene, "; ".join(reasons)))
            failed.append((scene, reasons))
        elif rec is None:
            dropped.append(scene)
        else:
            matches[scene] = rec
    return (matches, dropped) if on_status == "raise" else (matches, dropped, failed)


def decode_association_log(words, names, on_status="raise"):
    """Walk the records of an association log (int32 words as `AssociationLog` leaves them; `names[tag]` = scene name).
    Returns ({scene: SceneMatches} in log order, [names of the scenes without a cluster]): a record with n_keep == 0 yields no
    entry, as train.py:217-219 skips such a scene (tools/eval.py would count its ground-truth instances as misses: run
    assign_instances_for_scan for those names where that is wanted).  ValueError with the scene's name and the reason for any status bit.
    on_status="skip": a scene with status bits is left out of the matches instead and returned in a third list of
    (name, reasons), so one bad scene does not cost the epoch."""
    if on_status not in ("raise", "skip"):
        raise ValueError("on_status must be 'raise' or 'skip', got %r" % (on_status,))
    return _sort_records(_walk_association_log(words, names), on_status)


class AssociationLog(object):
    """The association of an epoch's scenes on the device: `append` enqueues ground-truth numbering (pbn_gt_index_dev), the
    overlap table of capacity-shaped clusters (pbn_instance_overlap_dev) and one record into the epoch log
    (pbn_ap_record_append); `collect` is the single read-back.  Neither `append` nor `append_refined` synchronises, and neither
    allocates once the buffers fit (given int32 clusters, float32 scores and int64 label ids, all contiguous): the work buffers
    grow only, as postprocess.PostWorkspace; the log and its state never move.  One log per stream.

    Capacities: `p_cap` prediction rows and `n_pts_cap` points (both grow on demand), `u_cap` distinct ground-truth ids per
    scene, `id_cap` the bound on an id (ScanNet: NYU40 * 1000 + instance + 1 < 41 000; at most 2^20), `n_inst_cap` the bound on
    an instance label of a (sem, ins) pair (default u_cap), `log_words` the int32 words of the epoch log."""

    def __init__(self, p_cap, n_pts_cap, u_cap=1024, id_cap=65536, log_words=4 << 20, device=None, n_inst_cap=None):
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.u_cap, self.id_cap, self.log_words = int(u_cap), int(id_cap), int(log_words)
        self.n_inst_cap = self.u_cap if n_inst_cap is None else int(n_inst_cap)
        if self.u_cap < 1 or self.n_inst_cap < 1 or self.log_words < 0 or not 1 <= self.id_cap <= (1 << 20):
            raise ValueError("u_cap and n_inst_cap must be positive, log_words >= 0 and id_cap in [1, 2^20]; got %d, %d, %d, %d"
                             % (self.u_cap, self.n_inst_cap, self.log_words, self.id_cap))
        i32 = lambda n: torch.zeros(max(int(n), 1), dtype=torch.int32, device=self.device)            # noqa: E731
        self.state, self.log = i32(8), i32(self.log_words)
        self.scalars = i32(2)                                         # n_gt | association status
        self.table, self.first = i32(self.id_cap), i32(self.n_inst_cap)
        self.uid, self.gt_vert = i32(self.u_cap), i32(self.u_cap)
        self.label_table = torch.tensor(SEMANTIC_LABEL_IDX, dtype=torch.int32, device=self.device)
        self.p_cap = self.n_pts_cap = 0
        self.inter = self.gt_index = self.ids = None
        self._grow(p_cap, n_pts_cap)
        self.batch_ws = self.batch_gt = None                          # append_batch's buffers, made by its first call
        self.batch_n_cap = self.batch_ws_bytes = 0
        self.names = []

    def _grow(self, p_cap, n_pts_cap):
        p, n = max(int(p_cap), self.p_cap, 1), max(int(n_pts_cap), self.n_pts_cap, 1)
        if p * self.u_cap >= 1 << 31:
            raise ValueError("p_cap * u_cap must stay below 2^31, got %d * %d" % (p, self.u_cap))
        if self.inter is None or p > self.p_cap:
            self.inter = torch.zeros(p * self.u_cap, dtype=torch.int32, device=self.device)
        if self.gt_index is None or n > self.n_pts_cap:
            self.gt_index = torch.zeros(n, dtype=torch.int32, device=self.device)
            self.ids = torch.zeros(n, dtype=torch.int32, device=self.device)
        self.p_cap, self.n_pts_cap = p, n

    def reset(self):
        """Forget the epoch: one fill, no synchronisation."""
        self.state.zero_()
        self.names = []

    @staticmethod
    def _labels(t, what, n):
        if not torch.is_tensor(t) or t.dtype not in (torch.int32, torch.int64) or t.dim() != 1 or int(t.shape[0]) != n:
            raise ValueError("%s must be an int32 or int64 device vector of %d entries" % (what, n))
        N.require_cuda(t)
        return t if n == 0 or t.stride(0) == 1 else t.contiguous()

    def append(self, name, clusters, scores, semantic_id, n_keep, status, gt):
        """Enqueue one scene.  `clusters` int32 [P, N] (non-zero = inside; rows from n_keep on are never read), `scores` f32 [P],
        `semantic_id` i64 [P], `n_keep` a device int32 scalar or None = all P rows, `status` the post-processing's device status
        word or None, `gt` a device id vector [N] (int32 / int64) or a (sem, ins) pair of device label vectors [N]."""
        N.require_cuda(clusters, scores, semantic_id, n_keep, status)
        if clusters.dim() != 2:
            raise ValueError("clusters must be [P, N], got %s" % (tuple(clusters.shape),))
        p, n = int(clusters.shape[0]), int(clusters.shape[1])
        if int(scores.numel()) != p or int(semantic_id.numel()) != p:
            raise ValueError("%d cluster rows, %d scores, %d label ids" % (p, scores.numel(), semantic_id.numel()))
        for t, what in ((n_keep, "n_keep"), (status, "status")):
            if t is not None and (t.dtype != torch.int32 or t.numel() != 1):
                raise TypeError("%s must be a device int32 scalar" % what)
        if p > self.p_cap or n > self.n_pts_cap:
            self._grow(p, n)
        clusters = clusters if clusters.dtype == torch.int32 else (clusters != 0).to(torch.int32)
        clusters = clusters.contiguous()
        scores = (scores if scores.dtype == torch.float32 else scores.float()).reshape(-1).contiguous()
        semantic_id = (semantic_id if semantic_id.dtype == torch.int64 else semantic_id.long()).reshape(-1).contiguous()
        lib, st = N.lib(), N.current_stream()
        n_gt, assoc = _word_ptr(self.scalars, 0), _word_ptr(self.scalars, 1)
        if isinstance(gt, (tuple, list)):
            sem, ins = self._labels(gt[0], "sem", n), self._labels(gt[1], "ins", n)
            N.check(lib.pbn_gt_encode_dev(N.ptr(sem), int(sem.dtype == torch.int64), N.ptr(ins), int(ins.dtype == torch.int64), n,
                                          N.ptr(self.label_table), int(self.label_table.numel()), N.ptr(self.first),
                                          self.n_inst_cap, N.ptr(self.ids), assoc, st), "pbn_gt_encode_dev")
            ids = self.ids
        else:
            ids = self._labels(gt, "gt", n)
        N.check(lib.pbn_gt_index_dev(N.ptr(ids), int(ids.dtype == torch.int64), n, N.ptr(self.table), self.id_cap, N.ptr(self.uid),
                                     N.ptr(self.gt_vert), self.u_cap, n_gt, N.ptr(self.gt_index), assoc, st), "pbn_gt_index_dev")
        N.check(lib.pbn_instance_overlap_dev(N.ptr(clusters), N.ptr(n_keep), p, n, N.ptr(self.gt_index), n_gt, self.u_cap,
                                             N.ptr(self.inter), st), "pbn_instance_overlap_dev")
        N.check(lib.pbn_ap_record_append(N.ptr(self.state), N.ptr(self.log), self.log_words, len(self.names), N.ptr(n_keep), p,
                                         n_gt, self.u_cap, n, N.ptr(status), assoc, N.ptr(self.uid), N.ptr(self.gt_vert),
                                         N.ptr(semantic_id), N.ptr(scores), N.ptr(self.inter), st), "pbn_ap_record_append")
        self.names.append(name)

    def append_refined(self, name, refined, gt):
        """`append` on what postprocess.refine_instances_device left: its capacity-sized views and device scalars."""
        self.append(name, refined.clusters, refined.scores, refined.semantic_id, refined.n_keep, refined.status, gt)

    def _grow_batch(self, n_total):
        """The buffers of `append_batch`: the workspace of pbn_ap_assoc_batch for MAX_SCENES scenes and two int64 rows for the
        concatenated ground truth.  They grow only, when a call does not fit."""
        if self.batch_ws is not None and n_total <= self.batch_n_cap:
            return
        n = max(int(n_total), self.batch_n_cap, 1)
        nbytes = int(N.lib().pbn_ap_assoc_batch_workspace_bytes(n, N.MAX_SCENES, self.u_cap, self.id_cap, self.n_inst_cap))
        if nbytes == 0:
            raise ValueError("no workspace for %d points with u_cap %d, id_cap %d, n_inst_cap %d" % (n, self.u_cap, self.id_cap,
                                                                                                    self.n_inst_cap))
        self.batch_ws = torch.zeros(nbytes, dtype=torch.uint8, device=self.device)
        self.batch_gt = torch.zeros(2, n, dtype=torch.int64, device=self.device)
        self.batch_n_cap, self.batch_ws_bytes = n, nbytes

    def append_batch(self, names, refined_batch, gts=None, copies=1, ids=None, sem=None, ins=None, tags=None):
        """Enqueue ALL scenes of one merged forward from what the batched post-processing left on the device (a
        `postprocess.RefinedBatch`: one label per folded point, no dense table): pbn_ap_assoc_batch, six launches whatever the
        number of scenes (eight with (sem, ins) pairs), B records appended in scene order.  The records are the ones `append`
        writes for `refined_batch.dense(j)`, byte for byte, so `collect` decodes them as before.

        names: one per scene.  gts: per scene a device id vector [n_j] (int32 / int64) or a (sem, ins) pair of device label
        vectors [n_j] -- the same form for every scene; they are concatenated into a buffer of this log (no allocation once it
        fits).  Or gts=None and the merged tensors over all N folded points directly: `ids=`, or `sem=` and `ins=`.
        copies: the copies of a scene in the merged forward (`refine_tta_merged_device`); the points here are the folded ones.
        tags: the records' scene tags, default the names' positions in `self.names`, which is what `collect` decodes with.
        Does not synchronise and reads nothing back."""
        rb = refined_batch
        b, starts, n_prop = rb.n_scenes, [int(v) for v in rb.point_starts], int(rb.n_prop)
        n_total = starts[-1]
        names = list(names)
        if len(names) != b:
            raise ValueError("%d names for %d scenes" % (len(names), b))
        tags = [len(self.names) + j for j in range(b)] if tags is None else [int(t) for t in tags]
        if len(tags) != b:
            raise ValueError("%d tags for %d scenes" % (len(tags), b))
        N.require_cuda(rb.point_instance, rb.scalars, rb.scores, rb.semantic_id)
        if (rb.point_instance.dtype != torch.int32 or rb.scores.dtype != torch.float32 or rb.semantic_id.dtype != torch.int64
                or rb.scalars.dtype != torch.int32 or int(rb.scalars.numel()) < 2 * b):
            raise TypeError("refined_batch must hold int32 point_instance and scalars, float32 scores and int64 semantic_id")
        if int(rb.point_instance.numel()) != n_total or int(rb.scores.numel()) != b * n_prop or int(rb.semantic_id.numel()) != b * n_prop:
            raise ValueError("refined_batch does not have the shapes of its scene table")
        self._grow_batch(n_total)
        if gts is not None:
            if ids is not None or sem is not None or ins is not None or len(gts) != b:
                raise ValueError("gts holds one entry per scene (%d) and excludes ids= / sem= / ins=" % b)
            pairs = [isinstance(g, (tuple, list)) for g in gts]
            if any(pairs) != all(pairs):
                raise ValueError("every scene of a call brings the same form of ground truth: ids or a (sem, ins) pair")
            rows = []
            for r in range(2 if pairs[0] else 1):
                parts = [self._labels(g[r] if pairs[0] else g, ("sem", "ins")[r] if pairs[0] else "gt", starts[j + 1] - starts[j])
                         for j, g in enumerate(gts)]
                if b == 1:
                    rows.append(parts[0])
                    continue
                for j, t in enumerate(parts):
                    self.batch_gt[r, starts[j]:starts[j + 1]].copy_(t)
                rows.append(self.batch_gt[r, :n_total])
            ids, sem, ins = (None, rows[0], rows[1]) if pairs[0] else (rows[0], None, None)
        elif ids is not None:
            if sem is not None or ins is not None:
                raise ValueError("ids= excludes sem= / ins=")
            ids = self._labels(ids, "ids", n_total)
        elif sem is not None and ins is not None:
            sem, ins = self._labels(sem, "sem", n_total), self._labels(ins, "ins", n_total)
        else:
            raise ValueError("append_batch needs ground truth: gts, ids= or sem= and ins=")
        table = N.TtaTable()
        table.n_scenes, table.copies = b, int(copies)
        for j in range(b + 1):
            table.point_start[j], table.sp_start[j] = starts[j], 0
        st = N.SceneTags()
        for j in range(b):
            st.tag[j] = tags[j]
        pi, sc = rb.point_instance.contiguous(), rb.scalars.contiguous()
        scores, sid = rb.scores.contiguous(), rb.semantic_id.contiguous()
        i64 = lambda t: int(t is not None and t.dtype == torch.int64)                                  # noqa: E731
        N.check(N.lib().pbn_ap_assoc_batch(table, N.ptr(pi), N.ptr(sc), N.ptr(scores), N.ptr(sid), n_prop, N.ptr(ids), i64(ids),
                                           N.ptr(sem), i64(sem), N.ptr(ins), i64(ins), N.ptr(self.label_table),
                                           int(self.label_table.numel()), self.u_cap, self.id_cap, self.n_inst_cap, st,
                                           N.ptr(self.state), N.ptr(self.log), self.log_words, N.ptr(self.batch_ws),
                                           self.batch_ws_bytes, N.current_stream()), "pbn_ap_assoc_batch")
        self.names.extend(names)

    def read_log(self):
        """The read-back behind `collect`: the used words of the log as a host array; RuntimeError when a record did not fit,
        with the word count the epoch wanted."""
        used, wanted, n_records, overflow = self.state[:4].tolist()
        if overflow:
            raise RuntimeError("the association log overflowed: %d of %d scenes fit in log_words = %d, the epoch wanted %d words"
                               % (n_records, len(self.names), self.log_words, wanted))
        return self.log[:used].cpu().numpy()

    def collect(self, on_status="raise"):
        """The single read-back of the epoch: the state block, then the used part of the log.  Returns what
        `decode_association_log` returns; RuntimeError when a record did not fit, with the word count the epoch wanted."""
        return decode_association_log(self.read_log(), self.names, on_status)


def _word_ptr(t, i):
    """Address of element i of a contiguous tensor."""
    return N.c_vp(t.data_ptr() + i * t.element_size())


class APTableOverflow(RuntimeError):
    """A capacity of an `APTable` did not hold the epoch.  `rec_cap` / `entry_cap`: capacities that hold what this attempt could
    count (records that did not fit were not matched, so their entries are not in the count yet)."""

    def __init__(self, message, rec_cap, entry_cap):
        RuntimeError.__init__(self, message)
        self.rec_cap, self.entry_cap = int(rec_cap), int(entry_cap)


class APTable(object):
    """`evaluate_matches` on the device (csrc/apeval.hip, pbn_ap_table_*): association logs are read where they lie, matched
    and integrated there, and `finish` reads back the table instead of the logs.  `add` does not synchronise and reads nothing
    back; `finish` is the one read-back: the scalar block, the AP cells, the cell counts and four words per record.

    Capacities: `rec_cap` records over all logs added, `entry_cap` (score, true) entries over all cells; the predictions of one
    log need a row each in the same capacity.  12 * (sum of n_keep) entries are always enough (include/pbnet_hip.h); the default
    allows 64 kept predictions per record on average.  Either overflow is reported by `finish` with the wanted capacity
    (`APTableOverflow`; `ap_table_of_logs` answers it by matching the logs again with that capacity)."""

    def __init__(self, rec_cap, entry_cap=None, device=None):
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.rec_cap = int(rec_cap)
        self.entry_cap = 12 * 64 * self.rec_cap if entry_cap is None else int(entry_cap)
        self.n_classes, self.n_overlaps = len(CLASS_LABELS), len(OVERLAPS)
        self.ws_bytes = int(N.lib().pbn_ap_table_workspace_bytes(self.rec_cap, self.entry_cap))
        if self.ws_bytes == 0:
            raise ValueError("no AP table for rec_cap %d and entry_cap %d" % (self.rec_cap, self.entry_cap))
        self.ws = torch.zeros(self.ws_bytes, dtype=torch.uint8, device=self.device)
        self._classes, self._overlaps = N.ApClassIds(), N.ApOverlaps()
        self._classes.n, self._overlaps.n = self.n_classes, self.n_overlaps
        for i, c in enumerate(VALID_CLASS_IDS):
            self._classes.id[i] = int(c)
        for i, th in enumerate(OVERLAPS):
            self._overlaps.th[i] = float(th)                # the np.arange doubles themselves, e.g. 0.6000000000000001
        cells = self.n_classes * self.n_overlaps
        # scalars | ap (float32 bits) | cells | flags | directory: one buffer, one read-back
        self._parts = np.cumsum([0, N.AP_TABLE_SCALARS, cells, 4 * cells, 2 * self.n_classes, 4 * self.rec_cap])
        self.out = torch.zeros(int(self._parts[-1]), dtype=torch.int32, device=self.device)
        self.readback_bytes = 4 * int(self._parts[-1])
        self.names, self.flags, self.scalars, self.directory = [], None, None, None
        self.reset()

    def reset(self):
        """Forget the epoch: one launch, no synchronisation."""
        N.check(N.lib().pbn_ap_table_reset(N.ptr(self.ws), self.ws_bytes, self.rec_cap, self.entry_cap, N.current_stream()),
                "pbn_ap_table_reset")
        self.names = []

    def add(self, log):
        """Match the records of an `AssociationLog` into the table.  Enqueued on the current stream, which must come after the
        stream that wrote the log; the log is only read."""
        self.add_words(log.log, log.state, log.log_words, log.names)

    def add_words(self, words, state, log_words, names, tag_base=None):
        """`add` on the parts of a log: `words` int32 [>= log_words] and `state` int32 [8] on the device (state[0] = the used
        words, state[3] = the log's overflow flag, state[1] the words it wanted), `names[tag]` the scenes' names.  The records'
        tags are shifted by `tag_base`, default the names held so far, so that they index `self.names`."""
        N.require_cuda(words, state)
        if words.dtype != torch.int32 or state.dtype != torch.int32 or int(state.numel()) < 4 or int(words.numel()) < log_words:
            raise TypeError("a log is int32 words with an int32 state block of at least 4 words")
        N.check(N.lib().pbn_ap_table_add_log(N.ptr(self.ws), self.ws_bytes, self.rec_cap, self.entry_cap, N.ptr(state),
                                             N.ptr(words), int(log_words), len(self.names) if tag_base is None else int(tag_base),
                                             self._classes, self._overlaps,
                                             MIN_REGION_SIZE, N.current_stream()), "pbn_ap_table_add_log")
        self.names.extend(names)

    def finish(self):
        """Integrate and read back.  Returns (ap float32 [1, classes, overlaps] as `evaluate_matches` gives it, names of the
        scenes without a cluster, [(name, reasons)] of the scenes left out for their status bits, cells int32 [classes,
        overlaps, 4] = entries | true entries | hard_fn | distinct scores).  RuntimeError when a log had overflowed or a capacity
        of the table did, with the wanted capacity; ValueError for a log that is not a sequence of whole records."""
        a = self._parts
        part = lambda i: _word_ptr(self.out, int(a[i]))                                               # noqa: E731
        N.check(N.lib().pbn_ap_table_finish(N.ptr(self.ws), self.ws_bytes, self.rec_cap, self.entry_cap, self.n_classes,
                                            self.n_overlaps, part(1), part(2), part(3), part(4), part(0), N.current_stream()),
                "pbn_ap_table_finish")
        host = self.out.cpu().numpy()
        sc = self.scalars = host[a[0]:a[1]].copy()
        n_rec, rec_wanted, entries_wanted, preds_wanted, overflow, malformed, malformed_at, log_over, log_wanted = \
            (int(v) for v in sc[:9])
        if log_over:
            raise RuntimeError("an association log overflowed: the epoch wanted %d words" % log_wanted)
        if malformed == 2:
            raise ValueError("the record at word %d of log %d has more than 65535 predictions" % (malformed_at, int(sc[11])))
        if malformed:
            raise ValueError("an association log is malformed: no whole record at word %d" % malformed_at)
        # 12 entries per prediction are always enough; a log whose rows did not fit was not matched, so its entries are not counted
        enough = 12 * preds_wanted * max(int(sc[11]), 1) if overflow & 4 else max(entries_wanted, preds_wanted, self.entry_cap)
        if overflow & 1:
            raise APTableOverflow("the AP table overflowed: rec_cap = %d, the epoch wanted %d records" % (self.rec_cap, rec_wanted),
                                  rec_wanted, enough)
        if overflow:
            raise APTableOverflow("the AP table overflowed: entry_cap = %d, the epoch wanted %d entries and its largest log %d "
                                  "prediction rows" % (self.entry_cap, entries_wanted, preds_wanted), self.rec_cap, enough)
        ap = host[a[1]:a[2]].view(np.float32).reshape(1, self.n_classes, self.n_overlaps).copy()
        cells = host[a[2]:a[3]].reshape(self.n_classes, self.n_overlaps, 4).copy()
        self.flags = host[a[3]:a[4]].reshape(2, self.n_classes).copy()
        self.directory = host[a[4]:a[5]].reshape(self.rec_cap, 4)[:n_rec].copy()
        dropped, failed = [], []
        for _, tag, status, n_keep in self.directory.tolist():
            scene = self.names[tag] if 0 <= tag < len(self.names) else "<scene tag %d>" % tag
            reasons = _status_reasons(status)
            if reasons:
                failed.append((scene, reasons))
            elif n_keep == 0:
                dropped.append(scene)
        return ap, dropped, failed, cells


def ap_table_of_logs(logs, names=None, rec_cap=None, entry_cap=None, device=None):
    """The `APTable` of an epoch's `AssociationLog`s: (ap, dropped, failed, cells, table).  `names` None: every log's tags count
    within its own names; else the tags of all logs index `names` (the serving front's global submission numbers).  The
    capacities are a first guess (default: one record per name, `APTable`'s entries): when the table reports an overflow the
    logs, which are only read, are matched again into a table of the capacities it asked for -- the records first, then the
    prediction rows, then the entries -- so an epoch is not lost to a guess.  Each attempt is one read-back."""
    logs = list(logs)
    if rec_cap is None:
        rec_cap = max(sum(len(log.names) for log in logs) if names is None else len(names), 1)
    device = logs[0].device if device is None and logs else device
    for attempt in range(4):
        table = APTable(rec_cap, entry_cap, device=device)
        if names is not None:
            table.names = list(names)
        for log in logs:
            table.add_words(log.log, log.state, log.log_words, log.names if names is None else (),
                            tag_base=None if names is None else 0)
        try:
            return table.finish() + (table,)
        except APTableOverflow as e:
            if attempt == 3:
                raise
            rec_cap, entry_cap = e.rec_cap, e.entry_cap


# ----------------------------------------------------------------------------------------------------------- AP
def _as_records(matches):
    out = []
    for scene, m in (matches.items() if isinstance(matches, dict) else enumerate(matches)):
        out.append(m if isinstance(m, SceneMatches) else SceneMatches.from_reference(scene, m["gt"], m["pred"]))
    return out


def _match_scene_class(m, g_sel, q_sel, th, visited):
    """Greedy assignment of one class in one scene at one overlap threshold (tools/eval.py:60-125).  Returns
    (y_true, y_score, hard false negatives).  `visited` (per prediction of the scene) is updated in place."""
    inter = m.inter[np.ix_(q_sel, g_sel)]
    union = m.pred_vert[q_sel][:, None] + m.gt_vert[g_sel][None, :] - inter
    over = (inter > 0) & (inter.astype(np.float64) / np.maximum(union, 1) > th)
    ok_gt = (m.gt_id[g_sel] >= 1000) & (m.gt_vert[g_sel] >= MIN_REGION_SIZE)                  # :49-51
    conf = m.pred_conf[q_sel]
    y_true, y_score, hard_fn = [], [], 0
    for g in np.nonzero(ok_gt)[0]:
        best = None
        for q in np.nonzero(inter[:, g] > 0)[0]:              # `matched_pred`, in prediction order
            if visited[q_sel[q]] or not over[q, g]:
                continue
            if best is None:
                best = conf[q]
                visited[q_sel[q]] = True
            else:                                             # second hit on a matched instance: the lower score is a
                y_true.append(0.0)                            # false positive and the prediction stays unvisited (:78-86)
                y_score.append(min(best, conf[q]))
                best = max(best, conf[q])
        if best is None:
            hard_fn += 1
        else:
            y_true.append(1.0)
            y_score.append(best)
    # predictions without any instance above the threshold (:102-121) -- all same-class instances count, also small ones
    lonely = ~over.any(axis=1)
    ignore = m.pred_void[q_sel] + (inter * (~ok_gt)[None, :]).sum(1)
    for q in np.nonzero(lonely)[0]:
        if float(ignore[q]) / m.pred_vert[q_sel[q]] <= th:
            y_true.append(0.0)
            y_score.append(conf[q])
    return y_true, y_score, hard_fn


def _average_precision(y_true, y_score, hard_fn):
    """Area under the precision/recall curve as tools/eval.py:131-176 integrates it."""
    order = np.argsort(y_score, kind="stable")
    score, true = y_score[order], y_true[order]
    _, first = np.unique(score, return_index=True)            # first position of every distinct score
    below = np.concatenate([[0.0], np.cumsum(true)])[first]    # true matches scored strictly lower
    n_true = float(true.sum())
    tp = n_true - below
    fp = (score.shape[0] - first) - tp
    fn = below + hard_fn
    precision = np.append(tp / (tp + fp), 1.0)                # the artificial last point (:161-162)
    recall = np.append(tp / (tp + fn), 0.0)
    r = np.concatenate([recall[:1], recall, [0.0]])
    width = np.convolve(r, [-0.5, 0, 0.5], "valid")
    return np.dot(precision, width)


def evaluate_matches(matches):
    """tools/eval.py:27-190.  `matches`: {scene: SceneMatches} or the reference's {scene: {'gt':…, 'pred':…}}.
    Returns ap float32[1, classes, overlaps] (nan = class without ground truth)."""
    recs = _as_records(matches)
    ap = np.zeros((1, len(CLASS_LABELS), len(OVERLAPS)), np.float32)
    sel = [[(np.nonzero(m.gt_class == li)[0], np.nonzero(m.pred_class == li)[0]) for li in range(len(CLASS_LABELS))]
           for m in recs]
    for oi, th in enumerate(OVERLAPS):
        visited = [np.zeros(m.pred_id.shape[0], bool) for m in recs]
        for li in range(len(CLASS_LABELS)):
            y_true, y_score, hard_fn, has_gt, has_pred = [], [], 0, False, False
            for si, m in enumerate(recs):
                g_sel, q_sel = sel[si][li]
                has_gt |= bool(((m.gt_id[g_sel] >= 1000) & (m.gt_vert[g_sel] >= MIN_REGION_SIZE)).any())
                has_pred |= q_sel.shape[0] > 0
                if g_sel.shape[0] == 0 and q_sel.shape[0] == 0:
                    continue
                t, s, h = _match_scene_class(m, g_sel, q_sel, th, visited[si])
                y_true += t
                y_score += s
                hard_fn += h
            if has_gt and has_pred:
                ap[0, li, oi] = _average_precision(np.array(y_true, np.float64), np.array(y_score, np.float64), hard_fn)
            elif has_gt:
                ap[0, li, oi] = 0.0
            else:
                ap[0, li, oi] = float("nan")
    return ap


def compute_averages(aps):
    """tools/eval.py:193-210 (same keys)."""
    o50 = np.where(np.isclose(OVERLAPS, 0.5))
    o25 = np.where(np.isclose(OVERLAPS, 0.25))
    rest = np.where(np.logical_not(np.isclose(OVERLAPS, 0.25)))
    avg = {"all_ap": np.nanmean(aps[0, :, rest]), "all_ap_50%": np.nanmean(aps[0, :, o50]),
           "all_ap_25%": np.nanmean(aps[0, :, o25]), "classes": {}}
    for li, name in enumerate(CLASS_LABELS):
        avg["classes"][name] = {"ap": np.average(aps[0, li, rest]), "ap50%": np.average(aps[0, li, o50]),
                                "ap25%": np.average(aps[0, li, o25])}
    return avg


def evaluate_served(server_or_model, units, cfg, logger=None, tta=3, device_table=False):
    """eval_map.py:40-158 on the serving front: every unit is submitted with its ground truth, the front post-processes and
    associates on the device (`SceneServer(..., refine=cfg, association=True)`), and the epoch ends in `evaluate_matches`,
    `compute_averages` and `print_results`.  `units`: (name, unit, gt) triples -- `unit` what `SceneServer.submit` takes (with tta
    the reference's evaluation unit of `tta` rotated copies), `gt` a device id vector over the scene's own points or a (sem, ins)
    pair.  `server_or_model`: a paused or running `SceneServer` built with association=True (it is closed here), or a model, for
    which one is made with refine=cfg and `tta` copies per unit (None: plain scenes).  Scenes without a kept instance are
    reported and left out (eval_map.py:102-104), as are scenes whose result or record reports an error.  Returns the averages.
    device_table=True: matching and integration run on the device as well (`SceneServer.ap_table`, `APTable`): the logs are not
    read back, the same lines are reported and the AP cells agree with the default form to one float32 ulp."""
    from .serving import SceneServer
    say = print if logger is None else logger.info
    server = server_or_model
    if not isinstance(server, SceneServer):
        server = SceneServer(server_or_model, refine=cfg, tta=tta, association=True)
    if not getattr(server, "association_on", False):
        raise ValueError("evaluate_served needs a SceneServer built with association=True")
    futs = [(name, server.submit(unit, gt=gt, name=name)) for name, unit, gt in units]
    server.close()
    for name, f in futs:
        if f.exception() is not None:
            say("%s: not served: %s" % (name, f.exception()))
    if device_table:
        ap, dropped, failed, _ = server.ap_table()
    else:
        matches, dropped, failed = server.association()
    for name in dropped:
        say("%s: no instance kept, left out" % (name,))
    for name, reasons in failed:
        say("%s: left out: %s" % (name, "; ".join(reasons)))
    avgs = compute_averages(ap if device_table else evaluate_matches(matches))
    print_results(avgs, logger)
    return avgs


def format_results(avgs):
    """The table tools/eval.py:253-290 prints, as a list of lines."""
    lines = ["", "#" * 64, "{:<15}:{:>15}{:>15}{:>15}".format("what", "AP", "AP_50%", "AP_25%"), "#" * 64]
    for name in CLASS_LABELS:
        c = avgs["classes"][name]
        lines.append("{:<15}:{:>15.3f}{:>15.3f}{:>15.3f}".format(name, c["ap"], c["ap50%"], c["ap25%"]))
    lines += ["-" * 64, "{:<15}:{:>15.3f}{:>15.3f}{:>15.3f}".format("average", avgs["all_ap"], avgs["all_ap_50%"],
                                                                   avgs["all_ap_25%"]), ""]
    return lines


def print_results(avgs, logger=None):
    """tools/eval.py:253-326: the table through `logger.info` (or print)."""
    for line in format_results(avgs):
        (print if logger is None else logger.info)(line)
