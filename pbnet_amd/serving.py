"""Serving front of the inference path (round 6): the scenes WAITING on a GPU are merged into one `PBNet.forward` through the
reference's own batch axis, and the results are handed back per scene.

Why: the coarse levels of the three U-Nets (stride 4 / 8 / 16: 93 of the 138 convolution launches of a forward) are launches of a
few hundred to a few thousand rows -- latency chains that one scene cannot fill; B scenes in one forward give
every launch B x the rows for the same number of launches.  The reference already batches this way: `dataset_preprocess.py:296`
collates with a batch index, `network/PBNet.py:167-176` groups per (class, batch element), its evaluation feeds the three
test-time copies of a scene as a batch of 3 (`eval_map.py:48-50`, `dataset_preprocess.py:324`).  `tests/test_batched_gpu.py` pins
the property this module rests on: a merged forward returns, for every scene, the proposals and scores of that scene's own forward.

    server = SceneServer(model, max_batch=4, forwards_in_flight=2)
    fut = server.submit(scene)           # scene: dict(xyz_voxel [V,4] int32, feat_voxel [V,C], xyz_original [N,3], v2p_index [N]) on the GPU
    res = fut.result()                   # dict(sem_pred_p [N], proposals (idx [M,2], offset [P+1]), clt_scores [P]) of THAT scene
    server.close()

With `SceneServer(..., refine=cfg)` a scene's result is what `eval_map.py` ends with instead of proposals: the merged forward's
post-processing runs once for all its scenes (`postprocess.refine_batch_device`, csrc/post_batch.hip) in place of `split_results`,
and `res["instances"]` is dict(point_instance [N], scores [K], semantic_id [K], npoints [K]).  A scene may then carry `sup`
(int64 device superpoint ids) and `n_superpoints` (their upper bound).

With `SceneServer(..., refine=cfg, tta=3)` what is submitted is the reference's evaluation unit (eval_map.py:48-70): the three rotated
copies of a scene as a batch of 3, as `DeviceMerge.val_merge([id])` or `synth.make_val_batch(copies=3)` build it.  Up to
MAX_SCENES // 3 = 2 waiting units share one forward (6 batch elements), the post-processing folds every unit's copies onto the
scene's own points (`postprocess.refine_tta_merged_device`), and `res["instances"]["point_instance"]` has one entry per point of
the scene, `res["sem_pred_p"]` the unit's 3 n labels.

With `SceneServer(..., refine=cfg, summary=True)` the scene summary (`postprocess.summarize_merged_device`, csrc/summary.hip)
runs behind the post-processing, ahead of the same read-back: `res["sem_fold"]` holds one label per point of the scene (with tta
the copies' scores summed in float32, copy after copy, then the first maximum), `res["instances"]` gains `class_vote` and
`class_points` (the class the instance's points vote for -- what the reference's submission writer records, eval_map.py:142-155
-- and its count), `box` [K, 6] and `centroid` [K, 3].  Coordinates are `xyz_original` without tta; with tta the unit's optional
`xyz_scene` (float32 [n, 3], the unrotated scene), and `box` / `centroid` are None for a unit without it.

With `SceneServer(..., refine=cfg, association=True)` the front scores its own output: every submission brings its ground truth
(`submit(scene, gt=ids)` or `gt=(sem, ins)`, device vectors over the scene's own points), and behind the post-processing of a
merged forward the AP association of all its scenes is enqueued on the worker's stream (`evaluate.AssociationLog.append_batch`,
csrc/apassoc_batch.hip: six launches per forward, nothing read back).  Results are unchanged; after `close()`,
`server.association()` reads every worker's log once and returns `(matches, dropped, failed)` in submission order, ready for
`evaluate.evaluate_matches` -- `evaluate.evaluate_served` is the whole of eval_map.py:40-158 on this front.

`merge_scenes` / `split_results` are the two pure functions; `SceneServer` is the small scheduler around them: F worker threads,
each with its own HIP stream (create the server FIRST in a process: the runtime maps a process's first streams to distinct
hardware queues), each taking up to `max_batch` waiting scenes per forward -- it never waits for a batch to fill:
a lone scene is served alone.
"""
import queue
import threading
from concurrent.futures import Future

import torch

from . import evaluate, postprocess
from ._native import MAX_SCENES


def merge_superpoints(scenes, point_starts):
    """The superpoint side of a merged batch: (ids int64 [N_total] or None, sp_starts [B + 1]).  Scene j's ids stay scene-local
    and vote in rows sp_starts[j] : sp_starts[j + 1] of one flat table; a scene without `sup` gets an empty slice (and zeros in
    the merged ids, which are never read).  Host arithmetic and one concatenation; None when no scene brings ids."""
    has = [s.get("sup") is not None for s in scenes]
    sp_starts = postprocess.superpoint_starts(point_starts, has, [s.get("n_superpoints") for s in scenes])
    if not any(has):
        return None, sp_starts
    parts = []
    for j, s in enumerate(scenes):
        n = point_starts[j + 1] - point_starts[j]
        if has[j]:
            if s["sup"].dtype != torch.int64 or int(s["sup"].numel()) != n:
                raise ValueError("scene %d: `sup` must hold %d int64 ids" % (j, n))
            parts.append(s["sup"].view(-1))
        else:
            parts.append(torch.zeros(n, dtype=torch.int64, device=s["xyz_original"].device))
    return (parts[0] if len(parts) == 1 else torch.cat(parts)), sp_starts


def merge_scenes(scenes, teachers=None, with_superpoints=False):
    """B scenes -> one batch: scene j becomes batch element j (the batch column of its voxel coordinates is overwritten), voxel
    and point arrays are concatenated in scene order, `v2p_index` is shifted by the voxels in front.  Returns (batch, teacher or
    None, point_starts [B + 1] -- the rows of xyz_original / sem_pred_p that belong to scene j are point_starts[j] : [j + 1]).
    with_superpoints: a fourth element, `merge_superpoints(scenes, point_starts)` -- with point_starts the scene table of
    `postprocess.refine_merged_device`."""
    if with_superpoints:
        batch, teacher, starts = merge_scenes(scenes, teachers)
        return batch, teacher, starts, merge_superpoints(scenes, starts)
    if len(scenes) == 1:                                  # a lone scene: nothing to concatenate
        s = scenes[0]
        xv = s["xyz_voxel"].clone()
        xv[:, 0] = 0
        return ({"xyz_voxel": xv, "feat_voxel": s["feat_voxel"], "xyz_original": s["xyz_original"], "v2p_index": s["v2p_index"]},
                None if teachers is None else teachers[0], [0, int(s["xyz_original"].shape[0])])
    vox, feat, xyz, v2p, starts = [], [], [], [], [0]
    nv = 0
    for j, s in enumerate(scenes):
        xv = s["xyz_voxel"].clone()
        xv[:, 0] = j
        vox.append(xv)
        feat.append(s["feat_voxel"])
        xyz.append(s["xyz_original"])
        v2p.append(s["v2p_index"] + nv)
        nv += int(xv.shape[0])
        starts.append(starts[-1] + int(s["xyz_original"].shape[0]))
    batch = {"xyz_voxel": torch.cat(vox), "feat_voxel": torch.cat(feat), "xyz_original": torch.cat(xyz), "v2p_index": torch.cat(v2p)}
    teacher = None
    if teachers is not None and teachers[0] is not None:
        teacher = {k: torch.cat([t[k] for t in teachers]) for k in teachers[0]}
    return batch, teacher, starts


def merge_tta_units(units, copies=3, teachers=None):
    """B test-time-augmentation units -> one batch of B * copies batch elements.  A unit is one scene as valMerge builds it:
    `copies` rotated copies one after the other -- xyz_voxel with batch column 0 .. copies - 1, feat_voxel, xyz_original
    [copies * n, 3], v2p_index [copies * n], optionally `sup` (int64 [n], one id per point of the scene) and `n_superpoints`.
    Unit j's batch column becomes copies * j + c, `v2p_index` is shifted by the voxels in front.  Returns (batch, point_starts,
    (superpoint ids int64 [N_folded] or None, sp_starts)) with point_starts the B + 1 starts over FOLDED points (unit j owns the
    merged points copies * point_starts[j] : copies * point_starts[j + 1]) -- the table of `postprocess.refine_tta_merged_device`.
    `teachers`: one dict per unit or None for all; the merged one is batch["teacher"] (None without)."""
    copies = int(copies)
    if copies < 1 or not 1 <= len(units) * copies <= MAX_SCENES:
        raise ValueError("a merged forward holds 1..%d batch elements, got %d units x %d copies" % (MAX_SCENES, len(units), copies))
    teachers = [None] * len(units) if teachers is None else list(teachers)
    if len(teachers) != len(units) or len({t is None for t in teachers}) > 1:
        raise ValueError("teachers must be given for every unit of a merged forward or for none")
    vox, feat, xyz, v2p, starts = [], [], [], [], [0]
    nv = 0
    for j, u in enumerate(units):
        n_all = int(u["xyz_original"].shape[0])
        if n_all % copies or int(u["v2p_index"].shape[0]) != n_all:
            raise ValueError("unit %d: %d points (%d v2p entries) are not %d copies of one scene" % (j, n_all, u["v2p_index"].shape[0],
                                                                                                  copies))
        xv = u["xyz_voxel"].clone()
        if j:
            xv[:, 0] += copies * j
        vox.append(xv)
        feat.append(u["feat_voxel"])
        xyz.append(u["xyz_original"])
        v2p.append(u["v2p_index"] + nv if nv else u["v2p_index"])
        nv += int(xv.shape[0])
        starts.append(starts[-1] + n_all // copies)
    one = len(units) == 1
    batch = {"xyz_voxel": vox[0] if one else torch.cat(vox), "feat_voxel": feat[0] if one else torch.cat(feat),
             "xyz_original": xyz[0] if one else torch.cat(xyz), "v2p_index": v2p[0] if one else torch.cat(v2p), "teacher": None}
    if teachers[0] is not None:
        batch["teacher"] = teachers[0] if one else {k: torch.cat([t[k] for t in teachers]) for k in teachers[0]}
    return batch, starts, merge_superpoints(units, starts)


def split_results(ret, point_starts):
    """The merged forward's results -> one result per scene, in the reference's own output form (`proposals_idx` rows are
    (proposal, point) with the proposal numbered from 0 and the point index local to the scene; `proposals_offset` starts at 0).
    A proposal belongs to the scene its points lie in (a local scene never crosses batch elements: PBNet.py:167-176).
    One small read-back (proposals and rows per scene); everything else stays on the device."""
    n_scenes = len(point_starts) - 1
    if n_scenes == 1:
        out = {"sem_pred_p": ret["sem_pred_p"]}
        if "proposals" in ret:
            out["proposals"], out["clt_scores"] = (ret["proposals"][0], ret["proposals"][1]), ret["clt_scores"]
        return [out]
    dev = ret["sem_pred_p"].device
    sem = ret["sem_pred_p"]
    out = [{"sem_pred_p": sem[point_starts[j]:point_starts[j + 1]]} for j in range(n_scenes)]
    if "proposals" not in ret:
        return out
    idx, off = ret["proposals"][0], ret["proposals"][1]
    scores = ret["clt_scores"]
    n_prop = int(off.shape[0]) - 1
    if n_prop <= 0:
        for o in out:
            o["proposals"] = (idx[:0], off[:1].clone())
            o["clt_scores"] = scores[:0]
        return out
    starts_d = torch.tensor(point_starts, dtype=idx.dtype, device=dev)
    off = off.to(torch.int64)
    sizes = off[1:] - off[:-1]
    first_pt = idx[off[:-1], 1]
    scene = torch.searchsorted(starts_d, first_pt, right=True) - 1                  # [P]
    order = torch.sort(scene, stable=True)[1]                                       # proposals grouped by scene, their order kept
    scene_s, sizes_s = scene[order], sizes[order]
    new_off = torch.zeros(n_prop + 1, dtype=torch.int64, device=dev)
    new_off[1:] = torch.cumsum(sizes_s, 0)
    # rows of proposal order[q] move to new_off[q] .. : source row of every destination row
    rep = torch.repeat_interleave(torch.arange(n_prop, device=dev), sizes_s, output_size=int(idx.shape[0]))   # destination row -> its (new) proposal
    src = off[order][rep] + (torch.arange(rep.shape[0], device=dev) - new_off[:-1][rep])
    rows = idx[src]
    pts_local = rows[:, 1] - starts_d[scene_s][rep]
    props = torch.bincount(scene_s, minlength=n_scenes)                             # proposals per scene
    nrows = torch.bincount(scene_s, weights=sizes_s.double(), minlength=n_scenes).long()
    counts = torch.stack([props, nrows]).cpu().tolist()                             # the one read-back
    scores_s = scores[order]
    p0 = r0 = 0
    for j in range(n_scenes):
        p1, r1 = p0 + int(counts[0][j]), r0 + int(counts[1][j])
        pid = rep[r0:r1] - p0
        out[j]["proposals"] = (torch.stack([pid.to(idx.dtype), pts_local[r0:r1]], 1), (new_off[p0:p1 + 1] - r0).to(ret["proposals"][1].dtype))
        out[j]["clt_scores"] = scores_s[p0:p1]
        p0, r0 = p1, r1
    return out


class SceneServer(object):
    """F forwards in flight x up to B scenes per forward.  `submit` returns a Future; `close` drains the queue."""

    def __init__(self, model, max_batch=None, forwards_in_flight=2, device=None, epoch=1, split=True, streams=None, refine=None,
                 paused=False, tta=None, summary=False, association=False):
        """refine: an object with TEST_SCORE_THRESH, TEST_NPOINT_THRESH and TEST_NMS_THRESH -- every scene's result is then
        dict(sem_pred_p, instances) (module docstring); a scene whose superpoint ids or classes are out of range gets a ValueError
        on its own future, its batch-mates their results.  None (default): the raw forward results, as before.
        paused: the workers start with `start()`, so scenes can be queued before the first forward is cut.
        streams: the HIP streams of the workers (default: `forwards_in_flight` new ones; a process that already owns its
        in-flight streams passes them: streams created later can share a hardware queue -- DESIGN.md section 5, round 5 item 6b).
        max_batch: scenes (with tta: units) per forward at most; default 4, with tta min(4, MAX_SCENES // tta).
        tta: copies per submitted unit (the reference evaluates with 3).  `submit` then takes a unit (`merge_tta_units`), a forward
        holds up to MAX_SCENES // tta units, and a unit's result is dict(sem_pred_p [tta * n], instances over the scene's n
        points), the copies folded in the post-processing -- which is why tta needs refine.  None (default): as before.
        summary: every result also carries the scene summary (module docstring); it reads the post-processing's results on the
        device, so it needs refine.  A scene whose summary status is set (a coordinate that is NaN or outside +-32768, a voted
        class outside the label table) gets a ValueError on its own future.  False (default): the results are as before.
        association: True, or a dict of `evaluate.AssociationLog` capacities (u_cap, id_cap, n_inst_cap, log_words): every
        submission brings `gt`, every worker appends the records of its forwards to a log of its own (one log per stream) with
        the GLOBAL submission number as the tag, and `association()` merges them after `close()`.  It reads the
        post-processing's results on the device, so it needs refine; it adds no read-back.  False (default): as before."""
        if association and refine is None:
            raise ValueError("association needs refine: it scores the instances of the post-processing")
        self.association_on = bool(association)
        self._assoc_kw = dict(association) if isinstance(association, dict) else {}
        self._logs, self._names, self._unserved, self._gt_pairs = [], [], [], None
        if summary and refine is None:
            raise ValueError("summary needs refine: it summarises the instances of the post-processing")
        self.summary = bool(summary)
        if tta is not None:
            if refine is None:
                raise ValueError("tta needs refine: the copies are folded in the post-processing")
            if not 1 <= int(tta) <= MAX_SCENES:
                raise ValueError("tta must be in 1..%d (the batch axis of the forward's tables), got %r" % (MAX_SCENES, tta))
            tta = int(tta)
        most = MAX_SCENES if tta is None else MAX_SCENES // tta
        if max_batch is None:
            max_batch = min(4, most)
        if not 1 <= int(max_batch) <= most:
            raise ValueError("max_batch must be in 1..%d (the batch axis of the forward's tables%s), got %r" % (
                most, "" if tta is None else ", %d copies per unit" % tta, max_batch))
        self.model, self.max_batch, self.epoch, self.split, self.refine, self.tta = model, int(max_batch), epoch, split, refine, tta
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self._q = queue.Queue()
        self._closed = False
        self.forwards = 0              # merged forwards run so far
        self.scenes = 0                # scenes served so far
        self._lock = threading.Lock()
        self._streams = list(streams) if streams is not None else [torch.cuda.Stream(self.device) for _ in range(int(forwards_in_flight))]
        self._threads = [threading.Thread(target=self._worker, args=(st,), daemon=True) for st in self._streams]
        self._started = False
        if not paused:
            self.start()

    def start(self):
        """Start the workers of a server created with paused=True (no effect on a running one)."""
        with self._lock:
            if self._started:
                return
            self._started = True
        for t in self._threads:
            t.start()

    def _gt_problem(self, scene, gt):
        """Why `gt` cannot be the ground truth of `scene` (None when it can): host checks only."""
        n = int(scene["xyz_original"].shape[0]) // (1 if self.tta is None else self.tta)
        parts = list(gt) if isinstance(gt, (tuple, list)) else [gt]
        if gt is None or len(parts) not in (1, 2) or (len(parts) == 1 and isinstance(gt, (tuple, list))):
            return "association needs `gt`: a device id vector or a (sem, ins) pair over the scene's %d points" % n
        for t in parts:
            if (not torch.is_tensor(t) or not t.is_cuda or t.dtype not in (torch.int32, torch.int64) or t.dim() != 1
                    or int(t.shape[0]) != n):
                return "`gt` must hold int32 or int64 device vectors of the scene's %d points" % n
        with self._lock:                        # a merged forward takes one form of ground truth: the first submission sets it
            if self._gt_pairs is None:
                self._gt_pairs = len(parts) == 2
        if self._gt_pairs != (len(parts) == 2):
            return "every submission of a server brings the same form of `gt`: id vectors or (sem, ins) pairs"
        return None

    def submit(self, scene, teacher=None, gt=None, name=None):
        """Queue one scene (with tta: one unit); returns its Future.  gt / name: with association, the scene's ground truth and
        the name of its record (default: the submission number); a submission whose `gt` is missing or not over the scene's own
        points gets a ValueError on its future and is not served."""
        if self._closed:
            raise RuntimeError("SceneServer is closed")
        f = Future()
        number = None
        if self.association_on:
            with self._lock:
                number = len(self._names)
                self._names.append(number if name is None else name)
            problem = self._gt_problem(scene, gt)
            if problem is not None:
                with self._lock:
                    self._unserved.append((number, problem))
                f.set_exception(ValueError("submission %r: %s" % (self._names[number], problem)))
                return f
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(self.device))        # the scene's tensors are ready when the submitting stream gets here
        self._q.put((scene, teacher, f, ev, gt, number))
        return f

    def association(self):
        """After `close()`: (matches, dropped, failed) of everything served with association=True -- what
        `evaluate.decode_association_log(..., on_status="skip")` returns, over the records of ALL workers merged in submission
        order, so the AP does not depend on how scenes were batched or which worker took them.  `failed` also lists the
        submissions that were refused for their `gt`.  Reads each worker's log once; RuntimeError when a log overflowed."""
        if not self.association_on:
            raise ValueError("this server was built without association=True")
        if not self._closed or any(t.is_alive() for t in self._threads):
            raise RuntimeError("association() reads the logs after close()")
        records = [(number, self._names[number], [problem], None) for number, problem in self._unserved]
        for log in self._logs:
            records += list(evaluate._walk_association_log(log.read_log(), self._names))
        records.sort(key=lambda r: r[0])
        return evaluate._sort_records(records, "skip")

    def ap_table(self, entry_cap=None):
        """After `close()`: `association()` followed by `evaluate.evaluate_matches`, on the device -- every worker's log is
        folded into one `evaluate.APTable` where it lies, and one read-back returns (ap float32 [1, classes, overlaps], dropped,
        failed, cells), the lists in submission order as `association()` gives them.  `entry_cap`: the table's first entry capacity
        (default: `APTable`'s; a table that overflows is built again with the capacity it asked for).  RuntimeError when a log
        overflowed."""
        if not self.association_on:
            raise ValueError("this server was built without association=True")
        if not self._closed or any(t.is_alive() for t in self._threads):
            raise RuntimeError("ap_table() reads the logs after close()")
        with torch.cuda.device(self.device):
            torch.cuda.synchronize(self.device)         # the workers' streams wrote the logs; this thread's stream reads them
            # the records carry the GLOBAL submission number, so every log's tags index self._names
            ap, _, _, cells, table = evaluate.ap_table_of_logs(self._logs, self._names, entry_cap=entry_cap, device=self.device)
        dropped = [(tag, self._names[tag]) for _, tag, status, n_keep in table.directory.tolist() if not status and not n_keep]
        failed = [(number, (self._names[number], [problem])) for number, problem in self._unserved]
        failed += [(tag, (self._names[tag], evaluate._status_reasons(status)))
                   for _, tag, status, _ in table.directory.tolist() if status]
        return ap, [name for _, name in sorted(dropped)], [f for _, f in sorted(failed, key=lambda t: t[0])], cells

    def close(self):
        self._closed = True
        self.start()                        # a paused server still serves what was queued
        for _ in self._threads:
            self._q.put(None)
        for t in self._threads:
            t.join()

    def _take(self):
        """Block for one scene, then take what else is waiting, up to max_batch; None = shut down."""
        first = self._q.get()
        if first is None:
            return None
        items = [first]
        while len(items) < self.max_batch:
            try:
                nxt = self._q.get_nowait()
            except queue.Empty:
                break
            if nxt is None:                 # a shutdown token meant for some worker: put it back behind this batch
                self._q.put(None)
                break
            items.append(nxt)
        return items

    def _associate(self, rb, copies, assoc):
        """Enqueue the association of a merged forward's scenes behind its post-processing: no read-back."""
        if assoc is not None:
            log, names, gts, numbers = assoc
            log.append_batch(names, rb, gts, copies=copies, tags=numbers)

    def _refined(self, ret, starts, sup, ws, xyz=None, has_xyz=None, assoc=None):
        """Post-process the merged result for all its scenes; one read-back.  Returns (per-scene results or exceptions, workspace).
        The outputs are copied out of the worker's workspace: the next forward of this worker overwrites it.  With summary the
        workspace is the pair (post-processing, summary); xyz: the merged scenes' own coordinates [N, 3] or None, has_xyz: which
        scenes brought them."""
        n_prop = max(int(ret["proposals"][1].shape[0]) - 1, 0)
        ws, sws = ws if isinstance(ws, tuple) else (ws, None)
        sizes = (n_prop, starts[-1], len(starts) - 1, sup[1][-1])
        ws = postprocess.PostBatchWorkspace(*sizes, device=self.device) if ws is None else ws.grown_for(*sizes)
        c = 1 if self.tta is None else self.tta     # with tta `starts` are over folded points and unit j holds c copies of them
        if self.tta is None:
            rb = postprocess.refine_merged_device(ret["sem_pred_p"], ret["proposals"], ret["clt_scores"], starts, sup[1], sup[0],
                                                  self.refine, workspace=ws)
        else:
            rb = postprocess.refine_tta_merged_device(ret["sem_pred_p"], ret["proposals"], ret["clt_scores"], starts, sup[1], sup[0],
                                                      self.refine, copies=c, workspace=ws)
        self._associate(rb, c, assoc)
        rb.point_instance, rb.scores, rb.semantic_id, rb.npoints = (t.clone() for t in (rb.point_instance, rb.scores,
                                                                                        rb.semantic_id, rb.npoints))
        if not self.summary:
            scalars = rb.scalars.tolist()                               # the one read-back (it also waits for the forward)
            res = []
            for j in range(len(starts) - 1):
                try:
                    res.append(dict(sem_pred_p=ret["sem_pred_p"][c * starts[j]:c * starts[j + 1]], instances=rb.scene(j, scalars)))
                except ValueError as e:
                    res.append(e)
            return res, ws
        score = ret["sem_pred_score_p"]
        sizes = (n_prop, starts[-1], len(starts) - 1, int(score.shape[1]))
        sws = postprocess.SummaryWorkspace(*sizes, device=self.device) if sws is None else sws.grown_for(*sizes)
        sm = postprocess.summarize_merged_device(score, rb, starts, copies=c, xyz=xyz, workspace=sws)
        sm.sem_fold, sm.class_vote, sm.class_points = sm.sem_fold.clone(), sm.class_vote.clone(), sm.class_points.clone()
        if xyz is not None:
            sm.box, sm.centroid = sm.box.clone(), sm.centroid.clone()
        scalars = sm.readback()                                         # the one read-back: both passes' scalars, concatenated
        res = []
        for j in range(len(starts) - 1):
            try:
                inst, extra = rb.scene(j, scalars[:2 * rb.n_scenes]), sm.scene(j, scalars)
                if has_xyz is not None and not has_xyz[j]:
                    extra["box"] = extra["centroid"] = None
                inst.update(class_vote=extra["class_vote"], class_points=extra["class_points"], box=extra["box"],
                            centroid=extra["centroid"])
                res.append(dict(sem_pred_p=ret["sem_pred_p"][c * starts[j]:c * starts[j + 1]], sem_fold=extra["sem_fold"],
                                instances=inst))
            except ValueError as e:
                res.append(e)
        return res, (ws, sws)

    def _unit_coordinates(self, units, starts):
        """The folded points' own coordinates for the summary of a tta forward: (float32 [N, 3] or None, which units brought
        `xyz_scene`).  A unit without it gets zeros, and no box."""
        has = [u.get("xyz_scene") is not None for u in units]
        if not self.summary or not any(has):
            return None, has
        parts = []
        for j, u in enumerate(units):
            n = starts[j + 1] - starts[j]
            if has[j]:
                if u["xyz_scene"].dtype != torch.float32 or tuple(u["xyz_scene"].shape) != (n, 3):
                    raise ValueError("unit %d: `xyz_scene` must be float32 [%d, 3]" % (j, n))
                parts.append(u["xyz_scene"])
            else:
                parts.append(torch.zeros(n, 3, dtype=torch.float32, device=self.device))
        return (parts[0] if len(parts) == 1 else torch.cat(parts)).contiguous(), has

    def _forward_tta(self, items, ws, assoc=None):
        """One merged forward of up to MAX_SCENES // tta units; returns (per-unit results or exceptions, workspace)."""
        t = self.tta
        batch, starts, sup = merge_tta_units([it[0] for it in items], t, [it[1] for it in items])
        with torch.no_grad():
            ret = self.model(batch["feat_voxel"], batch["xyz_voxel"], batch["xyz_original"], batch["v2p_index"], None, self.epoch,
                             "test", teacher=batch["teacher"], n_batch=t * len(items))
        if "proposals" in ret:
            xyz, has = self._unit_coordinates([it[0] for it in items], starts)
            return self._refined(ret, starts, sup, ws, xyz, has, assoc)
        return [dict(sem_pred_p=ret["sem_pred_p"][t * starts[j]:t * starts[j + 1]]) for j in range(len(items))], ws

    def _worker(self, stream):
        torch.cuda.set_device(self.device)
        ws = None                               # this worker's post-processing workspace (refine), grown when a batch does not fit
        alog = None                             # this worker's association log (association), made with its first forward
        with torch.cuda.stream(stream):
            while True:
                items = self._take()
                if items is None:
                    return
                futs = [it[2] for it in items]
                try:
                    assoc = None
                    if self.association_on:
                        if alog is None:                # this worker's log: one log per stream
                            alog = evaluate.AssociationLog(1, 1, device=self.device, **self._assoc_kw)
                            with self._lock:
                                self._logs.append(alog)
                        assoc = (alog, [self._names[it[5]] for it in items], [it[4] for it in items], [it[5] for it in items])
                    for it in items:
                        stream.wait_event(it[3])
                    if self.tta is not None:
                        res, ws = self._forward_tta(items, ws, assoc)
                    else:
                        merged = merge_scenes([it[0] for it in items], [it[1] for it in items],
                                              with_superpoints=self.refine is not None)
                        batch, teacher, starts, sup = merged if self.refine is not None else merged + (None,)
                        with torch.no_grad():
                            ret = self.model(batch["feat_voxel"], batch["xyz_voxel"], batch["xyz_original"], batch["v2p_index"], None,
                                             self.epoch, "test", teacher=teacher, n_batch=len(items))
                        if self.refine is not None and "proposals" in ret:
                            res, ws = self._refined(ret, starts, sup, ws, batch["xyz_original"] if self.summary else None,
                                                    assoc=assoc)
                        elif self.split:
                            res = split_results(ret, starts)
                        else:
                            res = [dict(ret, point_starts=starts, scene=j) for j in range(len(items))]
                    stream.synchronize()
                    with self._lock:
                        self.forwards += 1
                        self.scenes += len(items)
                    for f, r in zip(futs, res):
                        if isinstance(r, BaseException):
                            f.set_exception(r)
                        else:
                            f.set_result(r)
                except BaseException as e:      # noqa: BLE001 -- the exception belongs to the callers that wait on the futures
                    for f in futs:
                        if not f.done():
                            f.set_exception(e)
