"""numpy restatement of pbn_ap_assoc_batch, written from the contract in include/pbnet_hip.h and not from the kernels: per scene
np.unique over the ids in range, np.add.at on (label, index) for the labels in [0, n_keep), ap_record_ref.pack_record, and the
log's used | wanted | n_records | overflow | last offset state machine with its sticky overflow."""
import numpy as np

import ap_record_ref as R

ID_RANGE, ID_COUNT, LABEL_RANGE, INSTANCE_CAP, SEMANTIC_RANGE = 4, 8, 16, 32, 64
SEMANTIC_LABEL_IDX = np.array([1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 14, 16, 24, 28, 33, 34, 36, 39])
INT_MAX = 0x7fffffff


def encode_scene(sem, ins, n_inst_cap, label_table=SEMANTIC_LABEL_IDX):
    """(ids int64[n], status) of one scene as pbn_gt_encode_dev states it: label_table[sem of the instance's lowest point] * 1000 +
    instance + 1 (semantic -100 = class 0), 0 without an instance; an instance >= n_inst_cap or a semantic label outside the
    table sets its bit and the point gets 0."""
    sem, ins = np.asarray(sem).astype(np.int64), np.asarray(ins).astype(np.int64)
    ids, status = np.zeros(ins.shape[0], np.int64), 0
    if (ins >= n_inst_cap).any():
        status |= INSTANCE_CAP
    for inst in np.unique(ins[(ins >= 0) & (ins < n_inst_cap)]):
        at = np.nonzero(ins == inst)[0]
        s = int(sem[at[0]])
        s = 0 if s == -100 else s
        if s < 0 or s >= len(label_table):
            status |= SEMANTIC_RANGE
        else:
            ids[at] = int(label_table[s]) * 1000 + int(inst) + 1
    return ids, status


def scene_tables(labels, ids, n_keep, u_cap, id_cap):
    """(inter int64[n_keep, n_gt], uid, counts, status) of one scene from one label per point."""
    labels, ids = np.asarray(labels).astype(np.int64), np.asarray(ids).astype(np.int64)
    ok = (ids >= 0) & (ids < id_cap)
    status = 0 if ok.all() else ID_RANGE
    uid, counts = np.unique(ids[ok], return_counts=True)
    if uid.shape[0] > u_cap:
        status |= ID_COUNT
        uid, counts = uid[:u_cap], counts[:u_cap]
    index = np.full(ids.shape[0], -1, np.int64)
    pos = np.searchsorted(uid, ids)
    hit = ok & (pos < uid.shape[0])
    hit[hit] = uid[pos[hit]] == ids[hit]
    index[hit] = pos[hit]
    inter = np.zeros((n_keep, uid.shape[0]), np.int64)
    sel = (labels >= 0) & (labels < n_keep) & (index >= 0)
    np.add.at(inter, (labels[sel], index[sel]), 1)
    return inter, uid.astype(np.int64), counts.astype(np.int64), status


def clamped_keep(n_keep, n_prop):
    """n_keep per scene as pbn_scene_summary clamps it: never negative, the scenes' counts sum to at most n_prop."""
    out, total = [], 0
    for k in n_keep:
        k = max(0, min(int(k), n_prop - total))
        out.append(k)
        total += k
    return out


def append(state, log, record):
    """The log's state machine for one record (pbn_ap_record_append): state int64[8], log int32[log_words], both in place."""
    words = int(record.shape[0])
    state[1] = min(int(state[1]) + words, INT_MAX)
    used = int(state[0])
    if state[3] or used < 0 or used + words > log.shape[0]:
        state[3], state[4] = 1, -1
        return
    log[used:used + words] = record
    state[0], state[2], state[4] = used + words, state[2] + 1, used


def assoc_batch(point_starts, point_instance, n_keep, post_status, scores, semantic_id, tags, u_cap, id_cap, log_words, ids=None,
                sem=None, ins=None, n_inst_cap=None, state=None, log=None):
    """All scenes of one merged forward.  point_starts: B + 1 starts over folded points; point_instance int[N]; n_keep / post_status
    int[B]; scores f32[B, P], semantic_id i64[B, P]; ground truth `ids` [N] or (`sem`, `ins`) [N] with n_inst_cap.  Returns
    (state int32[8], log int32[log_words]); `state` / `log` continue an epoch."""
    b = len(point_starts) - 1
    n_prop = np.asarray(scores).size // b
    scores, semantic_id = np.asarray(scores, np.float32).reshape(b, n_prop), np.asarray(semantic_id, np.int64).reshape(b, n_prop)
    state = np.zeros(8, np.int64) if state is None else np.asarray(state).astype(np.int64)
    log = np.zeros(log_words, np.int32) if log is None else np.array(log, np.int32)
    keep = clamped_keep(n_keep, n_prop)
    for j in range(b):
        lo, hi = point_starts[j], point_starts[j + 1]
        status = int(post_status[j])
        if ids is None:
            scene_ids, bits = encode_scene(sem[lo:hi], ins[lo:hi], n_inst_cap)
            status |= bits
        else:
            scene_ids = np.asarray(ids[lo:hi])
        labels = np.asarray(point_instance[lo:hi]) if keep[j] else np.zeros(hi - lo, np.int64)
        inter, uid, counts, bits = scene_tables(labels, scene_ids, keep[j], u_cap, id_cap)
        status |= bits
        label_id = semantic_id[j, :keep[j]]
        if (label_id != label_id.astype(np.int32)).any():
            status |= LABEL_RANGE
        append(state, log, R.pack_record(int(tags[j]), hi - lo, inter, uid, counts, label_id, scores[j, :keep[j]], status))
    return state.astype(np.int32), log


def densify(labels, n_keep):
    """int32[n_keep, n]: row k = the points whose label is k (RefinedBatch.dense)."""
    return (np.asarray(labels)[None, :] == np.arange(n_keep)[:, None]).astype(np.int32)


def disjoint_labels(masks):
    """One label per point from masks that may overlap: the lowest mask index wins, -100 where no mask holds the point."""
    inside = np.asarray(masks) != 0
    labels = np.full(inside.shape[1], -100, np.int32)
    for p in range(inside.shape[0] - 1, -1, -1):
        labels[inside[p]] = p
    return labels
