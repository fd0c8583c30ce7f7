"""numpy packer of the association-log record, written from the contract in include/pbnet_hip.h (pbn_ap_record_append),
not from the kernel: header[8] = magic | scene tag | n_keep | n_gt | n_pts | status | record words | 0, then uid[n_gt] |
gt_vert[n_gt] | label_id[n_keep] | conf[n_keep] as float32 bit patterns | inter[n_keep, n_gt] row-major; a scene with
n_keep == 0 is its header alone.  Also the host statement of the tables a record holds (np.unique / np.bincount)."""
import numpy as np

MAGIC, HEADER = 0x41504c47, 8


def tables(masks, gt_ids):
    """(inter_all int64[P, U], uid int64[U], counts int64[U]) of one scene, the way evaluate.overlap_table defines them."""
    gt_ids = np.asarray(gt_ids).astype(np.int64).reshape(-1)
    uid, index = np.unique(gt_ids, return_inverse=True)
    inside = np.asarray(masks) != 0
    inter = np.zeros((inside.shape[0], uid.shape[0]), np.int64)
    for p in range(inside.shape[0]):
        inter[p] = np.bincount(index.reshape(-1)[inside[p]], minlength=uid.shape[0])
    return inter, uid, np.bincount(index.reshape(-1), minlength=uid.shape[0]).astype(np.int64)


def pack_record(tag, n_pts, inter_all, uid, counts, label_id, conf, status=0):
    """One record as int32 words."""
    n_keep, n_gt = int(np.asarray(label_id).shape[0]), int(np.asarray(uid).shape[0])
    if n_keep == 0:
        return np.array([MAGIC, tag, 0, n_gt, n_pts, status, HEADER, 0], np.int32)
    body = [np.asarray(uid, np.int64), np.asarray(counts, np.int64), np.asarray(label_id, np.int64),
            np.ascontiguousarray(conf, dtype=np.float32).view(np.int32).astype(np.int64),
            np.asarray(inter_all, np.int64).reshape(n_keep * n_gt)]
    size = HEADER + sum(b.shape[0] for b in body)
    head = np.array([MAGIC, tag, n_keep, n_gt, n_pts, status, size, 0], np.int64)
    return np.concatenate([head] + body).astype(np.int32)


def pack_log(scenes):
    """`scenes`: dicts with the keyword arguments of pack_record, in order; tags are their positions unless given."""
    recs = [pack_record(**dict(dict(tag=i), **s)) for i, s in enumerate(scenes)]
    return np.concatenate(recs) if recs else np.zeros(0, np.int32)
