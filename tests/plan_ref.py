"""Plain host references of the device-side control flow of the inference forward (csrc/plan.hip and the `_dev` forms of
csrc/front.hip, csrc/heads.hip), written from the contracts of include/pbnet_hip.h ("Capacity-planned inference") and the lines of
network/PBNet.py named there.  numpy only, explicit loops, int64 / float64 wherever arithmetic matters; float32 appears only
where the contract prescribes a float32 operation (the gates' int -> float conversion, d^2, the rounding of the weights, the
voxel coordinates).  Nothing here is fast and nothing here looks at how the kernels are organised.

tests/test_plan_ref_cpu.py anchors these functions to independent statements of the same operations (torch.cdist + stable
sort, cumsum / nonzero, searchsorted, the oracle's cluster_stage); tests/test_plan_gpu.py compares the kernels with them."""
import numpy as np

# counts words and overflow bits (include/pbnet_hip.h)
CNT_POINTS, CNT_CLUSTERS, CNT_ENTRIES, CNT_ROWS, CNT_SCENES, CNT_PROPOSAL_ROWS, CNT_PROPOSALS, CNT_OVERFLOW = range(8)
CNT_WORDS = 16
OVF_POINTS, OVF_CLUSTERS, OVF_ENTRIES, OVF_ROWS, OVF_SEGMENT, OVF_BATCH, OVF_LEVEL, OVF_CDIST = 1, 2, 4, 8, 16, 32, 64, 128

K_MAX = 6               # network/PBNet.py:35
SEG_CLUSTERS = 2048     # clusters of one (class, batch) segment whose neighbours the plan can rank
CDIST_DIRECT = 25       # torch.cdist computes direct differences up to this many rows
SEL_BLOCK = 1024        # rows per block of pbn_mask_count's block_cnt (pbn_select_blocks)


# ---- pbn_class_gate (PBNet.py:151-160, 172-173) -----------------------------------------------------------------------
def class_gate(table, thr05, nb, m_cap, n_points):
    """table int[n_cls, nb] -> dict(class_base int32[n_cls], seg_len int32[(n_cls-2)*nb], points, flags).
    A class is kept unless float32(total) < thr05[c]; classes 0 and 1 never are.  A table that does not sum to n_points
    (PBN_OVF_BATCH) or more kept points than m_cap (PBN_OVF_POINTS) drops every class."""
    table = np.asarray(table, dtype=np.int64).reshape(-1, nb)
    n_cls = table.shape[0]
    thr05 = np.asarray(thr05, dtype=np.float32)
    keep, base, m = [False] * n_cls, [-1] * n_cls, 0
    for c in range(2, n_cls):
        tot = int(table[c].sum())
        if not (np.float32(tot) < thr05[c]):
            keep[c], base[c] = True, m
            m += tot
    flags = 0
    if int(table.sum()) != int(n_points):
        flags |= OVF_BATCH
    if m > m_cap:
        flags |= OVF_POINTS
    seg_len = np.zeros((n_cls - 2) * nb, dtype=np.int32)
    if flags:
        base, m = [-1] * n_cls, 0
    else:
        for c in range(2, n_cls):
            if keep[c]:
                seg_len[(c - 2) * nb:(c - 1) * nb] = table[c]
    return {"class_base": np.asarray(base, dtype=np.int32), "seg_len": seg_len, "points": m, "flags": flags}


# ---- pbn_local_plan (PBNet.py:182-234, task 'test') ---------------------------------------------------------------------
def dist2_f32(a, b):
    """(dx^2 + dy^2) + dz^2 of two float32 points, every operation rounded to float32 on its own (no fused multiply-add)."""
    dx, dy, dz = np.float32(b[0]) - np.float32(a[0]), np.float32(b[1]) - np.float32(a[1]), np.float32(b[2]) - np.float32(a[2])
    return np.float32(np.float32(np.float32(dx * dx) + np.float32(dy * dy)) + np.float32(dz * dz))


def entry_weight(para_k, i):
    """Weight of neighbour i (0-based) of a scene with para_k neighbours: peak_v[i] of PBNet.py:196-198, float64 -> float32."""
    return np.float32(0.5 * float((para_k + 1) - i) / float(para_k + 1))


def local_plan(cluster_num, nb, member_start, centers, thr02, kmax, c_cap, e_cap, r_cap, n_clusters=None):
    """One local scene per cluster c < C = min(n_clusters, c_cap): entry 0 is the cluster itself with weight 1; when
    float32(size) > thr02[cls] and para_k = min(C_b - 1, kmax[cls], K_MAX) > 0, its para_k nearest clusters of the same
    (class, batch) segment follow in ascending (d^2, cluster id).  The segment tables describe ALL n_clusters clusters: a
    neighbour may be a cluster >= C.  Returns dict(scenes = [(ids, weights)], ent_row_start, ent_member_start, ent_scene,
    ent_weight (the documented extents only), counts = {ENTRIES, ROWS, SCENES, CLUSTERS}, flags)."""
    cluster_num = [int(v) for v in np.asarray(cluster_num).reshape(-1)]
    member_start = np.asarray(member_start, dtype=np.int64)
    centers = np.asarray(centers, dtype=np.float32).reshape(-1, 3)
    thr02 = np.asarray(thr02, dtype=np.float32)
    if n_clusters is None:
        n_clusters = sum(cluster_num)
    C = min(int(n_clusters), int(c_cap))
    flags = OVF_CLUSTERS if n_clusters > c_cap else 0
    seg_of, first_of = [], []
    for s, cb in enumerate(cluster_num):
        seg_of += [s] * cb
        first_of += [len(first_of)] * cb
    scenes = []
    for c in range(max(C, 0)):
        if c >= len(seg_of):                      # more clusters announced than the segment table holds: an empty scene
            scenes.append(([], []))
            continue
        seg, g0 = seg_of[c], first_of[c]
        cb = cluster_num[seg]
        cls = 2 + seg // nb
        para_k = min(cb - 1, int(kmax[cls]), K_MAX)
        size = int(member_start[c + 1] - member_start[c])
        ids, wts = [c], [np.float32(1.0)]
        if np.float32(size) > thr02[cls] and para_k > 0:
            if cb > SEG_CLUSTERS:
                flags |= OVF_SEGMENT
            else:
                if cb > CDIST_DIRECT:
                    flags |= OVF_CDIST
                cand = sorted((dist2_f32(centers[c], centers[o]), o) for o in range(g0, g0 + cb) if o != c)
                for i in range(para_k):
                    ids.append(cand[i][1])
                    wts.append(entry_weight(para_k, i))
        scenes.append((ids, wts))
    n_ent = sum(len(ids) for ids, _ in scenes)
    out = {"scenes": scenes, "n_ent_planned": n_ent}
    if n_ent > e_cap:
        # nothing is packed; ent_row_start[0] = 0 keeps a consumer that reads it harmless
        out.update(ent_row_start=np.zeros(1, dtype=np.int32), ent_member_start=np.zeros(0, dtype=np.int32),
                   ent_scene=np.zeros(0, dtype=np.int32), ent_weight=np.zeros(0, dtype=np.float32),
                   counts={"ENTRIES": 0, "ROWS": 0, "SCENES": 0, "CLUSTERS": max(C, 0)}, flags=flags | OVF_ENTRIES)
        return out
    row_start, mem, scn, wt, rows = [0], [], [], [], 0
    for s, (ids, wts) in enumerate(scenes):
        for cl, w in zip(ids, wts):
            mem.append(int(member_start[cl]))
            scn.append(s)
            wt.append(w)
            rows += int(member_start[cl + 1] - member_start[cl])
            row_start.append(rows)
    ovf = rows > r_cap
    if ovf:
        flags |= OVF_ROWS
    out.update(ent_row_start=np.asarray(row_start, dtype=np.int32), ent_member_start=np.asarray(mem, dtype=np.int32),
               ent_scene=np.asarray(scn, dtype=np.int32), ent_weight=np.asarray(wt, dtype=np.float32),
               counts={"ENTRIES": 0 if ovf else n_ent, "ROWS": 0 if ovf else rows, "SCENES": 0 if ovf else max(C, 0),
                       "CLUSTERS": max(C, 0)}, flags=flags)
    return out


# ---- pbn_proposal_offsets (PBNet.py:330-345) ----------------------------------------------------------------------------
def proposal_offsets(per_scene, n_scenes, s_cap=None):
    """Rows kept per local scene -> (proposals_offset int64[P+1], alive_ids int64[P], dense_of int32[S], P, rows) over the
    first S = min(n_scenes, s_cap) scenes; dense_of[s] = (number of alive scenes <= s) - 1."""
    S = int(n_scenes) if s_cap is None else min(int(n_scenes), int(s_cap))
    offsets, alive, dense, rows = [0], [], [], 0
    for s in range(max(S, 0)):
        v = int(per_scene[s])
        if v > 0:
            alive.append(s)
            rows += v
            offsets.append(rows)
        dense.append(len(alive) - 1)
    return (np.asarray(offsets, dtype=np.int64), np.asarray(alive, dtype=np.int64), np.asarray(dense, dtype=np.int32),
            len(alive), rows)


# ---- pbn_batch_starts -----------------------------------------------------------------------------------------------------
def batch_starts(batch_column, n, n_seg, n_cap=None):
    """seg_start int32[n_seg + 1]: first of the first min(n, n_cap) rows of a batch-sorted list whose batch index is >= s
    (the number of those rows when there is none)."""
    n = int(n) if n_cap is None else min(int(n), int(n_cap))
    out = np.zeros(n_seg + 1, dtype=np.int32)
    for s in range(n_seg + 1):
        first = n
        for r in range(n):
            if int(batch_column[r]) >= s:
                first = r
                break
        out[s] = first
    return out


# ---- the `_dev` forms of the stage kernels: the size-exact operation on the first min(n, cap) rows ------------------------
def dev_rows(n_dev, cap):
    """Rows a `_dev` kernel processes: the device-side count, clamped to the capacity (a NULL count means the capacity)."""
    return int(cap) if n_dev is None else max(0, min(int(n_dev), int(cap)))


def dev_expected(exact_rows, before, n_dev, cap):
    """What a capacity-sized per-row output holds after a `_dev` launch: the size-exact result in the first min(n, cap) rows,
    the previous content (`before`, a canary pattern) in every row beyond them."""
    k = dev_rows(n_dev, cap)
    out = np.array(before, copy=True)
    out[:k] = np.asarray(exact_rows)[:k]
    return out


def local_scene_rows(ent_row_start, ent_member_start, ent_scene, ent_weight, n_ent, n_rows, member_idx, ins_ind, xyz,
                     inv_voxel, point_feat, sem_prob):
    """Rows of the local scenes (PBNet.py:182-247): row r belongs to the entry e with ent_row_start[e] <= r <
    ent_row_start[e+1].  float32 features.  Returns (point_idx int64[R], row_scene int64[R], coords int32[R,4],
    feat float32[R, C+2] = point_feat | own-class score | entry weight)."""
    R, C = int(n_rows), point_feat.shape[1]
    point_idx, row_scene = np.zeros(R, dtype=np.int64), np.zeros(R, dtype=np.int64)
    coords, feat = np.zeros((R, 4), dtype=np.int32), np.zeros((R, C + 2), dtype=np.float32)
    e = 0
    for r in range(R):
        while e + 1 < n_ent and int(ent_row_start[e + 1]) <= r:
            e += 1
        p = int(ins_ind[int(member_idx[int(ent_member_start[e]) + r - int(ent_row_start[e])])])
        point_idx[r], row_scene[r] = p, int(ent_scene[e])
        coords[r, 0] = int(ent_scene[e])
        for k in range(3):
            coords[r, 1 + k] = int(np.floor(np.float32(xyz[p, k]) * np.float32(inv_voxel)))
        feat[r, :C], feat[r, C], feat[r, C + 1] = point_feat[p], sem_prob[p], ent_weight[e]
    return point_idx, row_scene, coords, feat


def gather_pad_rows(src, idx, idx2, n, width_out):
    """out[i, :C] = src[idx2[idx[i]]] (either level may be None), zero padding up to width_out."""
    out = np.zeros((int(n), width_out), dtype=src.dtype)
    for i in range(int(n)):
        r = i if idx is None else int(idx[i])
        if idx2 is not None:
            r = int(idx2[r])
        out[i, :src.shape[1]] = src[r]
    return out


def mask_count(score, thd, row_scene, n, n_scenes, n_cap):
    """Rows with float32(score) > thd among the first n: per local scene, and per block of SEL_BLOCK rows of the capacity."""
    per_scene = np.zeros(int(n_scenes), dtype=np.int32)
    block_cnt = np.zeros(max(-(-int(n_cap) // SEL_BLOCK), 0), dtype=np.int32)
    for i in range(int(n)):
        if np.float32(score[i]) > np.float32(thd):
            block_cnt[i // SEL_BLOCK] += 1
            if 0 <= int(row_scene[i]) < n_scenes:
                per_scene[int(row_scene[i])] += 1
    return per_scene, block_cnt


def proposal_rows(score, thd, row_scene, point_idx, n, dense_of, xyz, scale, inv_voxel, point_feat):
    """The kept rows among the first n, in row order: (proposals_idx int64[P,2], scores, coords int32[P,4], features)."""
    idx, ms, coords, feat = [], [], [], []
    for i in range(int(n)):
        if np.float32(score[i]) > np.float32(thd):
            p, d = int(point_idx[i]), int(dense_of[int(row_scene[i])])
            idx.append((d, p))
            ms.append(score[i])
            coords.append([d] + [int(np.floor(np.float32(np.float32(xyz[p, k]) * np.float32(scale)) * np.float32(inv_voxel)))
                                 for k in range(3)])
            feat.append(point_feat[p])
    return (np.asarray(idx, dtype=np.int64).reshape(-1, 2), np.asarray(ms, dtype=score.dtype),
            np.asarray(coords, dtype=np.int32).reshape(-1, 4),
            np.asarray(feat, dtype=point_feat.dtype).reshape(-1, point_feat.shape[1]))
