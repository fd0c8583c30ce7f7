"""Deliberately WRONG variants of the grouping specification, used to show that tests/cluster_cases.py is sharp: every mutant must
differ from tests/bruteforce_cluster.py on at least one case.  The specification file stays clean, so this module restates its
steps with one switch per mutant; `mutant=None` is the specification again, and tests/test_cluster_cases_cpu.py checks that this
restatement equals bruteforce_cluster bit for bit on every case before it trusts a kill.

Mutants 3 and 4 are mistakes of a CELL-DRIVEN implementation, so they use the cell model of cluster_cases.cell_index."""
import numpy as np
from scipy.sparse import csr_matrix
from scipy.sparse.csgraph import connected_components

import bruteforce_cluster as brute
from cluster_cases import cell_index, CLAMP

MUTANTS = (
    "strict_radius",            # 1. d2 <  r*r instead of <=
    "hp_strictly_more",         # 2. HP iff nb > min_pts
    "representative_only",      # 3. trusted cells joined only through their smallest-index HP (a dropped pass 1)
    "clamped_cells_trusted",    # 4. points of one clamped cell taken to be within r of each other
    "border_smallest",          # 5. border LP takes the smallest adjacent cluster
    "filter_le",                # 6. filter drops size <= threshold
    "nn_lowest_index",          # 7. NN ties go to the lowest index
    "nn_any_class",             # 8. NN ignores the class
    "centre_sum_over_n",        # 9. centre = float32 sum / N
)


def _segment(P, O, sem, radius, min_pts, para_f, nv_flag, id_base, mutant):
    n = P.shape[0]
    r = np.float32(radius)
    r2 = np.float32(r * r)
    dd = brute._d2(P, P)
    within = dd < r2 if mutant == "strict_radius" else dd <= r2
    cells = cell_index(P, radius)
    _, cell_id = np.unique(cells, axis=0, return_inverse=True)
    cell_id = cell_id.reshape(-1)
    untrusted = (np.abs(cells) >= CLAMP).any(axis=1)
    same_cell = cell_id[:, None] == cell_id[None, :]
    if mutant == "clamped_cells_trusted":
        within = within | (same_cell & untrusted[:, None])
    nb = within.sum(1).astype(np.int32) - 1
    hp = nb > min_pts if mutant == "hp_strictly_more" else nb >= min_pts
    label = np.full(n, -1, dtype=np.int64)
    clusters = []
    if hp.any():
        hp_idx = np.nonzero(hp)[0]
        sub = within[np.ix_(hp_idx, hp_idx)]
        if mutant == "representative_only":
            rep = np.full(cell_id.max() + 1, n, np.int64)
            np.minimum.at(rep, cell_id[hp_idx], hp_idx)
            is_rep = rep[cell_id[hp_idx]] == hp_idx
            free = untrusted[hp_idx]
            sub = sub & (same_cell[np.ix_(hp_idx, hp_idx)] | is_rep[:, None] | is_rep[None, :] | free[:, None] | free[None, :])
        _, comp_of = connected_components(csr_matrix(sub), directed=False)
        comp = np.full(n, -1, dtype=np.int64)
        comp[hp_idx] = comp_of
        seen = {}
        for i in hp_idx:
            key = (int(comp[i]), int(sem[i]))
            if key not in seen:
                seen[key] = len(clusters)
                clusters.append(key)
            label[i] = seen[key]
        for i in np.nonzero(~hp)[0]:
            adj = hp_idx[within[i, hp_idx]]
            ids = [seen[(int(k), int(sem[i]))] for k in set(int(c) for c in comp[adj]) if (int(k), int(sem[i])) in seen]
            if ids:
                label[i] = min(ids) if mutant == "border_smallest" else max(ids)
    keep_map, kept_sem = {}, []
    pf = np.float32(para_f)
    for cid, (_, s) in enumerate(clusters):
        size = np.float32(int((label == cid).sum()))
        thr = np.float32(brute.MEAN_COUNT[s - 2] * pf)
        if not (size <= thr if mutant == "filter_le" else size < thr):
            keep_map[cid] = len(kept_sem)
            kept_sem.append(s)
    label = np.array([keep_map.get(int(c), -1) for c in label], dtype=np.int64)
    if nv_flag:
        noise = np.nonzero(label < 0)[0]
        assigned = np.nonzero(label >= 0)[0]
        if len(noise) and len(assigned):
            do = brute._d2(O[noise], O[assigned])
            out = label.copy()
            for a, i in enumerate(noise):
                same = np.ones(len(assigned), bool) if mutant == "nn_any_class" else sem[assigned] == sem[i]
                if same.any():
                    cand = assigned[same]
                    dv = do[a][same]
                    ties = np.nonzero(dv == dv.min())[0]
                    out[i] = label[cand[ties.min() if mutant == "nn_lowest_index" else ties.max()]]
                else:
                    out[i] = label[assigned.max()]
            label = out
    centers = np.zeros((len(kept_sem), 3), dtype=np.float32)
    for c in range(len(kept_sem)):
        M = np.zeros(3, dtype=np.float32)
        N = 0
        for i in np.nonzero(label == c)[0]:
            N += 1
            if mutant == "centre_sum_over_n":
                M = (M + P[i].astype(np.float32)).astype(np.float32)
            else:
                M = (M + (P[i].astype(np.float32) - M) / np.float32(N)).astype(np.float32)
        centers[c] = (M / np.float32(N)).astype(np.float32) if mutant == "centre_sum_over_n" else M
    out_label = np.where(label >= 0, label + id_base, -1).astype(np.int32)
    return out_label, nb, centers, np.array(kept_sem, dtype=np.int32)


def binary_cluster(off_xyz, org_xyz, sem, seg_len, radius, min_pts, para_f=0.05, nv_flag=True, mutant=None):
    assert mutant is None or mutant in MUTANTS
    off_xyz = np.asarray(off_xyz, dtype=np.float32).reshape(-1, 3)
    org_xyz = np.asarray(org_xyz, dtype=np.float32).reshape(-1, 3)
    sem = np.asarray(sem, dtype=np.int32)
    ids, dens, ctrs, sems, nums = [], [], [], [], []
    start = base = 0
    for ln in seg_len:
        ln = int(ln)
        if ln == 0:
            nums.append(0)
            continue
        sl = slice(start, start + ln)
        lab, nb, c, s = _segment(off_xyz[sl], org_xyz[sl], sem[sl], radius, min_pts, para_f, nv_flag, base, mutant)
        ids.append(lab)
        dens.append(nb)
        ctrs.append(c)
        sems.append(s)
        nums.append(len(s))
        base += len(s)
        start += ln
    cat = lambda xs, dt, shape: (np.concatenate(xs).astype(dt) if xs else np.zeros(shape, dtype=dt))
    return dict(cluster_id=cat(ids, np.int32, (0,)), cluster_num=np.array(nums, dtype=np.int32),
                den_queue=cat(dens, np.int32, (0,)), center=cat(ctrs, np.float32, (0, 3)).reshape(-1, 3),
                clt_sem=cat(sems, np.int32, (0,)))
