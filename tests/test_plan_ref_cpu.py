"""CPU tier: tests/plan_ref.py against independent statements of the same operations, so that tests/test_plan_gpu.py does
not compare the kernels of csrc/plan.hip with a restatement of themselves.
  local_plan        torch.cdist + torch.sort(stable=True) per (class, batch) segment, the loop of oracle/pbnet_ref.py:
                    cluster_stage (PBNet.py:196-221); segments of at most 25 clusters (torch.cdist's direct path) whose
                    centres lie on a grid of multiples of 1/4, where d^2 is exact in float32
  proposal_offsets  cumsum / nonzero (PBNet.py:330-345)
  class_gate        the statements of cluster_stage (PBNet.py:151-160, 172-173) on a point list
  batch_starts      np.searchsorted"""
import numpy as np
import pytest
import torch

import plan_ref as R
from oracle.pbnet_ref import COUNT_MEAN, K_MAX


# ---- local_plan ---------------------------------------------------------------------------------------------------------
def _grid_centers(rng, n, span=40):
    """n distinct points whose coordinates are multiples of 1/4 (|x| <= span/4: d^2 * 16 is an integer below 2^14)."""
    seen, out = set(), []
    while len(out) < n:
        p = tuple(int(v) for v in rng.integers(-span, span + 1, 3))
        if p not in seen:
            seen.add(p)
            out.append(p)
    return np.asarray(out, dtype=np.float32) / np.float32(4.0)


def _plan_by_torch(cluster_num, nb, member_start, centers, thr02, kmax):
    """The loop of cluster_stage for task 'test', with the per-class K_max of the model: scenes as (ids, weights)."""
    scenes, g0 = [], 0
    ctr = torch.from_numpy(np.asarray(centers, dtype=np.float32).reshape(-1, 3))
    for seg, cb in enumerate(cluster_num):
        cb = int(cb)
        if cb == 0:
            continue
        cls = 2 + seg // nb
        para_k = min(cb - 1, int(kmax[cls]), K_MAX)
        if para_k > 0:
            peak_v = [0.5 * ((para_k + 1) - p_i) / (para_k + 1) for p_i in range(para_k + 1)]
            dist = torch.cdist(ctr[g0:g0 + cb], ctr[g0:g0 + cb])
            knn_idx = torch.sort(dist, dim=1, stable=True)[1]
        for c_i in range(cb):
            c = g0 + c_i
            size = int(member_start[c + 1] - member_start[c])
            ids, wts = [c], [np.float32(1.0)]
            if size > float(thr02[cls]) and para_k > 0:
                assert int(knn_idx[c_i, 0]) == c_i
                for k_i in range(para_k):
                    ids.append(g0 + int(knn_idx[c_i, k_i + 1]))
                    wts.append((torch.ones(1) * peak_v[k_i]).numpy()[0])
            scenes.append((ids, wts))
        g0 += cb
    return scenes


def _check_plan(cluster_num, nb, member_start, centers, thr02, kmax):
    C = int(np.sum(cluster_num))
    got = R.local_plan(cluster_num, nb, member_start, centers, thr02, kmax, C, 7 * C, 2 ** 31 - 1)
    want = _plan_by_torch(cluster_num, nb, member_start, centers, thr02, kmax)
    assert len(got["scenes"]) == len(want) == C
    for (gi, gw), (wi, ww) in zip(got["scenes"], want):
        assert gi == wi
        assert np.array_equal(np.asarray(gw, dtype=np.float32).view(np.int32), np.asarray(ww, dtype=np.float32).view(np.int32))
    # the packed arrays: entries in scene order, row offsets = running sum of the entries' cluster sizes
    ids = np.asarray([c for s in want for c in s[0]], dtype=np.int64)
    sizes = np.diff(np.asarray(member_start, dtype=np.int64))
    assert np.array_equal(got["ent_row_start"], np.concatenate([[0], np.cumsum(sizes[ids])]))
    assert np.array_equal(got["ent_member_start"], np.asarray(member_start)[ids])
    assert np.array_equal(got["ent_scene"], np.repeat(np.arange(C), [len(s[0]) for s in want]))
    assert np.array_equal(got["ent_weight"], np.asarray([w for s in want for w in s[1]], dtype=np.float32))
    assert got["counts"] == {"ENTRIES": len(ids), "ROWS": int(sizes[ids].sum()), "SCENES": C, "CLUSTERS": C}
    assert got["flags"] == 0
    return got


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_local_plan_matches_cdist_stable_sort(seed):
    rng = np.random.default_rng(seed)
    nb, n_cls = 3, 20
    cluster_num = rng.integers(0, 26, (n_cls - 2) * nb)
    cluster_num[rng.integers(0, len(cluster_num), 12)] = 0
    cluster_num[5], cluster_num[7], cluster_num[11] = 25, 1, 2
    C = int(cluster_num.sum())
    thr02 = np.concatenate([[-1, -1], rng.integers(20, 60, n_cls - 2)]).astype(np.float32)
    kmax = np.concatenate([[0, 0], rng.choice([0, 1, 3, 6, 9], n_cls - 2)]).astype(np.int32)
    sizes = rng.integers(1, 90, C)
    member_start = np.concatenate([[0], np.cumsum(sizes)])
    centers = np.concatenate([_grid_centers(rng, int(cb)) for cb in cluster_num if cb > 0])
    got = _check_plan(cluster_num, nb, member_start, centers, thr02, kmax)
    assert max(len(s[0]) for s in got["scenes"]) == 1 + K_MAX and min(len(s[0]) for s in got["scenes"]) == 1


def test_local_plan_size_gate_is_strict():
    cluster_num, nb = [3], 1
    thr02 = np.asarray([-1, -1, 50.0], dtype=np.float32)
    kmax = np.asarray([0, 0, 6], dtype=np.int32)
    member_start = np.asarray([0, 50, 101, 110])                  # sizes 50 (= thr02: not large), 51 (large), 9
    centers = np.asarray([[0, 0, 0], [1, 0, 0], [3, 0, 0]], dtype=np.float32)
    got = _check_plan(cluster_num, nb, member_start, centers, thr02, kmax)
    assert [s[0] for s in got["scenes"]] == [[0], [1, 0, 2], [2]]
    assert [float(w) for w in got["scenes"][1][1]] == [1.0, float(np.float32(0.5)), float(np.float32(0.5 * 2 / 3))]


def test_local_plan_ties_take_the_lower_id():
    """Two and three clusters at the same d^2 from the query: the stable sort, hence the plan, lists the lower id first."""
    nb = 1
    thr02 = np.asarray([-1, -1, 0.0], dtype=np.float32)
    member_start = np.arange(0, 8) * 10
    # cluster 3 is the query of interest: 0, 1 and 5 at d^2 = 1, 2 and 4 at d^2 = 4 (a pair), 6 further away
    centers = np.asarray([[1, 0, 0], [0, 1, 0], [0, 2, 0], [0, 0, 0], [-2, 0, 0], [0, 0, -1], [3, 3, 3]], dtype=np.float32)
    for k, want in ((1, [3, 0]), (2, [3, 0, 1]), (4, [3, 0, 1, 5, 2]), (6, [3, 0, 1, 5, 2, 4, 6])):
        kmax = np.asarray([0, 0, k], dtype=np.int32)
        got = _check_plan([7], nb, member_start, centers, thr02, kmax)
        assert got["scenes"][3][0] == want
    # the same with the tied clusters listed in the other order
    centers2 = centers[[5, 1, 4, 3, 2, 0, 6]]
    got = _check_plan([7], nb, member_start, centers2, thr02, np.asarray([0, 0, 6], dtype=np.int32))
    assert got["scenes"][3][0] == [3, 0, 1, 5, 2, 4, 6]


def test_local_plan_flags_and_capacities():
    rng = np.random.default_rng(9)
    nb = 2
    cluster_num = [4, 0, 26, 3]
    C = 33
    thr02 = np.asarray([-1, -1, 5.0, 5.0], dtype=np.float32)
    kmax = np.asarray([0, 0, 6, 6], dtype=np.int32)
    sizes = np.full(C, 3)
    sizes[[1, 10, 31]] = 40
    member_start = np.concatenate([[0], np.cumsum(sizes)])
    centers = _grid_centers(rng, C)
    full = R.local_plan(cluster_num, nb, member_start, centers, thr02, kmax, C, 7 * C, 10 ** 9)
    assert full["flags"] == R.OVF_CDIST                           # the 26-cluster segment ranked a neighbour
    assert [len(s[0]) for s in full["scenes"]] == [1, 4] + [1] * 2 + [1] * 6 + [7] + [1] * 19 + [1, 3, 1]
    n_ent, rows = full["counts"]["ENTRIES"], full["counts"]["ROWS"]
    assert n_ent == C + 3 + 6 + 2 and rows == int(full["ent_row_start"][-1])
    # clusters beyond c_cap make no scene, but stay neighbours
    cut = R.local_plan(cluster_num, nb, member_start, centers, thr02, kmax, 11, 7 * C, 10 ** 9, n_clusters=C)
    assert cut["flags"] == R.OVF_CDIST | R.OVF_CLUSTERS and cut["scenes"] == full["scenes"][:11]
    assert cut["counts"]["SCENES"] == cut["counts"]["CLUSTERS"] == 11
    # entries: exactly at the capacity, one below it
    assert R.local_plan(cluster_num, nb, member_start, centers, thr02, kmax, C, n_ent, 10 ** 9)["flags"] == R.OVF_CDIST
    over = R.local_plan(cluster_num, nb, member_start, centers, thr02, kmax, C, n_ent - 1, 10 ** 9)
    assert over["flags"] == R.OVF_CDIST | R.OVF_ENTRIES
    assert over["counts"] == {"ENTRIES": 0, "ROWS": 0, "SCENES": 0, "CLUSTERS": C} and list(over["ent_row_start"]) == [0]
    # rows: the same
    assert R.local_plan(cluster_num, nb, member_start, centers, thr02, kmax, C, n_ent, rows)["flags"] == R.OVF_CDIST
    over = R.local_plan(cluster_num, nb, member_start, centers, thr02, kmax, C, n_ent, rows - 1)
    assert over["flags"] == R.OVF_CDIST | R.OVF_ROWS
    assert over["counts"] == {"ENTRIES": 0, "ROWS": 0, "SCENES": 0, "CLUSTERS": C}
    assert np.array_equal(over["ent_row_start"], full["ent_row_start"])


def test_entry_weights_are_the_float32_of_the_float64_quotient():
    for para_k in range(1, K_MAX + 1):
        for i in range(para_k):
            want = (torch.ones(1) * (0.5 * ((para_k + 1) - i) / (para_k + 1))).numpy()[0]
            assert R.entry_weight(para_k, i).view(np.int32) == want.view(np.int32)


def test_dist2_is_unfused_float32():
    # dx^2 + dy^2 rounds before dz^2 is added: (2^24 + 1) + 1 differs between one rounding and two
    a = np.zeros(3, dtype=np.float32)
    b = np.asarray([4096.0, 1.0, 1.0], dtype=np.float32)
    assert float(R.dist2_f32(a, b)) == 2.0 ** 24                  # (2^24 + 1 -> 2^24) + 1 -> 2^24; exact would be 2^24 + 2
    rng = np.random.default_rng(4)
    p = rng.normal(0, 3, (200, 3)).astype(np.float32)
    for i in range(0, 200, 2):
        d = p[i + 1] - p[i]
        sq = d * d                                                 # float32 array arithmetic: one rounding per operation
        assert R.dist2_f32(p[i], p[i + 1]).view(np.int32) == np.float32(np.float32(sq[0] + sq[1]) + sq[2]).view(np.int32)


# ---- proposal_offsets -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,mode", [(1, "alive"), (1, "dead"), (256, "random"), (257, "alternate"), (1000, "random"),
                                    (1000, "dead"), (1000, "alive")])
def test_proposal_offsets_matches_cumsum_nonzero(S, mode):
    rng = np.random.default_rng(S)
    per = rng.integers(1, 500, S)
    if mode == "dead":
        per[:] = 0
    elif mode == "alternate":
        per[::2] = 0
    elif mode == "random":
        per[rng.random(S) < 0.4] = 0
    off, alive, dense, n_prop, n_rows = R.proposal_offsets(per, S)
    t = torch.from_numpy(per)
    keep = torch.nonzero(t > 0).view(-1)                          # PBNet.py:342-345
    assert np.array_equal(alive, keep.numpy())
    assert np.array_equal(off, np.concatenate([[0], torch.cumsum(t[keep], 0).numpy()]))
    assert np.array_equal(dense, (torch.cumsum((t > 0).long(), 0) - 1).numpy())
    assert n_prop == keep.numel() and n_rows == int(per.sum())
    # a scene count above the capacity: the first s_cap scenes only
    cut = R.proposal_offsets(per, S + 7, s_cap=max(S // 2, 1))
    want = R.proposal_offsets(per[:max(S // 2, 1)], max(S // 2, 1))
    assert all(np.array_equal(a, b) for a, b in zip(cut, want))


# ---- class_gate -----------------------------------------------------------------------------------------------------------
def _gate_by_statements(sem_pred, batch, n_cls, nb, count_mean):
    """cluster_stage's statements on a point list: kept classes in ascending order, their points per batch index."""
    class_base, seg_len, m = [-1] * n_cls, [0] * ((n_cls - 2) * nb), 0
    for sem_id in range(2, n_cls):
        ins_ind = torch.sort(torch.nonzero(sem_pred == sem_id).view(-1))[0]
        if ins_ind.shape[0] < count_mean[sem_id] * 0.05:
            continue
        ins_bh = batch[ins_ind]
        ins_bp = [int((ins_bh == i).sum()) for i in range(nb)]
        assert sum(ins_bp) == ins_bh.shape[0]
        class_base[sem_id] = m
        seg_len[(sem_id - 2) * nb:(sem_id - 1) * nb] = ins_bp
        m += ins_ind.shape[0]
    return class_base, seg_len, m


@pytest.mark.parametrize("nb", [1, 3, 8])
def test_class_gate_matches_cluster_stage(nb):
    rng = np.random.default_rng(nb)
    n_cls = 20
    thr = (COUNT_MEAN * 0.05).numpy()                             # float32 products, as PBNet.py:157 forms them
    pop = [int(v) for v in rng.integers(0, 900, n_cls)]
    pop[0], pop[1] = 5000, 7000                                   # never grouped, however large
    pop[4] = int(np.ceil(thr[4]))                                 # the first count that is not below the gate
    pop[5] = int(np.ceil(thr[5])) - 1                             # one point below it
    pop[16] = 106                                                 # count_mean 2120 * 0.05 = 106 exactly: kept
    assert float(thr[16]) == 106.0 and not (pop[4] < thr[4]) and pop[5] < thr[5]
    sem_pred = torch.from_numpy(rng.permutation(np.repeat(np.arange(n_cls), pop)))
    batch = torch.from_numpy(rng.integers(0, nb, sem_pred.shape[0]))
    table = np.bincount(sem_pred.numpy() * nb + batch.numpy(), minlength=n_cls * nb).reshape(n_cls, nb)
    want_base, want_seg, want_m = _gate_by_statements(sem_pred, batch, n_cls, nb, COUNT_MEAN)
    got = R.class_gate(table, thr, nb, want_m, sem_pred.shape[0])
    assert got["flags"] == 0 and got["points"] == want_m
    assert list(got["class_base"]) == want_base and list(got["seg_len"]) == want_seg
    assert got["class_base"][4] >= 0 and got["class_base"][16] >= 0 and got["class_base"][5] == -1
    assert got["class_base"][0] == got["class_base"][1] == -1
    # capacities and the batch assertion (PBNet.py:286)
    over = R.class_gate(table, thr, nb, want_m - 1, sem_pred.shape[0])
    assert over["flags"] == R.OVF_POINTS and over["points"] == 0
    assert (over["class_base"] == -1).all() and (over["seg_len"] == 0).all()
    bad = R.class_gate(table, thr, nb, want_m, sem_pred.shape[0] + 1)
    assert bad["flags"] == R.OVF_BATCH and bad["points"] == 0 and (bad["class_base"] == -1).all() and (bad["seg_len"] == 0).all()


# ---- batch_starts ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_seg", [0, 1, 9, 300])
def test_batch_starts_matches_searchsorted(n_seg):
    rng = np.random.default_rng(n_seg)
    present = [b for b in range(1, max(n_seg - 2, 2)) if b % 5 != 3]          # none at the front, gaps, none at the end
    col = np.sort(rng.choice(present, 700))
    for n in (0, 1, 350, 700):
        want = np.searchsorted(col[:n], np.arange(n_seg + 1), side="left")
        assert np.array_equal(R.batch_starts(col, n, n_seg), want)
    assert np.array_equal(R.batch_starts(col, 900, n_seg, n_cap=700), np.searchsorted(col, np.arange(n_seg + 1)))


# ---- the `_dev` composition -----------------------------------------------------------------------------------------------
def test_dev_expected_keeps_rows_beyond_the_count():
    exact = np.arange(40).reshape(10, 4)
    before = np.full((12, 4), -7)
    for n, k in ((0, 0), (1, 1), (9, 9), (10, 10), (15, 10), (None, 10)):
        out = R.dev_expected(exact, before, n, 10)
        assert R.dev_rows(n, 10) == k and np.array_equal(out[:k], exact[:k]) and (out[k:] == -7).all()
