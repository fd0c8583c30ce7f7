"""GPU tier: the fused stage-glue launches (csrc/front.hip, csrc/heads.hip) against the tensor-op form they replace
(/root/reference/network/PBNet.py:182-247 and friends).  Integer outputs bit-exact; feature rows bit-exact (copies)."""
import numpy as np
import pytest
import torch

from pbnet_amd import stage_ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _entries(rng, n_clusters, sizes, n_scenes):
    """Random local-scene plan: each scene = 1..4 entries (clusters, possibly repeated across scenes)."""
    ent_cluster, ent_weight, scene_len = [], [], []
    for _ in range(n_scenes):
        k = int(rng.integers(1, 5))
        scene_len.append(k)
        for j in range(k):
            ent_cluster.append(int(rng.integers(0, n_clusters)))
            ent_weight.append(1.0 if j == 0 else float(rng.uniform(0.05, 0.5)))
    return ent_cluster, ent_weight, scene_len


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_local_scene_rows_matches_tensor_ops(dtype):
    rng = np.random.default_rng(3)
    n_points, m, n_clusters, c, n_cls = 5000, 3000, 37, 32, 20
    sizes = rng.integers(1, 120, n_clusters)
    sizes[5] = 700                                              # one long cluster
    member_start = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    total = int(member_start[-1])
    member_idx = rng.integers(0, m, total).astype(np.int32)
    ins_ind = torch.from_numpy(rng.permutation(n_points)[:m].astype(np.int64)).to(DEV)
    xyz = torch.from_numpy(rng.uniform(-3, 6, (n_points, 3)).astype(np.float32)).to(DEV)
    point_feat = torch.randn(n_points, c, device=DEV).to(dtype)
    sem_score = torch.softmax(torch.randn(n_points, n_cls, device=DEV), 1).to(dtype)
    sem_pred = sem_score.float().max(1)[1]
    ent_cluster, ent_weight, scene_len = _entries(rng, n_clusters, sizes, 23)
    ec = torch.tensor(ent_cluster, dtype=torch.long)
    ent_rows = torch.from_numpy(sizes.astype(np.int64))[ec]
    n_ent = len(ent_cluster)
    row_start = torch.zeros(n_ent + 1, dtype=torch.int32)
    row_start[1:] = torch.cumsum(ent_rows, 0)
    n_rows = int(row_start[-1])
    ent_scene = torch.repeat_interleave(torch.arange(len(scene_len), dtype=torch.int32), torch.tensor(scene_len))
    ms = torch.from_numpy(member_start)
    packed = torch.cat([row_start, ms[:-1][ec].to(torch.int32), ent_scene,
                        torch.tensor(ent_weight, dtype=torch.float32).view(torch.int32)]).to(DEV)
    midx = torch.from_numpy(member_idx).to(DEV)
    voxel = 0.02
    point_idx, row_scene, coords, feat = stage_ops.local_scene_rows(packed, n_ent, n_rows, midx, ins_ind, xyz, voxel,
                                                                   point_feat, sem_score, sem_pred)
    # tensor-op form (what PBNet.forward does with autograd enabled)
    row_ent = torch.repeat_interleave(torch.arange(n_ent, device=DEV), ent_rows.to(DEV))
    ent_first = (torch.cumsum(ent_rows, 0) - ent_rows).to(DEV)
    pos = torch.arange(n_rows, device=DEV) - ent_first[row_ent]
    want_p = ins_ind[midx[ms[:-1][ec].to(DEV)[row_ent] + pos].long()]
    want_scene = ent_scene.to(DEV).long()[row_ent]
    want_w = torch.tensor(ent_weight, dtype=torch.float32, device=DEV)[row_ent]
    want_feat = torch.cat([point_feat[want_p], sem_score[want_p, sem_pred[want_p]].view(-1, 1),
                           want_w.view(-1, 1).to(dtype)], 1)
    want_coords = torch.cat([want_scene.view(-1, 1).to(torch.int32), torch.floor(xyz[want_p] / voxel).to(torch.int32)], 1)
    assert torch.equal(point_idx, want_p)
    assert torch.equal(row_scene, want_scene)
    assert torch.equal(coords, want_coords)
    assert torch.equal(feat.view(torch.uint8), want_feat.contiguous().view(torch.uint8))


def test_gather_pad_rows():
    from pbnet_amd import _native as N
    import ctypes
    x = torch.randn(1000, 34, device=DEV).to(torch.bfloat16)
    idx = torch.randperm(1000, device=DEV)[:777]
    out = torch.empty(777, 40, dtype=torch.bfloat16, device=DEV)
    rc = N.lib().pbn_gather_pad_rows(ctypes.c_void_p(x.data_ptr()), 68, 68, ctypes.c_void_p(idx.data_ptr()), None, 777, None,
                                     ctypes.c_void_p(out.data_ptr()), 80, N.current_stream())
    assert rc == 0
    assert torch.equal(out[:, :34], x[idx]) and (out[:, 34:] == 0).all()


@pytest.mark.parametrize("which", ["n_ent_dev", "n_rows_dev"])
def test_local_scene_rows_wants_both_counts_or_neither(which):
    """pbn_local_scene_rows with exactly one of its two device counts: PBN_ERR_ARG (-1), decided before any launch -- the outputs
    keep their pattern."""
    from pbnet_amd import _native as N
    n_rows, c = 5, 32
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=DEV)
    row_start, zero = i32([0, n_rows]), i32([0])
    weight = torch.ones(1, device=DEV)
    member_idx = torch.arange(n_rows, dtype=torch.int32, device=DEV)
    ins_ind = torch.arange(n_rows, dtype=torch.int64, device=DEV)
    xyz = torch.rand(n_rows, 3, device=DEV)
    feat, score = torch.randn(n_rows, c, device=DEV), torch.rand(n_rows, 1, device=DEV)
    point_idx = torch.full((n_rows,), -7, dtype=torch.int64, device=DEV)
    row_scene, coords = point_idx.clone(), torch.full((n_rows, 4), -7, dtype=torch.int32, device=DEV)
    out = torch.full((n_rows, c + 2), -7.0, device=DEV)
    count = i32([n_rows if which == "n_rows_dev" else 1])
    rc = N.lib().pbn_local_scene_rows(
        N.ptr(row_start), N.ptr(zero), N.ptr(zero), N.ptr(weight), 1, n_rows, N.ptr(count) if which == "n_ent_dev" else None,
        N.ptr(count) if which == "n_rows_dev" else None, N.ptr(member_idx), N.ptr(ins_ind), N.ptr(xyz),
        stage_ops.reciprocal_f32(0.02), N.ptr(feat), c, c, N.ptr(score), 1, None, 0, N.ptr(point_idx), N.ptr(row_scene),
        N.ptr(coords), N.ptr(out), c + 2, N.current_stream())
    assert rc == -1
    torch.cuda.synchronize()
    assert (point_idx == -7).all() and (row_scene == -7).all() and (coords == -7).all() and (out == -7.0).all()


@pytest.mark.parametrize("dtype,tol", [(torch.float32, 1e-5), (torch.bfloat16, 2e-2)])
@pytest.mark.parametrize("n_out,sigmoid,hidden", [(20, False, 16), (3, False, 16), (1, True, 16), (32, False, 32)])
def test_mlp_rows_matches_modules(dtype, tol, n_out, sigmoid, hidden):
    """PBNet.py:43-82 heads: Linear -> BatchNorm(eval) -> PReLU -> Linear [-> Sigmoid], with a two-level row index."""
    import pbnet_amd.MinkowskiEngine as ME
    torch.manual_seed(n_out)
    layers = [ME.MinkowskiLinear(32, hidden, bias=False), ME.MinkowskiBatchNorm(hidden), ME.MinkowskiPReLU(),
              ME.MinkowskiLinear(hidden, n_out, bias=True)]
    if sigmoid:
        layers.append(ME.MinkowskiSigmoid())
    head = torch.nn.Sequential(*layers).eval()
    with torch.no_grad():
        head[1].bn.running_mean.normal_(0, 0.3)
        head[1].bn.running_var.uniform_(0.5, 2.0)
        head[1].bn.weight.uniform_(0.5, 1.5)
        head[1].bn.bias.normal_(0, 0.2)
        head[2].module.weight.fill_(0.2)
    x = torch.randn(3000, 32)
    idx_a = torch.randint(0, 2500, (4000,))
    idx_b = torch.randperm(3000)[:2500]
    with torch.no_grad():
        h = head[0].linear(x)
        h = head[2].module(head[1].bn(h))
        want = head[3].linear(h)
        if sigmoid:
            want = torch.sigmoid(want)
        want = want[idx_b[idx_a]]
    head = head.to(DEV)
    got = stage_ops.mlp_rows(head, x.to(DEV).to(dtype), idx_a.to(DEV), idx_b.to(DEV))
    assert got.shape == (4000, n_out) and got.dtype == dtype
    err = (got.float().cpu() - want).abs().max().item()
    # fp32: absolute; bf16: bound relative to the output range (not the parity configuration)
    assert err <= (tol if dtype == torch.float32 else tol * max(1.0, want.abs().max().item())), err


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_sem_argmax_table_and_select_points(dtype):
    """PBNet.py:134,151-170: arg-max / own-class softmax / population table, then the stable class-major selection."""
    torch.manual_seed(4)
    n, s, nb = 70001, 20, 3
    score = (torch.randn(n, s) * 3).to(dtype).to(DEV)
    score[:5000, 7] += 20                                           # long single-class runs
    batch = torch.randint(0, nb, (n,), dtype=torch.int32, device=DEV)
    sem_pred, sem_prob, table, block_hist = stage_ops.sem_argmax_table(score, batch, nb)
    sf = score.float()
    want_pred = sf.max(1)[1]
    assert torch.equal(sem_pred, want_pred)
    want_prob = torch.softmax(sf, 1).gather(1, want_pred.view(-1, 1)).view(-1)
    assert (sem_prob.float() - want_prob).abs().max().item() <= (1e-6 if dtype == torch.float32 else 4e-3)
    want_table = torch.bincount(want_pred * nb + batch.long(), minlength=s * nb).view(s, nb)
    assert torch.equal(table.long(), want_table)
    assert torch.equal(block_hist.sum(0).long(), want_table.sum(1))
    # selection: drop classes 0, 1 and two more
    per_class = want_table.sum(1).cpu()
    classes = [c for c in range(2, s) if c not in (5, 11)]
    class_base = torch.full((s,), -1, dtype=torch.int32)
    run = 0
    for c in classes:
        class_base[c] = run
        run += int(per_class[c])
    xyz = torch.randn(n, 3, device=DEV)
    offset = torch.randn(n, 3, device=DEV).to(dtype)
    ins_ind, ins_orig, ins_off, ins_sem = stage_ops.select_points(sem_pred, class_base.to(DEV), block_hist, xyz, offset, run)
    keep = torch.zeros(s, dtype=torch.bool)
    keep[classes] = True
    key = torch.where(keep.to(DEV)[want_pred], want_pred, torch.full_like(want_pred, s))
    order = torch.sort(key, stable=True)[1][:run]
    assert torch.equal(ins_ind, order)
    assert torch.equal(ins_orig, xyz[order])
    assert torch.equal(ins_off, xyz[order] + offset[order].float())
    assert torch.equal(ins_sem, want_pred[order].to(torch.int32))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_proposal_compaction_matches_get_proposal(dtype):
    """PBNet.py:317-347 (+240-252): threshold, per-scene counts, dense renumbering of surviving scenes, order kept."""
    torch.manual_seed(8)
    n_scenes, n_points = 41, 9000
    lens = torch.randint(0, 900, (n_scenes,))
    lens[3] = 0
    lens[17] = 5000
    row_scene = torch.repeat_interleave(torch.arange(n_scenes), lens).to(DEV)
    r = int(row_scene.shape[0])
    point_idx = torch.randint(0, n_points, (r,), device=DEV)
    score = torch.rand(r, 1, device=DEV).to(dtype)
    score[row_scene == 9] = 0.1                                     # a scene that dies entirely
    xyz = (torch.rand(n_points, 3, device=DEV) * 8 - 2)
    feat = torch.randn(n_points, 32, device=DEV).to(dtype)
    thd, scale, voxel = 0.45, 1, 0.02
    per_scene_d, block_cnt = stage_ops.mask_count(score, thd, row_scene, n_scenes)
    keep = score.view(-1).float() > thd
    want_per_scene = torch.bincount(row_scene[keep], minlength=n_scenes)
    assert torch.equal(per_scene_d.long(), want_per_scene)
    per_scene = want_per_scene.cpu()
    alive = per_scene > 0
    dense_of = (torch.cumsum(alive.to(torch.int32), 0) - 1).to(torch.int32)
    total = int(per_scene.sum())
    pidx, pms, coords, f3 = stage_ops.proposal_rows(score, thd, row_scene, point_idx, dense_of.to(DEV), block_cnt, total,
                                                    xyz, scale, voxel, feat)
    valid = torch.nonzero(keep).view(-1)
    want_idx = torch.stack([dense_of.to(DEV).long()[row_scene[valid]], point_idx[valid]], 1)
    assert torch.equal(pidx, want_idx)
    assert torch.equal(pms, score[valid].view(-1))
    p = want_idx[:, 1]
    want_c = torch.cat([want_idx[:, 0:1].to(torch.int32), torch.floor(xyz[p] * scale / voxel).to(torch.int32)], 1)
    assert torch.equal(coords, want_c)
    assert torch.equal(f3, feat[p])


N_CAP, N_SCENES, E_CAP = 1500, 12, 64


@pytest.fixture(scope="module")
def capacity_case():
    """Inputs of the capacity-form test, built once per dtype: N_CAP rows of 32 channels in N_SCENES local scenes.  Everything
    past a count is in range too (and would change the result if it were read: scores above the threshold)."""
    made = {}

    def make(dtype):
        if dtype not in made:
            g = torch.Generator().manual_seed(11)
            n_points, m, n_members = 4000, 3000, 2500
            c = dict(n_points=n_points, m=m, n_members=n_members)
            c["xyz"] = (torch.rand(n_points, 3, generator=g) * 8 - 2).to(DEV)
            c["point_feat"] = torch.randn(n_points, 32, generator=g).to(dtype).to(DEV)
            c["sem_prob"] = torch.rand(n_points, 1, generator=g).to(dtype).to(DEV)
            c["ins_ind"] = torch.randperm(n_points, generator=g)[:m].to(DEV)
            c["member_idx"] = torch.randint(0, m, (n_members,), generator=g, dtype=torch.int32).to(DEV)
            c["row_scene"] = torch.sort(torch.randint(0, N_SCENES, (N_CAP,), generator=g))[0].to(DEV)
            c["point_idx"] = torch.randint(0, n_points, (N_CAP,), generator=g).to(DEV)
            score = torch.rand(N_CAP, 1, generator=g)
            score[c["row_scene"].cpu() == 4] = 0.1                   # a scene that dies entirely
            c["score"] = score.to(dtype).to(DEV)
            c["idx"] = torch.randint(0, 2000, (N_CAP,), generator=g).to(DEV)
            c["idx2"] = torch.randperm(n_points, generator=g)[:2000].to(DEV)
            import pbnet_amd.MinkowskiEngine as ME
            torch.manual_seed(5)
            c["head"] = torch.nn.Sequential(ME.MinkowskiLinear(32, 16, bias=False), ME.MinkowskiBatchNorm(16), ME.MinkowskiPReLU(),
                                            ME.MinkowskiLinear(16, 3, bias=True)).eval().to(DEV)
            made[dtype] = c
        return made[dtype]
    return make


def _entry_tables(n, c):
    """n rows split over at most 20 entries: (size-exact packed table, n_ent, the same entries in an E_CAP-entry table)."""
    rng = np.random.default_rng(n)
    n_ent = min(n, 20)
    cuts = np.sort(rng.choice(np.arange(1, n), n_ent - 1, replace=False)) if n_ent > 1 else np.zeros(0, dtype=np.int64)
    row_start = np.concatenate([[0], cuts, [n]]).astype(np.int32) if n_ent else np.zeros(1, dtype=np.int32)
    sizes = np.diff(row_start)
    cols = [row_start, np.asarray([rng.integers(0, c["n_members"] - s + 1) for s in sizes], dtype=np.int32),
            np.sort(rng.integers(0, N_SCENES, n_ent)).astype(np.int32), rng.uniform(0.05, 1.0, n_ent).astype(np.float32).view(np.int32)]
    wide = np.zeros(4 * E_CAP + 1, dtype=np.int32)
    for k, col in enumerate(cols):
        at = k * E_CAP + 1 if k else 0
        wide[at:at + len(col)] = col
    return torch.from_numpy(np.concatenate(cols)).to(DEV), n_ent, stage_ops.EntryTable(torch.from_numpy(wide).to(DEV), E_CAP)


@pytest.mark.parametrize("n", [0, 1, 1025, 1500])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_capacity_form_equals_size_exact_form(capacity_case, dtype, n):
    """The wrappers' own marshalling: each stage op on n rows (host sizes) against the same op at capacity N_CAP with the count n
    on the device -- N_CAP crosses one 1024-row selection block and several 256-thread blocks.  Bit equality on the first n rows."""
    c = capacity_case(dtype)
    CNT = stage_ops.CNT
    counts = torch.zeros(CNT.WORDS, dtype=torch.int32)
    packed, n_ent, wide = _entry_tables(n, c)
    counts[CNT.ENTRIES], counts[CNT.ROWS], counts[CNT.SCENES] = n_ent, n, N_SCENES      # (proposal_offsets reads SCENES)
    counts = counts.to(DEV)
    n_d = counts[CNT.ROWS:CNT.ROWS + 1]
    same = lambda got, want, k: all(torch.equal(g[:k], w) for g, w in zip(got, want))

    # local_scene_rows
    common = (c["member_idx"], c["ins_ind"], c["xyz"], 0.02, c["point_feat"], c["sem_prob"], None)
    want = stage_ops.local_scene_rows(packed, n_ent, n, *common)
    got = stage_ops.local_scene_rows(wide, E_CAP, N_CAP, *common, n_ent_dev=counts[CNT.ENTRIES:CNT.ENTRIES + 1], n_rows_dev=n_d)
    assert want[3].shape == (n, 34) and got[3].shape == (N_CAP, 34) and same(got, want, n)

    # mlp_rows (two index levels; in_rows = the rows of the input)
    feats = c["point_feat"]
    want = stage_ops.mlp_rows(c["head"], feats, c["idx"][:n], c["idx2"])
    got = stage_ops.mlp_rows(c["head"], feats, c["idx"], c["idx2"], N_CAP, n_dev=n_d, in_rows=c["n_points"])
    assert want.shape == (n, 3) and got.shape == (N_CAP, 3) and torch.equal(got[:n], want)

    # gather_pad_rows: one index, and (capacity form only) two
    x = c["point_feat"]
    want = stage_ops.gather_pad_rows(x, 40, c["idx"][:n])
    got = stage_ops.gather_pad_rows(x, 40, c["idx"], None, N_CAP, n_d)
    assert want.shape == (n, 40) and torch.equal(got[:n], want) and torch.equal(want[:, :32], x[c["idx"][:n]]) and not want[:, 32:].any()
    got = stage_ops.gather_pad_rows(x, 40, c["idx"], c["idx2"], N_CAP, n_d)
    assert torch.equal(got[:n], stage_ops.gather_pad_rows(x, 40, c["idx2"][c["idx"][:n]]))

    # mask_count -> proposal_offsets -> proposal_rows; the size-exact form takes its offsets from the host (PBNet._proposals_fused)
    thd, rs, pi, sc = 0.45, c["row_scene"], c["point_idx"], c["score"]
    per_scene, block_cnt = stage_ops.mask_count(sc[:n], thd, rs[:n], N_SCENES)
    per_scene_h = per_scene.cpu().long()
    alive = per_scene_h > 0
    total, n_alive = int(per_scene_h.sum()), int(alive.sum())
    dense_of = (torch.cumsum(alive.to(torch.int32), 0) - 1).to(torch.int32).to(DEV)
    want = stage_ops.proposal_rows(sc[:n], thd, rs[:n], pi[:n], dense_of, block_cnt, total, c["xyz"], 1, 0.02, c["point_feat"])
    per_scene_c, block_cnt_c = stage_ops.mask_count(sc, thd, rs, N_SCENES, n_dev=n_d)
    assert torch.equal(per_scene_c, per_scene)
    offsets, alive_ids, dense_of_c = stage_ops.proposal_offsets(per_scene_c, counts)
    got = stage_ops.proposal_rows(sc, thd, rs, pi, dense_of_c, block_cnt_c, N_CAP, c["xyz"], 1, 0.02, c["point_feat"], n_dev=n_d)
    h = counts.cpu().tolist()
    assert h[CNT.PROPOSAL_ROWS] == total and h[CNT.PROPOSALS] == n_alive and h[CNT.OVERFLOW] == 0
    assert torch.equal(offsets[:n_alive + 1].cpu(), torch.cat([torch.zeros(1, dtype=torch.long), torch.cumsum(per_scene_h[alive], 0)]))
    assert torch.equal(alive_ids[:n_alive].cpu(), torch.nonzero(alive).view(-1))
    assert got[0].shape == (N_CAP, 2) and same(got, want, total)
