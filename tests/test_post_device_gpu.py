"""GPU tier: the device-resident post-processing (postprocess.refine_instances_device: pbn_post_select, pbn_mask_iou_dev,
pbn_post_nms, pbn_superpoint_refine_dev, pbn_post_compact of csrc/post.hip).  Everything is integer work or an fp32 quotient of
exact integers, so every comparison is bit-equal.

Yardsticks: the recorded goldens of the reference's own functions, tests/post_ref.py (the numpy restatement under the device tie
rule: score descending, lower survivor index first among equal scores; tests/test_post_ref_cpu.py runs it over the goldens on the
CPU) and the untouched host form `refine_instances`.

post_P1, P2 and P3 are compared with the goldens as recorded.  post_P4 is compared as recorded on `out_pointnum` and
`out_cross_ious` and from `pick` onward against tests/post_ref.py: its tied pair of survivors (score 0.6217706, IoU 0.60 > 0.1)
was walked higher index first by the unstable argsort of the numpy that recorded it, which picks survivor 1 where the device rule
picks survivor 0 (shown on the CPU in test_post_ref_cpu.py)."""
import glob
import os
import types

import numpy as np
import pytest
import torch

import post_ref as R
from pbnet_amd import postprocess as PP

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HERE = os.path.dirname(os.path.abspath(__file__))
CASES = sorted(glob.glob(os.path.join(HERE, "golden", "post_P*.npz")))
AS_RECORDED = ("post_P1", "post_P2", "post_P3")


def cfg_of(score_t=0.07, npoint_t=101, nms_t=0.1):
    return types.SimpleNamespace(TEST_SCORE_THRESH=float(score_t), TEST_NPOINT_THRESH=int(npoint_t), TEST_NMS_THRESH=float(nms_t))


def golden_inputs(g):
    return dict(pred_sem=g["in_pred_sem"], pidx=g["in_proposals_idx"], off=g["in_proposals_offset"], clt=g["in_clt"],
                point_num=int(g["in_point_num"]), sp=g["in_superpoint"])


def random_inputs(seed, n_prop, n_fold, n_sp, members=(20, 60), scores=None):
    """Proposals of `members` distinct random points each, spread over the three copies."""
    rng = np.random.default_rng(seed)
    rows = []
    for p in range(n_prop):
        pts = rng.permutation(n_fold)[:min(n_fold, int(rng.integers(members[0], members[1] + 1)))]
        pts = np.sort(pts + n_fold * rng.integers(0, 3, pts.shape[0]))
        rows.append(np.stack([np.full(pts.shape[0], p, np.int64), pts.astype(np.int64)], 1))
    pidx = np.concatenate(rows)
    off = np.concatenate([[0], np.cumsum([r.shape[0] for r in rows])]).astype(np.int64)
    clt = rng.random(n_prop).astype(np.float32) if scores is None else np.asarray(scores, np.float32)
    return dict(pred_sem=rng.integers(0, 20, 3 * n_fold).astype(np.int64), pidx=pidx, off=off, clt=clt, point_num=3 * n_fold,
                sp=rng.integers(0, n_sp, n_fold).astype(np.int64))


def to_device(inp):
    return {k: (torch.from_numpy(np.ascontiguousarray(v)).to(DEV) if isinstance(v, np.ndarray) else v) for k, v in inp.items()}


def run_device(d, cfg, n_sp=None, ws=None):
    return PP.refine_instances_device(d["pred_sem"], (d["pidx"], d["off"]), d["clt"], d["point_num"], d["sp"], cfg,
                                      n_superpoints=n_sp, workspace=ws)


def run_ref(inp, cfg, n_sp=None):
    return R.refine(inp["pred_sem"], inp["pidx"], inp["off"], inp["clt"], inp["point_num"], inp["sp"], cfg.TEST_SCORE_THRESH,
                    cfg.TEST_NPOINT_THRESH, cfg.TEST_NMS_THRESH, n_superpoints=n_sp)


def outputs(res, check_status=True):
    """Every array of a result under post_ref's names, cut to the live counts (this is where the test synchronises)."""
    n_rows, n_pick, n_keep, status = res.scalars.tolist()
    h = lambda t: t.cpu().numpy()
    out = dict(pointnum=h(res.pointnum), rows=h(res.rows)[:n_rows], cross_ious=h(res.cross_ious)[:n_rows, :n_rows],
               pick=h(res.pick)[:n_pick], pick_rows=h(res.pick_rows)[:n_pick], seg=h(res.seg), seg_refined=h(res.seg_refined),
               keep=h(res.keep)[:n_keep], status=status)
    if check_status:
        clusters, scores, sem_id = res.sliced()
        assert clusters.shape == (n_keep, res.n_fold) and scores.shape == (n_keep,) and sem_id.shape == (n_keep,)
        out.update(clusters=h(clusters), scores=h(scores), semantic_id=h(sem_id))
        # the tails past the live counts are defined too
        assert (h(res.rows)[n_rows:] == -1).all() and (h(res.pick)[n_pick:] == -1).all() and (h(res.keep)[n_keep:] == -1).all()
        assert not h(res.clusters)[n_keep:].any()
    return out


def assert_same(got, want, keys=None):
    for key in (keys or [k for k in want if k in got]):
        a, b = np.asarray(got[key]), np.asarray(want[key])
        assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b, equal_nan=a.dtype.kind == "f"), key


def check_against_ref(inp, cfg, n_sp=None):
    got = outputs(run_device(to_device(inp), cfg, n_sp))
    want = run_ref(inp, cfg, n_sp)
    assert_same(got, want)
    return got


# ---- 1. goldens --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", CASES, ids=[os.path.basename(p)[:-4] for p in CASES])
def test_goldens(path):
    g = np.load(path)
    name = os.path.basename(path)[:-4]
    cfg = cfg_of(g["score_t"], g["npoint_t"], g["nms_t"])
    inp = golden_inputs(g)
    got = outputs(run_device(to_device(inp), cfg))
    recorded = {v: g[k] for k, v in R.GOLDEN_KEYS.items()}
    if name in AS_RECORDED:
        assert_same(got, recorded, list(recorded))
    else:                                                                     # post_P4: see the module docstring
        assert_same(got, recorded, ["pointnum", "cross_ious"])
        assert_same(got, run_ref(inp, cfg), ["pick", "seg", "seg_refined", "clusters", "scores", "semantic_id"])
    if name == "post_P1":
        assert got["pick"].shape[0] == 4 and got["keep"].shape[0] == 0        # every picked cluster vanishes in the vote
    if name == "post_P4":
        assert got["pointnum"].shape[0] == 6 and got["seg"].shape[0] == 997


# ---- 2. boundary shapes ------------------------------------------------------------------------------------------------------
def test_one_proposal():
    got = check_against_ref(random_inputs(1, 1, 300, 7, members=(120, 120), scores=[0.5]), cfg_of(npoint_t=10), 7)
    assert got["rows"].tolist() == [0] and got["pick"].tolist() == [0]


def test_no_survivor_leaves_every_later_kernel_cleanly():
    got = check_against_ref(random_inputs(2, 12, 400, 9), cfg_of(score_t=2.0, npoint_t=5), 9)
    assert got["rows"].shape[0] == 0 and got["pick"].shape[0] == 0 and got["clusters"].shape == (0, 400)
    assert (got["seg"] == -100).all() and (got["seg_refined"] == -100).all()


@pytest.mark.parametrize("n_fold", [31, 32, 33])
def test_bitset_word_edges(n_fold):
    got = check_against_ref(random_inputs(3 + n_fold, 9, n_fold, 5, members=(6, 14)), cfg_of(score_t=0.05, npoint_t=3, nms_t=0.3), 5)
    assert got["rows"].shape[0] > 1 and got["pick"].shape[0] > 0


@pytest.mark.parametrize("n_prop", [65, 129])
def test_equal_scores_the_tie_rule_alone_decides(n_prop):
    inp = random_inputs(50 + n_prop, n_prop, 200, 23, members=(30, 50), scores=np.full(n_prop, 0.5))
    got = check_against_ref(inp, cfg_of(npoint_t=5), 23)
    assert got["rows"].shape[0] == n_prop and got["pick"][0] == 0             # lower index first
    assert 1 < got["pick"].shape[0] < n_prop                                   # some suppressed, some not


def test_iou_equal_to_the_threshold_is_not_suppressed():
    # |A| = |B| = |C| = 5; A & B = 2 points -> 2 / 8 = 0.25 exactly; A & C = 3 points -> 3 / 7
    members = [[0, 1, 2, 3, 4], [3, 4, 5, 6, 7], [0, 1, 2, 8, 9]]
    pidx = np.array([[p, pt] for p, m in enumerate(members) for pt in m], np.int64)
    inp = dict(pred_sem=np.arange(120, dtype=np.int64) % 20, pidx=pidx, off=np.array([0, 5, 10, 15], np.int64),
               clt=np.array([0.9, 0.8, 0.7], np.float32), point_num=120, sp=np.arange(40, dtype=np.int64))
    got = check_against_ref(inp, cfg_of(npoint_t=0, nms_t=0.25), 40)
    assert got["cross_ious"][0, 1] == np.float32(0.25) and got["pick"].tolist() == [0, 1]


def test_superpoint_id_at_the_last_row_of_the_table():
    inp = host_like_inputs(41)
    inp["sp"][(inp["sp"] >= 140) & (inp["sp"] < 160)] = 299                    # n_superpoints - 1: the last row of the vote table
    assert inp["sp"].max() == 299
    got = check_against_ref(inp, cfg_of(), 300)
    assert got["status"] == 0 and got["keep"].shape[0] > 1 and (got["seg_refined"][inp["sp"] == 299] >= 0).any()


# ---- 3. equality with the host form ------------------------------------------------------------------------------------------
def host_like_inputs(seed, n_prop=40, n_fold=5000, n_sp=300):
    """Proposals that are runs of neighbouring points (so that pairs overlap and superpoints agree with them), scores a
    permutation of distinct float32 values."""
    rng = np.random.default_rng(seed)
    rows = []
    for p in range(n_prop):
        start, length = int(rng.integers(0, n_fold - 700)), int(rng.integers(60, 700))
        pts = np.arange(start, start + length)[rng.random(length) < 0.8]
        pts = np.sort(pts + n_fold * rng.integers(0, 3, pts.shape[0]))
        rows.append(np.stack([np.full(pts.shape[0], p, np.int64), pts.astype(np.int64)], 1))
    scores = rng.permutation(np.linspace(0.04, 0.96, n_prop).astype(np.float32))
    assert np.unique(scores).shape[0] == n_prop
    return dict(pred_sem=rng.integers(0, 20, 3 * n_fold).astype(np.int64), pidx=np.concatenate(rows),
                off=np.concatenate([[0], np.cumsum([r.shape[0] for r in rows])]).astype(np.int64), clt=scores,
                point_num=3 * n_fold, sp=(np.arange(n_fold) * n_sp // n_fold).astype(np.int64))


def test_equals_the_host_form_without_tied_scores():
    cfg = cfg_of()
    ws = PP.PostWorkspace(40, 5000, 300, DEV)
    picked = 0
    for seed in range(20):
        inp = host_like_inputs(seed)
        d = to_device(inp)
        clusters, scores, sem_id, dbg = PP.refine_instances(d["pred_sem"], (d["pidx"], d["off"]), d["clt"], d["point_num"],
                                                            inp["sp"], cfg, return_debug=True)
        want = dict(pointnum=dbg["pointnum"].cpu().numpy(), cross_ious=dbg["cross_ious"].cpu().numpy(), pick=dbg["pick"],
                    seg=dbg["seg"].cpu().numpy(), seg_refined=dbg["seg_refined"].cpu().numpy(), clusters=clusters.cpu().numpy(),
                    scores=scores.cpu().numpy(), semantic_id=sem_id.cpu().numpy())
        got = outputs(run_device(d, cfg, 300, ws))
        assert_same(got, want, list(want))
        picked += int(0 < want["pick"].shape[0] < got["rows"].shape[0])
    assert picked == 20                                                        # every seed picks and suppresses something


# ---- 4. no host wait ---------------------------------------------------------------------------------------------------------
def p3_sized_down(g2, g3):
    """post_P3's inputs in the shapes of post_P2's buffers: points folded into P2's range, the 15 missing proposals and the
    missing member entries drawn from a seed."""
    rng = np.random.default_rng(33)
    n2, e2, p2 = int(g2["in_point_num"]), g2["in_proposals_idx"].shape[0], g2["in_clt"].shape[0]
    pidx3 = g3["in_proposals_idx"].copy()
    pidx3[:, 1] %= n2
    p3 = g3["in_clt"].shape[0]
    extra = e2 - pidx3.shape[0]
    owner = np.sort(p3 + np.arange(extra) % (p2 - p3))
    pidx = np.concatenate([pidx3, np.stack([owner, rng.integers(0, n2, extra)], 1).astype(np.int64)])
    off = np.concatenate([[0], np.cumsum(np.bincount(pidx[:, 0], minlength=p2))]).astype(np.int64)
    clt = np.concatenate([g3["in_clt"].reshape(-1), rng.random(p2 - p3).astype(np.float32)])
    return dict(pred_sem=g3["in_pred_sem"][:n2].copy(), pidx=pidx, off=off, clt=clt, point_num=n2,
                sp=g3["in_superpoint"][:n2 // 3].copy())


def test_one_call_is_capturable_and_allocates_nothing():
    g2, g3 = np.load(CASES[1]), np.load(CASES[2])
    cfg = cfg_of()
    first, second = golden_inputs(g2), p3_sized_down(g2, g3)
    for key in ("pred_sem", "pidx", "off", "clt", "sp"):
        assert first[key].shape == second[key].shape and first[key].dtype == second[key].dtype, key
    n_sp = int(max(first["sp"].max(), second["sp"].max())) + 1
    buf = to_device(first)
    ws = PP.PostWorkspace(first["clt"].shape[0], first["point_num"] // 3, n_sp, DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run_device(buf, cfg, n_sp, ws)                                         # loads the code objects outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                              # raises on any synchronising call
        res = run_device(buf, cfg, n_sp, ws)
    for inp in (first, second):
        for key in ("pred_sem", "pidx", "off", "clt", "sp"):
            buf[key].copy_(torch.from_numpy(np.ascontiguousarray(inp[key])))
        ws.scalars.fill_(-7)
        graph.replay()
        assert_same(outputs(res), run_ref(inp, cfg, n_sp))
    del graph
    run_device(buf, cfg, n_sp, ws)
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    again = run_device(buf, cfg, n_sp, ws)
    assert torch.cuda.memory_allocated() == before
    assert_same(outputs(again), run_ref(second, cfg, n_sp))


# ---- 5. a superpoint id the table has no row for -----------------------------------------------------------------------------
def test_overflowing_superpoint_id_sets_the_status_and_writes_nothing_out_of_bounds():
    n_prop, n_fold, n_sp, guard, sentinel = 40, 5000, 290, 4096, 0x5A5A5A5A
    inp = host_like_inputs(42)                                                 # ids 0..299: 290 is the first id past the table
    inp["sp"][300] = 1 << 40
    over = np.nonzero(inp["sp"] >= n_sp)[0]
    assert inp["sp"].min() == 0 and (inp["sp"] == n_sp).any() and over.shape[0] > 100
    cfg = cfg_of()
    ws = PP.PostWorkspace(n_prop, n_fold, n_sp, DEV)
    n_hist, n_lab = ws.hist.numel(), ws.sp_label.numel()
    hist_guard = torch.full((guard + n_hist + guard,), sentinel, dtype=torch.int32, device=DEV)
    label_guard = torch.full((guard + n_lab + guard,), sentinel, dtype=torch.int64, device=DEV)
    ws.hist, ws.sp_label = hist_guard[guard:guard + n_hist], label_guard[guard:guard + n_lab]
    res = run_device(to_device(inp), cfg, n_sp, ws)
    got = outputs(res, check_status=False)
    assert got["status"] & PP.STATUS_SUPERPOINT_RANGE
    with pytest.raises(ValueError):
        res.sliced()
    for g, n in ((hist_guard, n_hist), (label_guard, n_lab)):
        assert bool((g[:guard] == sentinel).all()) and bool((g[guard + n:] == sentinel).all())
    want = run_ref(inp, cfg, n_sp)
    assert want["status"] == R.STATUS_SUPERPOINT_RANGE
    assert_same(got, want, ["pointnum", "rows", "cross_ious", "pick", "seg", "seg_refined", "keep"])
    assert (got["seg_refined"][over] == -100).all() and (got["seg_refined"] >= 0).any()


def test_capacity_limit_and_argument_checks():
    lib = PP.N.lib()
    assert lib.pbn_post_max_proposals() == 4096
    z = torch.zeros(8, dtype=torch.int32, device=DEV)
    f = torch.zeros(8, dtype=torch.float32, device=DEV)
    st = PP.N.current_stream()
    assert lib.pbn_post_select(PP.N.ptr(f), PP.N.ptr(z), 4097, 0.1, 1, PP.N.ptr(z), PP.N.ptr(z), PP.N.ptr(z), st) == PP.N.PBN_ERR_UNSUPPORTED
    assert lib.pbn_post_nms(PP.N.ptr(f), PP.N.ptr(z), PP.N.ptr(z), 4097, PP.N.ptr(f), 0.1, PP.N.ptr(z), PP.N.ptr(z), PP.N.ptr(z),
                            st) == PP.N.PBN_ERR_UNSUPPORTED
    assert lib.pbn_post_select(None, PP.N.ptr(z), 4, 0.1, 1, PP.N.ptr(z), PP.N.ptr(z), PP.N.ptr(z), st) == PP.N.PBN_ERR_ARG
    with pytest.raises(ValueError):
        PP.PostWorkspace(4097, 100, 10, DEV)
    d = to_device(random_inputs(1, 3, 64, 4))
    with pytest.raises(ValueError):                                            # a workspace that does not fit
        run_device(d, cfg_of(), 4, PP.PostWorkspace(2, 64, 4, DEV))
    with pytest.raises(TypeError):                                             # ids must already be int64 on the device
        PP.refine_instances_device(d["pred_sem"], (d["pidx"], d["off"]), d["clt"], d["point_num"], d["sp"].int(), cfg_of())
