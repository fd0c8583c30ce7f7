"""GPU tier: the batched post-processing (postprocess.refine_batch_device, csrc/post_batch.hip) on the synthetic merged batches
of tests/post_batch_cases.py against two yardsticks this file does not own, both run PER SCENE on the scene's own rows with
point_num = 3 * n_j: tests/post_ref.py (numpy, device tie rule) and postprocess.refine_instances_device.  Everything compared is
integer work, an fp32 quotient of exact integers or a copied score: every comparison is bit-equality."""
import types

import numpy as np
import pytest
import torch

import post_batch_cases as C
from pbnet_amd import _native as N
from pbnet_amd import postprocess as PP

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAMES = [c["name"] for c in C.cases()]
SENTINEL = 0x5A


def cfg_of(c):
    return types.SimpleNamespace(TEST_SCORE_THRESH=c["score_t"], TEST_NPOINT_THRESH=c["npoint_t"], TEST_NMS_THRESH=c["nms_t"])


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def run_batch(c, ws=None):
    sups = [None if s is None else dev(s) for s in c["sups"]]
    n_sp = None if all(v is None for v in c["n_sp"]) else c["n_sp"]
    return PP.refine_batch_device(dev(c["pred_sem"]), (dev(c["pidx"]), dev(c["off"])), dev(c["clt"]), c["point_starts"], sups,
                                  cfg_of(c), n_superpoints=n_sp, workspace=ws)


def assert_equal(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want), what


def check_scene(c, rb, scalars, j, want):
    what = "%s scene %d: " % (c["name"], j)
    n_j, b = c["sizes"][j], len(c["sizes"])
    inst = rb.scene(j, scalars)
    dense = rb.dense(j, scalars).cpu().numpy()
    k = scalars[j]
    assert k == want["keep"].shape[0], what + "n_keep"
    assert dense.shape == (k, n_j) and inst["point_instance"].shape == (n_j,)
    assert_equal(dense, want["clusters"].reshape(k, n_j), what + "clusters")
    assert_equal(inst["scores"].cpu().numpy(), want["scores"], what + "scores")
    assert_equal(inst["semantic_id"].cpu().numpy(), want["semantic_id"], what + "semantic_id")
    assert_equal(inst["npoints"].cpu().numpy(), want["npoints"], what + "npoints")
    pi = inst["point_instance"].cpu().numpy()
    assert pi.dtype == np.int32 and ((pi == -100) | ((pi >= 0) & (pi < k))).all()
    for r in range(k):
        assert np.array_equal(dense[r] != 0, pi == r), what + "dense row %d" % r
    # the internal lists, under post_ref's names
    p = rb.n_prop
    if p:
        n_rows, n_pick = int(rb.table("n_rows")[j]), int(rb.table("n_pick")[j])
        mine = C.scene_inputs(c, j)["merged_proposals"]
        assert_equal(rb.table("rows")[:b * p].view(b, p)[j, :n_rows].cpu().numpy(), mine[want["rows"]].astype(np.int32), what + "rows")
        assert_equal(rb.table("pick_rows")[:b * p].view(b, p)[j, :n_pick].cpu().numpy(), mine[want["pick_rows"]].astype(np.int32),
                     what + "pick_rows")
        lo, hi = c["point_starts"][j], c["point_starts"][j + 1]
        assert_equal(rb.table("seg")[lo:hi].cpu().numpy(), want["seg"].astype(np.int32), what + "seg")
    # the tails of the capacity-shaped arrays are defined
    assert not rb.scores[j, k:].any() and bool((rb.semantic_id[j, k:] == -1).all()) and not rb.npoints[j, k:].any()


def device_form_per_scene(c, j):
    """The parent's device form on scene j's own rows: (clusters, scores, semantic_id) as numpy."""
    i = C.scene_inputs(c, j)
    res = PP.refine_instances_device(dev(i["pred_sem"]), (dev(i["pidx"]), dev(i["off"])), dev(i["clt"]), i["point_num"], dev(i["sp"]),
                                     cfg_of(c), n_superpoints=i["n_sp"])
    return tuple(t.cpu().numpy() for t in res.sliced())


@pytest.mark.parametrize("name", NAMES)
def test_every_scene_equals_both_yardsticks(name):
    c = C.case(name)
    rb = run_batch(c)
    scalars = rb.scalars.tolist()
    b = len(c["sizes"])
    assert rb.point_instance.dtype == torch.int32 and rb.point_instance.shape == (c["point_starts"][-1],)
    assert rb.scores.shape == rb.semantic_id.shape == rb.npoints.shape == (b, rb.n_prop) and len(scalars) == 2 * b
    for j, want in enumerate(C.reference(name)):
        if j == c["error_scene"]:
            assert scalars[b + j] == PP.STATUS_SUPERPOINT_RANGE
            with pytest.raises(ValueError):
                rb.scene(j, scalars)
            with pytest.raises(ValueError):
                rb.dense(j)
            continue
        assert scalars[b + j] == 0
        check_scene(c, rb, scalars, j, want)
        clusters, scores, sem = device_form_per_scene(c, j)
        assert_equal(rb.dense(j, scalars).cpu().numpy(), clusters, "%s scene %d: clusters of the device form" % (name, j))
        inst = rb.scene(j, scalars)
        assert_equal(inst["scores"].cpu().numpy(), scores, "scores of the device form")
        assert_equal(inst["semantic_id"].cpu().numpy(), sem, "semantic_id of the device form")
        assert_equal(inst["npoints"].cpu().numpy(), clusters.sum(1).astype(np.int32), "npoints of the device form")


def test_superpoint_id_at_the_bound_touches_no_other_scene():
    """The id at scene e's bound would index the first vote row of scene e + 1.  Every byte of the workspace is set to a sentinel
    before the call with the id in range and before the call with the id at the bound: the vote rows and labels outside scene e's
    slice are the same bytes after both, the columns of scene e's rows past its live buckets and everything behind the tables
    still hold the sentinel."""
    c = C.case("sp_error")
    e, b = c["error_scene"], len(c["sizes"])
    n_prop = c["clt"].shape[0]
    sp_starts = PP.superpoint_starts(c["point_starts"], [s is not None for s in c["sups"]], c["n_sp"])
    ws = PP.PostBatchWorkspace(n_prop, c["point_starts"][-1], b, sp_starts[-1] + 9, DEV)
    lay = N.PostBatchLayout()
    used = N.lib().pbn_post_batch_workspace_bytes(n_prop, c["point_starts"][-1], b, sp_starts[-1], lay)
    assert used < ws.nbytes
    snaps = []
    for case in (C.without_error(c), c):
        ws.buffer.fill_(SENTINEL)
        rb = run_batch(case, ws)
        votes = rb.table("votes")[:sp_starts[-1] * (n_prop + 1)].view(sp_starts[-1], n_prop + 1)
        snaps.append((votes.clone(), rb.table("sp_label")[:sp_starts[-1]].clone(), rb.scalars.tolist(), int(rb.table("n_pick")[e])))
        assert bool((ws.buffer[used:] == SENTINEL).all())
        assert rb.sp_starts == sp_starts
    (votes0, label0, sc0, _), (votes1, label1, sc1, n_pick_e) = snaps
    assert sc0[b:] == [0] * b and sc1[b:] == [PP.STATUS_SUPERPOINT_RANGE if j == e else 0 for j in range(b)]
    outside = torch.ones(sp_starts[-1], dtype=torch.bool, device=DEV)
    outside[sp_starts[e]:sp_starts[e + 1]] = False
    assert torch.equal(votes0[outside], votes1[outside]) and torch.equal(label0[outside], label1[outside])
    word = int(np.frombuffer(bytes([SENTINEL] * 4), np.int32)[0])
    assert bool((votes1[sp_starts[e]:sp_starts[e + 1], n_pick_e + 1:] == word).all()) and n_pick_e + 1 < n_prop + 1
    # the raised id took no part: one vote fewer in scene e's slice, none more anywhere
    live0, live1 = votes0[sp_starts[e]:sp_starts[e + 1], :n_pick_e + 1], votes1[sp_starts[e]:sp_starts[e + 1], :n_pick_e + 1]
    assert int(live0.sum()) == c["sizes"][e] and int(live1.sum()) == c["sizes"][e] - 1


@pytest.mark.parametrize("name", ["b8", "stride"])
def test_a_second_call_gives_the_same_bytes(name):
    c = C.case(name)
    rb = run_batch(c)
    ws = rb.workspace
    outs = lambda: [t.clone() for t in (ws.point_instance, ws.scores, ws.semantic_id, ws.npoints, ws.scalars, ws.buffer)]
    first = outs()
    run_batch(c, ws)
    for a, b in zip(first, outs()):
        assert torch.equal(a, b)


def test_a_fitting_call_stops_nowhere_and_allocates_nothing():
    c = C.case("b8")
    cfg = cfg_of(c)
    sups = [None if s is None else dev(s) for s in c["sups"]]
    sem, pidx, off, clt = dev(c["pred_sem"]), dev(c["pidx"]), dev(c["off"]), dev(c["clt"])
    sp_starts = PP.superpoint_starts(c["point_starts"], [s is not None for s in c["sups"]], c["n_sp"])
    ws = PP.PostBatchWorkspace(clt.shape[0] + 5, c["point_starts"][-1] + 100, 8, sp_starts[-1] + 3, DEV)
    PP.refine_batch_device(sem, (pidx, off), clt, c["point_starts"], sups, cfg, n_superpoints=c["n_sp"], workspace=ws)
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    torch.cuda.set_sync_debug_mode("error")
    try:
        rb = PP.refine_batch_device(sem, (pidx, off), clt, c["point_starts"], sups, cfg, n_superpoints=c["n_sp"], workspace=ws)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.cuda.memory_allocated() == before
    scalars = rb.scalars.tolist()
    for j, want in enumerate(C.reference("b8")):
        check_scene(c, rb, scalars, j, want)


def test_capacity_and_argument_checks():
    lib = N.lib()
    c = C.case("b2")
    cfg = cfg_of(c)
    too_many = lib.pbn_post_max_proposals() + 1
    with pytest.raises(ValueError):
        PP.PostBatchWorkspace(too_many, 100, 2, 10, DEV)
    off = torch.zeros(too_many + 1, dtype=torch.int64, device=DEV)
    with pytest.raises(ValueError):
        PP.refine_batch_device(dev(c["pred_sem"]), (dev(c["pidx"]), off), torch.zeros(too_many, device=DEV), c["point_starts"], None, cfg)
    # the C entry itself refuses before any launch (the pointers are never dereferenced)
    t = PP.scene_table([0, 70, 103], [0, 0, 0])
    fake = N.c_vp(1 << 20)
    call = lambda n_prop, table, n_total=103, ws_bytes=1 << 40: lib.pbn_post_batch(
        fake, 10, fake, 1, n_prop, fake, 0, fake, 1, n_total, table, None, 0.3, 4, 0.3, fake, 20, fake, fake, fake, fake, fake, fake,
        ws_bytes, None)
    assert call(too_many, t) == N.PBN_ERR_UNSUPPORTED
    assert call(10, t, n_total=104) == N.PBN_ERR_ARG                       # the table does not cover the points
    assert call(10, PP.scene_table([0, 70, 60], [0, 0, 0]), n_total=60) == N.PBN_ERR_ARG
    assert call(10, t, ws_bytes=64) == N.PBN_ERR_WORKSPACE
    small = PP.PostBatchWorkspace(2, 50, 1, 0, DEV)
    with pytest.raises(ValueError):
        run_batch(c, small)
