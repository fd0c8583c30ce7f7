"""GPU tier: the folding batched post-processing (postprocess.refine_tta_merged_device, pbn_post_batch_tta in csrc/post_batch.hip)
on the synthetic merged TTA batches of tests/post_tta_cases.py against two yardsticks this file does not own, both run PER SCENE on
the scene's own slice with point_num = 3 * n_j: tests/post_ref.py (numpy, device tie rule) and postprocess.refine_instances_device
(csrc/post.hip, which folds with % n_j).  With copies = 1 the entry is pbn_post_batch, byte for byte, on the cases of
tests/post_batch_cases.py.  Everything compared is integer work, an fp32 quotient of exact integers or a copied score: every
comparison is bit-equality."""
import types

import numpy as np
import pytest
import torch

import post_batch_cases as B
import post_tta_cases as C
from pbnet_amd import _native as N
from pbnet_amd import postprocess as PP

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAMES = [c["name"] for c in C.cases()]


def cfg_of(c):
    return types.SimpleNamespace(TEST_SCORE_THRESH=c["score_t"], TEST_NPOINT_THRESH=c["npoint_t"], TEST_NMS_THRESH=c["nms_t"])


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def merged_ids(c):
    """(ids int64[N folded] on the device or None, sp_starts): what serving.merge_superpoints builds from per-scene ids."""
    sp_starts = PP.superpoint_starts(c["point_starts"], [s is not None for s in c["sups"]], c["n_sp"])
    if sp_starts[-1] == 0:
        return None, sp_starts
    return dev(np.concatenate([np.zeros(n, np.int64) if s is None else s for s, n in zip(c["sups"], c["sizes"])])), sp_starts


def run_tta(c, ws=None, copies=None):
    sup, sp_starts = merged_ids(c)
    return PP.refine_tta_merged_device(dev(c["pred_sem"]), (dev(c["pidx"]), dev(c["off"])), dev(c["clt"]), c["point_starts"], sp_starts,
                                       sup, cfg_of(c), copies=c["copies"] if copies is None else copies, workspace=ws)


def assert_equal(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want), what


def check_scene(c, rb, scalars, j, want):
    """Scene j of the batched result against post_ref's dict: the outputs, then the internal lists under post_ref's names."""
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
    p = rb.n_prop
    if p:
        n_rows, n_pick = int(rb.table("n_rows")[j]), int(rb.table("n_pick")[j])
        mine = C.scene_inputs(c, j)["merged_proposals"]
        assert_equal(rb.table("counts")[:p].cpu().numpy()[mine], want["pointnum"], what + "folded sizes")
        assert_equal(rb.table("rows")[:b * p].view(b, p)[j, :n_rows].cpu().numpy(), mine[want["rows"]].astype(np.int32), what + "rows")
        assert_equal(rb.table("pick_rows")[:b * p].view(b, p)[j, :n_pick].cpu().numpy(), mine[want["pick_rows"]].astype(np.int32),
                     what + "pick_rows")
        lo, hi = c["point_starts"][j], c["point_starts"][j + 1]
        assert_equal(rb.table("seg")[lo:hi].cpu().numpy(), want["seg"].astype(np.int32), what + "seg")
    assert not rb.scores[j, k:].any() and bool((rb.semantic_id[j, k:] == -1).all()) and not rb.npoints[j, k:].any()


def device_form_per_scene(c, j):
    """The single-scene device form on scene j's own slice: (clusters, scores, semantic_id) as numpy."""
    i = C.scene_inputs(c, j)
    res = PP.refine_instances_device(dev(i["pred_sem"]), (dev(i["pidx"]), dev(i["off"])), dev(i["clt"]), i["point_num"], dev(i["sp"]),
                                     cfg_of(c), n_superpoints=i["n_sp"])
    return tuple(t.cpu().numpy() for t in res.sliced())


@pytest.mark.parametrize("name", NAMES)
def test_every_scene_equals_both_yardsticks(name):
    c = C.case(name)
    rb = run_tta(c)
    scalars = rb.scalars.tolist()
    b = len(c["sizes"])
    assert rb.point_instance.dtype == torch.int32 and rb.point_instance.shape == (c["point_starts"][-1],)        # folded points
    assert rb.scores.shape == rb.semantic_id.shape == rb.npoints.shape == (b, rb.n_prop) and len(scalars) == 2 * b
    for j, want in enumerate(C.reference(name)):
        if j == c["error_scene"]:
            assert scalars[b + j] == PP.STATUS_SUPERPOINT_RANGE
            with pytest.raises(ValueError):
                rb.scene(j, scalars)
            continue
        assert scalars[b + j] == 0
        check_scene(c, rb, scalars, j, want)
        clusters, scores, sem = device_form_per_scene(c, j)
        assert_equal(rb.dense(j, scalars).cpu().numpy(), clusters, "%s scene %d: clusters of the device form" % (name, j))
        inst = rb.scene(j, scalars)
        assert_equal(inst["scores"].cpu().numpy(), scores, "scores of the device form")
        assert_equal(inst["semantic_id"].cpu().numpy(), sem, "semantic_id of the device form")
        assert_equal(inst["npoints"].cpu().numpy(), clusters.sum(1).astype(np.int32), "npoints of the device form")


@pytest.mark.parametrize("name", [c["name"] for c in B.cases()])
def test_one_copy_is_the_batched_entry_byte_for_byte(name):
    """pbn_post_batch_tta with copies = 1 on the cases of tests/post_batch_cases.py: every output and every workspace byte."""
    c = B.case(name)
    sups = [None if s is None else dev(s) for s in c["sups"]]
    n_sp = None if all(v is None for v in c["n_sp"]) else c["n_sp"]
    want = PP.refine_batch_device(dev(c["pred_sem"]), (dev(c["pidx"]), dev(c["off"])), dev(c["clt"]), c["point_starts"], sups,
                                  cfg_of(c), n_superpoints=n_sp)
    got = run_tta(c, copies=1)
    assert got.sp_starts == want.sp_starts and got.workspace.nbytes == want.workspace.nbytes
    for key in ("point_instance", "scores", "semantic_id", "npoints", "scalars", "buffer"):
        assert torch.equal(getattr(got.workspace, key), getattr(want.workspace, key)), "%s: %s" % (name, key)


def test_one_scene_of_three_copies_is_the_single_scene_device_form():
    c = C.case("t1")
    i = C.scene_inputs(c, 0)
    assert len(c["sizes"]) == 1 and c["copies"] == 3 and np.array_equal(i["pidx"], c["pidx"])       # the slice is the whole input
    res = PP.refine_instances_device(dev(c["pred_sem"]), (dev(c["pidx"]), dev(c["off"])), dev(c["clt"]), 3 * c["sizes"][0],
                                     dev(c["sups"][0]), cfg_of(c), n_superpoints=c["n_sp"][0])
    n_rows, n_pick, n_keep, status = res.scalars.tolist()
    clusters, scores, sem = res.sliced()
    rb = run_tta(c)
    scalars = rb.scalars.tolist()
    assert scalars == [n_keep, status] and status == 0 and n_keep >= 2
    assert torch.equal(rb.dense(0, scalars), clusters) and torch.equal(rb.scores[0, :n_keep], scores)
    assert torch.equal(rb.semantic_id[0, :n_keep], sem) and torch.equal(rb.npoints[0, :n_keep], clusters.sum(1).to(torch.int32))
    assert int(rb.table("n_rows")[0]) == n_rows and int(rb.table("n_pick")[0]) == n_pick
    assert torch.equal(rb.table("pick_rows")[:n_pick], res.pick_rows[:n_pick]) and torch.equal(rb.table("rows")[:n_rows], res.rows[:n_rows])
    assert torch.equal(rb.table("counts")[:rb.n_prop], res.pointnum)
    assert torch.equal(rb.table("seg")[:c["sizes"][0]].long(), res.seg) and torch.equal(rb.table("seg_refined")[:c["sizes"][0]].long(), res.seg_refined)


@pytest.mark.parametrize("name", ["t2", "many"])
def test_a_second_call_gives_the_same_bytes(name):
    c = C.case(name)
    rb = run_tta(c)
    ws = rb.workspace
    outs = lambda: [t.clone() for t in (ws.point_instance, ws.scores, ws.semantic_id, ws.npoints, ws.scalars, ws.buffer)]
    first = outs()
    run_tta(c, ws)
    for a, b in zip(first, outs()):
        assert torch.equal(a, b)


def test_a_fitting_call_stops_nowhere_and_allocates_nothing():
    c = C.case("t2")
    cfg = cfg_of(c)
    sup, sp_starts = merged_ids(c)
    sem, pidx, off, clt = dev(c["pred_sem"]), dev(c["pidx"]), dev(c["off"]), dev(c["clt"])
    ws = PP.PostBatchWorkspace(clt.shape[0] + 5, c["point_starts"][-1] + 100, 2, sp_starts[-1] + 3, DEV)
    call = lambda: PP.refine_tta_merged_device(sem, (pidx, off), clt, c["point_starts"], sp_starts, sup, cfg, copies=3, workspace=ws)
    call()
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    torch.cuda.set_sync_debug_mode("error")
    try:
        rb = call()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.cuda.memory_allocated() == before
    scalars = rb.scalars.tolist()
    for j, want in enumerate(C.reference("t2")):
        check_scene(c, rb, scalars, j, want)


def test_an_id_at_the_bound_fails_scene_1_and_leaves_scene_0_alone():
    c = C.case("sp_error")
    assert c["error_scene"] == 1
    outs = []
    for case in (C.without_error(c), c):
        rb = run_tta(case)
        sc = rb.scalars.tolist()
        outs.append((sc, rb.point_instance[:c["point_starts"][1]].clone(), rb.scores[0].clone(), rb.semantic_id[0].clone(),
                     rb.npoints[0].clone()))
    (sc0, *clean), (sc1, *err) = outs
    assert sc0[2:] == [0, 0] and sc1[2:] == [0, PP.STATUS_SUPERPOINT_RANGE] and sc0[0] == sc1[0] and sc0[0] > 0
    for a, b in zip(clean, err):
        assert torch.equal(a, b)


def test_zero_proposals():
    c = C.case("p0")
    rb = run_tta(c)
    assert rb.n_prop == 0 and rb.scalars.tolist() == [0, 0, 0, 0]
    assert rb.point_instance.shape == (103,) and bool((rb.point_instance == -100).all())
    for j in range(2):
        inst = rb.scene(j)
        assert inst["scores"].numel() == 0 and inst["point_instance"].shape == (c["sizes"][j],)


def test_capacity_and_argument_checks():
    lib = N.lib()
    c = C.case("t2")
    fake = N.c_vp(1 << 20)

    def call(table, n_merged, n_prop=10, ws_bytes=1 << 40):            # the pointers are never dereferenced: refused before any launch
        return lib.pbn_post_batch_tta(fake, 10, fake, 1, n_prop, fake, 0, fake, 1, n_merged, table, None, 0.3, 4, 0.3, fake, 20, fake,
                                      fake, fake, fake, fake, fake, ws_bytes, None)
    t = PP.tta_table([0, 70, 103], [0, 0, 0], 3)
    nine = N.TtaTable()                                                # tta_table refuses to build it
    nine.n_scenes, nine.copies = 3, 3
    for j, s in enumerate([0, 10, 20, 30]):
        nine.point_start[j] = s
    assert call(nine, 90) == N.PBN_ERR_ARG
    zero = PP.tta_table([0, 70, 103], [0, 0, 0], 3)
    zero.copies = 0
    assert call(zero, 0) == N.PBN_ERR_ARG and call(zero, 103) == N.PBN_ERR_ARG
    assert call(t, 103) == N.PBN_ERR_ARG and call(t, 310) == N.PBN_ERR_ARG            # not copies * point_start[B]
    assert call(PP.tta_table([0, 70, 60], [0, 0, 0], 3), 180) == N.PBN_ERR_ARG
    assert call(t, 309, n_prop=lib.pbn_post_max_proposals() + 1) == N.PBN_ERR_UNSUPPORTED
    assert call(t, 309, ws_bytes=64) == N.PBN_ERR_WORKSPACE
    # the Python entry: sizes that do not match, a workspace that does not fit
    sup, sp_starts = merged_ids(c)
    args = lambda sem: (sem, (dev(c["pidx"]), dev(c["off"])), dev(c["clt"]), c["point_starts"], sp_starts, sup, cfg_of(c))
    with pytest.raises(ValueError):
        PP.refine_tta_merged_device(*args(dev(c["pred_sem"][:103])), copies=3)                    # labels of one copy only
    with pytest.raises(ValueError):
        PP.refine_tta_merged_device(*args(dev(c["pred_sem"])), copies=3, workspace=PP.PostBatchWorkspace(2, 50, 1, 0, DEV))
    with pytest.raises(TypeError):
        PP.refine_tta_merged_device(*args(dev(c["pred_sem"]).float()), copies=3)
