"""GPU tier: the AP association without a host stop (csrc/apassoc.hip through evaluate.AssociationLog) against the golden
vectors of the reference's tools/eval.py, against evaluate.assign_instances_for_scan on seeded scenes, and its gates, guards,
status bits, log overflow, ground-truth encoding, absence of synchronisation / allocation and determinism.  Integers bit-exact."""
import glob
import os

import numpy as np
import pytest
import torch

import ap_record_ref as R
import test_ap_record_cpu as C
from pbnet_amd import evaluate as E

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
HERE = os.path.dirname(os.path.abspath(__file__))
CASES = sorted(glob.glob(os.path.join(HERE, "golden", "eval_E*.npz")))
GUARD, PAD = 0x5a5a5a5a, 16


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t if dtype is None else t.to(dtype)


def guarded_log(p_cap, n_pts, **kw):
    """An AssociationLog whose inter / uid / gt_index / log buffers sit between guard words; returns (log, check)."""
    al = E.AssociationLog(p_cap, n_pts, device=DEV, **kw)
    beds = {}
    for name in ("inter", "uid", "gt_index", "log"):
        n = int(getattr(al, name).numel())
        bed = torch.full((n + 2 * PAD,), GUARD, dtype=torch.int32, device=DEV)
        bed[PAD:PAD + n] = 0
        beds[name] = bed
        setattr(al, name, bed[PAD:PAD + n])

    def check():
        for name, bed in beds.items():
            h = bed.cpu().numpy()
            assert (h[:PAD] == GUARD).all() and (h[-PAD:] == GUARD).all(), "guard words around %s were written" % name
    return al, check


def scene(seed, n_pts, n_inst=7, n_pred=6, top_id=None):
    """Seeded scene in the style of test_eval_gpu._big_scene at any size from one point up: instances are runs of points
    (scattered by a permutation for odd seeds), predictions are intervals with values 1..4 plus stray points."""
    rng = np.random.default_rng(seed)
    codes = np.array([0] + [[3, 4, 5, 7, 39, 1, 2][j % 7] * 1000 + j + 1 for j in range(n_inst)], np.int64)
    if top_id is not None:
        codes[-1] = top_id
    gt = codes[(np.arange(n_pts) * (n_inst + 1)) // n_pts]
    masks = np.zeros((n_pred, n_pts), np.int32)
    label = np.zeros(n_pred, np.int64)
    for p in range(n_pred):
        a = int(rng.integers(0, n_pts))
        b = min(n_pts, a + 1 + int(rng.integers(0, max(1, n_pts // 3))))
        masks[p, a:b] = int(rng.integers(1, 5))
        masks[p, rng.integers(0, n_pts, 5)] = 1
        label[p] = [3, 4, 5, 7, 39, 13][int(rng.integers(0, 6))]
    if seed % 2:
        perm = rng.permutation(n_pts)
        gt, masks = gt[perm], np.ascontiguousarray(masks[:, perm])
    return gt, dict(conf=rng.random(n_pred).astype(np.float32), label_id=label, mask=masks)


def append_scene(al, name, gt, pred, ids_dtype=torch.int64, n_keep=None, status=None):
    al.append(name, dev(pred["mask"]), dev(pred["conf"]), dev(pred["label_id"]), n_keep, status, dev(gt, ids_dtype))


def same_record(a, b):
    for field in E.SceneMatches.__slots__:
        x, y = getattr(a, field), getattr(b, field)
        assert (x == y) if isinstance(x, str) else np.array_equal(np.asarray(x), np.asarray(y)), field
    assert np.array_equal(np.asarray(a.pred_conf, np.float32).view(np.int32), np.asarray(b.pred_conf, np.float32).view(np.int32))


# ------------------------------------------------------------------------------------------------------------- goldens
@pytest.mark.parametrize("path", CASES, ids=[os.path.basename(p)[:-4] for p in CASES])
def test_goldens_through_a_capacity_with_garbage_rows(path):
    g = np.load(path)
    n = int(g["n_scenes"])
    names = ["scene%04d_00" % s for s in range(n)]
    p_max = max(int(g["s%d_label" % s].shape[0]) for s in range(n)) + 3
    al, check = guarded_log(p_max, max(int(g["s%d_gt" % s].shape[0]) for s in range(n)), log_words=1 << 16)
    for s, name in enumerate(names):
        mask, p = g["s%d_mask" % s].astype(np.int32), int(g["s%d_label" % s].shape[0])
        # three rows past n_keep: masks of ones, a score and a label id that would raise the label-range bit if they were read
        clusters = np.concatenate([mask, np.ones((3, mask.shape[1]), np.int32)])
        scores = np.concatenate([g["s%d_conf" % s], np.full(3, 9.0, np.float32)])
        labels = np.concatenate([g["s%d_label" % s], np.full(3, 1 << 40, np.int64)])
        al.append(name, dev(clusters), dev(scores), dev(labels), torch.tensor(p, dtype=torch.int32, device=DEV), None,
                  dev(g["s%d_gt" % s], torch.int32 if s % 2 else torch.int64))
    matches, dropped = al.collect()
    check()
    C.finish_epoch(matches, dropped, g, names)


# -------------------------------------------------------------------------------------------------- against the host path
@pytest.mark.parametrize("n_pts", [1, 63, 64, 65, 4095, 4096, 4097, 10000])
def test_equals_the_host_association(n_pts):
    gt, pred = scene(n_pts, n_pts)
    want = E.assign_instances_for_scan("s", pred, gt, device=DEV)
    al, check = guarded_log(6, n_pts, log_words=1 << 12)
    append_scene(al, "s", gt, pred, torch.int32 if n_pts % 2 else torch.int64)
    matches, dropped = al.collect()
    check()
    assert dropped == []
    same_record(matches["s"], want)


def test_u_cap_equal_to_the_id_count_and_the_top_id():
    id_cap = 40000
    gt, pred = scene(4, 5000, top_id=id_cap - 1)
    n_ids = int(np.unique(gt).shape[0])
    want = E.assign_instances_for_scan("s", pred, gt, device=DEV)
    assert (id_cap - 1) in want.gt_id
    al, check = guarded_log(6, 5000, u_cap=n_ids, id_cap=id_cap, log_words=1 << 12)
    append_scene(al, "s", gt, pred)
    matches, _ = al.collect()
    check()
    same_record(matches["s"], want)


def test_wide_table_takes_the_global_atomic_path():
    gt, pred = scene(5, 10000)
    want = E.assign_instances_for_scan("s", pred, gt, device=DEV)
    al, check = guarded_log(6, 10000, u_cap=9000, log_words=1 << 12)
    append_scene(al, "s", gt, pred)
    matches, _ = al.collect()
    check()
    same_record(matches["s"], want)


# ------------------------------------------------------------------------------------------------------ gates and guards
def test_n_keep_gates_the_rows():
    gt, pred = scene(6, 4097)
    want = E.assign_instances_for_scan("s", pred, gt, device=DEV)
    first4 = dict(conf=pred["conf"][:4], label_id=pred["label_id"][:4], mask=pred["mask"][:4])
    want4 = E.assign_instances_for_scan("four", first4, gt, device=DEV)
    al, check = guarded_log(6, 4097, log_words=1 << 12)
    scalar = lambda v: torch.tensor(v, dtype=torch.int32, device=DEV)                                 # noqa: E731
    append_scene(al, "none", gt, pred, n_keep=scalar(0))
    used_after_first = al.state[:4].tolist()
    append_scene(al, "four", gt, pred, n_keep=scalar(4))
    append_scene(al, "s", gt, pred, n_keep=scalar(1000))                   # above p_cap: clamped to the six rows
    append_scene(al, "negative", gt, pred, n_keep=scalar(-3))              # below zero: no rows
    matches, dropped = al.collect()
    check()
    assert used_after_first == [R.HEADER, R.HEADER, 1, 0]                  # header-only record
    assert dropped == ["none", "negative"] and list(matches) == ["four", "s"]
    same_record(matches["four"], want4)
    same_record(matches["s"], want)


def raises_from(al, kind, *needles):
    with pytest.raises(kind) as err:
        al.collect()
    for needle in needles:
        assert needle in str(err.value), (needle, str(err.value))


def test_status_bits_and_bounds():
    gt, pred = scene(8, 4097)
    for bad, u_cap, text in ((65536, 1024, "id_cap"), (-1, 1024, "negative"), (None, 5, "u_cap")):
        ids = gt.copy()
        if bad is not None:
            ids[7] = bad
        al, check = guarded_log(6, 4097, u_cap=u_cap, log_words=1 << 12)
        if u_cap == 1024:
            append_scene(al, "fine", gt, pred)
        append_scene(al, "bad_scene", ids, pred)
        raises_from(al, ValueError, "bad_scene", text)
        check()
    # a label id that does not fit 32 bits, and the post-processing's own status word, both end up in the record
    al, check = guarded_log(6, 4097, log_words=1 << 12)
    append_scene(al, "wide", gt, dict(pred, label_id=pred["label_id"] + (1 << 33)))
    raises_from(al, ValueError, "wide", "32 bits")
    al.reset()
    append_scene(al, "post", gt, pred, status=torch.tensor(1, dtype=torch.int32, device=DEV))
    raises_from(al, ValueError, "post", "superpoint")
    al.reset()
    append_scene(al, "clean", gt, pred)                                    # the status word does not leak into the next scene
    assert list(al.collect()[0]) == ["clean"]
    check()


def test_log_too_small_for_the_third_scene():
    scenes = [scene(10 + i, 4097) for i in range(3)]
    sizes = [R.HEADER + 2 * np.unique(gt).shape[0] + 2 * 6 + 6 * np.unique(gt).shape[0] for gt, _ in scenes]
    al, check = guarded_log(6, 4097, log_words=sum(sizes) - 1)
    for i, (gt, pred) in enumerate(scenes):
        append_scene(al, "s%d" % i, gt, pred)
    append_scene(al, "after", *scenes[0])                                  # sticky: nothing is written after the overflow
    assert al.state[:4].tolist() == [sizes[0] + sizes[1], sum(sizes) + sizes[0], 2, 1]
    raises_from(al, RuntimeError, str(sum(sizes) + sizes[0]), "overflow")
    check()
    assert not al.log[sizes[0] + sizes[1]:].any()
    al.reset()
    append_scene(al, "s0", *scenes[0])
    assert list(al.collect()[0]) == ["s0"]


# --------------------------------------------------------------------------------------------------- ground-truth encoding
@pytest.mark.parametrize("dtype", [torch.int32, torch.int64], ids=["i32", "i64"])
@pytest.mark.parametrize("n_pts", [1, 65, 4097])
def test_gt_encode_equals_the_host_form(n_pts, dtype):
    rng = np.random.default_rng(n_pts)
    n_inst = 1 if n_pts == 1 else 9
    ins = rng.integers(-1, n_inst, n_pts).astype(np.int64)
    ins[ins == 4] = -100                                       # instance 4 has no points: a gap; -100 and -1 both mean none
    sem = rng.integers(0, 20, n_pts).astype(np.int64)
    sem[rng.random(n_pts) < 0.2] = -100
    for i in (0, 2):                                           # instances whose lowest-index point carries -100
        at = np.nonzero(ins == i)[0]
        if at.shape[0]:
            sem[at[0]] = -100
    if n_pts == 1:
        ins[:], sem[:] = 0, -100
    clusters, one = torch.ones(1, n_pts, dtype=torch.int32, device=DEV), torch.ones(1, device=DEV)
    al, check = guarded_log(1, n_pts, log_words=1 << 12)
    for k, (s, i) in enumerate(((sem, ins), (sem, np.full(n_pts, -100, np.int64)))):
        al.append("e%d" % k, clusters, one, one.long(), None, None, (dev(s, dtype), dev(i, dtype)))
        want = E.encode_gt_ids(s, i)
        assert np.array_equal(al.ids[:n_pts].cpu().numpy(), want)
        assert k == 1 or want.any()
    matches, _ = al.collect()                                  # no status bit; the ids went on into the association
    check()
    want = E.assign_instances_for_scan("e0", dict(conf=np.ones(1, np.float32), label_id=np.ones(1, np.int64),
                                                  mask=np.ones((1, n_pts), np.int32)), E.encode_gt_ids(sem, ins), device=DEV)
    same_record(matches["e0"], want)


def test_gt_encode_reports_labels_it_cannot_place():
    n = 300
    clusters, one = torch.ones(1, n, dtype=torch.int32, device=DEV), torch.ones(1, device=DEV)
    sem, ins = np.zeros(n, np.int64), np.zeros(n, np.int64)
    for bad_sem, bad_ins, text in ((20, 0, "semantic label"), (-5, 0, "semantic label"), (0, 8, "n_inst_cap")):
        s, i = sem.copy(), ins.copy()
        s[0], i[5] = bad_sem, bad_ins
        al, check = guarded_log(1, n, log_words=1 << 12, n_inst_cap=8)
        al.append("bad_scene", clusters, one, one.long(), None, None, (dev(s), dev(i)))
        raises_from(al, ValueError, "bad_scene", text)
        check()


# ------------------------------------------------------------------------------------ append_refined: no stop, no allocation
def refined_by_hand(gt, pred, extra_rows=2):
    """A RefinedInstances over a PostWorkspace filled by hand: the views and scalars refine_instances_device would leave."""
    from pbnet_amd.postprocess import PostWorkspace, RefinedInstances
    p, n = pred["mask"].shape[0] + extra_rows, pred["mask"].shape[1]
    ws = PostWorkspace(p, n, 4, DEV)
    ws.clusters[:pred["mask"].size].copy_(dev(pred["mask"]).reshape(-1))
    ws.scores[:p - extra_rows].copy_(dev(pred["conf"]))
    ws.semantic_id[:p - extra_rows].copy_(dev(pred["label_id"]))
    ws.scalars.copy_(torch.tensor([p, p, p - extra_rows, 0], dtype=torch.int32))
    views = dict(clusters=ws.clusters[:p * n].view(p, n), scores=ws.scores[:p], semantic_id=ws.semantic_id[:p], pick=ws.pick[:p],
                 pick_rows=ws.pick_rows[:p], keep=ws.keep[:p], rows=ws.rows[:p], pointnum=ws.counts[:p],
                 cross_ious=ws.iou[:p * p].view(p, p), seg=ws.seg[:n], seg_refined=ws.seg_refined[:n])
    return RefinedInstances(ws, p, n, views)


def test_append_refined_neither_stops_nor_allocates():
    gt, pred = scene(12, 4097)
    refined, ids = refined_by_hand(gt, pred), dev(gt)
    al, check = guarded_log(refined.n_prop, refined.n_fold, log_words=1 << 12)
    al.append_refined("warm", refined, ids)
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    torch.cuda.set_sync_debug_mode("error")
    try:
        al.append_refined("s", refined, ids)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.cuda.memory_allocated() == before
    matches, dropped = al.collect()
    assert dropped == [] and list(matches) == ["warm", "s"]
    same_record(matches["s"], E.assign_instances_for_scan("s", pred, gt, device=DEV))
    check()


def test_two_epochs_give_byte_identical_logs():
    scenes = [scene(20 + i, 10000) for i in range(3)]
    logs = []
    for _ in range(2):
        al, check = guarded_log(6, 10000, log_words=1 << 13)
        for i, (gt, pred) in enumerate(scenes):
            append_scene(al, "s%d" % i, gt, pred)
        used = al.state[0].item()
        logs.append(al.log[:used].cpu().numpy().tobytes())
        check()
    assert len(logs[0]) > 3 * 4 * R.HEADER and logs[0] == logs[1]
