"""GPU tier of the scene summary (pbn_scene_summary, csrc/summary.hip) against the numpy restatement of its contract
(tests/scene_summary_ref.py) on the shared cases (tests/scene_summary_cases.py): integers and class_vote exactly, box and centroid
with np.array_equal on float32 (NaNs equal).  The kernels are called through the C ABI with synthetic point_instance / n_keep, so
both accumulator paths, the status bits and the table tails are reached without a forward.  Every output buffer lies between guard
elements, and is filled with a pattern first: what a call must write is seen to be written, and nothing else."""
import numpy as np
import pytest
import torch

import scene_summary_cases as C
import scene_summary_ref as R
from pbnet_amd import _native as N
from pbnet_amd import postprocess as PP
from pbnet_amd import stage_ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
GUARD, FILL = 16, 77


def _lds_instances(n_cls):
    return int(N.lib().pbn_scene_summary_lds_instances(n_cls))


CASES = None


def _cases():
    global CASES
    if CASES is None:
        CASES = C.cases(_lds_instances)
    return CASES


CASE_NAMES = [c["name"] for c in C.cases()]          # the names do not depend on the LDS bound (a stand-in here); the n_keep values do


class Guarded(object):
    """n elements of dtype between two guards, everything filled with FILL."""

    def __init__(self, n, dtype):
        self.n, self.whole = n, torch.full((n + 2 * GUARD,), FILL, dtype=dtype, device=DEV)
        self.view = self.whole[GUARD:GUARD + n]

    def ptr(self):
        return N.c_vp(self.view.data_ptr())

    def guards_intact(self):
        return bool((self.whole[:GUARD] == FILL).all()) and bool((self.whole[GUARD + self.n:] == FILL).all())

    def untouched(self):
        return bool((self.whole == FILL).all())


def _inputs(case):
    dt = DTYPES[case["dtype"]]
    rows, k = case["scores"].shape
    full = torch.full((rows, case["ld"]), 100.0, dtype=dt, device=DEV)          # the padding would win every argmax if it were read
    full[:, :k] = torch.from_numpy(case["scores"]).to(DEV).to(dt)
    b = len(case["n_keep"])
    return dict(score=full, widened=full[:, :k].float().cpu().numpy(),
                table=PP.tta_table(case["point_starts"], [0] * (b + 1), case["copies"]),
                point_instance=torch.from_numpy(case["point_instance"]).to(DEV),
                scalars=torch.tensor(list(case["n_keep"]) + [0] * b, dtype=torch.int32, device=DEV),
                xyz=None if case["xyz"] is None else torch.from_numpy(case["xyz"]).to(DEV).contiguous(),
                labels=torch.tensor(case["labels"], dtype=torch.int64, device=DEV))


def _outputs(case):
    b, p, n = len(case["n_keep"]), case["n_prop"], case["point_starts"][-1]
    nbytes = int(N.lib().pbn_scene_summary_workspace_bytes(p, case["n_cls"]))
    return dict(sem_fold=Guarded(n, torch.int32), class_vote=Guarded(b * p, torch.int64), class_points=Guarded(b * p, torch.int32),
                box=Guarded(b * p * 6, torch.float32), centroid=Guarded(b * p * 3, torch.float32), status=Guarded(b, torch.int32),
                workspace=torch.zeros(max(nbytes, 8), dtype=torch.uint8, device=DEV), nbytes=nbytes)


def _call(case, inp, out, **over):
    a = dict(ld=case["ld"], n_cls=case["n_cls"], n_merged=case["copies"] * case["point_starts"][-1], table=inp["table"],
             n_prop=case["n_prop"], nbytes=out["nbytes"], n_labels=len(case["labels"]))
    a.update(over)
    return N.lib().pbn_scene_summary(N.c_vp(inp["score"].data_ptr()), a["ld"], a["n_cls"], N.DT[inp["score"].dtype], a["n_merged"],
                                     a["table"], N.ptr(inp["point_instance"]), N.ptr(inp["scalars"]), a["n_prop"], N.ptr(inp["xyz"]),
                                     N.ptr(inp["labels"]), a["n_labels"], out["sem_fold"].ptr(), out["class_vote"].ptr(),
                                     out["class_points"].ptr(), out["box"].ptr(), out["centroid"].ptr(), out["status"].ptr(),
                                     N.ptr(out["workspace"]), a["nbytes"], N.current_stream())


def _host(out, case):
    b, p = len(case["n_keep"]), case["n_prop"]
    torch.cuda.synchronize()
    return dict(sem_fold=out["sem_fold"].view.cpu().numpy(), class_vote=out["class_vote"].view.cpu().numpy().reshape(b, p),
                class_points=out["class_points"].view.cpu().numpy().reshape(b, p),
                box=out["box"].view.cpu().numpy().reshape(b, p, 6), centroid=out["centroid"].view.cpu().numpy().reshape(b, p, 3),
                status=out["status"].view.cpu().numpy())


def _want(case, inp):
    return R.summarize(inp["widened"], case["point_starts"], case["copies"], case["point_instance"], case["n_keep"], case["n_prop"],
                       case["xyz"], case["labels"])


def _assert_equal(got, want, case):
    assert np.array_equal(got["sem_fold"], want["sem_fold"])
    assert np.array_equal(got["status"], want["status"]), (got["status"], want["status"])
    assert got["class_vote"].dtype == np.int64 and np.array_equal(got["class_vote"], want["class_vote"])
    assert np.array_equal(got["class_points"], want["class_points"])
    if case["xyz"] is None:
        assert (got["box"] == FILL).all() and (got["centroid"] == FILL).all()          # left untouched
    else:
        assert got["box"].dtype == np.float32 and np.array_equal(got["box"], want["box"], equal_nan=True)
        assert np.array_equal(got["centroid"], want["centroid"], equal_nan=True)


@pytest.mark.parametrize("index", range(len(CASE_NAMES)), ids=CASE_NAMES)
def test_case_equals_the_restatement(index):
    case = _cases()[index]
    inp, out = _inputs(case), _outputs(case)
    assert _call(case, inp, out) == N.PBN_OK
    got, want = _host(out, case), _want(case, inp)
    _assert_equal(got, want, case)
    for name in ("sem_fold", "class_vote", "class_points", "box", "centroid", "status"):
        assert out[name].guards_intact(), name
    # what the case is there to pin is really in it
    if case["name"] == "invalid coordinates":
        assert list(want["status"]) == [4, 4] and np.isnan(want["box"][1, :2]).all() and np.isnan(want["centroid"][1, :2]).all()
        assert np.isfinite(want["box"][0, :3]).all()
    if case["name"] == "point_instance out of range":
        assert list(want["status"]) == [8, 8, 0]
    if case["name"] == "class outside the label table":
        assert list(want["status"]) == [0, 2] and (want["class_vote"][1, :2] == -1).all() and (want["class_vote"][0, :2] == 8).all()
    if case["name"] == "equal vote counts":
        assert want["class_vote"][0, 0] == C.LABELS[2] and want["class_points"][0, 0] == 2
    if case["name"] == "equal folded sums":
        assert list(want["sem_fold"][:2]) == [0, 3]
    if case["name"] == "copy order":
        assert (want["sem_fold"] == 1).all()
    if case["name"] == "nan and inf scores":
        assert list(want["sem_fold"][:6]) == [0, 1, 2, 0, 0, 3]
    if case["name"] == "no proposals":
        assert got["class_vote"].size == 0 and got["sem_fold"].shape == (80,)
    if case["name"] == "every point in one instance":
        assert want["class_points"][0, 0] == np.bincount(want["sem_fold"]).max()


def test_both_accumulator_paths_are_in_the_cases():
    by_name = {c["name"]: c for c in _cases()}
    assert list(by_name) == CASE_NAMES
    for k in (20, C.MAX_CLASSES):
        edge = _lds_instances(k)
        assert edge >= 1, "no privatised path for %d classes: the L rows of the case list would be missing" % k
        assert by_name["n_keep=L n_cls=%d" % k]["n_keep"][1] == edge and by_name["n_keep=L+1 n_cls=%d" % k]["n_keep"][1] == edge + 1


def test_two_calls_give_the_same_bytes():
    case = [c for c in _cases() if c["name"] == "tta layout"][0]
    inp = _inputs(case)
    runs = []
    for _ in range(2):
        out = _outputs(case)
        assert _call(case, inp, out) == N.PBN_OK
        torch.cuda.synchronize()
        runs.append({k: out[k].whole.clone() for k in ("sem_fold", "class_vote", "class_points", "box", "centroid", "status")})
    for k in runs[0]:
        assert torch.equal(runs[0][k].view(torch.uint8), runs[1][k].view(torch.uint8)), k


def test_one_copy_equals_sem_argmax_table():
    """copies = 1, K = 20: sem_fold is pbn_sem_argmax_table's sem_pred on the same random scores, ties included."""
    rng = np.random.default_rng(9)
    for dt in (torch.float32, torch.bfloat16):
        scores = torch.from_numpy((rng.integers(-5, 6, size=(1500, 20)) / 4.0).astype(np.float32)).to(DEV).to(dt)
        top = torch.sort(scores.float(), 1)[0]
        assert bool((top[:, -1] == top[:, -2]).any())
        sem_pred = stage_ops.sem_argmax_table(scores, None, 1)[0]
        case = dict(n_keep=[0], n_prop=0, point_starts=[0, 1500], n_cls=20, ld=20, copies=1, labels=C.LABELS)
        inp = dict(score=scores, table=PP.tta_table([0, 1500], [0, 0], 1), point_instance=None, scalars=None, xyz=None,
                   labels=torch.tensor(C.LABELS, dtype=torch.int64, device=DEV))
        out = _outputs(case)
        assert _call(case, inp, out) == N.PBN_OK
        torch.cuda.synchronize()
        assert torch.equal(out["sem_fold"].view.long(), sem_pred)


def test_bad_calls_are_refused_before_any_launch():
    case = [c for c in _cases() if c["name"] == "tta layout"][0]
    inp, out = _inputs(case), _outputs(case)
    starts, b = case["point_starts"], len(case["n_keep"])

    def table(point_starts, copies=3):
        t = PP.tta_table(point_starts, [0] * len(point_starts), copies)
        return t

    shifted, descending = table([1] + starts[1:]), table([0, starts[2], starts[1]])
    no_scene = table(starts)
    no_scene.n_scenes = 0
    too_many = table(starts)
    too_many.copies = 5                                                  # 2 scenes x 5 copies > PBN_MAX_SCENES
    calls = [(dict(table=shifted), N.PBN_ERR_ARG), (dict(table=descending), N.PBN_ERR_ARG), (dict(table=no_scene), N.PBN_ERR_ARG),
             (dict(table=too_many, n_merged=5 * starts[-1]), N.PBN_ERR_ARG), (dict(n_merged=3 * starts[-1] + 1), N.PBN_ERR_ARG),
             (dict(n_cls=0), N.PBN_ERR_ARG), (dict(n_cls=C.MAX_CLASSES + 1, ld=C.MAX_CLASSES + 1), N.PBN_ERR_ARG),
             (dict(ld=case["n_cls"] - 1), N.PBN_ERR_ARG), (dict(n_prop=-1), N.PBN_ERR_ARG),
             (dict(nbytes=out["nbytes"] - 1), N.PBN_ERR_WORKSPACE), (dict(nbytes=0), N.PBN_ERR_WORKSPACE),
             (dict(n_prop=int(N.lib().pbn_post_max_proposals()) + 1), N.PBN_ERR_UNSUPPORTED)]
    for over, code in calls:
        assert _call(case, inp, out, **over) == code, over
    torch.cuda.synchronize()
    for name in ("sem_fold", "class_vote", "class_points", "box", "centroid", "status"):
        assert out[name].untouched(), name
    assert not bool(out["workspace"].any())
    lib = N.lib()
    assert lib.pbn_scene_summary_workspace_bytes(-1, 20) == 0 and lib.pbn_scene_summary_workspace_bytes(10, C.MAX_CLASSES + 1) == 0
    assert lib.pbn_scene_summary_workspace_bytes(4097, 20) == 0 and lib.pbn_scene_summary_workspace_bytes(0, 20) == 0
    assert lib.pbn_scene_summary_lds_instances(0) == 0 and lib.pbn_scene_summary_lds_instances(C.MAX_CLASSES) >= 1
    assert _call(case, inp, out) == N.PBN_OK                             # the same buffers are served by a good call
    _assert_equal(_host(out, case), _want(case, inp), case)


def test_python_entry_on_a_synthetic_refined_batch():
    """`summarize_merged_device` on a hand-made RefinedBatch: the views, the shared read-back and the error of a scene alone."""
    case = [c for c in _cases() if c["name"] == "invalid coordinates"][0]
    starts, p, b = case["point_starts"], case["n_prop"], 2
    ws = PP.PostBatchWorkspace(p, starts[-1], b, 0, DEV)
    rb = PP.RefinedBatch(ws, p, starts, [0] * (b + 1))
    rb.point_instance.copy_(torch.from_numpy(case["point_instance"]).to(DEV))
    rb.scalars.copy_(torch.tensor(list(case["n_keep"]) + [0] * b, dtype=torch.int32, device=DEV))
    scores = torch.from_numpy(case["scores"]).to(DEV)
    xyz = torch.from_numpy(case["xyz"]).to(DEV)
    xyz[80:, 0] = 0.0                                                   # scene 1 becomes clean, scene 0 keeps its NaN
    sm = PP.summarize_merged_device(scores, rb, starts, copies=1, xyz=xyz)
    scalars = sm.readback()
    assert len(scalars) == 3 * b and scalars[:b] == list(case["n_keep"]) and scalars[2 * b:] == [4, 0]
    with pytest.raises(ValueError, match="scene 0"):
        sm.scene(0, scalars)
    want = R.summarize(case["scores"], starts, 1, case["point_instance"], case["n_keep"], p, xyz.cpu().numpy(), C.LABELS)
    got = sm.scene(1)
    k = case["n_keep"][1]
    assert np.array_equal(got["sem_fold"].cpu().numpy(), want["sem_fold"][starts[1]:])
    assert np.array_equal(got["class_vote"].cpu().numpy(), want["class_vote"][1, :k])
    assert np.array_equal(got["class_points"].cpu().numpy(), want["class_points"][1, :k])
    assert np.array_equal(got["box"].cpu().numpy(), want["box"][1, :k], equal_nan=True)
    assert np.array_equal(got["centroid"].cpu().numpy(), want["centroid"][1, :k], equal_nan=True)
    grown = sm.workspace.grown_for(p + 1, starts[-1], b, 20)
    assert grown is not sm.workspace and grown.n_prop == p + 1 and sm.workspace.grown_for(p, 1, 1, 20) is sm.workspace
    no_xyz = PP.summarize_merged_device(scores, rb, starts, copies=1, workspace=grown).scene(1)
    assert no_xyz["box"] is None and no_xyz["centroid"] is None
    assert np.array_equal(no_xyz["class_vote"].cpu().numpy(), want["class_vote"][1, :k])
