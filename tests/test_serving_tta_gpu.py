"""GPU tier: the serving front with the TTA fold (`SceneServer(refine=cfg, tta=3)`, pbnet_amd/serving.py).  Two units of different
sizes -- each the three rotated copies of one synthetic scene, as `synth.make_val_batch(copies=3)` builds them -- are served in ONE
merged forward of six batch elements (paused server, both queued, one worker) and compared per unit with the evaluation unit run
alone: the unit's own `model(..., n_batch=3)` followed by `refine_instances_device(...).sliced()`.

The rule is the one tests/test_serving_refine_gpu.py and tests/test_batched_gpu.py use for a merged forward against single ones:
integers exact, scores within 1e-4.  A merged forward may move a score by that much, so an exact comparison of the integers needs
every decision that reads a score to come out the same way; the size and IoU thresholds compare integers and quotients of integers,
which the merge does not move.  The test ASSERTS this instead of tolerating a mismatch:
  * the score threshold lies in a wide gap of the units' own scores, further than 1e-4 from every one of them (a score
    moved by at most 1e-4 then stays on its side);
  * the walk order of the NMS cannot be given that margin: the three copies of one object score within 1e-4 of each other by
    construction (that is what test-time augmentation feeds the NMS), whatever the seed.  So the merged forward is also run
    directly, its scores are asserted to lie within 1e-4 of the own forwards' (the rule above), and the walk order of every
    unit's survivors -- score descending, lower index first -- is asserted to be the same under both sets of scores."""
import types

import numpy as np
import pytest
import torch

from pbnet_amd import postprocess as PP
from pbnet_amd import synth
from pbnet_amd.config import get_config
from pbnet_amd.network.PBNet import PBNet
from pbnet_amd.serving import SceneServer, merge_tta_units

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
UNITS = ((41, (1.6, 1.3, 1.2), 4), (42, (1.1, 1.0, 1.0), 5))            # seed, room, boxes
TOL = 1e-4                  # tests/test_batched_gpu.py: a merged forward moves a score by at most this
MARGIN = TOL                # a score moved by at most TOL cannot cross a threshold that is further than TOL away


def _cells(xyz, size=0.1):
    """Stand-in superpoints: the ids of the 10 cm cells the points lie in (scene-local, dense from 0)."""
    ids = torch.unique(torch.floor(xyz / size).long(), dim=0, return_inverse=True)[1]
    return ids.contiguous(), int(ids.max().item()) + 1


def _serve(model, units, refine, max_batch=None):
    server = SceneServer(model, max_batch=max_batch, forwards_in_flight=1, refine=refine, tta=3, paused=True)
    futs = [server.submit(u, t) for u, t in units]
    server.start()
    out = []
    for f in futs:
        try:
            out.append(f.result(timeout=300))
        except ValueError as e:
            out.append(e)
    server.close()
    return out, server.forwards


def _own_forward(model, unit, teacher, n_batch=3):
    with torch.no_grad():
        ret = model(unit["feat_voxel"], unit["xyz_voxel"], unit["xyz_original"], unit["v2p_index"], None, 1, "test", teacher=teacher,
                    n_batch=n_batch)
    torch.cuda.synchronize()
    return ret


def _evaluation_unit(unit, ret, thr):
    """The reference's unit on the unit's own forward: (clusters, scores, semantic_id, n_pick, n_rows)."""
    n3 = int(unit["xyz_original"].shape[0])
    res = PP.refine_instances_device(ret["sem_pred_p"], ret["proposals"], ret["clt_scores"], n3, unit["sup"], thr,
                                     n_superpoints=unit["n_superpoints"])
    n_rows, n_pick, n_keep, status = res.scalars.tolist()
    assert status == 0
    clusters, scores, sem = res.sliced()
    return clusters.clone(), scores.clone(), sem.clone(), n_pick, n_rows, res.pointnum.clone()


@pytest.fixture(scope="module")
def served():
    cfg = get_config(test=True)
    torch.manual_seed(22)
    model = PBNet(cfg).to(DEV).eval()
    units = []
    for seed, room, boxes in UNITS:
        b, t, _ = synth.make_val_batch(seed=seed, copies=3, room=room, n_boxes=boxes, pitch=0.03, classes=(17, 10, 5))
        u = {k: torch.from_numpy(v).to(DEV) for k, v in b.items() if k != "ins"}
        n = int(u["xyz_original"].shape[0]) // 3
        u["sup"], u["n_superpoints"] = _cells(u["xyz_original"][:n])                 # the scene's points: copy 0
        units.append((u, {k: torch.from_numpy(v).to(DEV) for k, v in t.items()}))
    assert len({int(u["xyz_original"].shape[0]) for u, _ in units}) == 2
    own = [_own_forward(model, u, t) for u, t in units]
    # thresholds from what the forwards gave, so that some proposals survive and some do not: the score threshold in the middle of
    # the widest gap of the scores up to the lower of the units' best scores, the size threshold at the lower quartile of the sizes
    scores = torch.sort(torch.cat([r["clt_scores"].float().view(-1) for r in own]))[0]
    sizes = torch.cat([(r["proposals"][1][1:] - r["proposals"][1][:-1]).float() for r in own])
    assert scores.numel() >= 8
    print("own scores per unit: %s" % [[round(float(v), 5) for v in torch.sort(r["clt_scores"].float().view(-1))[0]] for r in own])
    lowest_best = min(float(r["clt_scores"].float().max()) for r in own)           # every unit keeps a score above the threshold
    below = scores[scores <= lowest_best]
    assert below.numel() >= 2
    at = int(torch.argmax(below[1:] - below[:-1]))
    thr = types.SimpleNamespace(TEST_SCORE_THRESH=float((below[at] + below[at + 1]) / 2), TEST_NPOINT_THRESH=int(torch.quantile(sizes, 0.25)),
                                TEST_NMS_THRESH=0.1)
    return model, units, own, thr, _merged_scores(model, units)


def _merged_scores(model, units):
    """The scores of the two-unit merged forward per unit, in the merged order (which is each unit's own order)."""
    batch, starts, _ = merge_tta_units([u for u, _ in units], 3, [t for _, t in units])
    ret = _own_forward(model, batch, batch["teacher"], n_batch=6)
    idx, off = ret["proposals"][0], ret["proposals"][1].long()
    unit_of = torch.searchsorted(3 * torch.tensor(starts, device=DEV), idx[off[:-1], 1], right=True) - 1
    return [ret["clt_scores"].float().view(-1)[unit_of == j] for j in range(len(units))]


def _walk_order(s):
    """Survivor positions in the NMS walk: score descending, among equal scores the lower position first."""
    s = s.cpu().numpy()
    return np.lexsort((np.arange(s.shape[0]), -s.astype(np.float64)))


def _assert_no_decision_flips(own, merged, want, thr):
    for r, m, w in zip(own, merged, want):
        s = r["clt_scores"].float().view(-1)
        assert m.shape == s.shape
        gap, moved = float((s - np.float32(thr.TEST_SCORE_THRESH)).abs().min()), float((m - s).abs().max())
        live = (s > np.float32(thr.TEST_SCORE_THRESH)) & (w[5] > thr.TEST_NPOINT_THRESH)
        print("scores to the threshold >= %.2e, moved by the merge <= %.2e, %d survivors" % (gap, moved, int(live.sum())))
        assert gap > MARGIN and moved <= TOL and int(live.sum()) == w[4]
        assert np.array_equal(_walk_order(s[live]), _walk_order(m[live]))


def _assert_instances(got, ret, want, n):
    clusters, scores, sem = want[:3]
    inst = got["instances"]
    k = int(clusters.shape[0])
    pi = inst["point_instance"]
    assert torch.equal(got["sem_pred_p"], ret["sem_pred_p"]) and got["sem_pred_p"].shape == (3 * n,)
    assert pi.dtype == torch.int32 and pi.shape == (n,) and inst["scores"].shape == (k,)
    dense = (pi[None, :] == torch.arange(k, dtype=torch.int32, device=pi.device)[:, None]).to(torch.int32)
    assert torch.equal(dense, clusters) and bool(((pi == -100) | ((pi >= 0) & (pi < k))).all())
    assert torch.equal(inst["semantic_id"], sem) and torch.equal(inst["npoints"], clusters.sum(1).to(torch.int32))
    err = float((inst["scores"] - scores.to(inst["scores"].dtype)).abs().max()) if k else 0.0
    print("kept %d, scores max |diff| %.2e" % (k, err))
    assert err <= TOL


def test_two_units_in_one_forward_equal_their_own_evaluation_units(served):
    model, units, own, thr, merged = served
    want = [_evaluation_unit(u, r, thr) for (u, _), r in zip(units, own)]
    n_prop = sum(int(r["proposals"][1].shape[0]) - 1 for r in own)
    kept, picked = [int(w[0].shape[0]) for w in want], sum(w[3] for w in want)
    print("proposals %d, picked %d, kept per unit %s" % (n_prop, picked, kept))
    assert min(kept) >= 1 and max(kept) >= 2 and picked < n_prop
    _assert_no_decision_flips(own, merged, want, thr)
    got, forwards = _serve(model, units, thr)
    assert forwards == 1
    for (u, _), r, g, w in zip(units, own, got, want):
        _assert_instances(g, r, w, int(u["xyz_original"].shape[0]) // 3)


def test_a_lone_unit_is_served_alone(served):
    model, units, own, thr, merged = served
    got, forwards = _serve(model, units[1:], thr)
    assert forwards == 1 and len(got) == 1
    _assert_instances(got[0], own[1], _evaluation_unit(units[1][0], own[1], thr), int(units[1][0]["xyz_original"].shape[0]) // 3)
    # max_batch = 1: two queued units, two forwards
    got, forwards = _serve(model, units, thr, max_batch=1)
    assert forwards == 2
    for (u, _), r, g in zip(units, own, got):
        _assert_instances(g, r, _evaluation_unit(u, r, thr), int(u["xyz_original"].shape[0]) // 3)


def test_a_unit_with_an_id_at_its_bound_fails_alone(served):
    model, units, own, thr, merged = served
    bad = dict(units[1][0])
    bad["sup"] = bad["sup"].clone()
    bad["sup"][0] = bad["n_superpoints"]
    got, forwards = _serve(model, [units[0], (bad, units[1][1])], thr)
    assert forwards == 1 and isinstance(got[1], ValueError)
    _assert_instances(got[0], own[0], _evaluation_unit(units[0][0], own[0], thr), int(units[0][0]["xyz_original"].shape[0]) // 3)
