"""GPU tier: the serving front with refine (pbnet_amd/serving.py): four synthetic scenes of different sizes served twice through
the SAME merged forward (paused server, all four queued, one worker, max_batch = 4) -- once raw, followed by the parent's
composition (`refine_instances_device` per scene on the split results), once with refine=cfg -- agree exactly per scene; and a
scene whose superpoint ids overflow its bound fails alone."""
import types

import numpy as np
import pytest
import torch

from pbnet_amd import postprocess as PP
from pbnet_amd import synth
from pbnet_amd.config import get_config
from pbnet_amd.network.PBNet import PBNet
from pbnet_amd.serving import SceneServer

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOMS = ((1.6, 1.3, 1.2), (1.1, 1.0, 1.0), (2.0, 1.5, 1.2), (1.4, 1.7, 0.9))


def _cells(xyz, size=0.1):
    """Stand-in superpoints: the ids of the 10 cm cells the points lie in (scene-local, dense from 0)."""
    ids = torch.unique(torch.floor(xyz / size).long(), dim=0, return_inverse=True)[1]
    return ids.contiguous(), int(ids.max().item()) + 1


def _serve(model, scenes, refine, max_batch=4):
    server = SceneServer(model, max_batch=max_batch, forwards_in_flight=1, refine=refine, paused=True)
    futs = [server.submit(s, t) for s, t in scenes]
    server.start()
    out = []
    for f in futs:
        try:
            out.append(f.result(timeout=300))
        except ValueError as e:
            out.append(e)
    server.close()
    return out, server.forwards


@pytest.fixture(scope="module")
def served():
    cfg = get_config(test=True)
    torch.manual_seed(22)
    model = PBNet(cfg).to(DEV).eval()
    scenes = []
    for s, room in enumerate(ROOMS):
        b, t, _ = synth.make_val_batch(seed=40 + s, copies=1, room=room, n_boxes=4 + s, pitch=0.03, classes=(17, 10, 5))
        bd = {k: torch.from_numpy(v).to(DEV) for k, v in b.items() if k != "ins"}
        bd["sup"], bd["n_superpoints"] = _cells(bd["xyz_original"])
        scenes.append((bd, {k: torch.from_numpy(v).to(DEV) for k, v in t.items()}))
    assert len({int(s["xyz_original"].shape[0]) for s, _ in scenes}) == 4
    raw, forwards = _serve(model, scenes, None)
    assert forwards == 1
    # thresholds from the scores and sizes the forward gave, so that some proposals survive and some do not
    scores = torch.cat([r["clt_scores"].float().view(-1) for r in raw])
    sizes = torch.cat([(r["proposals"][1][1:] - r["proposals"][1][:-1]).float() for r in raw])
    assert scores.numel() >= 8
    thr = types.SimpleNamespace(TEST_SCORE_THRESH=float(torch.quantile(scores, 0.25)), TEST_NPOINT_THRESH=int(torch.quantile(sizes, 0.25)),
                                TEST_NMS_THRESH=0.1)
    return model, scenes, raw, thr


def _composition(scene, r, thr):
    n = int(scene["xyz_original"].shape[0])
    res = PP.refine_instances_device(r["sem_pred_p"], r["proposals"], r["clt_scores"], 3 * n, scene["sup"], thr,
                                     n_superpoints=scene["n_superpoints"])
    n_rows, n_pick, n_keep, status = res.scalars.tolist()
    assert status == 0
    clusters, scores, sem = res.sliced()
    return clusters.clone(), scores.clone(), sem.clone(), n_pick


def _assert_instances(inst, want, n):
    clusters, scores, sem, _ = want
    k = int(clusters.shape[0])
    pi = inst["point_instance"]
    assert pi.dtype == torch.int32 and pi.shape == (n,) and inst["scores"].shape == (k,)
    dense = (pi[None, :] == torch.arange(k, dtype=torch.int32, device=pi.device)[:, None]).to(torch.int32)
    assert torch.equal(dense, clusters) and bool(((pi == -100) | ((pi >= 0) & (pi < k))).all())
    assert torch.equal(inst["scores"], scores.to(inst["scores"].dtype)) and torch.equal(inst["semantic_id"], sem)
    assert torch.equal(inst["npoints"], clusters.sum(1).to(torch.int32))


def test_refined_serving_equals_the_composition_per_scene(served):
    model, scenes, raw, thr = served
    want = [_composition(s, r, thr) for (s, _), r in zip(scenes, raw)]
    n_prop = sum(int(r["proposals"][1].shape[0]) - 1 for r in raw)
    kept, picked = [int(w[0].shape[0]) for w in want], sum(w[3] for w in want)
    print("proposals %d, picked %d, kept per scene %s" % (n_prop, picked, kept))
    assert max(kept) >= 2 and picked < n_prop
    got, forwards = _serve(model, scenes, thr)
    assert forwards == 1
    for (s, _), r, g, w in zip(scenes, raw, got, want):
        assert torch.equal(g["sem_pred_p"], r["sem_pred_p"])
        _assert_instances(g["instances"], w, int(s["xyz_original"].shape[0]))


def test_a_scene_with_an_id_at_its_bound_fails_alone(served):
    model, scenes, raw, thr = served
    bad = dict(scenes[1][0])
    bad["sup"] = bad["sup"].clone()
    bad["sup"][0] = bad["n_superpoints"]
    batch = [scenes[0], (bad, scenes[1][1]), scenes[2]]
    got, forwards = _serve(model, batch, thr)
    assert forwards == 1
    assert isinstance(got[1], ValueError)
    # the forward of three scenes gives each scene its own forward's proposals with scores within 1e-4 (tests/test_batched_gpu.py),
    # not the four-scene forward's bits: the batch-mates are checked against the composition on THIS forward's raw results
    raw3, _ = _serve(model, batch, None)
    for j in (0, 2):
        _assert_instances(got[j]["instances"], _composition(batch[j][0], raw3[j], thr), int(batch[j][0]["xyz_original"].shape[0]))
