"""CPU tier of the batched post-processing: (1) the synthetic cases of tests/post_batch_cases.py are not vacuous -- tests/post_ref.py
alone, run per scene, shows every situation the GPU tier (tests/test_post_batch_gpu.py) relies on; (2) the host side of the
serving front's refine path: the scene table `merge_scenes` builds, and the bound on max_batch."""
import os
import re

import numpy as np
import pytest
import torch

import post_batch_cases as C
import post_ref as R


def _scenes():
    for c in C.cases():
        for j, r in enumerate(C.reference(c["name"])):
            yield c, j, r, C.scene_inputs(c, j)


def test_generator_covers_the_listed_shapes():
    names = {c["name"]: c for c in C.cases()}
    assert names["b8"]["sizes"] == C.SIZES == (70, 33, 257, 1, 64, 100, 31, 96)
    assert sorted(len(c["sizes"]) for c in C.cases() if c["name"] in ("b1", "b2", "b3")) == [1, 2, 3]
    assert names["p0"]["off"].shape[0] == 1 and names["p0"]["pidx"].shape[0] == 0
    b8 = names["b8"]
    assert b8["sups"][5] is None and C.scene_inputs(b8, 4)["clt"].shape[0] == 0           # no superpoints; no proposals
    assert C.scene_inputs(b8, 6)["clt"].shape[0] > 0 and (C.scene_inputs(b8, 6)["clt"] <= b8["score_t"]).all()
    for c in C.cases():                                                                    # proposals of 3..30 members
        sizes = np.diff(c["off"].astype(np.int64))
        assert ((sizes >= 1) & (sizes <= 30)).all() and (sizes[sizes < 3] == 1).all()      # 1: the one-point scene's
        off = c["off"].astype(np.int64)
        first = c["pidx"][off[:-1], 1] if off.shape[0] > 1 else np.zeros(0, np.int64)
        scene = np.searchsorted(np.asarray(c["point_starts"]), first, side="right") - 1
        if len(c["sizes"]) > 1 and scene.shape[0] > 4:
            assert (np.diff(scene) < 0).any(), "%s: the scenes' proposals are not interleaved" % c["name"]
        for p in range(off.shape[0] - 1):                                                  # every proposal lies in one scene
            pts = c["pidx"][off[p]:off[p + 1], 1]
            assert c["point_starts"][scene[p]] <= pts.min() and pts.max() < c["point_starts"][scene[p] + 1]


def test_some_scene_loses_every_proposal_to_a_threshold():
    assert any(r["rows"].shape[0] == 0 and i["clt"].shape[0] > 0 for _, _, r, i in _scenes())


def test_some_scene_has_suppressed_survivors():
    assert any(r["pick"].shape[0] < r["rows"].shape[0] for _, _, r, _ in _scenes())


def test_some_cluster_vanishes_in_the_vote():
    assert any(r["keep"].shape[0] < r["pick"].shape[0] for _, _, r, _ in _scenes())


def test_some_pick_depends_on_the_tie_rule():
    hit = False
    for c, j, r, i in _scenes():
        s = i["clt"][r["rows"]]
        if np.unique(s).shape[0] == s.shape[0]:
            continue
        other = C.greedy_nms_other_tie_rule(r["cross_ious"], s, c["nms_t"])
        hit |= not np.array_equal(other, r["pick"])
    assert hit


def test_equal_scores_across_two_scenes():
    c = C.case("b8")
    s0, s2 = C.scene_inputs(c, 0)["clt"], C.scene_inputs(c, 2)["clt"]
    assert np.intersect1d(s0, s2).shape[0] >= 1


def test_the_stride_case_has_120_survivors_next_to_3():
    r = C.reference("stride")
    assert r[0]["rows"].shape[0] >= 120 and r[1]["rows"].shape[0] == 3
    assert r[0]["rows"].shape[0] ** 2 > 8192                     # more live pairs than the IoU grid has workgroups


def test_status_is_set_in_the_error_case_alone():
    for c, j, r, _ in _scenes():
        want = R.STATUS_SUPERPOINT_RANGE if (c["error_scene"] is not None and j == c["error_scene"]) else 0
        assert r["status"] == want, (c["name"], j)
    c = C.case("sp_error")
    e = c["error_scene"]
    assert 0 < e < len(c["sizes"]) - 1 and (c["sups"][e] == c["n_sp"][e]).sum() == 1 and c["sups"][e].max() == c["n_sp"][e]
    assert any(r["keep"].shape[0] > 0 for j, r in enumerate(C.reference("sp_error")) if j != e)


# ---- the host side of the serving front's refine path ---------------------------------------------------------------------------
def _cpu_scene(n, n_vox, sup=None, n_superpoints=None):
    s = dict(xyz_voxel=torch.zeros(n_vox, 4, dtype=torch.int32), feat_voxel=torch.zeros(n_vox, 3), xyz_original=torch.zeros(n, 3),
             v2p_index=torch.zeros(n, dtype=torch.int64))
    if sup is not None:
        s["sup"] = sup
    if n_superpoints is not None:
        s["n_superpoints"] = n_superpoints
    return s


def test_merge_scenes_builds_the_scene_table():
    from pbnet_amd.serving import merge_scenes
    from pbnet_amd import postprocess as PP
    sup0, sup2 = torch.arange(5, dtype=torch.int64) % 3, torch.arange(4, dtype=torch.int64)
    scenes = [_cpu_scene(5, 2, sup0, 3), _cpu_scene(7, 3), _cpu_scene(4, 1, sup2)]
    batch, teacher, starts, (sup, sp_starts) = merge_scenes(scenes, [None] * 3, with_superpoints=True)
    assert starts == [0, 5, 12, 16] and teacher is None and batch["xyz_original"].shape[0] == 16
    assert sp_starts == [0, 3, 3, 7]                            # the stated bound; no ids: an empty slice; default: the point count
    assert sup.dtype == torch.int64 and sup.shape == (16,)
    assert torch.equal(sup[:5], sup0) and torch.equal(sup[12:], sup2)          # ids stay scene-local
    t = PP.scene_table(starts, sp_starts)
    assert t.n_scenes == 3 and list(t.point_start)[:4] == starts and list(t.sp_start)[:4] == sp_starts
    # no scene brings ids: nothing to concatenate, every slice empty
    _, _, starts1, (none, sp1) = merge_scenes([_cpu_scene(5, 2)], [None], with_superpoints=True)
    assert none is None and sp1 == [0, 0] and starts1 == [0, 5]
    # the three-element form is untouched
    assert len(merge_scenes(scenes, [None] * 3)) == 3
    with pytest.raises(ValueError):
        merge_scenes([_cpu_scene(5, 2, torch.zeros(4, dtype=torch.int64))], [None], with_superpoints=True)
    with pytest.raises(ValueError):
        PP.scene_table(list(range(10)), list(range(10)))        # nine scenes


@pytest.mark.parametrize("max_batch", [0, 9, -1])
def test_max_batch_outside_the_shared_bound_is_refused(max_batch):
    from pbnet_amd import _native
    from pbnet_amd.serving import SceneServer
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "pbnet_hip.h")).read()
    assert _native.MAX_SCENES == int(re.search(r"#define PBN_MAX_SCENES (\d+)", header).group(1)) == 8      # stated once, shared
    with pytest.raises(ValueError):
        SceneServer(None, max_batch=max_batch, streams=[])
