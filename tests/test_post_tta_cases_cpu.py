"""CPU tier of the folding batched post-processing: (1) the synthetic cases of tests/post_tta_cases.py are not vacuous --
tests/post_ref.py alone, run per scene, shows every situation the GPU tier (tests/test_post_batch_tta_gpu.py) relies on; (2) the
host side: the table `tta_table` builds, `merge_tta_units` on CPU tensors, the argument checks of `SceneServer(tta=...)`."""
import numpy as np
import pytest
import torch

import post_batch_cases as B
import post_ref as R
import post_tta_cases as C


def _scenes():
    for c in C.cases():
        for j, r in enumerate(C.reference(c["name"])):
            yield c, j, r, C.scene_inputs(c, j)


def _copy_of(c, pts):
    """(scene, copy) of merged unfolded points."""
    k, starts = c["copies"], np.asarray(c["point_starts"])
    scene = np.searchsorted(k * starts, pts, side="right") - 1
    return scene, (pts - k * starts[scene]) // np.asarray(c["sizes"])[scene]


def _members(c, p):
    off = c["off"].astype(np.int64)
    return c["pidx"][off[p]:off[p + 1], 1]


def test_generator_covers_the_listed_shapes():
    sizes = [c["sizes"] for c in C.cases()]
    assert any(n % 32 for s in sizes for n in s) and any(33 in s for s in sizes)
    assert any(len(s) == 2 and s[0] != s[1] for s in sizes) and any(len(s) == 1 for s in sizes)
    assert any(c["clt"].shape[0] > 256 for c in C.cases())                       # the block scans take two trips
    assert C.case("p0")["off"].shape[0] == 1 and C.case("p0")["pidx"].shape[0] == 0
    for c in C.cases():
        assert len(c["sizes"]) * c["copies"] <= 8 and c["pred_sem"].shape[0] == c["copies"] * c["point_starts"][-1]
        scene = C.scene_of_proposals(c)
        assert (scene >= 0).all()
        if len(c["sizes"]) > 1 and scene.shape[0] > 4:
            assert (np.diff(scene) < 0).any(), "%s: the scenes' proposals are not interleaved" % c["name"]
    assert {c["copies"] for c in C.cases()} == {2, 3}
    # the class of an instance depends on reading pred_sem UNFOLDED: folded first members name other classes
    c = C.case("t2")
    i = C.scene_inputs(c, 0)
    first = i["pidx"][i["off"][:-1], 1]
    assert (i["pred_sem"][first] != i["pred_sem"][first % c["sizes"][0]]).any()


def test_fold_dependent_pair():
    """Two proposals from different copies of a scene: IoU 0 without the fold, above the NMS threshold with it, and the pick list
    of the scene is not the one an implementation without the fold computes."""
    hits = 0
    for c in C.cases():
        for a, b in c["planted"]["fold_pairs"]:
            (sa, ca), (sb, cb) = _copy_of(c, _members(c, a)), _copy_of(c, _members(c, b))
            assert len(set(sa) | set(sb)) == 1 and len(set(ca)) == len(set(cb)) == 1 and ca[0] != cb[0]
            j = int(sa[0])
            i, want, other = C.scene_inputs(c, j), C.reference(c["name"])[j], C.reference_without_fold(c["name"])[j]
            qa, qb = (int(np.nonzero(i["merged_proposals"] == p)[0][0]) for p in (a, b))
            n = c["sizes"][j]
            folded, unfolded = R.fold_masks(i["pidx"], i["clt"].shape[0], n), R.fold_masks(i["pidx"], i["clt"].shape[0], c["copies"] * n)
            iou = lambda m: R.mask_iou(m[[qa, qb]], m[[qa, qb]].sum(1).astype(np.int32))[0, 1]
            assert iou(unfolded) == 0 and iou(folded) > np.float32(c["nms_t"])
            assert qa in want["rows"] and qb in want["rows"]
            if not np.array_equal(want["pick_rows"], other["pick_rows"]):
                hits += 1
    assert hits >= 3


def test_cross_copy_proposal():
    n = 0
    for c in C.cases():
        for p in c["planted"]["cross_copy"]:
            scene, copy = _copy_of(c, _members(c, p))
            assert len(set(scene)) == 1 and len(set(copy)) == 2
            n += 1
    assert n >= 3


def test_foreign_member():
    n = 0
    for c in C.cases():
        for p in c["planted"]["foreign"]:
            scene, _ = _copy_of(c, _members(c, p))
            own = C.scene_of_proposals(c)[p]
            assert scene[0] == own and (scene != own).sum() == 1
            i = C.scene_inputs(c, int(own))
            q = int(np.nonzero(i["merged_proposals"] == p)[0][0])
            assert i["off"][q + 1] - i["off"][q] == scene.shape[0] - 1                 # dropped from the scene's slice
            n += 1
    assert n >= 3


def test_some_scene_loses_every_proposal_to_a_threshold():
    assert any(r["rows"].shape[0] == 0 and i["clt"].shape[0] > 0 for _, _, r, i in _scenes())


def test_some_cluster_vanishes_in_the_vote():
    assert any(r["keep"].shape[0] < r["pick"].shape[0] for _, _, r, _ in _scenes())


def test_some_pick_depends_on_the_tie_rule():
    hit = False
    for c, j, r, i in _scenes():
        s = i["clt"][r["rows"]]
        if np.unique(s).shape[0] == s.shape[0]:
            continue
        other = B.greedy_nms_other_tie_rule(r["cross_ious"], s, c["nms_t"])
        hit |= not np.array_equal(other, r["pick"])
    assert hit


def test_status_is_set_in_scene_1_of_the_error_case_alone():
    for c, j, r, _ in _scenes():
        want = R.STATUS_SUPERPOINT_RANGE if (c["error_scene"] is not None and j == c["error_scene"]) else 0
        assert r["status"] == want, (c["name"], j)
    c = C.case("sp_error")
    assert c["error_scene"] == 1 and (c["sups"][1] == c["n_sp"][1]).sum() == 1 and c["sups"][1].max() == c["n_sp"][1]
    assert c["sups"][0].max() < c["n_sp"][0] and C.reference("sp_error")[0]["keep"].shape[0] > 0


# ---- the host side ----------------------------------------------------------------------------------------------------------
def test_tta_table_limits():
    from pbnet_amd import postprocess as PP
    t = PP.tta_table([0, 70, 103], [0, 9, 9], 3)
    assert (t.n_scenes, t.copies) == (2, 3) and list(t.point_start)[:3] == [0, 70, 103] and list(t.sp_start)[:3] == [0, 9, 9]
    assert PP.tta_table(list(range(9)), [0] * 9, 1).n_scenes == 8 and PP.tta_table([0, 5], [0, 0], 8).copies == 8
    for starts, sp, copies in (([0, 1, 2, 3], [0, 0, 0, 0], 3),           # three scenes of three copies: nine batch elements
                               ([0, 5], [0, 0], 9), ([0, 5], [0, 0], 0), ([0, 5], [0, 0], -1),
                               ([0, 5, 9], [0, 0], 3), ([0], [0], 3)):
        with pytest.raises(ValueError):
            PP.tta_table(starts, sp, copies)


def _cpu_unit(n, n_vox, copies=3, sup=None, n_superpoints=None):
    """A unit on the CPU: copy c has n_vox + c voxels with batch column c."""
    vox = torch.cat([torch.cat([torch.full((n_vox + c, 1), c, dtype=torch.int32), torch.zeros(n_vox + c, 3, dtype=torch.int32)], 1)
                     for c in range(copies)])
    u = dict(xyz_voxel=vox, feat_voxel=torch.zeros(vox.shape[0], 3), xyz_original=torch.zeros(copies * n, 3),
             v2p_index=torch.arange(copies * n, dtype=torch.int64) % vox.shape[0])
    if sup is not None:
        u["sup"] = sup
    if n_superpoints is not None:
        u["n_superpoints"] = n_superpoints
    return u


def test_merge_tta_units_on_cpu_tensors():
    from pbnet_amd.serving import merge_tta_units
    sup0 = torch.arange(5, dtype=torch.int64) % 3
    units = [_cpu_unit(5, 2, sup=sup0, n_superpoints=3), _cpu_unit(7, 4)]
    before = units[1]["xyz_voxel"].clone()
    batch, starts, (sup, sp_starts) = merge_tta_units(units, copies=3)
    assert starts == [0, 5, 12] and sp_starts == [0, 3, 3] and batch["teacher"] is None
    v0, v1 = int(units[0]["xyz_voxel"].shape[0]), int(units[1]["xyz_voxel"].shape[0])
    assert batch["xyz_voxel"].shape[0] == batch["feat_voxel"].shape[0] == v0 + v1 and batch["xyz_original"].shape[0] == 36
    assert torch.equal(batch["xyz_voxel"][:v0, 0], units[0]["xyz_voxel"][:, 0])                    # unit 0: columns 0..2
    assert torch.equal(batch["xyz_voxel"][v0:, 0], before[:, 0] + 3)                               # unit 1: 3 + c
    assert sorted(set(batch["xyz_voxel"][:, 0].tolist())) == list(range(6))
    assert torch.equal(units[1]["xyz_voxel"], before)                                              # the caller's unit is not written
    assert torch.equal(batch["v2p_index"][:15], units[0]["v2p_index"]) and torch.equal(batch["v2p_index"][15:], units[1]["v2p_index"] + v0)
    assert sup.dtype == torch.int64 and sup.shape == (12,) and torch.equal(sup[:5], sup0)          # over folded points
    # a lone unit; no ids at all
    b1, s1, (none, sp1) = merge_tta_units([_cpu_unit(7, 4)], copies=3)
    assert s1 == [0, 7] and none is None and sp1 == [0, 0] and sorted(set(b1["xyz_voxel"][:, 0].tolist())) == [0, 1, 2]
    # teachers: all or none
    t = lambda n: dict(sem_score=torch.zeros(3 * n, 20), offset=torch.zeros(3 * n, 3))
    bt, _, _ = merge_tta_units(units, 3, [t(5), t(7)])
    assert bt["teacher"]["sem_score"].shape == (36, 20) and bt["teacher"]["offset"].shape == (36, 3)
    with pytest.raises(ValueError):
        merge_tta_units(units, 3, [t(5), None])
    bad = _cpu_unit(5, 2)
    bad["xyz_original"], bad["v2p_index"] = bad["xyz_original"][:14], bad["v2p_index"][:14]        # 14 points: no three copies
    with pytest.raises(ValueError):
        merge_tta_units([bad], copies=3)
    with pytest.raises(ValueError):
        merge_tta_units([_cpu_unit(5, 2, sup=torch.zeros(15, dtype=torch.int64))], copies=3)       # ids per unfolded point
    with pytest.raises(ValueError):
        merge_tta_units([_cpu_unit(5, 2, sup=torch.zeros(5, dtype=torch.int32))], copies=3)
    with pytest.raises(ValueError):
        merge_tta_units([_cpu_unit(5, 2)] * 3, copies=3)                                           # nine batch elements


def test_scene_server_tta_argument_checks():
    from pbnet_amd.serving import SceneServer
    cfg = object()
    with pytest.raises(ValueError):
        SceneServer(None, streams=[], tta=3)                                 # the fold exists only in the post-processing
    with pytest.raises(ValueError):
        SceneServer(None, streams=[], refine=cfg, tta=3, max_batch=3)        # nine batch elements
    with pytest.raises(ValueError):
        SceneServer(None, streams=[], refine=cfg, tta=0)
    with pytest.raises(ValueError):
        SceneServer(None, streams=[], refine=cfg, tta=9)
    s = SceneServer(None, streams=[], refine=cfg, tta=3, device="cpu")
    assert s.max_batch == 2 and s.tta == 3                                   # the default is clamped to MAX_SCENES // tta
    assert SceneServer(None, streams=[], refine=cfg, tta=3, max_batch=1, device="cpu").max_batch == 1
    assert SceneServer(None, streams=[], refine=cfg, tta=2, device="cpu").max_batch == 4
    plain = SceneServer(None, streams=[], device="cpu")
    assert plain.max_batch == 4 and plain.tta is None                        # the default path is as before
