"""CPU tier for the posed-depth-frames front end: the designed cases of tests/frames_cases.py against the two statements of
the contract (tests/frames_ref.py vectorised, tests/frames_mutants.py pixel by pixel), the kill matrix of the mutants, and
two checks that do not go through the restatement's own formula: ray-cast planes come back on their planes within a bound
derived here, and the edge test drops silhouette pixels and nothing else."""
import numpy as np
import pytest

import frames_cases as C
import frames_mutants as M
import frames_ref as R

NAMES = list(C.CASES)


def _ref(name):
    depth, pose, intr, colour, kw = C.arguments(C.CASES[name])
    return R.frames_ref(depth, pose, intr, colour, **kw)


@pytest.mark.parametrize("name", NAMES)
def test_both_statements_agree(name):
    assert M.same(M.decode(C.CASES[name]), _ref(name)), C.CASES[name]["why"]


def test_every_mutant_is_killed():
    small = [n for n in NAMES if n != "big"] + ["big"]
    refs = {}
    matrix = {}
    for mutant in M.MUTANTS:
        for name in small:
            if name not in refs:
                refs[name] = _ref(name)
            if not M.same(M.decode(C.CASES[name], mutant), refs[name]):
                matrix[mutant] = name
                break
    print("\n".join("%-28s killed by %s" % (m, matrix.get(m)) for m in M.MUTANTS))
    assert sorted(matrix) == sorted(M.MUTANTS), "survivors: %s" % sorted(set(M.MUTANTS) - set(matrix))


def test_designed_cases_have_their_properties():
    assert C.BLOCK_PIXELS == 1024
    for name, hw in (("block_minus_1", C.BLOCK_PIXELS - 1), ("block", C.BLOCK_PIXELS), ("block_plus_1", C.BLOCK_PIXELS + 1)):
        assert C.CASES[name]["depth"].shape[1] * C.CASES[name]["depth"].shape[2] == hw
    assert [C.CASES[n]["depth"].shape[2] for n in ("w63", "w64", "w65")] == [63, 64, 65]
    assert _ref("none_valid")["n"] == 0 and _ref("skip_every")["n"] == 0
    last = _ref("last_only")
    assert last["n"] == 1 and last["pixel"][0] == C.CASES["last_only"]["depth"].size - 1
    full = _ref("all_valid")
    assert full["n"] == C.CASES["all_valid"]["depth"].size
    for name, frame in (("skip_first", 0), ("skip_last", 3), ("skip_middle", 2)):
        fs = _ref(name)["frame_start"]
        counts = np.diff(fs)
        assert counts[frame] == 0 and all(counts[f] > 0 for f in range(4) if f != frame)
    assert np.diff(_ref("bottom_row")["frame_start"])[0] > 0
    assert _ref("max_cut")["n"] == 18 and _ref("max_inclusive")["n"] == 20
    mn = _ref("min_cut")
    assert 1 * 5 * 8 > mn["n"] > 0 and (2 * 8 + 3) in mn["pixel"] and (2 * 8 + 4) not in mn["pixel"]
    sp = _ref("f32_specials")
    assert not set(range(5)) & set(sp["pixel"].tolist())                       # NaN, inf, -0.0, negative, 0
    assert {24 + 18 + 3, 24 + 18 + 5} <= set(sp["pixel"].tolist()) and 24 + 18 + 2 not in sp["pixel"]
    far = _ref("far_translation")
    assert np.abs(far["xyz"]).max() > 9.0e3 and np.all(np.isfinite(far["xyz"]))
    over = _ref("overflow")
    assert np.diff(over["frame_start"]).tolist()[0] == 0 and over["n"] > 0
    for name, stride in (("stride2", 2), ("stride3", 3), ("stride_plain", 2)):
        d = C.CASES[name]["depth"]
        pix = _ref(name)["pixel"]
        u, v = pix % d.shape[2], pix // d.shape[2] % d.shape[1]
        assert d.shape[1] % stride and d.shape[2] % stride and pix.size
        assert np.all(u % stride == 0) and np.all(v % stride == 0)
    eb = _ref("edge_borders")
    kept = np.zeros(64, bool)
    kept[eb["pixel"]] = True
    kept = kept.reshape(8, 8)
    assert not (kept[0, 0] or kept[0, 7] or kept[7, 0] or kept[7, 7])                   # the corners jump
    assert not (kept[0, 4] or kept[7, 3] or kept[3, 0] or kept[4, 7])                   # and a pixel of every border
    assert kept[0, 2] and kept[7, 5] and kept[5, 0] and kept[2, 7] and kept[3, 3]       # smooth border pixels stay
    assert "rgb" not in _ref("no_colour") and "rgb" in _ref("shared_intr")
    assert not M.same(_ref("shared_intr"), _ref("per_frame_intr"))
    big = np.diff(_ref("big")["frame_start"])
    assert C.CASES["big"]["depth"].shape == (4, 96, 128) and np.all(big > 3 * C.BLOCK_PIXELS)


def test_host_centres_are_the_restatement():
    from pbnet_amd import frames
    for name in ("skip_middle", "skip_every", "overflow", "far_translation", "bottom_row"):
        pose = C.CASES[name]["pose"]
        got = frames.host_centres(np.ascontiguousarray(pose.reshape(-1, 16)))
        want = R.centres_ref(pose)
        assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()


# --------------------------------------------------------------------------------------------------------- geometry
ROOM_INTR = (60.0, 60.0, 31.5, 23.5)
H, W = 48, 64


@pytest.mark.parametrize("form", ["u16", "f32"])
@pytest.mark.parametrize("eye,target,plane", [((0.3, -0.2, 1.1), (0.5, 3.0, 0.9), (1, 3.0)),
                                              ((1.0, 1.0, 1.6), (2.0, 2.5, 0.0), (2, 0.0)),
                                              ((-1.0, 0.5, 1.2), (2.0, 0.8, 1.0), (0, 2.0))])
def test_ray_cast_planes_come_back_on_their_planes(form, eye, target, plane):
    """Independent of the restatement's formula: a plane x[axis] = offset rendered analytically and back-projected lies on
    that plane.  The bound is derived, not tuned: the stored depth is off by at most half a quantum q -- 1 / depth_scale
    for uint16, the float32 spacing at the largest depth for float32 -- which moves the point along its ray by at most
    (q / 2) * |ray| / z; the float32 store moves a coordinate by at most half the float32 spacing at the scene's extent,
    taken whole here to cover the float64 arithmetic in between (its error is 1e-9 of that spacing)."""
    scale = 1000.0
    pose = R.look_at(eye, target)
    img = R.render(pose, ROOM_INTR, H, W, planes=[(plane[0], plane[1], (200, 10, 10))], depth_scale=scale)
    out = R.frames_ref(img[form][None], pose[None], ROOM_INTR, depth_scale=scale)
    assert out["n"] > H * W // 2
    z = img["z"].reshape(-1)[out["pixel"]]
    quantum = 1.0 / scale if form == "u16" else float(np.spacing(np.float32(z.max())))
    extent = float(np.abs(out["xyz"]).max())
    bound = 0.5 * quantum * float(img["ray"].max()) + float(np.spacing(np.float32(extent)))
    dist = np.abs(out["xyz"][:, plane[0]].astype(np.float64) - plane[1])
    print("max distance %.3e, bound %.3e" % (dist.max(), bound))
    assert dist.max() <= bound


def test_edge_drops_silhouette_pixels_and_nothing_else():
    """A box in front of a wall, both facing the camera, the box centred on the optical axis so that no side face is seen.
    Every pixel the edge test drops has a 4-neighbour on the other surface, which is also the cap: at most the pixels
    adjacent to the silhouette are dropped.  Both sides of the silhouette lose pixels."""
    pose = R.look_at((0.0, 0.0, 1.0), (0.0, 3.0, 1.0))
    img = R.render(pose, ROOM_INTR, H, W, planes=[(1, 3.0, (90, 90, 90))], box=((-0.4, 1.8, 0.6), (0.4, 2.2, 1.4), (10, 200, 10)))
    surface = img["surface"]
    assert set(np.unique(surface).tolist()) == {0, 1}
    plain = R.frames_ref(img["u16"][None], pose[None], ROOM_INTR)
    edged = R.frames_ref(img["u16"][None], pose[None], ROOM_INTR, edge=0.1)
    assert plain["n"] == H * W
    dropped = np.ones(H * W, bool)
    dropped[edged["pixel"]] = False
    dropped = dropped.reshape(H, W)
    adjacent = np.zeros((H, W), bool)
    adjacent[:, 1:] |= surface[:, 1:] != surface[:, :-1]
    adjacent[:, :-1] |= surface[:, :-1] != surface[:, 1:]
    adjacent[1:, :] |= surface[1:, :] != surface[:-1, :]
    adjacent[:-1, :] |= surface[:-1, :] != surface[1:, :]
    assert dropped.sum() > 0 and not np.any(dropped & ~adjacent)
    assert dropped.sum() <= adjacent.sum()
    assert np.any(dropped & (surface == 0)) and np.any(dropped & (surface == 1))
