"""CPU tier of the floor plane and upright frame: the numpy twin (tests/upright_ref.py) gives the stated winners on the
designed cases and recovers the room's up; its rotation is one; four mutants of the contract are each told apart by a
named case; and pbnet_amd.mesh's argument checks raise before the device or the library is touched."""
import numpy as np
import pytest
import torch

import upright_ref as U
from pbnet_amd import mesh

H = 1024


def _normal(name, n_hyp=H):
    return U.want(name, n_hyp)["plane"][:3]


# ---------------------------------------------------------------------------------------------------------- winners
@pytest.mark.parametrize("name", ["n0", "n1", "n2", "coincident", "collinear"])
def test_no_plane(name):
    xyz = U.cases()[name][0]
    w = U.want(name, H)
    assert w["info"].tolist() == [0] * 8
    assert np.array_equal(w["R"], np.eye(3).reshape(9)) and w["xyz"].tobytes() == xyz.tobytes()
    assert not w["floor"].any() and not w["height"].any() and not w["plane"].any() and not w["moments"].any()


def test_three_points_are_one_exact_plane():
    w = U.want("n3", H)
    assert w["info"][0] == 1 and w["info"][2] == 3 and w["info"][5] == 3
    assert np.abs(w["height"]).max() <= 1e-6 and w["floor"].all()


@pytest.mark.parametrize("n", [U.SUM_BLOCK - 1, U.SUM_BLOCK, U.SUM_BLOCK + 1, U.SCORE_CHUNK - 1, U.SCORE_CHUNK, U.SCORE_CHUNK + 1])
def test_slabs_find_their_plane(n):
    w = U.want("slab%d" % n, H)
    true_up = U._rot((1, 1, 0), 20) @ np.array([0.0, 0.0, 1.0])
    assert w["info"][0] == 1 and w["info"][2] >= (n - n // 5) * 0.9
    assert U.angle_to(w["plane"][:3], true_up) <= np.arctan(2 * 0.02 / 4.0)


def test_two_slabs():
    # without a hint floor and ceiling tie in everything; the lowest hypothesis decides, and it may be either
    w = U.want("two_slabs", H)
    planes, live, cin, _ = U.scored("two_slabs")
    top = cin[:H][live[:H]].max()
    assert w["info"][2] == top == 256 and w["info"][4] == 0
    assert w["info"][1] == min(h for h in range(H) if live[h] and cin[h] == top)
    assert abs(abs(w["plane"][2]) - 1.0) <= 1e-12
    up, down = U.want("two_slabs_up", H), U.want("two_slabs_down", H)
    assert np.array_equal(up["plane"], [0.0, 0.0, 1.0, 0.0]) and np.array_equal(up["R"], np.eye(3).reshape(9))
    assert np.array_equal(down["plane"], [0.0, 0.0, -1.0, 2.5])                       # the ceiling, seen from above it
    assert np.array_equal(down["R"], [1, 0, 0, 0, -1, 0, 0, 0, -1])                   # the 1 + c <= 0 branch
    assert np.array_equal(down["xyz"][:, 2], -U.cases()["two_slabs"][0][:, 2])


def test_big_wall():
    assert abs(_normal("big_wall")[0]) >= 0.999                                        # no hint: the wall, the larger plane
    assert _normal("big_wall_up")[2] >= 0.999 and U.want("big_wall_up", H)["info"][2] >= 400


def test_table():
    floor, table = U.want("table", H), U.want("table_any", H)
    assert floor["plane"][2] >= 0.999 and abs(floor["plane"][3]) <= 1e-9 and floor["info"][2] == 225
    assert table["plane"][2] >= 0.999 and abs(table["plane"][3] + 0.75) <= 1e-9 and table["info"][2] == 400
    assert table["info"][4] == 225                                                     # the floor beneath it


def test_tilt_limit():
    w = U.want("tilt_limit", H)
    tilt = np.rad2deg(U.angle_to(w["plane"][:3], U.UP))
    assert w["info"][0] == 1 and w["info"][2] == 300 and abs(tilt - (U.TILT_LIMIT - 0.1)) <= 0.01
    xyz, t, kw = U.cases()["tilt_limit"]
    wide = U.upright_ref(xyz, t, H, **dict(kw, max_tilt=U.TILT_LIMIT + 0.2))
    assert wide["info"][2] == 500


@pytest.mark.parametrize("name", ["room", "room_no_hint"])
def test_room_recovers_up(name):
    """Every floor point lies within +-t of the fitted plane across the extent L, so the plane leans at most
    arctan(2t / L) away from the true floor."""
    bound = np.arctan(2 * U.ROOM_T / U.ROOM_L)
    for n_hyp in (256, H):
        w = U.want(name, n_hyp)
        assert w["info"][0] == 1 and w["info"][2] >= 1600
        assert U.angle_to(w["plane"][:3], U.ROOM_UP) <= bound
        z = w["xyz"].astype(np.float64)[w["floor"]][:, 2]
        assert z.max() - z.min() <= 2 * U.ROOM_T + 1e-5                               # the floor is level afterwards


def test_smaller_h_is_a_prefix():
    xyz, t, kw = U.cases()["room"]
    direct = U.upright_ref(xyz, t, 65, **kw)
    for k, v in U.want("room", 65).items():
        assert np.asarray(v).tobytes() == np.asarray(direct[k]).tobytes(), k


# --------------------------------------------------------------------------------------------------------- rotation
def test_rotation_is_one():
    rng = np.random.default_rng(0)
    normals = [rng.normal(size=3) for _ in range(50)] + [[0, 0, 1], [0, 0, -1], [1, 0, 0], [0, -1, 0], [1e-9, 0, -1]]
    for v in normals:
        n = np.asarray(v, np.float64) / np.linalg.norm(v)
        R = U.rotation_ref(np.append(n, 0.0)).reshape(3, 3)
        if 1.0 + n[2] > 1e-6:                                # next to -z the formula divides by 1 + c: no 1e-12 there
            assert np.abs(R @ n - [0, 0, 1]).max() <= 1e-12
            assert np.abs(R @ R.T - np.eye(3)).max() <= 1e-12
            assert abs(np.linalg.det(R) - 1.0) <= 1e-12
    R = U.rotation_ref([0.0, 0.0, -1.0, 0.0]).reshape(3, 3)
    assert np.array_equal(R @ [0, 0, -1], [0, 0, 1]) and np.array_equal(R @ R.T, np.eye(3)) and np.linalg.det(R) == 1.0


# ---------------------------------------------------------------------------------------------------------- mutants
def _fused_s(plane, xyz):
    """s with the products folded into the sums (fma): each product is exact in float64, so one float64 sum rounded to
    float32 is the fused result up to a double rounding."""
    plane = np.asarray(plane, np.float32)
    x, y, z = (xyz[:, j].astype(np.float64) for j in range(3))
    a, b, c, d = (plane[..., j, None].astype(np.float64) if plane.ndim == 2 else np.float64(plane[j]) for j in range(4))
    s = (a * x).astype(np.float32)
    s = (b * y + s).astype(np.float32)
    s = (c * z + s).astype(np.float32)
    return (s + d.astype(np.float32) if plane.ndim == 2 else s + np.float32(d)).astype(np.float32)


def test_mutant_strict_inequality_is_told_apart_by_on_threshold():
    xyz, t, _ = U.cases()["on_threshold"]
    planes, live, cin, cab = U.scored("on_threshold")
    flat = np.array([[0, 0, 1, 0]], np.float32)
    want_in, _, _ = U.score_ref(xyz, flat, np.ones(1, bool), t)
    lt_in, _, _ = U.score_ref(xyz, flat, np.ones(1, bool), t, inside=np.less)
    assert want_in[0] == 256 + 4 * 8 and lt_in[0] == 256 + 2 * 8     # z = +-t and the float32 below each | only those below
    mut_in, mut_ab, _ = U.score_ref(xyz, planes, live, t, inside=np.less)
    n = xyz.shape[0]
    a = U.select_ref(planes[:H], live[:H], cin[:H], cab[:H], n, True, -1)
    b = U.select_ref(planes[:H], live[:H], mut_in[:H], mut_ab[:H], n, True, -1)
    assert (a["h"], a["in"]) != (b["h"], b["in"])                    # the device's info would differ too


def test_mutant_fused_s_is_told_apart_by_room():
    xyz, t, _ = U.cases()["room"]
    w = U.want("room", H)
    _, _, height = U.apply_ref(xyz, w["plane"], w["R"], t, s_of=_fused_s)
    assert height.tobytes() != w["height"].tobytes()
    assert np.abs(height.astype(np.float64) - w["height"]).max() <= 1e-6      # a rounding apart, no more


def test_mutant_ties_to_the_highest_h_is_told_apart_by_two_slabs():
    planes, live, cin, cab = (v[:H] for v in U.scored("two_slabs"))
    n = U.cases()["two_slabs"][0].shape[0]
    a = U.select_ref(planes, live, cin, cab, n, False, 5)
    b = U.select_ref(planes, live, cin, cab, n, False, 5, highest=True)
    assert a["in"] == b["in"] and a["h"] < b["h"]


def test_mutant_index_order_sum_is_told_apart_by_room():
    xyz, t, _ = U.cases()["room"]
    mask = U.inlier_mask(xyz, U.selected("room", H)["plane0"], t)
    a, b = U.moments_ref(xyz, mask), U.moments_ref(xyz, mask, total=U.index_order_sum)
    assert a.tobytes() != b.tobytes() and np.allclose(a, b, rtol=1e-9, atol=1e-12)


# -------------------------------------------------------------------------------------------------------- arguments
XYZ = torch.zeros(8, 3)                                      # a CPU tensor: past the checks it would raise RuntimeError

BAD = [
    (dict(threshold=0.0), ValueError), (dict(threshold=-1.0), ValueError), (dict(threshold=float("nan")), ValueError),
    (dict(threshold=float("inf")), ValueError), (dict(threshold=1e39), ValueError), (dict(threshold="0.02"), TypeError),
    (dict(hypotheses=0), ValueError), (dict(hypotheses=4097), ValueError), (dict(hypotheses=16.0), ValueError),
    (dict(seed=-1), ValueError), (dict(seed=1 << 64), ValueError),
    (dict(up_hint=(0, 0)), ValueError), (dict(up_hint=(0, 0, 0)), ValueError), (dict(up_hint=(0, float("nan"), 1)), ValueError),
    (dict(up_hint=(0, float("inf"), 1)), ValueError), (dict(up_hint="up"), TypeError),
    (dict(max_tilt=0.0), ValueError), (dict(max_tilt=90.5), ValueError), (dict(max_tilt=float("nan")), ValueError),
    (dict(max_tilt=None), TypeError),
    (dict(below_frac=-0.1), ValueError), (dict(below_frac=1.5), ValueError), (dict(below_frac=float("nan")), ValueError),
    (dict(below_frac="1%"), TypeError),
]


@pytest.mark.parametrize("fn", ["fit_plane", "upright"])
@pytest.mark.parametrize("kw,exc", BAD)
def test_bad_arguments_raise_before_the_device(fn, kw, exc):
    args = dict(threshold=0.02)
    args.update(kw)
    with pytest.raises(exc):
        getattr(mesh, fn)(XYZ, **args)


@pytest.mark.parametrize("fn", ["fit_plane", "upright"])
def test_bad_points_raise_before_the_device(fn):
    for bad in (torch.zeros(8, 3, dtype=torch.float64), torch.zeros(8, 2), torch.zeros(24), np.zeros((8, 3), np.float32)):
        with pytest.raises(TypeError):
            getattr(mesh, fn)(bad, 0.02)
    with pytest.raises(RuntimeError):                        # every value is fine: only now is the device asked for
        getattr(mesh, fn)(XYZ, 0.02)


@pytest.mark.parametrize("kw,exc", BAD[:5] + BAD[6:] + [(dict(rounds=3), TypeError)])
def test_decode_points_checks_upright_before_the_device(kw, exc):
    src = (np.zeros((8, 3), np.float32), np.zeros((8, 3), np.float32))
    with pytest.raises(exc):
        mesh.decode_points(src, device="cpu", upright=kw)
    with pytest.raises(exc):
        mesh.decode_points(src, device="cpu", pitch=0.05, upright=kw)


def test_decode_points_upright_type():
    src = (np.zeros((8, 3), np.float32), np.zeros((8, 3), np.float32))
    for bad in ("floor", 1.0, ["up_hint"]):
        with pytest.raises(TypeError):
            mesh.decode_points(src, device="cpu", upright=bad)


def test_bookkeeping_names():
    assert {"R", "plane", "floor", "height"} <= set(mesh.SCENE_BOOKKEEPING)
    assert mesh.UPRIGHT_MAX_HYP == U.MAX_HYP and len(mesh.UPRIGHT_STAGES) == 4
