"""End to end on the GPU for a scan in its sensor's frame: tests/upright_ref.py's room (floor, walls, ceiling and clutter,
rotated 25 degrees about a skew axis) goes through pbnet_amd.mesh.decode_points(pitch, upright).  The result must equal
the chain written out by hand -- thin_points, upright, then the decode of before on the upright points -- carry the room's
true up on +z, map kept_xyz through R bit for bit, stay out of the scene files, and feed SceneCache.  upright=None is the
decode of before, byte for byte."""
import os

import numpy as np
import pytest
import torch

import upright_ref as U
from pbnet_amd import mesh
from test_mesh_e2e_gpu import DEV, _labels, _run

pytestmark = pytest.mark.gpu

K, PITCH = 16, 0.05
OPTION = {"up_hint": tuple(U.ROOM_UP), "threshold": U.ROOM_T, "seed": 11}


@pytest.fixture(scope="module")
def room():
    xyz = U.cases()["room"][0]
    colours = np.random.default_rng(2).integers(0, 256, xyz.shape).astype(np.uint8)
    return xyz, colours


@pytest.fixture(scope="module")
def decoded(room):
    dec = mesh.decode_points(room, device=DEV, k=K, pitch=PITCH, upright=OPTION, return_kept=True)
    assert all(v.is_cuda for v in dec.values())
    return {k: v.cpu().numpy() for k, v in dec.items()}


def test_upright_none_is_the_decode_of_before(room):
    for kw in ({}, {"pitch": PITCH}):
        a = mesh.decode_points(room, device=DEV, k=K, **kw)
        b = mesh.decode_points(room, device=DEV, k=K, upright=None, **kw)
        assert sorted(a) == sorted(b) and not {"R", "plane", "floor", "height"} & set(a)
        for k in a:
            assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape
            assert a[k].cpu().numpy().tobytes() == b[k].cpu().numpy().tobytes(), k


def test_decode_is_the_chain_written_out(room, decoded):
    xyz, colours = room
    d = decoded
    assert sorted(d) == ["R", "count", "floor", "height", "kept_rgb", "kept_xyz", "nl", "plane", "raw_index", "rgb", "sup", "xyz"]
    th = mesh.thin_points(torch.from_numpy(xyz).to(DEV), torch.from_numpy(colours.astype(np.float32)).to(DEV), PITCH)
    up = mesh.upright(th["xyz"], **OPTION)
    assert up["found"]
    plain = mesh.decode_points((up["xyz"].cpu().numpy(), th["rgb"].cpu().numpy()), device=DEV, k=K)
    for k in ("xyz", "rgb", "nl", "sup"):
        got, want = d[k], plain[k].cpu().numpy()
        assert got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes(), k
    for k, v in (("R", up["R"]), ("plane", up["plane"]), ("floor", up["floor"]), ("height", up["height"]),
                 ("kept_xyz", th["xyz"]), ("kept_rgb", th["rgb"]), ("count", th["count"]), ("raw_index", th["inverse"])):
        want = v.cpu().numpy()
        assert d[k].dtype == want.dtype and d[k].shape == want.shape and d[k].tobytes() == want.tobytes(), k
    m = d["kept_xyz"].shape[0]
    assert d["R"].shape == (3, 3) and d["plane"].shape == (4,) and d["floor"].shape == (m,) and d["floor"].dtype == bool
    assert d["height"].shape == (m,) and d["height"].dtype == np.float32


def test_up_is_recovered_and_r_maps_the_kept_points(room, decoded):
    d = decoded
    bound = np.arctan(2 * U.ROOM_T / U.ROOM_L)                # every floor point within +-t of the plane across L
    assert U.angle_to(d["R"] @ U.ROOM_UP, (0.0, 0.0, 1.0)) <= bound
    assert U.angle_to(d["plane"][:3], U.ROOM_UP) <= bound
    out, floor, height = U.apply_ref(d["kept_xyz"], d["plane"], d["R"], U.ROOM_T)
    centred, _ = mesh.centre_and_scale(out, d["kept_rgb"])
    assert d["xyz"].tobytes() == np.ascontiguousarray(centred, np.float32).tobytes()
    assert d["floor"].tobytes() == floor.tobytes() and d["height"].tobytes() == height.tobytes()
    assert d["floor"].sum() >= 1500
    z = d["xyz"][d["floor"]][:, 2].astype(np.float64)
    assert z.max() - z.min() <= 2 * U.ROOM_T + 1e-5           # level
    assert np.median(d["xyz"][~d["floor"]][:, 2]) > np.median(z)      # and beneath the room


def test_without_a_front_it_runs_after_the_upload(room):
    xyz, colours = room
    dec = mesh.decode_points(room, device=DEV, k=K, upright=dict(OPTION))
    up = mesh.upright(torch.from_numpy(xyz).to(DEV), **OPTION)
    plain = mesh.decode_points((up["xyz"].cpu().numpy(), colours.astype(np.float32)), device=DEV, k=K)
    assert sorted(dec) == ["R", "floor", "height", "nl", "plane", "rgb", "sup", "xyz"]
    for k in ("xyz", "rgb", "nl", "sup"):
        assert dec[k].cpu().numpy().tobytes() == plain[k].cpu().numpy().tobytes(), k
    assert dec["R"].cpu().numpy().tobytes() == up["R"].cpu().numpy().tobytes()


def test_threshold_defaults_to_the_pitch(room):
    xyz, colours = room
    dec = mesh.decode_points(room, device=DEV, k=K, pitch=PITCH, upright={"up_hint": OPTION["up_hint"]})
    th = mesh.thin_points(torch.from_numpy(xyz).to(DEV), torch.from_numpy(colours.astype(np.float32)).to(DEV), PITCH)
    up = mesh.upright(th["xyz"], PITCH, up_hint=OPTION["up_hint"])
    assert dec["plane"].cpu().numpy().tobytes() == up["plane"].cpu().numpy().tobytes()
    assert dec["floor"].cpu().numpy().tobytes() == up["floor"].cpu().numpy().tobytes()


def test_bookkeeping_stays_out_of_the_scene_files(decoded, tmp_path):
    mesh.save_decoded(str(tmp_path), "scene0000_00", {k: v for k, v in decoded.items() if not k.startswith("kept_")})
    names = sorted(os.listdir(str(tmp_path)))
    assert names and all(n.startswith("scene0000_00_") for n in names)
    written = {n[len("scene0000_00_"):-len(".npy")] for n in names}
    assert not written & {"R", "plane", "floor", "height"} and {"xyz", "rgb", "nl", "sup"} <= written


def test_scene_cache_takes_the_result(decoded):
    m = decoded["xyz"].shape[0]
    sem, ins = _labels(m)
    batch, (c, s, i, dbg) = _run(dict(decoded, sem_label=sem, ins_label=ins))
    assert int(batch["xyz_original"].shape[0]) > 0


def test_two_points_have_no_floor():
    src = (np.array([[0, 0, 0], [1, 0, 0]], np.float32), np.zeros((2, 3), np.float32))
    with pytest.raises(ValueError, match="no floor plane found"):
        mesh.decode_points(src, device=DEV, k=K, upright=True)
