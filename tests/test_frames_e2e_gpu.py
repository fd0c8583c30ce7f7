"""End to end on the GPU for posed depth frames: a ray-cast room (floor, two walls, a box; tests/frames_ref.py's renderer), six
frames of 60 x 80 of which one has lost its pose, through pbnet_amd.mesh.decode_frames.  One camera stands behind the wall
x = 2 and sees it from outside: its points' normals must face that camera, which one viewpoint for the cloud cannot give."""
import os

import numpy as np
import pytest
import torch

import frames_ref as R
from pbnet_amd import mesh
from test_mesh_e2e_gpu import DEV, _labels, _run

pytestmark = pytest.mark.gpu

H, W, K, PITCH = 60, 80, 16, 0.05
INTR = (70.0, 70.0, 39.5, 29.5)
PLANES = [(2, 0.0, (120, 100, 80)), (1, 3.0, (200, 200, 190)), (0, 2.0, (90, 120, 160))]      # floor, wall y = 3, wall x = 2
BOX = ((0.2, 2.0, 0.0), (0.8, 2.6, 0.5), (30, 160, 60))
CAMERAS = [((0.2, 0.2, 1.4), (0.6, 3.0, 0.4)), ((1.0, 0.0, 1.5), (0.4, 3.0, 0.3)), ((1.5, 0.5, 1.2), (0.0, 2.5, 0.2)),
           ((0.5, 1.0, 1.6), (0.5, 2.4, 0.0)), ((-0.5, 0.3, 1.3), (1.0, 3.0, 0.6)), ((3.6, 1.5, 1.2), (2.0, 1.6, 0.9))]
LOST, OUTSIDE = 3, 5
FRAME_KW = dict(depth_max=4.5, edge=0.05)


@pytest.fixture(scope="module")
def frames():
    pose = np.stack([R.look_at(e, t) for e, t in CAMERAS])
    img = [R.render(p, INTR, H, W, PLANES, BOX) for p in pose]
    pose[LOST] = -np.inf
    surface = np.stack([i["surface"] for i in img])
    return {"depth": np.stack([i["u16"] for i in img]), "colour": np.stack([i["colour"] for i in img]), "pose": pose,
            "sem": surface.astype(np.int32) + 2, "ins": np.where(surface == 3, 7, -100).astype(np.int64)}


def _decode(fr, **kw):
    return mesh.decode_frames(fr["depth"], fr["pose"], INTR, fr["colour"], device=DEV, k=K, **dict(FRAME_KW, **kw))


def _np(d):
    return {k: v.cpu().numpy() if torch.is_tensor(v) else v for k, v in d.items()}


def _bytes_equal(got, want, keys):
    for k in keys:
        g, w = got[k], want[k]
        assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes(), k


@pytest.fixture(scope="module")
def cloud(frames):
    fr = frames
    return mesh.frames_to_points(torch.from_numpy(fr["depth"]).to(DEV), fr["pose"], INTR, torch.from_numpy(fr["colour"]).to(DEV),
                                 **FRAME_KW)


@pytest.fixture(scope="module")
def sensor(frames):
    return _np(_decode(frames, pitch=PITCH, return_graph=True, return_kept=True))


@pytest.fixture(scope="module")
def single(frames):
    return _np(_decode(frames, pitch=PITCH, normals=None))


def _mean32(xyz):
    """centre_and_scale's mean: float32, over the first three columns of its [M, 6] layout."""
    v = np.zeros((xyz.shape[0], 6), np.float32)
    v[:, :3] = xyz
    return v[:, :3].mean(0)


def test_the_cloud_is_the_restatement(frames, cloud):
    want = R.frames_ref(frames["depth"], frames["pose"], INTR, frames["colour"], **FRAME_KW)
    _bytes_equal(_np(cloud), want, ("xyz", "rgb", "pixel", "frame_start"))
    counts = np.diff(want["frame_start"])
    assert counts[LOST] == 0 and all(counts[f] > 1000 for f in range(6) if f != LOST)
    assert cloud["skipped"].tolist() == [f == LOST for f in range(6)]


def test_without_sensor_normals_it_is_decode_points_on_the_cloud(cloud, single):
    plain = _np(mesh.decode_points((cloud["xyz"], cloud["rgb"]), device=DEV, k=K, pitch=PITCH))
    assert sorted(single) == sorted(list(plain) + ["pixel", "frame", "centres", "frame_start", "skipped"])
    _bytes_equal(single, plain, list(plain))
    _bytes_equal(single, _np(cloud), ("pixel", "centres", "frame_start", "skipped"))


def test_sensor_normals_are_the_restatement(cloud, sensor, single):
    d = sensor
    th = mesh.thin_points(cloud["xyz"], cloud["rgb"], PITCH)
    frame = (cloud["pixel"].cpu().numpy() // (H * W))[th["first"].cpu().numpy()].astype(np.int32)
    _bytes_equal(d, {"frame": frame, "kept_xyz": th["xyz"].cpu().numpy()}, ("frame", "kept_xyz"))
    assert LOST not in frame and set(frame.tolist()) == set(range(6)) - {LOST}
    centres = R.centres_ref(np.stack([R.look_at(e, t) for e, t in CAMERAS]))[0]
    views = (centres.astype(np.float64) - _mean32(d["kept_xyz"]).astype(np.float64)).astype(np.float32)
    want = R.normals_views_ref(d["xyz"], d["idx"], views, d["frame"])
    assert d["nl"].tobytes() == want.tobytes()
    # every normal faces the sensor that saw its point
    has = d["nl"].any(axis=1)
    to_view = views[d["frame"]].astype(np.float64) - d["xyz"].astype(np.float64)
    facing = np.einsum("ij,ij->i", d["nl"].astype(np.float64), to_view)
    assert has.sum() > 0.99 * has.size and np.all(facing[has] >= -1e-6)
    # and one viewpoint for the cloud cannot do that on the wall seen from outside: on the device and in the restatement
    _bytes_equal(single, d, ("xyz",))
    vp = d["xyz"].astype(np.float64).mean(0).astype(np.float32)
    one = R.normals_views_ref(d["xyz"], d["idx"], vp[None], np.zeros(has.size, np.int32))
    assert single["nl"].tobytes() == one.tobytes()
    for a, b in ((d["nl"], single["nl"]), (want, one)):
        differs = np.einsum("ij,ij->i", a, b) < 0
        wall = differs & (d["frame"] == OUTSIDE) & (np.abs(d["kept_xyz"][:, 0] - 2.0) < 0.02)
        assert wall.sum() > 50 and np.all(a[wall][:, 0] > 0.5)                # towards +x, where that camera stands


def test_label_images_arrive_as_gathered_labels(frames, cloud):
    got = _np(_decode(frames, pitch=PITCH, normals=None, sem_label=frames["sem"], ins_label=frames["ins"], n_classes=8))
    pixel = cloud["pixel"].cpu().numpy()
    want = _np(mesh.decode_points((cloud["xyz"], cloud["rgb"]), device=DEV, k=K, pitch=PITCH, n_classes=8,
                                  sem_label=frames["sem"].reshape(-1)[pixel], ins_label=frames["ins"].reshape(-1)[pixel]))
    _bytes_equal(got, want, list(want))
    assert set(np.unique(got["sem_label"]).tolist()) == {2, 3, 4, 5} and got["ins_old_id"].tolist() == [7]


def test_upright_composes(frames):
    option = {"up_hint": (0.1, -0.05, 1.0), "threshold": 0.03, "seed": 3}
    d = _np(_decode(frames, pitch=PITCH, upright=option, return_graph=True, return_kept=True))
    up = mesh.upright(torch.from_numpy(d["kept_xyz"]).to(DEV), **option)
    assert d["R"].tobytes() == up["R"].cpu().numpy().tobytes()
    Rm, c = d["R"], d["centres"].astype(np.float64)
    turned = np.stack([(Rm[r, 0] * c[:, 0] + Rm[r, 1] * c[:, 1]) + Rm[r, 2] * c[:, 2] for r in range(3)], axis=1)
    views = (turned - _mean32(up["xyz"].cpu().numpy()).astype(np.float64)).astype(np.float32)
    assert d["nl"].tobytes() == R.normals_views_ref(d["xyz"], d["idx"], views, d["frame"]).tobytes()
    assert np.isnan(views[LOST]).all() and np.isfinite(np.delete(views, LOST, axis=0)).all()


def test_graph_orientation_may_follow(frames, sensor):
    d = _np(_decode(frames, pitch=PITCH, orient="graph"))
    want = mesh.orient_normals(torch.from_numpy(sensor["nl"]).to(DEV), torch.from_numpy(sensor["idx"]).to(DEV))
    assert d["nl"].tobytes() == want["nl"].cpu().numpy().tobytes() and d["flipped"].tobytes() == want["flipped"].cpu().numpy().tobytes()


def test_without_a_front_the_point_is_its_own_first(frames):
    d = _np(_decode(frames, stride=4, return_graph=True))
    assert np.array_equal(d["frame"], d["pixel"] // (H * W)) and "raw_index" not in d
    c = R.centres_ref(np.stack([R.look_at(e, t) for e, t in CAMERAS]))[0].astype(np.float64)
    raw = R.frames_ref(frames["depth"], frames["pose"], INTR, stride=4, **FRAME_KW)["xyz"]
    views = (c - _mean32(raw).astype(np.float64)).astype(np.float32)
    assert d["nl"].tobytes() == R.normals_views_ref(d["xyz"], d["idx"], views, d["frame"]).tobytes()


def test_the_result_is_a_scene(sensor, tmp_path):
    scene = {k: v for k, v in sensor.items() if not k.startswith("kept_") and k not in ("idx", "d2")}
    mesh.save_decoded(str(tmp_path), "scene0000_00", scene)
    written = {n[len("scene0000_00_"):-len(".npy")] for n in os.listdir(str(tmp_path))}
    assert written == {"xyz", "rgb", "nl", "sup"}
    sem, ins = _labels(scene["xyz"].shape[0])
    batch, _ = _run(dict(scene, sem_label=sem, ins_label=ins))
    assert int(batch["xyz_original"].shape[0]) > 0
