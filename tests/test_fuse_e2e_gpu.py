"""End to end on the GPU for depth-frame fusion: the ray-cast room of tests/test_frames_e2e_gpu.py (six frames of 60 x 80, one
lost) through pbnet_amd.mesh.decode_frames(fuse=...), with and without `upright`, with the fused normals and with the
chain's own; fuse=None is the decode of before."""
import numpy as np
import pytest
import torch

import frames_ref as R
import fuse_ref as FR
from pbnet_amd import frames as F, mesh
from test_frames_e2e_gpu import CAMERAS, BOX, FRAME_KW, H, INTR, K, LOST, PLANES, W, _np
from test_mesh_e2e_gpu import DEV

pytestmark = pytest.mark.gpu

PITCH, FUSE = 0.05, {"voxel": 0.04}
UP = {"up_hint": (0.1, -0.05, 1.0), "threshold": 0.03, "seed": 3}


@pytest.fixture(scope="module")
def frames():
    pose = np.stack([R.look_at(e, t) for e, t in CAMERAS])
    img = [R.render(p, INTR, H, W, PLANES, BOX) for p in pose]
    pose[LOST] = -np.inf
    return {"depth": np.stack([i["u16"] for i in img]), "colour": np.stack([i["colour"] for i in img]), "pose": pose}


def _decode(fr, colour=True, **kw):
    return _np(mesh.decode_frames(fr["depth"], fr["pose"], INTR, fr["colour"] if colour else None, device=DEV, k=K,
                                  **dict(FRAME_KW, **kw)))


@pytest.fixture(scope="module")
def surface(frames):
    fr = frames
    return _np(F.fuse_frames(torch.from_numpy(fr["depth"]).to(DEV), fr["pose"], INTR, torch.from_numpy(fr["colour"]).to(DEV),
                             **dict(FRAME_KW, **FUSE)))


@pytest.fixture(scope="module")
def thinned(surface):
    th = mesh.thin_points(torch.from_numpy(surface["xyz"]).to(DEV), torch.from_numpy(surface["rgb"]).to(DEV), PITCH)
    return _np(th)


def test_the_surface_is_the_restatement(frames, surface):
    want = FR.fuse_ref(frames["depth"], frames["pose"], INTR, frames["colour"], **dict(FRAME_KW, **FUSE))
    for k in ("xyz", "rgb", "nl", "weight", "voxel_id"):
        assert surface[k].dtype == want[k].dtype and surface[k].tobytes() == want[k].tobytes(), k
    assert surface["n_blocks"] == want["block_key"].shape[0] > 100 and want["n"] > 2000
    assert surface["skipped"].tolist() == [f == LOST for f in range(6)]
    length = np.linalg.norm(surface["nl"].astype(np.float64), axis=1)
    assert np.all((np.abs(length - 1.0) < 1e-6) | (length == 0.0)) and np.mean(length > 0) > 0.99


@pytest.mark.parametrize("upright", [None, UP])
@pytest.mark.parametrize("normals", ["tsdf", None])
def test_fused_decode(frames, surface, thinned, upright, normals):
    out = _decode(frames, fuse=FUSE, pitch=PITCH, normals=normals, upright=upright)
    m = thinned["xyz"].shape[0]
    assert m == out["xyz"].shape[0] and 500 < m < surface["xyz"].shape[0]
    for k, dtype, shape in (("xyz", np.float32, (m, 3)), ("rgb", np.float32, (m, 3)), ("nl", np.float32, (m, 3)),
                            ("fuse_weight", np.int32, (m,)), ("count", np.int32, (m,)),
                            ("raw_index", np.int32, (surface["xyz"].shape[0],))):
        assert out[k].dtype == dtype and out[k].shape == shape, k
    assert all(np.all(np.isfinite(out[k])) for k in ("xyz", "rgb", "nl")) and out["sup"].shape == (m,)
    assert not {"pixel", "frame", "frame_start"} & set(out) and out["n_blocks"] == surface["n_blocks"]
    assert {"fuse_weight", "n_blocks", "centres", "skipped"} <= set(out) and set(out) - {"xyz", "rgb", "nl", "sup"} <= set(mesh.SCENE_BOOKKEEPING)
    assert ("R" in out) == (upright is not None)
    first = thinned["first"].astype(np.int64)
    assert out["fuse_weight"].tobytes() == surface["weight"][first].tobytes()
    nl = surface["nl"][first].astype(np.float64)
    if upright is not None:
        Rm = out["R"]
        assert abs(Rm[2] @ np.array([0.0, 0.0, 1.0])) > 0.99                         # the floor is level: z stays up
        nl = np.stack([(Rm[r, 0] * nl[:, 0] + Rm[r, 1] * nl[:, 1]) + Rm[r, 2] * nl[:, 2] for r in range(3)], axis=1)
    if normals == "tsdf":
        assert out["nl"].tobytes() == nl.astype(np.float32).tobytes()
    else:
        assert out["nl"].tobytes() != nl.astype(np.float32).tobytes()
        cos = np.abs(np.sum(out["nl"].astype(np.float64) * nl, axis=1))
        assert np.median(cos) > 0.95                                                # PCA and the field's gradient agree on the planes


def test_without_colour_the_surface_is_black(frames):
    out = _decode(frames, colour=False, fuse=FUSE, pitch=PITCH)
    assert out["rgb"].shape[0] > 500 and len(np.unique(out["rgb"])) == 1


def test_fuse_none_is_the_decode_of_before(frames):
    a = _decode(frames, pitch=PITCH)
    b = _decode(frames, pitch=PITCH, fuse=None, normals="sensor")
    c = _decode(frames, pitch=PITCH, fuse=False)
    assert sorted(a) == sorted(b) == sorted(c) and "pixel" in a and "fuse_weight" not in a
    for k in a:
        assert a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes() == c[k].tobytes(), k
