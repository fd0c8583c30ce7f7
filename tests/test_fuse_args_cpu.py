"""Every host-side refusal of fuse_frames and of decode_frames(fuse=) is raised on CPU (or meta) tensors, before a device or
the library is asked for anything."""
import numpy as np
import pytest
import torch

from pbnet_amd import _native as N, frames, mesh

F, H, W = 2, 3, 4
POSES = np.tile(np.eye(4), (F, 1, 1))
INTR = (50.0, 50.0, 1.5, 1.0)


@pytest.fixture(autouse=True)
def no_library(monkeypatch):
    def lib():
        raise AssertionError("the library was asked before the arguments were checked")
    monkeypatch.setattr(N, "lib", lib)
    monkeypatch.setattr(N, "require_cuda", lambda *t: (_ for _ in ()).throw(AssertionError("the device was asked first")))


def _depth(dtype=torch.uint16, shape=(F, H, W)):
    return torch.zeros(shape, dtype=dtype)


def _fake(shape):
    """A shape without its memory."""
    return torch.empty(shape, dtype=torch.uint16, device="meta")


CALLS = {
    "voxel_zero": (ValueError, "voxel must be positive and finite", dict(voxel=0.0)),
    "voxel_negative": (ValueError, "voxel must be positive and finite", dict(voxel=-0.02)),
    "voxel_nan": (ValueError, "voxel must be positive and finite", dict(voxel=float("nan"))),
    "voxel_inf": (ValueError, "voxel must be positive and finite", dict(voxel=float("inf"))),
    "voxel_type": (TypeError, "voxel must be a number", dict(voxel="0.02")),
    "trunc_zero": (ValueError, "trunc must be finite with 0 < trunc <= 8 \\* voxel", dict(trunc=0.0)),
    "trunc_negative": (ValueError, "trunc must be finite with 0 < trunc <= 8 \\* voxel", dict(trunc=-0.01)),
    "trunc_nan": (ValueError, "trunc must be finite with 0 < trunc <= 8 \\* voxel", dict(trunc=float("nan"))),
    "trunc_above_8_voxels": (ValueError, "trunc must be finite with 0 < trunc <= 8 \\* voxel", dict(voxel=0.02, trunc=0.1601)),
    "trunc_type": (TypeError, "trunc must be a number or None", dict(trunc="0.08")),
    "min_weight_zero": (ValueError, "min_weight must be an int in 1", dict(min_weight=0)),
    "min_weight_float": (ValueError, "min_weight must be an int in 1", dict(min_weight=2.0)),
    "min_weight_bool": (ValueError, "min_weight must be an int in 1", dict(min_weight=True)),
}
FRAMES = {
    "depth_dtype": (TypeError, "depth must be a uint16 or float32", dict(depth=_depth(torch.int32))),
    "colour_shape": (TypeError, "colour must be a uint8", dict(colour=torch.zeros(F, H, W, 4, dtype=torch.uint8))),
    "poses_shape": (ValueError, "poses must have shape", dict(poses=np.zeros((F + 1, 4, 4)))),
    "fx_zero": (ValueError, "fx and fy must be positive", dict(intrinsics=(0.0, 50.0, 1.0, 1.0))),
    "scale_zero": (ValueError, "depth_scale must be positive", dict(depth_scale=0.0)),
    "min_above_max": (ValueError, "depth_min must not exceed depth_max", dict(depth_min=2.0, depth_max=1.0)),
    "pixels_2_31": (ValueError, "exceed 2\\^31 - 1", dict(depth=_fake((1 << 11, 1 << 10, 1 << 10)), poses=np.zeros((1 << 11, 4, 4)))),
    "sampled_2_28": (ValueError, "exceed 2\\^28", dict(depth=_fake((1 << 9, 1 << 10, (1 << 9) + 1)), poses=np.zeros((1 << 9, 4, 4)))),
}


@pytest.mark.parametrize("name", list(CALLS) + list(FRAMES))
def test_fuse_frames_refuses(name):
    exc, message, changed = {**CALLS, **FRAMES}[name]
    kw = dict(depth=_depth(), poses=POSES, intrinsics=INTR)
    kw.update(changed)
    with pytest.raises(exc, match=message):
        frames.fuse_frames(**kw)


@pytest.mark.parametrize("name", list(CALLS))
def test_decode_frames_refuses_the_same_through_fuse(name):
    exc, message, changed = CALLS[name]
    with pytest.raises(exc, match=message):
        mesh.decode_frames(_depth(), POSES, INTR, fuse=changed)


def test_the_limits_sit_where_the_library_has_them():
    """trunc = 8 * voxel, min_weight = 1 and 2^28 pixels pass the host's checks: the next thing asked is the device."""
    for kw in (dict(voxel=0.02, trunc=0.16), dict(min_weight=1), dict(voxel=1e-3, trunc=1e-9)):
        with pytest.raises(AssertionError, match="the device was asked first"):
            frames.fuse_frames(_depth(), POSES, INTR, **kw)
    with pytest.raises(AssertionError, match="the device was asked first"):
        frames.fuse_frames(_fake((1 << 8, 1 << 10, 1 << 10)), np.zeros((1 << 8, 4, 4)), INTR)
    assert frames._fuse_args("f", 0.02, None, 1) == (0.02, 0.08, 1)


LABELS = dict(sem_label=np.zeros((F, H, W), np.int32), ins_label=np.zeros((F, H, W), np.int32))
DECODE = {
    "fuse_type": (TypeError, "fuse must be None, True or a dict", dict(fuse=0.02)),
    "fuse_unknown_key": (TypeError, "fuse has no argument 'stride'", dict(fuse={"stride": 2})),
    "sensor_normals": (ValueError, "normals=\"sensor\" needs one frame per point", dict(fuse=True, normals="sensor")),
    "other_normals": (ValueError, "normals must be None or \"tsdf\" with fuse", dict(fuse=True, normals="pca")),
    "labels": (ValueError, "sem_label / ins_label cannot be given with fuse", dict(fuse=True, **LABELS)),
    "one_label": (ValueError, "sem_label / ins_label cannot be given with fuse", dict(fuse=True, ins_label=LABELS["ins_label"])),
    "stride": (ValueError, "stride must be 1 with fuse", dict(fuse={"voxel": 0.05}, stride=2)),
    "tsdf_without_fuse": (ValueError, "normals must be None or \"sensor\"", dict(normals="tsdf")),
    "orient": (ValueError, "orient must be None or \"graph\"", dict(fuse=True, orient="tree")),
    "return_kept": (ValueError, "return_kept needs pitch", dict(fuse=True, return_kept=True)),
    "depth_dtype": (TypeError, "depth must be a uint16 or float32", dict(fuse=True, depth=_depth(torch.int32))),
}


@pytest.mark.parametrize("name", list(DECODE))
def test_decode_frames_refuses(name):
    exc, message, changed = DECODE[name]
    kw = dict(depth=_depth(), poses=POSES, intrinsics=INTR)
    kw.update(changed)
    with pytest.raises(exc, match=message):
        mesh.decode_frames(**kw)


def test_fused_decodes_reach_the_device_next():
    for kw in (dict(fuse=True), dict(fuse={"voxel": 0.05, "trunc": 0.1, "min_weight": 2}, normals=None, pitch=0.05),
               dict(fuse=True, normals="tsdf", upright=True, orient="graph")):
        with pytest.raises(AssertionError, match="the device was asked first|the library was asked"):
            mesh.decode_frames(_depth(), POSES, INTR, device="cpu", **kw)
    assert {"fuse_weight", "n_blocks"} <= set(mesh.SCENE_BOOKKEEPING)
