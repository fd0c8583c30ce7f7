"""CPU tier: `scene_io.write_submission` writes the files of eval_map.py:142-155, byte for byte -- `<scene>.txt` with one line
`predicted_masks/<scene>_%03d.txt <label> %.4f` per instance and no newline after the last, and one 0/1 mask per instance, a point
per line (np.savetxt with fmt='%d')."""
import os

import numpy as np
import torch

from pbnet_amd.scene_io import write_submission

SCENE = "scene0011_00"
POINT_INSTANCE = np.array([0, -100, 2, 0, 2, -100, 0], dtype=np.int32)         # instance 1 owns no point
SCORES = np.array([0.98766, 0.5, 0.12344], dtype=np.float32)
LABELS = np.array([5, 39, 12], dtype=np.int64)
WANT_LIST = (b"predicted_masks/scene0011_00_000.txt 5 0.9877\n"
             b"predicted_masks/scene0011_00_001.txt 39 0.5000\n"
             b"predicted_masks/scene0011_00_002.txt 12 0.1234")
WANT_MASKS = [b"1\n0\n0\n1\n0\n0\n1\n", b"0\n0\n0\n0\n0\n0\n0\n", b"0\n0\n1\n0\n1\n0\n0\n"]


def _read(*parts):
    with open(os.path.join(*parts), "rb") as f:
        return f.read()


def _check(root):
    assert _read(root, SCENE + ".txt") == WANT_LIST
    assert sorted(os.listdir(os.path.join(root, "predicted_masks"))) == ["%s_%03d.txt" % (SCENE, k) for k in range(3)]
    for k, want in enumerate(WANT_MASKS):
        assert _read(root, "predicted_masks", "%s_%03d.txt" % (SCENE, k)) == want


def test_files_equal_the_reference_format(tmp_path):
    write_submission(str(tmp_path), SCENE, POINT_INSTANCE, SCORES, LABELS)
    _check(str(tmp_path))


def test_tensors_are_taken_as_well(tmp_path):
    write_submission(str(tmp_path), SCENE, torch.from_numpy(POINT_INSTANCE), torch.from_numpy(SCORES), torch.from_numpy(LABELS))
    _check(str(tmp_path))


def test_no_trailing_newline_and_a_scene_without_instances(tmp_path):
    write_submission(str(tmp_path), SCENE, POINT_INSTANCE, SCORES[:1], LABELS[:1])
    assert _read(str(tmp_path), SCENE + ".txt") == b"predicted_masks/scene0011_00_000.txt 5 0.9877"
    write_submission(str(tmp_path), "empty", POINT_INSTANCE, SCORES[:0], LABELS[:0])
    assert _read(str(tmp_path), "empty.txt") == b""
