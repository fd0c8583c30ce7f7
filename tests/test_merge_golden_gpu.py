"""GPU tier: DeviceMerge (pbnet_amd/loader.py over csrc/augment.hip) replays the draws the reference's own trainMerge /
valMerge consumed (tests/golden/merge_*.npz) and rebuilds their batches: integers and feat_voxel exact, xyz_original and
inst_info within one float32 ulp."""
import glob
import os

import numpy as np
import pytest
import torch

import merge_ref
from pbnet_amd.loader import DeviceMerge, SceneCache

GOLDEN = sorted(glob.glob(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "merge_*.npz")))
DEV = torch.device("cuda:0")


@pytest.mark.gpu
@pytest.mark.parametrize("path", GOLDEN, ids=[os.path.basename(p)[6:-4] for p in GOLDEN])
def test_device_merge_replays_reference(path):
    kind, scenes, names, ids, draws, cfg, want = merge_ref.load_golden(path)
    cache = SceneCache(scenes, DEV, train=names, val=names)
    merge = DeviceMerge(cache, cfg)
    got = merge.train_merge(ids, draws) if kind == "train" else merge.val_merge(ids, draws)
    for k in merge_ref.OUT_KEYS:
        assert got[k].device.type == "cuda", k
    assert got["fn"] == [names[i] for i in (ids if kind == "train" else ids * 3)]
    merge_ref.assert_batch(merge_ref.to_numpy(got), want, os.path.basename(path))
    if kind == "train":
        assert np.array_equal(merge.last_crop_used, want["crop_used"])
    else:
        assert np.array_equal(got["sup"].cpu().numpy(), want["sup"])
    assert merge.readbacks <= 4
