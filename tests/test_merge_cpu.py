"""CPU tier: tests/merge_ref.py (the float64 restatement DeviceMerge is checked against at scale) reproduces the batches
the reference's own trainMerge / valMerge built (tests/golden/merge_*.npz, tests/golden/make_merge_golden.py); its blur
and interpolation match scipy; MergeDraws keeps its bounds."""
import glob
import os

import numpy as np
import pytest
import torch

import merge_ref
from pbnet_amd import loader
from pbnet_amd.config import get_config

GOLDEN = sorted(glob.glob(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "merge_*.npz")))


def test_fixtures_present():
    names = [os.path.basename(p) for p in GOLDEN]
    assert names == ["merge_T1.npz", "merge_T2.npz", "merge_T3.npz", "merge_V1.npz", "merge_V2.npz"]
    for p in GOLDEN:
        assert os.path.getsize(p) < 500 * 1024


@pytest.mark.parametrize("path", GOLDEN, ids=[os.path.basename(p)[6:-4] for p in GOLDEN])
def test_restatement_matches_reference(path):
    kind, scenes, names, ids, draws, cfg, want = merge_ref.load_golden(path)
    if kind == "train":
        got = merge_ref.train_merge(scenes, names, ids, draws, cfg)
        assert np.array_equal(got["crop_used"], want["crop_used"])
        assert all(s.crop.shape[0] <= loader.CROP_TRIES * loader.CROP_LEVELS for s in draws.scenes)
    else:
        got = merge_ref.val_merge(scenes, names, ids, draws, cfg)
        assert np.array_equal(got["sup"], want["sup"])
        assert len(got["fn"]) == 3 * len(ids)
    merge_ref.assert_batch(got, want, os.path.basename(path))


def test_fixture_quirks():
    """The cases cover what they claim: T2 fails all tries, T3 shifts the partner by -99, T1 crops."""
    g = {os.path.basename(p)[6:-4]: merge_ref.load_golden(p) for p in GOLDEN}
    d = np.load(GOLDEN[1])
    assert not d["crop_success"].any() and (d["crop_used"] > 0).all()
    assert np.load(GOLDEN[0])["crop_success"].all()
    kind, scenes, names, ids, draws, cfg, want = g["T3"]
    assert (scenes[names[ids[0]]]["ins_label"] == -100).all()
    ins = want["ins"]
    assert ((ins < 0) & (ins != -100)).any()                 # partner labels shifted below zero


def test_blur_matches_scipy():
    nd = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(0)
    w = [np.ones(s).astype("float32") / 3 for s in ((3, 1, 1), (1, 3, 1), (1, 1, 3))]
    for shape in ((3, 3, 3), (4, 5, 3), (7, 3, 6)):
        n = rng.standard_normal(shape).astype(np.float32)
        want = n
        for k in (0, 1, 2, 0, 1, 2):
            want = nd.convolve(want, w[k], mode="constant", cval=0)
        got = merge_ref.blur(n)
        assert got.dtype == np.float32 and np.array_equal(got, want)


def test_interp_matches_scipy():
    si = pytest.importorskip("scipy.interpolate")
    rng = np.random.default_rng(1)
    for gran, shape in ((6, (3, 4, 3)), (20, (4, 3, 5))):
        ax = merge_ref.axes(shape, gran)
        v = rng.standard_normal(shape).astype(np.float32)
        x = rng.uniform(-1.2, 1.2, (4000, 3)) * np.array([a[-1] for a in ax])
        x[:10] = np.array([a[1] for a in ax])                   # on grid lines
        want = si.RegularGridInterpolator(ax, v, bounds_error=0, fill_value=0)(x)
        got = merge_ref.interp(ax, v, x)
        assert ((x < -np.array([a[-1] for a in ax])) | (x > np.array([a[-1] for a in ax]))).any()
        np.testing.assert_allclose(got, want, rtol=0, atol=1e-15)


def test_mergedraws_bounds():
    gen = torch.Generator().manual_seed(3)
    d = loader.MergeDraws.draw_train(gen, 4, 10, lambda i, m: 400000 if i % 2 == 0 else 1000, 300000)
    assert [s.crop.shape for s in d.scenes] == [(85, 3), (0, 3), (85, 3), (0, 3)]
    for s in d.scenes:
        for a in (s.primary, s.partner):
            assert a.jitter.shape == (3, 3) and a.shift.shape == (3,) and 0.95 <= a.scale <= 1.05 and a.elastic
    a = d.scenes[0].primary
    g = d.noise_for(a, 0, (3, 4, 5))
    assert [x.shape for x in g] == [(3, 4, 5)] * 3 and g[0].dtype == np.float32
    with pytest.raises(AssertionError):
        d.noise_for(a, 0, (3, 4, 6))
    # replayed grid shapes are asserted
    kind, scenes, names, ids, draws, cfg, want = merge_ref.load_golden(GOLDEN[0])
    a = draws.scenes[0].primary
    shape = a.noise[0][0].shape
    assert draws.noise_for(a, 0, shape) is a.noise[0]
    with pytest.raises(AssertionError):
        draws.noise_for(a, 0, tuple(s + 1 for s in shape))
    v = loader.MergeDraws.draw_val(gen, 2)
    assert len(v.copies) == 6 and all(c.jitter is None and c.shift.shape == (3,) for c in v.copies)


def test_crop_levels_reach_zero():
    cfg = get_config()
    lv = loader.crop_levels(cfg)
    assert lv.shape == (17, 3) and abs(lv[16, 0]) < 1e-12 and lv[16, 2] == 512 / 50.0
    assert cfg.max_crop_p == 300000 and cfg.min_crop_p == 50000


def test_elastic_shape():
    assert loader.elastic_shape([5.9, 12.0, 0.2], 6) == (3, 5, 3)
    assert loader.elastic_shape([41.5, 19.99, 20.0], 20) == (5, 3, 4)
