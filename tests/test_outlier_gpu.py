"""GPU tier of outlier removal and the raw index: pbnet_amd.mesh.outlier_mask (keep and the float64 stats) and
pbnet_amd.mesh.raw_index are compared BIT FOR BIT with tests/thin_ref.py on the designed cases of tests/thin_cases.py."""
import numpy as np
import pytest
import torch

import thin_cases as C
import thin_ref as R
from pbnet_amd import mesh
from test_thin_ref_cpu import same_outlier

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")


def _run(d2, ratio):
    keep, stats = mesh.outlier_mask(torch.from_numpy(d2).to(DEV), ratio)
    assert keep.dtype == torch.bool and keep.shape == (d2.shape[0],) and stats.dtype == torch.float64 and stats.shape == (3,)
    return keep.cpu().numpy(), stats.cpu().numpy()


@pytest.mark.parametrize("name", sorted(C.OUTLIER))
def test_outlier_mask_is_the_restatement_bit_for_bit(name):
    d2, ratio = C.OUTLIER[name]
    assert same_outlier(_run(d2, ratio), R.outlier(d2, ratio))


def test_a_point_exactly_on_the_threshold_is_kept():
    keep, stats = _run(*C.OUTLIER["exact_threshold"])
    assert stats.tolist() == [2.0, 1.0, 4.0] and keep.tolist() == [True] * 4


def test_room_with_far_points():
    """The d2 table comes from the device's own graph (pinned to the brute force by tests/test_cloud_gpu.py)."""
    pts = C.far_room()
    idx, d2 = mesh.knn_graph(torch.from_numpy(pts).to(DEV), k=16)
    keep, stats = mesh.outlier_mask(d2, 2.0)
    want = R.outlier(d2.cpu().numpy(), 2.0)
    assert same_outlier((keep.cpu().numpy(), stats.cpu().numpy()), want)
    assert not want[0][-30:].any() and want[0][:-30].mean() > 0.97
    again = mesh.outlier_mask(d2, 2.0)
    assert torch.equal(keep, again[0]) and torch.equal(stats.view(torch.int64), again[1].view(torch.int64))
    # the way back: every raw point of the room answers for itself or for a kept neighbour
    inverse = torch.arange(pts.shape[0], dtype=torch.int32, device=DEV)
    raw = mesh.raw_index(inverse, keep, idx).cpu().numpy()
    assert np.array_equal(raw, R.raw_index(inverse.cpu().numpy(), want[0], idx.cpu().numpy()))
    assert np.array_equal(raw[want[0]], np.arange(int(want[0].sum())))


@pytest.mark.parametrize("name", sorted(C.RAW))
def test_raw_index_is_the_restatement(name):
    inverse, keep, idx = C.RAW[name]
    got = mesh.raw_index(torch.from_numpy(inverse).to(DEV), torch.from_numpy(keep).to(DEV), torch.from_numpy(idx).to(DEV))
    assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), R.raw_index(inverse, keep, idx))


def test_raw_index_designed_rows():
    inverse, keep, idx = C.RAW["designed"]
    got = mesh.raw_index(torch.from_numpy(inverse).to(DEV), torch.from_numpy(keep).to(DEV), torch.from_numpy(idx).to(DEV))
    got = got.cpu().numpy()
    assert got[1] == 2          # thinned point 2, an outlier: its first kept neighbour in rank order is 3 = kept row 2
    assert got[4] == -1         # thinned point 4: no kept neighbour
    assert got[3] == 1          # thinned point 5: its first-rank neighbour 4 is an outlier, the next (1) is kept row 1
    assert not np.array_equal(got, R.raw_index(inverse, keep, idx, wrong="by_index"))
    labels = torch.tensor([10, 11, 12], device=DEV)
    carried = mesh.carry_labels(labels, torch.from_numpy(got).to(DEV)).cpu().numpy()
    assert np.array_equal(carried, R.carry(np.array([10, 11, 12]), got))
