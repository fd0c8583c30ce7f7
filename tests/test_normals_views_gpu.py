"""point_normals(views=, view_of=) on the GPU: bit for bit tests/frames_ref.py's normals_views_ref on a 300-point cloud with
three views, view_of entries outside the range and neighbourhoods of fewer than three points; with all views equal it is
point_normals(viewpoint=) byte for byte."""
import numpy as np
import pytest
import torch

import cloud_ref
import frames_ref as R
from pbnet_amd import mesh

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
N_POINTS, K = 300, 8
VIEWS = np.array([[0.0, 0.0, 3.0], [4.0, -1.0, 0.5], [-2.0, 2.5, -1.0]], np.float32)


@pytest.fixture(scope="module")
def cloud():
    rng = np.random.default_rng(41)
    floor = np.concatenate([rng.uniform(-1, 1, (150, 2)), rng.normal(0, 0.01, (150, 1))], axis=1)
    wall = np.concatenate([rng.normal(1.0, 0.01, (150, 1)), rng.uniform(-1, 1, (150, 2))], axis=1)
    xyz = np.concatenate([floor, wall]).astype(np.float32)
    idx = np.ascontiguousarray(cloud_ref.knn(xyz, K)[0].astype(np.int32))
    idx[5, :] = -1                                             # |S| = 1
    idx[6, 1:] = -1                                            # |S| = 2
    idx[7, 2:] = -1                                            # |S| = 3: the smallest neighbourhood with a normal
    idx[8, ::2] = N_POINTS                                     # out of range is no neighbour either
    view_of = rng.integers(0, 3, N_POINTS).astype(np.int32)
    view_of[[10, 11, 12, 13]] = (-1, 3, 100, -(2 ** 31))       # outside [0, 3): the sign stays
    return xyz, idx, view_of


def _run(xyz, idx, **kw):
    kw = {k: torch.from_numpy(v).to(DEV) if isinstance(v, np.ndarray) else v for k, v in kw.items()}
    return mesh.point_normals(torch.from_numpy(xyz).to(DEV), torch.from_numpy(idx).to(DEV), **kw).cpu().numpy()


def test_views_are_the_restatement_bit_for_bit(cloud):
    xyz, idx, view_of = cloud
    got = _run(xyz, idx, views=VIEWS, view_of=view_of)
    want = R.normals_views_ref(xyz, idx, VIEWS, view_of)
    assert got.dtype == np.float32 and got.shape == (N_POINTS, 3)
    assert got.tobytes() == want.tobytes()
    assert not got[5].any() and not got[6].any() and got[7].any()
    seen = view_of[(view_of >= 0) & (view_of < 3)]
    assert set(seen.tolist()) == {0, 1, 2}
    ok = (view_of >= 0) & (view_of < 3) & got.any(axis=1)
    to_view = VIEWS[view_of[ok]].astype(np.float64) - xyz[ok].astype(np.float64)
    assert np.all(np.einsum("ij,ij->i", got[ok].astype(np.float64), to_view) >= -1e-6)
    flips = np.einsum("ij,ij->i", got, _run(xyz, idx, viewpoint=tuple(VIEWS[0]))) < 0
    assert flips.any()                                         # three views do turn some normals another way than one


def test_equal_views_are_the_single_viewpoint_bytes(cloud):
    xyz, idx, view_of = cloud
    inside = np.where((view_of >= 0) & (view_of < 3), view_of, 0).astype(np.int32)
    for v in VIEWS:
        got = _run(xyz, idx, views=np.tile(v, (3, 1)), view_of=inside)
        assert got.tobytes() == _run(xyz, idx, viewpoint=tuple(float(a) for a in v)).tobytes()


def test_no_view_keeps_the_eigenvector_sign(cloud):
    xyz, idx, _ = cloud
    nobody = np.full(N_POINTS, -1, np.int32)
    got = _run(xyz, idx, views=VIEWS, view_of=nobody)
    assert got.tobytes() == R.normals_views_ref(xyz, idx, VIEWS, nobody).tobytes()
    assert got.tobytes() == _run(xyz, idx, views=np.zeros((0, 3), np.float32), view_of=nobody).tobytes()
