"""GPU tier of the point-cloud front: pbnet_amd.mesh.knn_graph is compared BIT FOR BIT (idx and d2) with the brute force
of tests/cloud_ref.py on every designed case of tests/cloud_cases.py, for k in {1, 6, 16, 32} and for every cell size;
pbnet_amd.mesh.point_normals against float64 covariance + numpy.linalg.eigh within 1e-6."""
import functools

import numpy as np
import pytest
import torch

import cloud_cases as C
import cloud_ref
from pbnet_amd import mesh

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
KMAX = max(C.KS)


@functools.lru_cache(maxsize=None)
def _ref_keys(name):
    """The brute force once per case at k = 32: the key order is total and the padding key sorts last, so the row for a
    smaller k is its prefix (tests/test_cloud_ref_cpu.py checks that of the restatement)."""
    keys = cloud_ref.knn_keys(C.CASES[name][0], KMAX)
    keys.setflags(write=False)
    return keys


def _want(name, k):
    return cloud_ref.split(np.ascontiguousarray(_ref_keys(name)[:, :k]))


def _run(pts, k, cell):
    idx, d2 = mesh.knn_graph(torch.from_numpy(pts).to(DEV), k=k, cell=cell)
    assert idx.dtype == torch.int32 and d2.dtype == torch.float32 and idx.shape == d2.shape == (pts.shape[0], k)
    return idx.cpu().numpy(), d2.cpu().numpy()


def _same(got, want):
    assert np.array_equal(got[0], want[0])
    assert np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32))


@pytest.mark.parametrize("k", C.KS)
@pytest.mark.parametrize("name", sorted(C.CASES))
def test_knn_is_the_brute_force_bit_for_bit(name, k):
    pts, cell = C.CASES[name]
    _same(_run(pts, k, cell), _want(name, k))


@pytest.mark.parametrize("k", C.KS)
def test_padding_at_n_equal_k_and_k_plus_one(k):
    for n in (k, k + 1):
        idx, d2 = _run(C.CASES["n%d" % n][0], k, None)
        _same((idx, d2), _want("n%d" % n, k))
        if n == k:
            assert np.all(idx[:, -1] == -1) and np.all(np.isposinf(d2[:, -1])) and np.all(idx[:, :k - 1] >= 0)
        else:
            assert np.all(idx >= 0) and np.all(np.isfinite(d2))


@pytest.mark.parametrize("k", (6, 16))
@pytest.mark.parametrize("seed", (1, 2, 3))
def test_cell_size_never_changes_the_bytes(seed, k):
    name = "room%d" % seed
    want = _want(name, k)
    for cell in C.ROOM_CELLS:
        _same(_run(C.CASES[name][0], k, cell), want)


def test_other_cells_on_the_awkward_cases():
    for name, cells in (("lattice", (0.5, 1.0, 3.0, None)), ("line", (C.LINE_CELL, 1.0e-6, 7.0)), ("blob", (0.01, 100.0)),
                        ("coincident", (1.0e-30, 1.0e30)), ("offset", (1.0e-4, 0.3))):
        for cell in cells:
            _same(_run(C.CASES[name][0], 16, cell), _want(name, 16))


def test_two_runs_give_the_same_bytes():
    pts = C.CASES["room1"][0]
    a, b = _run(pts, 16, None), _run(pts, 16, None)
    _same(a, b)
    x = torch.from_numpy(pts).to(DEV)
    idx = torch.from_numpy(a[0]).to(DEV)
    n1, n2 = mesh.point_normals(x, idx), mesh.point_normals(x, idx)
    assert torch.equal(n1.view(torch.int32), n2.view(torch.int32))


@pytest.mark.parametrize("name,k", [("n0", 6), ("n2", 1), ("n65", 6)])
def test_timed_entry_gives_the_plain_bytes_and_four_stage_times(name, k):
    """pbn_cloud_knn_timed against pbn_cloud_knn.  n2 at k = 1 is the smallest designed cloud whose automatic grid has
    more than one cell (1 x 3 x 1: h = sqrt(area * k / 2n) is below the y extent); n65 at k = 6 has 2 x 2 x 3 cells and
    more than one wave; n0 takes the entry's short form, which still records every event."""
    x = torch.from_numpy(C.CASES[name][0]).to(DEV)
    plain = mesh.knn_graph(x, k=k)
    times = {}
    timed = mesh.knn_graph(x, k=k, times=times)
    _same(tuple(t.cpu().numpy() for t in timed), tuple(t.cpu().numpy() for t in plain))
    _same(tuple(t.cpu().numpy() for t in timed), _want(name, k))
    assert tuple(times) == mesh.CLOUD_STAGES and len(times) == 4
    assert all(np.isfinite(v) and v >= 0.0 for v in times.values()), times


def test_non_finite_coordinates_raise():
    for bad in (np.nan, np.inf, -np.inf):
        pts = C.CASES["n257"][0].copy()
        pts[100, 1] = bad
        with pytest.raises(ValueError):
            mesh.knn_graph(torch.from_numpy(pts).to(DEV), k=6)
    with pytest.raises(ValueError):
        mesh.knn_graph(torch.from_numpy(C.CASES["n65"][0]).to(DEV), k=33)
    with pytest.raises(ValueError):
        mesh.knn_graph(torch.from_numpy(C.CASES["n65"][0]).to(DEV), k=6, cell=-1.0)


def _normals(name, k, viewpoint):
    pts = C.CASES[name][0]
    idx = _want(name, k)[0]
    got = mesh.point_normals(torch.from_numpy(pts).to(DEV), torch.from_numpy(np.ascontiguousarray(idx)).to(DEV), viewpoint)
    assert got.dtype == torch.float32 and got.shape == (pts.shape[0], 3)
    return pts, idx, got.cpu().numpy().astype(np.float64)


@pytest.mark.parametrize("name,viewpoint", [("room1", None), ("room2", None), ("room3", (2.0, 2.0, 1.5)),
                                            ("sheet", C.SHEET_VIEWPOINT)])
def test_normals_match_eigh(name, viewpoint):
    """Bounds: float32 rounding of a unit vector is 6e-8 per component and the float64 eigenvector error is below 1e-12 at
    a relative gap of 1e-3, so 1e-6 leaves a factor of ten.  Points with a gap below 1e-3 (the eigenvector is ill
    defined) or with the viewpoint within 1e-3 of the tangent plane (the orientation is) are skipped; at most 1 % may be."""
    pts, idx, n = _normals(name, 16, viewpoint)
    ref, gap, m = cloud_ref.normals(pts, idx, viewpoint)
    assert np.all(m == 17)
    p = pts.astype(np.float64)
    vp = (p.mean(0) if viewpoint is None else np.asarray(viewpoint, np.float64)).astype(np.float32).astype(np.float64)
    to_vp = vp[None, :] - p
    facing = np.abs(np.einsum("ij,ij->i", ref, to_vp)) / np.linalg.norm(to_vp, axis=1)
    s = np.sign(np.einsum("ij,ij->i", ref, n))
    checked = (gap >= 1e-3) & (facing >= 1e-3)
    skipped = 1.0 - checked.mean()
    err = np.abs(n - s[:, None] * ref)[checked].max()
    unit = np.abs(np.linalg.norm(n, axis=1) - 1.0).max()
    print("%s: skipped %.4f %%, max |n - s n_ref| %.3e, max | |n| - 1 | %.3e, min gap %.4f" %
          (name, 100 * skipped, err, unit, gap.min()))
    assert skipped <= 0.01
    assert np.all(np.isfinite(n)) and unit <= 1e-6
    assert err <= 1e-6
    assert np.all(s[checked] == 1)


def test_lattice_normals_are_finite_unit_vectors():
    """An inner lattice point's neighbourhood is symmetric: its eigenvalue gaps are exactly zero and no direction is the
    normal, so only finiteness and unit length are checked here."""
    for k in (6, 32):
        _, _, n = _normals("lattice", k, None)
        assert np.all(np.isfinite(n))
        assert np.abs(np.linalg.norm(n, axis=1) - 1.0).max() <= 1e-6


def test_fewer_than_three_points_give_zero_normals():
    for name, zero in (("n1", True), ("n2", True), ("n6", False)):
        _, _, n = _normals(name, 6, None)
        assert np.all(n == 0) == zero
    # a row of -1 among real ones: |S| = 1 for that point only
    pts = C.CASES["n65"][0]
    idx = _want("n65", 6)[0].copy()
    idx[7] = -1
    idx[9, 1:] = -1                                          # |S| = 2
    n = mesh.point_normals(torch.from_numpy(pts).to(DEV), torch.from_numpy(idx).to(DEV)).cpu().numpy()
    assert np.all(n[7] == 0) and np.all(n[9] == 0)
    rest = np.delete(np.arange(65), [7, 9])
    assert np.abs(np.linalg.norm(n[rest].astype(np.float64), axis=1) - 1.0).max() <= 1e-6
    # coincident points: a zero covariance still gives a finite unit vector
    _, _, n = _normals("coincident", 6, None)
    assert np.all(np.isfinite(n)) and np.abs(np.linalg.norm(n, axis=1) - 1.0).max() <= 1e-6
