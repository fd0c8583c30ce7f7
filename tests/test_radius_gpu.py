"""GPU tier of the fixed-radius queries: pbnet_amd.mesh.radius_count / radius_outlier_mask / radius_raw_index are compared
BIT FOR BIT with the numpy restatement of tests/radius_ref.py on every designed case of that file
(tests/test_radius_ref_cpu.py shows, without a GPU, which case tells each possible mistake from the contract), under every
cell size (the bytes never depend on it) and every cap."""
import functools
import warnings

import numpy as np
import pytest
import torch

import radius_ref as R
from pbnet_amd import mesh

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@functools.lru_cache(maxsize=None)
def _full(name):
    """The restatement's uncapped count, once per case."""
    return R.radius_count_ref(*R.COUNT[name])


def _cell(cell, radius):
    return radius if cell == "radius" else cell


@pytest.mark.parametrize("name", sorted(R.COUNT))
def test_count_is_the_restatement_under_every_cell_and_cap(name):
    xyz, radius = R.COUNT[name]
    x, full = _dev(xyz), _full(name)
    for cell in R.CELLS:
        for cap in R.CAPS:
            got = mesh.radius_count(x, radius, cap=cap, cell=_cell(cell, radius))
            assert got.is_cuda and got.dtype == torch.int32 and got.shape == (xyz.shape[0],)
            want = full if cap is None else np.minimum(full, cap)
            assert np.array_equal(got.cpu().numpy(), want), (cell, cap)


def test_lattice_counts():
    x = _dev(R.COUNT["lattice_r1"][0])
    inner = np.all((R.COUNT["lattice_r1"][0] > 0) & (R.COUNT["lattice_r1"][0] < 11), axis=1)
    for radius, want in ((1.0, 6), (1.5, 18), (R.BELOW_ONE, 0)):
        got = mesh.radius_count(x, radius, cell=1.0).cpu().numpy()          # cell = 1: every point on a cell face
        assert set(got[inner].tolist()) == {want}, radius
    assert mesh.radius_count(_dev(R.COUNT["coincident"][0]), 0.1, cap=7).cpu().tolist() == [7] * 200
    blob = mesh.radius_count(_dev(R.COUNT["blob"][0]), R.COUNT["blob"][1]).cpu().numpy()
    assert blob[-1] == 0 and blob[:-1].min() > 0            # the point 40 cells away is alone


@pytest.mark.parametrize("name", ["n0", "n1", "n257", "coincident", "lattice_r1", "blob", "room_20cm"])
@pytest.mark.parametrize("min_pts", [1, 4])
def test_mask_is_the_restatement(name, min_pts):
    xyz, radius = R.COUNT[name]
    for cell in R.CELLS:
        got = mesh.radius_outlier_mask(_dev(xyz), radius, min_pts, cell=_cell(cell, radius))
        assert got.is_cuda and got.dtype == torch.bool
        assert np.array_equal(got.cpu().numpy(), _full(name) >= min_pts), cell


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), -float("inf")])
def test_non_finite_coordinates_raise(bad):
    xyz = R.COUNT["n257"][0].copy()
    xyz[200, 1] = bad
    with pytest.raises(ValueError, match="NaN or infinite"):
        mesh.radius_count(_dev(xyz), 0.7)
    with pytest.raises(ValueError, match="NaN or infinite"):
        mesh.radius_outlier_mask(_dev(xyz), 0.7, 2)
    keep = torch.ones(257, dtype=torch.bool, device=DEV)
    keep[3] = False
    with pytest.raises(ValueError, match="NaN or infinite"):
        mesh.radius_raw_index(torch.arange(257, dtype=torch.int32, device=DEV), keep, _dev(xyz), 0.7)


@pytest.mark.parametrize("name", sorted(R.ROUTE))
def test_route_is_the_restatement_under_every_cell(name):
    inverse, keep, xyz, radius = R.ROUTE[name]
    want = R.radius_raw_index_ref(inverse, keep, xyz, radius)
    for cell in R.CELLS:
        got = mesh.radius_raw_index(_dev(inverse), _dev(keep), _dev(xyz), radius, cell=_cell(cell, radius))
        assert got.is_cuda and got.dtype == torch.int32 and got.shape == inverse.shape
        assert np.array_equal(got.cpu().numpy(), want), cell


def test_route_follows_the_devices_own_mask():
    xyz, radius = R.COUNT["room_20cm"]
    keep = mesh.radius_outlier_mask(_dev(xyz), radius, 6)
    inverse = np.random.default_rng(5).integers(0, xyz.shape[0], 4000).astype(np.int32)
    got = mesh.radius_raw_index(_dev(inverse), keep, _dev(xyz), radius).cpu().numpy()
    k = keep.cpu().numpy()
    assert 0 < (~k).sum() < k.shape[0] // 2 and np.array_equal(k, R.radius_mask_ref(xyz, radius, 6))
    assert np.array_equal(got, R.radius_raw_index_ref(inverse, k, xyz, radius))


def test_points_outside_the_kept_cloud_route_nowhere():
    inverse, keep, xyz, radius = R.ROUTE["one_kept"]
    odd = np.array([0, -1, 3, 1, 2 ** 31 - 1, -2 ** 31], np.int32)           # rows the M points do not have
    got = mesh.radius_raw_index(_dev(odd), _dev(keep), _dev(xyz), radius).cpu().tolist()
    assert got == [0, -1, -1, 0, -1, -1]
    none = mesh.radius_raw_index(_dev(inverse), torch.zeros(0, dtype=torch.bool, device=DEV),
                                 torch.zeros(0, 3, device=DEV), radius)       # no points at all
    assert none.cpu().tolist() == [-1, -1, -1]


def test_two_runs_give_the_same_bytes():
    for name in ("room_5cm", "lattice_r1.5", "line"):
        xyz, radius = R.COUNT[name]
        a, b = (mesh.radius_count(_dev(xyz), radius).cpu().numpy() for _ in range(2))
        assert a.tobytes() == b.tobytes(), name
    inverse, keep, xyz, radius = R.ROUTE["room"]
    a, b = (mesh.radius_raw_index(_dev(inverse), _dev(keep), _dev(xyz), radius).cpu().numpy() for _ in range(2))
    assert a.tobytes() == b.tobytes()


def _syncs(fn):
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as seen:
            warnings.simplefilter("always")
            out = fn()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    return out, len([w for w in seen if "synchroniz" in str(w.message).lower()])


def test_one_read_back_per_function_and_the_timed_entry_gives_the_same_bytes():
    inverse, keep, xyz, radius = R.ROUTE["room"]
    x, inv, kp = _dev(xyz), _dev(inverse), _dev(keep)
    plain = mesh.radius_count(x, radius, cap=9)              # first use: the library and its kernels are loaded
    mesh.radius_raw_index(inv, kp, x, radius)
    again, n = _syncs(lambda: mesh.radius_count(x, radius, cap=9))
    assert n == 1 and torch.equal(plain, again)
    mask, n = _syncs(lambda: mesh.radius_outlier_mask(x, radius, 4))
    assert n == 1 and mask.dtype == torch.bool
    _, n = _syncs(lambda: mesh.radius_raw_index(inv, kp, x, radius))
    assert n == 1
    times = {}
    timed = mesh.radius_count(x, radius, cap=9, times=times)
    assert torch.equal(plain, timed)
    assert sorted(times) == sorted(mesh.RADIUS_STAGES) and all(t >= 0.0 for t in times.values())
