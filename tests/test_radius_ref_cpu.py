"""CPU tier of the fixed-radius queries: the numpy restatement (tests/radius_ref.py) against plain Python double loops on
every designed case, the host argument checks of pbnet_amd.mesh and of the library, and for every named mistake of the
restatement a designed case that tells it from the contract -- so the GPU tier (tests/test_radius_gpu.py), which pins the
device to the restatement bit for bit on the same cases, would catch that mistake in the kernels."""
import numpy as np
import pytest
import torch

import radius_ref as R
from pbnet_amd import mesh

LOOP_ROWS = 24           # the double loop answers this many evenly spread queries of a large case, each against every point


def _rows(n):
    return range(n) if n <= 300 else sorted(set(np.linspace(0, n - 1, LOOP_ROWS).astype(int).tolist()) | {n - 1})


@pytest.mark.parametrize("name", sorted(R.COUNT))
def test_count_restatement_is_the_double_loop(name):
    xyz, radius = R.COUNT[name]
    rows = _rows(xyz.shape[0])
    for cap in R.CAPS:
        got = R.radius_count_ref(xyz, radius, cap)
        assert got.dtype == np.int32 and got.shape == (xyz.shape[0],)
        want = R.radius_count_loop(xyz, radius, cap, rows=rows)
        assert [int(got[i]) for i in rows] == [want[i] for i in rows], cap
    full = R.radius_count_ref(xyz, radius)
    for m in (1, 4):
        assert np.array_equal(R.radius_count_ref(xyz, radius, m), np.minimum(full, m))
        assert np.array_equal(R.radius_mask_ref(xyz, radius, m), full >= m)


def test_count_cases_have_the_shapes_they_were_designed_for():
    count = {k: R.radius_count_ref(*v) for k, v in R.COUNT.items()}
    assert count["n0"].shape == (0,) and count["n1"].tolist() == [0] and count["n2"].tolist() == [1, 1]
    assert count["coincident"].tolist() == [199] * 200
    assert R.r2_of(R.COUNT["coincident_r2_zero"][1]) == 0 and count["coincident_r2_zero"].tolist() == [199] * 400
    lat = R.COUNT["lattice_r1"][0]
    inner = np.all((lat > 0) & (lat < 11), axis=1)
    assert inner.sum() == 1000
    assert set(count["lattice_r1"][inner].tolist()) == {6} and count["lattice_r1"].min() == 3
    assert set(count["lattice_r1.5"][inner].tolist()) == {18}
    assert R.BELOW_ONE < 1.0 and not count["lattice_below1"].any()
    assert np.ptp(R.COUNT["sheet"][0][:, 2]) == 0 and count["sheet"].max() > 10
    assert count["blob"][-1] == 0 and count["blob"][:-1].min() > 0
    assert np.ptp(R.COUNT["line"][0][:, 2]) > 9000 and count["line"].max() <= 1
    assert np.abs(R.COUNT["offset"][0]).min() > 990 and count["offset"].max() > 4
    assert 0 < count["room_5cm"].mean() < count["room_20cm"].mean() and (count["room_5cm"] == 0).any()
    assert count["room_5cm"][777] >= 1 and count["room_5cm"][-1] >= 1          # the coincident pair
    for name, up in (("r2_rounds_up", True), ("r2_rounds_down", False)):
        xyz, radius = R.COUNT[name]
        rf = np.float32(radius)
        assert float(rf) == radius and R.d2_scalar(xyz[1], xyz[0]) == R.r2_of(radius)        # the pair sits exactly at r2
        assert (np.float64(R.r2_of(radius)) > np.float64(rf) * np.float64(rf)) == up
        assert count[name].tolist() == [1, 1]


def _count_differs(wrong, cap=None):
    return [n for n in sorted(R.COUNT) if not np.array_equal(R.radius_count_ref(*R.COUNT[n], cap=cap),
                                                             R.radius_count_ref(*R.COUNT[n], cap=cap, wrong=wrong))]


@pytest.mark.parametrize("wrong,cap,must", [("lt", None, "lattice_r1"), ("lt", None, "coincident_r2_zero"),
                                            ("self", None, "n1"), ("self", None, "room_5cm"),
                                            ("nocap", 4, "coincident"), ("nocap", 1, "lattice_r1.5"),
                                            ("r2_f64", None, "r2_rounds_up"), ("d2_f64", None, "r2_rounds_down")])
def test_count_mistakes_are_told_apart(wrong, cap, must):
    assert wrong in R.COUNT_WRONG and must in _count_differs(wrong, cap)


@pytest.mark.parametrize("name", sorted(R.ROUTE))
def test_route_restatement_is_the_double_loop(name):
    inverse, keep, xyz, radius = R.ROUTE[name]
    got = R.radius_raw_index_ref(inverse, keep, xyz, radius)
    assert got.dtype == np.int32 and got.shape == inverse.shape
    some = inverse if inverse.shape[0] <= 300 else inverse[np.flatnonzero(~keep[inverse])[:LOOP_ROWS]]
    pick = np.arange(inverse.shape[0]) if inverse.shape[0] <= 300 else np.flatnonzero(~keep[inverse])[:LOOP_ROWS]
    assert np.array_equal(got[pick], R.radius_raw_index_loop(some, keep, xyz, radius))
    kept = keep[inverse]
    assert np.array_equal(got[kept], (np.cumsum(keep) - keep)[inverse[kept]])
    assert got.max(initial=-1) < keep.sum()


def test_route_cases_have_the_shapes_they_were_designed_for():
    route = {k: R.radius_raw_index_ref(*v).tolist() for k, v in R.ROUTE.items()}
    assert route["one_kept"] == [0, 0, 1]
    assert route["none_within"] == [-1, 0, 1]
    assert route["tie"] == [0, 1, 2, 1]                      # two kept points at the same d2: the lower index
    assert route["nearest_is_dropped"] == [0, 1, 1, 1]       # 2 and 3 are each other's nearest and both dropped
    assert route["at_r2"] == [0, 0]
    assert route["all_kept"] == list(range(65)) and route["none_kept"] == [-1] * 65
    assert route["repeated_rows"] == [1, 1, 0, 0, 0, 1, 0, 1, 1] and route["n_raw0"] == []
    inverse, keep, _, _ = R.ROUTE["room"]
    got = np.array(route["room"])
    assert 0.1 < (~keep).mean() < 0.5 and (got[~keep[inverse]] >= 0).sum() > 300 and (got == -1).sum() > 0


def _route_differs(wrong):
    return [n for n in sorted(R.ROUTE) if not np.array_equal(R.radius_raw_index_ref(*R.ROUTE[n]),
                                                             R.radius_raw_index_ref(*R.ROUTE[n], wrong=wrong))]


@pytest.mark.parametrize("wrong,must", [("lt", "at_r2"), ("any", "nearest_is_dropped"), ("tie_high", "tie"),
                                        ("beyond", "none_within"), ("rank_all", "one_kept")])
def test_route_mistakes_are_told_apart(wrong, must):
    assert wrong in R.ROUTE_WRONG and must in _route_differs(wrong)


def test_restatement_refuses():
    xyz = R.COUNT["n65"][0]
    for radius in (0.0, -1.0, float("nan"), float("inf"), 1e-50, 1e39):       # the last two are 0 and inf as float32
        with pytest.raises(ValueError):
            R.radius_count_ref(xyz, radius)
    for cap in (0, -3, 1 << 31):
        with pytest.raises(ValueError):
            R.radius_count_ref(xyz, 1.0, cap)
    with pytest.raises(ValueError):
        R.radius_mask_ref(xyz, 1.0, 0)


# -------------------------------------------------------------------------------------------------- host argument checks
def test_host_argument_checks():
    """Refused on the host, before the library or a device is touched (the tensors here live on the CPU, which the device
    entry points refuse next)."""
    x = torch.zeros(4, 3)
    inv, keep = torch.zeros(4, dtype=torch.int32), torch.ones(4, dtype=torch.bool)
    for radius in (0.0, -0.5, float("nan"), float("inf"), 1e-50, 1e39):
        with pytest.raises(ValueError, match="radius"):
            mesh.radius_count(x, radius)
        with pytest.raises(ValueError, match="radius"):
            mesh.radius_outlier_mask(x, radius, 4)
        with pytest.raises(ValueError, match="radius"):
            mesh.radius_raw_index(inv, keep, x, radius)
    for cap in (0, -1, 1 << 31, 2.5, True):
        with pytest.raises(ValueError, match="cap"):
            mesh.radius_count(x, 1.0, cap=cap)
        with pytest.raises(ValueError, match="min_pts"):
            mesh.radius_outlier_mask(x, 1.0, cap)
    with pytest.raises(ValueError, match="min_pts"):
        mesh.radius_outlier_mask(x, 1.0, None)
    for cell in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="cell"):
            mesh.radius_count(x, 1.0, cell=cell)
    for bad in (x.double(), torch.zeros(4, 2), torch.zeros(12), np.zeros((4, 3), np.float32)):
        with pytest.raises(TypeError, match="xyz"):
            mesh.radius_count(bad, 1.0)
        with pytest.raises(TypeError, match="xyz"):
            mesh.radius_raw_index(inv, keep, bad, 1.0)
    with pytest.raises(TypeError, match="inverse"):
        mesh.radius_raw_index(inv.long(), keep, x, 1.0)
    with pytest.raises(TypeError, match="keep"):
        mesh.radius_raw_index(inv, keep.to(torch.uint8), x, 1.0)
    with pytest.raises(TypeError, match="keep"):
        mesh.radius_raw_index(inv, keep[:3], x, 1.0)
    with pytest.raises(RuntimeError):
        mesh.radius_count(x, 1.0)                            # a CPU tensor: no CPU path
    with pytest.raises(RuntimeError):
        mesh.radius_raw_index(inv, keep, x, 1.0)
    scan = (np.zeros((4, 3), np.float32), np.zeros((4, 3), np.uint8))
    with pytest.raises(ValueError, match="outlier_min_pts"):
        mesh.decode_points(scan, outlier_radius=0.05)
    with pytest.raises(ValueError, match="outlier_radius"):
        mesh.decode_points(scan, outlier_min_pts=4)
    with pytest.raises(ValueError, match="outlier_ratio"):
        mesh.decode_points(scan, outlier_radius=0.05, outlier_min_pts=4, outlier_ratio=2.0)


def test_library_refuses_bad_arguments_before_any_launch():
    """The entry points check sizes, radius, cap and pointers on the host (the pointers are never dereferenced)."""
    from pbnet_amd import _native as N
    lib, vp, fake, big, over = N.lib(), N.c_vp, 1 << 20, 1 << 40, (1 << 28) + 1

    def count(n=8, radius=0.1, cap=4, xyz=vp(fake), out=vp(fake), status=vp(fake), ws=vp(fake), nbytes=big, timed=False):
        args = (xyz, n, radius, cap, 0.0, out, status, ws, nbytes, None)
        if timed:
            return lib.pbn_cloud_radius_count_timed(*args, None)
        return lib.pbn_cloud_radius_count(*args)

    def route(n=8, n_raw=8, radius=0.1, xyz=vp(fake), keep=vp(fake), inverse=vp(fake), out=vp(fake), status=vp(fake), ws=vp(fake),
              nbytes=big):
        return lib.pbn_cloud_radius_raw_index(xyz, n, keep, radius, 0.0, inverse, n_raw, out, status, ws, nbytes, None)

    for radius in (0.0, -1.0, float("nan"), float("inf")):
        assert count(radius=radius) == N.PBN_ERR_ARG and route(radius=radius) == N.PBN_ERR_ARG
    assert count(cap=0) == N.PBN_ERR_ARG and count(cap=-1) == N.PBN_ERR_ARG
    assert count(n=-1) == N.PBN_ERR_ARG and count(n=over) == N.PBN_ERR_ARG
    assert route(n=-1) == N.PBN_ERR_ARG and route(n_raw=-1) == N.PBN_ERR_ARG and route(n_raw=over) == N.PBN_ERR_ARG
    for missing in ("xyz", "out", "status", "ws"):
        assert count(**{missing: None}) == N.PBN_ERR_ARG, missing
    for missing in ("xyz", "keep", "inverse", "out", "status", "ws"):
        assert route(**{missing: None}) == N.PBN_ERR_ARG, missing
    assert count(timed=True) == N.PBN_ERR_ARG                 # no times_ms
    assert count(nbytes=16) == N.PBN_ERR_WORKSPACE and route(nbytes=16) == N.PBN_ERR_WORKSPACE
    # the count's workspace is the kNN front's; the routing adds its own rows; both refuse a size out of range with 0
    for n in (0, 1, 257, 100000):
        assert lib.pbn_cloud_radius_workspace_bytes(n) == lib.pbn_cloud_workspace_bytes(n, 1)
        assert lib.pbn_cloud_radius_raw_index_workspace_bytes(n, 5) > lib.pbn_cloud_radius_workspace_bytes(n)
    assert lib.pbn_cloud_radius_workspace_bytes(over) == 0 and lib.pbn_cloud_radius_workspace_bytes(-1) == 0
    assert lib.pbn_cloud_radius_raw_index_workspace_bytes(over, 1) == 0
    assert lib.pbn_cloud_radius_raw_index_workspace_bytes(1, over) == 0
    assert lib.pbn_cloud_radius_raw_index_workspace_bytes(1 << 28, 1 << 28) > 0
