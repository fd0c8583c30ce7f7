"""CPU tier of the raw-scan front: the numpy restatement (tests/thin_ref.py) against plain Python loops on every designed
case (tests/thin_cases.py), the host argument checks of pbnet_amd.mesh, and for every named mistake of the restatement a
designed case that tells it from the contract -- so the GPU tier, which pins the device to the restatement bit for bit on
the same cases, would catch that mistake in the kernels."""
import numpy as np
import pytest
import torch

import thin_cases as C
import thin_ref as R
from pbnet_amd import mesh


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a.view(np.uint64) if a.dtype == np.float64 else a


def same_thin(a, b):
    return sorted(a) == sorted(b) and all(a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and
                                          np.array_equal(_bits(a[k]), _bits(b[k])) for k in a)


def same_outlier(a, b):
    nan = np.isnan(a[1])                                     # the sign of 0 / 0 is the machine's: NaN equals NaN
    return (np.array_equal(a[0], b[0]) and np.array_equal(nan, np.isnan(b[1])) and
            np.array_equal(_bits(a[1][~nan]), _bits(b[1][~nan])))


@pytest.mark.parametrize("name", sorted(C.THIN))
def test_thin_restatement_is_the_dict_of_cells(name):
    xyz, rgb, pitch = C.THIN[name]
    got = R.thin(xyz, rgb, pitch)
    assert same_thin(got, R.thin_loop(xyz, rgb, pitch))
    n, m = xyz.shape[0], got["xyz"].shape[0]
    assert got["inverse"].shape == (n,) and got["count"].sum() == n and (m > 0) == (n > 0)
    assert np.array_equal(np.bincount(got["inverse"], minlength=m), got["count"])
    assert np.array_equal(got["inverse"][got["first"]], np.arange(m))


def test_thin_cases_have_the_shapes_they_were_designed_for():
    for n in (63, 64, 65, 255, 256, 257):
        assert R.thin(*C.THIN["cell%d" % n])["count"].tolist() == [n]
    assert R.thin(*C.THIN["coincident"])["count"].tolist() == [200]
    assert R.thin(*C.THIN["lattice_1"])["count"].tolist() == [1] * 343          # every point on a cell face, none shared
    assert R.thin(*C.THIN["lattice_half"])["xyz"].shape[0] == 343
    assert C.THIN["negative"][0].max() < 0
    for name, axis in (("far_z", 2), ("far_y", 1)):
        c = R.cells(C.THIN[name][0], 1.0)
        assert c[:, axis].max() >= 1500000 and c[:, axis].min() == 0
    assert R.cells(*C.THIN["extent_max"][::2])[:, 0].max() == (1 << 21) - 1
    for k, pitch in (("room_2cm", 0.02), ("room_5cm", 0.05)):
        got = R.thin(*C.THIN[k])
        assert C.THIN[k][2] == pitch and 1 < got["count"].max() and got["xyz"].shape[0] < 3000
    assert R.thin(*C.THIN["room_5cm"])["xyz"].shape[0] < R.thin(*C.THIN["room_2cm"])["xyz"].shape[0]


@pytest.mark.parametrize("name", sorted(C.THIN_RAISES))
def test_thin_restatement_refuses(name):
    with pytest.raises(ValueError):
        R.thin(C.THIN_RAISES[name][0], None, C.THIN_RAISES[name][1])


def _thin_differs(wrong):
    return [n for n in sorted(C.THIN) if not same_thin(R.thin(*C.THIN[n]), R.thin(*C.THIN[n], wrong=wrong))]


@pytest.mark.parametrize("wrong,must", [("reversed", "order"), ("float32", "room_5cm"), ("xmajor", "lattice_1"),
                                        ("ties", "cell65"), ("low_word", "far_z"), ("low_word", "far_y")])
def test_thin_mistakes_are_told_apart(wrong, must):
    assert wrong in R.THIN_WRONG and must in _thin_differs(wrong)


def test_truncation_cannot_be_told_from_floor():
    """The cell is floor((p - o) / pitch) with o the minimum of the axis: p - o >= 0 and pitch > 0, so the quotient is
    never negative (nor -0.0 / NaN for finite input) and trunc(q) == floor(q) for EVERY input the contract admits,
    negative coordinates included.  No designed case can differ; the equality itself is what is checked here, on every
    case, so that a change of the origin rule that made the difference real would show."""
    assert "trunc" in R.THIN_WRONG and _thin_differs("trunc") == []
    q = (C.THIN["negative"][0].astype(np.float64) - C.THIN["negative"][0].min(0).astype(np.float64)) / 0.25
    assert q.min() == 0.0 and np.array_equal(np.trunc(q), np.floor(q))


# ------------------------------------------------------------------------------------------------------------ outliers
def _outlier_cases():
    c = dict(C.OUTLIER)
    c["far_room"] = (C.far_room_graph()[1], 2.0)
    return c


@pytest.mark.parametrize("name", sorted(_outlier_cases()))
def test_outlier_restatement_is_the_loop(name):
    d2, ratio = _outlier_cases()[name]
    got = R.outlier(d2, ratio)
    assert got[0].dtype == bool and got[0].shape == (d2.shape[0],) and got[1].dtype == np.float64
    assert same_outlier(got, R.outlier_loop(d2, ratio))


def test_outlier_cases_have_the_shapes_they_were_designed_for():
    keep, stats = R.outlier(*C.OUTLIER["exact_threshold"])
    assert stats.tolist() == [2.0, 1.0, 4.0] and keep.tolist() == [True] * 4
    keep, stats = R.outlier(*C.OUTLIER["row_all_inf"])
    assert not keep[7] and not keep[256] and stats[2] == 298
    keep, stats = R.outlier(*C.OUTLIER["only_inf"])
    assert not keep.any() and np.isnan(stats[0]) and np.isnan(stats[1]) and stats[2] == 0
    assert np.isinf(C.OUTLIER["short_rows"][0][0, -5:]).all() and np.isfinite(C.OUTLIER["short_rows"][0][0, :-5]).all()
    keep, stats = R.outlier(*_outlier_cases()["far_room"])
    assert not keep[-30:].any() and keep[:-30].mean() > 0.97          # the far points go, the room stays
    assert R.outlier(np.zeros((0, 16), np.float32))[0].shape == (0,)


@pytest.mark.parametrize("wrong,must", [("sample", "n257_k16"), ("lt", "exact_threshold")])
def test_outlier_mistakes_are_told_apart(wrong, must):
    assert wrong in R.OUTLIER_WRONG
    d2, ratio = C.OUTLIER[must]
    assert not same_outlier(R.outlier(d2, ratio), R.outlier(d2, ratio, wrong=wrong))
    if wrong == "lt":
        assert R.outlier(d2, ratio, wrong=wrong)[0].tolist() == [True, True, False, False]


def test_block_sum_has_the_contracts_shape():
    """1e16 (spacing 2) and two ones: the tree adds v[64] + v[192] = 2 first, a running sum loses each 1 to a tie."""
    v = np.zeros(257)
    v[0], v[64], v[192] = 1e16, 1.0, 1.0
    assert R.block_sum(v) == 1e16 + 2.0 and np.cumsum(v)[-1] == 1e16


# ----------------------------------------------------------------------------------------------------------- raw index
def test_raw_index_cases():
    inverse, keep, idx = C.RAW["designed"]
    want = np.array([0, 2, 2, 1, -1, 1, 2, -1, 1, 0, 2], np.int32)
    #   raw point -> thinned 0 (kept, row 0) | 2 (outlier: first kept neighbour by rank is 3 = row 2) | 5 (first neighbour 4 is
    #   an outlier, the next, 1, is row 1) | 4 (no kept neighbour) | 1 (kept, row 1) | 3 (kept, row 2)
    assert np.array_equal(R.raw_index(inverse, keep, idx), want)
    assert not np.array_equal(R.raw_index(inverse, keep, idx, wrong="by_index"), want) and "by_index" in R.RAW_WRONG
    assert np.all(R.raw_index(*C.RAW["none_kept"]) == -1)
    assert np.array_equal(R.raw_index(*C.RAW["all_kept"]), inverse)
    assert R.raw_index(*C.RAW["empty"]).shape == (0,)
    labels = np.array([[7, 70], [8, 80], [9, 90]], np.int64)
    got = mesh.carry_labels(torch.from_numpy(labels), torch.from_numpy(want), fill=-5).numpy()
    assert np.array_equal(got, R.carry(labels, want, fill=-5)) and np.all(got[want < 0] == -5)
    assert np.array_equal(got[want >= 0], labels[want[want >= 0]])


# -------------------------------------------------------------------------------------------------- host argument checks
def test_host_argument_checks():
    """Refused on the host, before the library or a device is touched (the tensors here live on the CPU, which the device
    entry points refuse next)."""
    x = torch.zeros(4, 3)
    for pitch in (0.0, -0.02, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="pitch"):
            mesh.thin_points(x, None, pitch)
    for ratio in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="ratio"):
            mesh.outlier_mask(torch.zeros(4, 3), ratio)
    with pytest.raises(RuntimeError):
        mesh.thin_points(x, None, 0.02)                      # a CPU tensor: no CPU path
    with pytest.raises(RuntimeError):
        mesh.outlier_mask(torch.zeros(4, 3), 2.0)
    with pytest.raises(RuntimeError):
        mesh.raw_index(torch.zeros(4, dtype=torch.int32), torch.ones(4, dtype=torch.bool), torch.zeros(4, 3, dtype=torch.int32))
    with pytest.raises(TypeError):
        mesh.carry_labels(torch.zeros(3), torch.zeros(3, dtype=torch.int32))
    with pytest.raises(ValueError):
        mesh.decode_points((np.zeros((4, 3), np.float32), np.zeros((4, 3), np.uint8)), return_kept=True)


def test_library_refuses_bad_arguments_before_any_launch():
    """pbn_thin_points / pbn_cloud_outlier_mask check pitch and ratio on the host (the pointers are never dereferenced)."""
    from pbnet_amd import _native as N
    lib, vp, fake = N.lib(), N.c_vp, 1 << 20
    big = 1 << 30

    def thin(pitch, n=8):
        return lib.pbn_thin_points(vp(fake), None, n, pitch, vp(fake), None, vp(fake), vp(fake), vp(fake), vp(fake), vp(fake), big,
                                   None)
    for pitch in (0.0, -1.0, float("nan"), float("inf")):
        assert thin(pitch) == N.PBN_ERR_ARG
    assert thin(0.02, n=-1) == N.PBN_ERR_ARG
    assert lib.pbn_thin_points(vp(fake), None, 8, 0.02, vp(fake), None, vp(fake), vp(fake), vp(fake), vp(fake), vp(fake), 16,
                               None) == N.PBN_ERR_WORKSPACE
    for ratio in (-0.5, float("nan"), float("inf")):
        assert lib.pbn_cloud_outlier_mask(vp(fake), 8, 4, ratio, vp(fake), vp(fake), vp(fake), big, None) == N.PBN_ERR_ARG
    assert lib.pbn_cloud_outlier_mask(vp(fake), 8, 33, 2.0, vp(fake), vp(fake), vp(fake), big, None) == N.PBN_ERR_ARG
    assert lib.pbn_cloud_raw_index(vp(fake), 8, vp(fake), vp(fake), 8, 0, vp(fake), vp(fake), big, None) == N.PBN_ERR_ARG
    assert 0 < lib.pbn_thin_workspace_bytes(1000) < lib.pbn_thin_workspace_bytes(100000)
    assert lib.pbn_thin_workspace_bytes(-1) == 0 and lib.pbn_cloud_outlier_workspace_bytes((1 << 28) + 1) == 0
