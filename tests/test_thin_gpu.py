"""GPU tier of grid thinning: pbnet_amd.mesh.thin_points is compared BIT FOR BIT (xyz, rgb, count, first, inverse) with the
numpy restatement of tests/thin_ref.py on every designed case of tests/thin_cases.py (tests/test_thin_ref_cpu.py shows,
without a GPU, which case tells each possible mistake from the contract)."""
import functools

import numpy as np
import pytest
import torch

import thin_cases as C
import thin_ref as R
from pbnet_amd import mesh
from test_thin_ref_cpu import same_thin

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def _want(name):
    return R.thin(*C.THIN[name])


def _run(xyz, rgb, pitch, **kw):
    got = mesh.thin_points(torch.from_numpy(xyz).to(DEV), None if rgb is None else torch.from_numpy(rgb).to(DEV), pitch, **kw)
    assert all(v.is_cuda for v in got.values())
    return {k: v.cpu().numpy() for k, v in got.items()}


@pytest.mark.parametrize("name", sorted(C.THIN))
def test_thin_is_the_restatement_bit_for_bit(name):
    got, want = _run(*C.THIN[name]), _want(name)
    for k in want:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
    assert same_thin(got, want)


@pytest.mark.parametrize("name", sorted(C.THIN_RAISES))
def test_thin_refuses(name):
    xyz, pitch = C.THIN_RAISES[name]
    with pytest.raises(ValueError):
        _run(xyz, None, pitch)
    with pytest.raises(ValueError):
        _run(xyz, np.zeros_like(xyz), pitch)


def test_the_high_key_word_decides():
    """The device agrees with the full (key, index) order on the two far-cluster cases, and the restatement sorted by the
    low key word alone does not: a device that skipped the second sort would fail here."""
    for name in ("far_z", "far_y"):
        got = _run(*C.THIN[name])
        assert same_thin(got, _want(name)) and not same_thin(got, R.thin(*C.THIN[name], wrong="low_word"))


def test_float64_order_matters_and_is_the_contracts():
    got = _run(*C.THIN["order"])
    assert same_thin(got, _want("order")) and not same_thin(got, R.thin(*C.THIN["order"], wrong="reversed"))


def test_two_runs_and_the_timed_entry_give_the_same_bytes():
    a, b = _run(*C.THIN["room_5cm"]), _run(*C.THIN["room_5cm"])
    assert same_thin(a, b)
    times = {}
    assert same_thin(a, _run(*C.THIN["room_5cm"], times=times))
    assert sorted(times) == sorted(mesh.THIN_STAGES) and all(t >= 0.0 for t in times.values())
