"""pbnet_amd.mesh.orient_normals (csrc/orient.hip) on the GPU: every output equals the numpy restatement
(tests/orient_ref.py: a sequential Kruskal) bit for bit on every designed case, two runs give the same bytes, and the
argument checks raise.  The forest is unique under the strict edge order, so the device's Boruvka rounds have nothing to
choose."""
import numpy as np
import pytest
import torch

import orient_ref as R
from pbnet_amd import mesh

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
KEYS = ("nl", "flipped", "tree", "stats")


def _run(nl, idx, **kw):
    out = mesh.orient_normals(torch.from_numpy(np.ascontiguousarray(nl)).to(DEV),
                              torch.from_numpy(np.ascontiguousarray(idx)).to(DEV), **kw)
    assert all(out[k].is_cuda for k in KEYS)
    return {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in out.items()}


def _assert_same(got, want, what):
    assert got["nl"].dtype == np.float32 and got["flipped"].dtype == bool and got["tree"].dtype == np.int32
    assert got["stats"].dtype == np.int32 and got["stats"].shape == (4,)
    for k in KEYS:
        assert got[k].shape == want[k].shape and got[k].tobytes() == want[k].tobytes(), (what, k)


@pytest.mark.parametrize("name", sorted(R.cases()))
def test_every_output_is_the_restatement(name):
    nl, idx = R.cases()[name]
    _assert_same(_run(nl, idx), R.want(name), name)


@pytest.mark.parametrize("name", ["n257_k16", "chain", "islands", "null_mixed"])
def test_two_runs_give_the_same_bytes(name):
    nl, idx = R.cases()[name]
    a, b = _run(nl, idx), _run(nl, idx)
    for k in KEYS:
        assert a[k].tobytes() == b[k].tobytes(), k
    assert a["rounds"] == b["rounds"]


def test_rounds_are_reported_and_bounded():
    for name in ("n0", "n1", "all_null"):
        assert _run(*R.cases()[name])["rounds"] == 0
    assert _run(*R.cases()["n2"])["rounds"] == 1
    nl, idx = R.cases()["chain"]
    assert 1 <= _run(nl, idx)["rounds"] <= 12                                # ceil(log2(4096))
    assert _run(*R.cases()["n257_k16"])["rounds"] == len(R.boruvka(*R.cases()["n257_k16"])[1])


def test_stage_times():
    nl, idx = R.cases()["n257_k16"]
    times = {}
    got = _run(nl, idx, times=times)
    assert list(times) == list(mesh.ORIENT_STAGES) and len(times) == 3 and all(t >= 0.0 for t in times.values())
    _assert_same(got, R.want("n257_k16"), "timed entry")


def test_arguments_are_checked():
    nl = torch.zeros(8, 3, device=DEV)
    for k in (0, 33):
        with pytest.raises(ValueError):
            mesh.orient_normals(nl, torch.zeros(8, k, dtype=torch.int32, device=DEV))
    with pytest.raises(RuntimeError):
        mesh.orient_normals(nl.cpu(), torch.zeros(8, 4, dtype=torch.int32))
    with pytest.raises(RuntimeError):
        mesh.orient_normals(nl, torch.zeros(8, 4, dtype=torch.int32))
    with pytest.raises(TypeError):
        mesh.orient_normals(nl, torch.zeros(8, 4, dtype=torch.int64, device=DEV))
    with pytest.raises(TypeError):
        mesh.orient_normals(nl, torch.zeros(7, 4, dtype=torch.int32, device=DEV))
