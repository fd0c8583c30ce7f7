"""pbnet_amd.mesh.fit_plane / upright (csrc/upright.hip) on the GPU against the numpy twin (tests/upright_ref.py), for every
designed case and every hypothesis count: info, plane0 and moments bit for bit; the refit normal within point_normals'
bound against numpy.linalg.eigh; R, xyz, height and floor bit for bit the twin's rotation and apply stages fed the
device's own plane.  Two runs and two launch geometries give the same bytes."""
import numpy as np
import pytest
import torch

import upright_ref as U
from pbnet_amd import _native as N
from pbnet_amd import mesh

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
KEYS = ("plane", "plane0", "floor", "height", "moments", "info", "R", "xyz")
# tests/test_cloud_gpu.py test_normals_match_eigh: the Jacobi eigenvector against numpy.linalg.eigh within 1e-6 wherever
# the relative eigenvalue gap is at least 1e-3 (below that the eigenvector is ill defined)
EIGH_TOL, EIGH_GAP = 1e-6, 1e-3


def _run(name, n_hyp, fn=mesh.upright, **extra):
    xyz, t, kw = U.cases()[name]
    out = fn(torch.from_numpy(xyz).to(DEV), t, hypotheses=n_hyp, **dict(kw, **extra))
    return {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in out.items()}


def _same(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), what


def _check(name, n_hyp, got):
    xyz, t, _ = U.cases()[name]
    want = U.want(name, n_hyp)
    assert got["found"] == bool(want["info"][0]) and got["hypothesis"] == want["info"][1] and got["inliers"] == want["info"][2]
    _same(got["info"], want["info"], (name, n_hyp, "info"))
    _same(got["plane0"], want["plane0"], (name, n_hyp, "plane0"))
    _same(got["moments"], want["moments"], (name, n_hyp, "moments"))
    plane, R = got["plane"], got["R"]
    assert plane.dtype == np.float64 and R.dtype == np.float64 and R.shape == (3, 3)
    if want["info"][0] and want["moments"][0] >= 3:
        m = want["moments"]
        cov = np.array([[m[4], m[5], m[6]], [m[5], m[7], m[8]], [m[6], m[8], m[9]]])
        w, v = np.linalg.eigh(cov)
        assert abs(np.linalg.norm(plane[:3]) - 1.0) <= EIGH_TOL
        assert np.dot(plane[:3], want["plane0"][:3].astype(np.float64)) >= 0.0
        if (w[1] - w[0]) >= EIGH_GAP * max(w[2], 1e-300):
            ref = v[:, 0] * np.sign(np.dot(v[:, 0], plane[:3]))
            assert np.abs(plane[:3] - ref).max() <= EIGH_TOL, (name, n_hyp)
        assert abs(plane[3] + np.dot(plane[:3], m[1:4])) <= EIGH_TOL * (1.0 + np.abs(m[1:4]).max())
    else:
        _same(plane, want["plane"], (name, n_hyp, "plane"))
    if want["info"][0]:
        _same(R.reshape(9), U.rotation_ref(plane), (name, n_hyp, "R"))
        out, floor, height = U.apply_ref(xyz, plane, R, t)
    else:
        _same(R, np.eye(3), (name, n_hyp, "R"))
        out, floor, height = xyz, np.zeros(xyz.shape[0], bool), np.zeros(xyz.shape[0], np.float32)
    _same(got["xyz"], out, (name, n_hyp, "xyz"))
    _same(got["floor"], floor, (name, n_hyp, "floor"))
    _same(got["height"], height, (name, n_hyp, "height"))
    return np.array_equal(plane, want["plane"])


@pytest.mark.parametrize("n_hyp", U.HYPOTHESES)
@pytest.mark.parametrize("name", sorted(U.cases()))
def test_every_output_is_the_restatement(name, n_hyp):
    exact = _check(name, n_hyp, _run(name, n_hyp))
    print("%s H=%d: refit plane %s the twin's Jacobi" % (name, n_hyp, "bit-equal to" if exact else "differs from"))


def test_constants_are_the_kernels():
    lib = N.lib()
    assert lib.pbn_cloud_upright_chunk() == U.SCORE_CHUNK and lib.pbn_cloud_upright_hyp_block() == U.HYP_BLOCK
    assert lib.pbn_cloud_upright_max_hyp() == U.MAX_HYP == mesh.UPRIGHT_MAX_HYP


@pytest.mark.parametrize("name", ["room", "two_slabs", "slab1025", "on_threshold"])
def test_two_runs_give_the_same_bytes(name):
    a, b = _run(name, 1024), _run(name, 1024)
    for k in KEYS:
        _same(a[k], b[k], (name, k))


def test_seed_changes_the_hypotheses():
    a, b = _run("room", 64, seed=1), _run("room", 64, seed=2)
    assert a["plane0"].tobytes() != b["plane0"].tobytes()
    xyz, t, kw = U.cases()["room"]
    for seed, got in ((1, a), (2, b)):
        want = U.upright_ref(xyz, t, 64, **dict(kw, seed=seed))
        _same(got["info"], want["info"], seed)
        _same(got["plane0"], want["plane0"], seed)


@pytest.mark.parametrize("chunk", [1, 7, 256, 1000, 2048])
def test_launch_geometry_changes_nothing(chunk):
    xyz, t, kw = U.cases()["room"]
    kw = U._kw(kw)
    got = mesh._upright("upright", True, torch.from_numpy(xyz).to(DEV), t, 257, kw["seed"], kw["up_hint"], kw["max_tilt"],
                        kw["below_frac"], None, chunk=chunk)
    want = _run("room", 257)
    for k in KEYS:
        _same(got[k].cpu().numpy(), want[k], (chunk, k))


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), float("-inf")])
@pytest.mark.parametrize("where", [0, 1500, -1])
def test_nonfinite_coordinate_raises(bad, where):
    xyz = U.cases()["room"][0].copy()
    xyz[where, 1] = bad
    for fn in (mesh.fit_plane, mesh.upright):
        with pytest.raises(ValueError, match="NaN or infinite"):
            fn(torch.from_numpy(xyz).to(DEV), 0.02, hypotheses=64)
    two = np.array([[0, 0, 0], [bad, 0, 0]], np.float32)     # no hypothesis is alive: the points are still read
    with pytest.raises(ValueError, match="NaN or infinite"):
        mesh.fit_plane(torch.from_numpy(two).to(DEV), 0.02, hypotheses=1)


@pytest.mark.parametrize("name", ["n0", "n1", "n2", "coincident", "collinear"])
def test_not_found_is_the_identity(name):
    xyz = U.cases()[name][0]
    got = _run(name, 1024)
    assert got["found"] is False and got["hypothesis"] == 0 and got["inliers"] == 0
    assert not got["info"].any() and not got["plane"].any() and not got["moments"].any() and not got["plane0"].any()
    _same(got["R"], np.eye(3), name)
    _same(got["xyz"], xyz, name)
    assert not got["floor"].any() and not got["height"].any()


@pytest.mark.parametrize("name", ["room", "table", "n2", "slab257"])
def test_fit_plane_and_upright_agree(name):
    a, b = _run(name, 1024, fn=mesh.fit_plane), _run(name, 1024)
    assert set(b) - set(a) == {"R", "xyz"}
    for k in a:
        _same(a[k], b[k], (name, k))


def test_stage_times():
    times = {}
    got = _run("room", 1024, times=times)
    assert list(times) == list(mesh.UPRIGHT_STAGES) and all(v >= 0.0 for v in times.values())
    _check("room", 1024, got)


def test_library_refuses_bad_sizes():
    lib = N.lib()
    assert lib.pbn_cloud_upright_workspace_bytes(-1, 16) == 0 and lib.pbn_cloud_upright_workspace_bytes((1 << 28) + 1, 16) == 0
    assert lib.pbn_cloud_upright_workspace_bytes(8, 0) == 0 and lib.pbn_cloud_upright_workspace_bytes(8, 4097) == 0
    xyz = torch.zeros(8, 3, device=DEV)
    with pytest.raises(RuntimeError):
        mesh._upright("upright", True, xyz, 0.02, 16, 0, None, 30.0, 0.01, None, chunk=4096)
