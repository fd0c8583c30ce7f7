"""CPU tier of the point-cloud front (pbnet_amd.mesh.knn_graph / point_normals / decode_points): the numpy restatement
tests/cloud_ref.py against a second, independent statement; the designed cases of tests/cloud_cases.py have the properties
they are named for; the host-side argument checks of the two entry points; the vertex-only PLY reader."""
import os

import numpy as np
import pytest
import torch

import cloud_cases as C
import cloud_ref
import mesh_ref
from pbnet_amd import _native as N
from pbnet_amd import mesh

HERE = os.path.dirname(os.path.abspath(__file__))


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("name,k", [("n0", 6), ("n1", 1), ("n2", 6), ("n7", 6), ("n65", 16), ("coincident", 6),
                                    ("lattice5", 32), ("offset200", 6)])
def test_restatement_agrees_with_the_row_loop(name, k):
    pts = {"lattice5": C.lattice(5), "offset200": C.offset(200)}.get(name)
    if pts is None:
        pts = C.CASES[name][0]
    i1, d1 = cloud_ref.knn(pts, k)
    i2, d2 = cloud_ref.knn_loop(pts, k)
    assert i1.dtype == np.int32 and d1.dtype == np.float32 and i1.shape == (pts.shape[0], k)
    assert np.array_equal(i1, i2)
    assert np.array_equal(_bits(d1), _bits(d2))


def test_restatement_rows_are_sorted_self_free_and_padded():
    pts = C.CASES["n17"][0]
    idx, d2 = cloud_ref.knn(pts, 32)
    assert np.all(idx[:, :16] >= 0) and np.all(idx[:, 16:] == -1) and np.all(np.isposinf(d2[:, 16:]))
    assert not np.any(idx == np.arange(17)[:, None])
    keys = cloud_ref.knn_keys(pts, 16)
    assert np.all(keys[:, 1:] > keys[:, :-1])
    for k in C.KS:                                           # the order is total: a shorter row is a prefix of a longer one
        assert np.array_equal(cloud_ref.knn(pts, k)[0], idx[:, :k])


def test_restatement_feeds_segment_point_on_the_fixture():
    g = np.load(os.path.join(HERE, "golden", "mesh_point.npz"))
    idx, _ = cloud_ref.knn(g["points"], 6)
    e = cloud_ref.edges(idx)
    assert e.shape == (g["points"].shape[0] * 6, 2) and e.dtype == np.int64
    assert np.array_equal(e[:, 0], np.repeat(np.arange(g["points"].shape[0]), 6))      # i-major, rank-minor
    sup = mesh_ref.segment_point(g["points"], g["normals"], e, float(g["k_thresh"]), int(g["seg_min_verts"]))
    assert sup.shape == (g["points"].shape[0],) and sup.min() == 0
    assert np.array_equal(np.unique(sup), np.arange(sup.max() + 1))


def test_designed_cases_have_their_properties():
    cases = C.CASES
    for n in (0, 1, 2, 63, 64, 65, 255, 256, 257) + tuple(k for k in C.KS) + tuple(k + 1 for k in C.KS):
        assert cases["n%d" % n][0].shape == (n, 3)
    co = cases["coincident"][0]
    assert co.shape[0] == 200 and np.all(co == co[0])
    assert np.all(cloud_ref.knn(co, 6)[1] == 0) and np.array_equal(cloud_ref.knn(co, 3)[0][:2], [[1, 2, 3], [0, 2, 3]])
    la, cell = cases["lattice"]
    assert la.shape[0] == 12 ** 3 and cell == 1.0 and np.all(la == np.round(la))       # every point on a cell face
    d2 = cloud_ref.knn(la, 32)[1]
    inner = np.all((la >= 1) & (la <= 10), axis=1)
    assert np.all(d2[inner, 5] == cell * cell) and np.all(d2[inner, 6] == 2.0)         # k = 6: k-th d2 == the first bound
    assert np.unique(d2).shape[0] <= 12 and d2.size > 50000                            # thousands of tied distances
    sh = cases["sheet"][0]
    assert np.ptp(sh[:, 2]) == 0 and np.ptp(sh[:, 0]) > 0.9
    bl, bcell = cases["blob"]
    assert (bl[-1, 0] - bl[:-1, 0].max()) / bcell >= 39.9 and np.ptp(bl[:-1], axis=0).max() <= 1.0
    assert np.array_equal(cases["blob_auto"][0], bl) and cases["blob_auto"][1] is None
    li, lcell = cases["line"]
    assert np.ptp(li[:, 2]) / lcell > 1024 * 100 and np.ptp(li[:, 0]) <= 1.0
    of = cases["offset"][0]
    assert np.abs(of).min() > 900 and (of[:, 1] < 0).all() and (of[:, 0] > 0).all()
    for seed in (1, 2, 3):
        ro = cases["room%d" % seed][0]
        assert ro.shape == (3000, 3)
        _, counts = np.unique(ro, axis=0, return_counts=True)
        assert counts.max() == 2 and np.sum(counts == 2) == 1                         # one coincident pair
        idx, d2 = cloud_ref.knn(ro, 16)
        assert np.sum(d2[:, 0] == 0) == 2 and idx[777, 0] == 2999 and idx[2999, 0] == 777
        nrm, gap, m = cloud_ref.normals(ro, idx)
        assert np.all(m == 17) and np.mean(gap < 1e-3) <= 0.01
        assert np.allclose(np.linalg.norm(nrm, axis=1), 1.0, atol=1e-12)
        # the floor's normals point along z, but for the ~12 % of it within a neighbourhood's reach of the walls
        assert np.mean(np.abs(nrm[:1400, 2]) > 0.99) > 0.8


def test_normals_restatement_small_sets_and_orientation():
    pts = C.CASES["n2"][0]
    nrm, _, m = cloud_ref.normals(pts, cloud_ref.knn(pts, 6)[0])
    assert np.all(m == 2) and np.all(nrm == 0)
    sh = C.CASES["sheet"][0]
    nrm, gap, _ = cloud_ref.normals(sh, cloud_ref.knn(sh, 16)[0], C.SHEET_VIEWPOINT)
    assert np.all(gap > 1e-3) and np.allclose(nrm, [0, 0, 1], atol=1e-9)


def test_host_argument_checks():
    """The checks run on the host before any launch: the pointers below are never dereferenced."""
    lib = N.lib()
    vp = N.c_vp
    fake = 1 << 20
    assert lib.pbn_cloud_max_k() == 32
    assert lib.pbn_cloud_workspace_bytes(-1, 16) == 0
    assert lib.pbn_cloud_workspace_bytes(100, 0) == 0 and lib.pbn_cloud_workspace_bytes(100, 33) == 0
    assert lib.pbn_cloud_workspace_bytes(1 << 30, 16) == 0
    small, big = lib.pbn_cloud_workspace_bytes(100, 16), lib.pbn_cloud_workspace_bytes(200000, 16)
    assert 0 < small < big

    def knn(xyz=fake, n=100, k=16, idx=fake, d2=fake, status=fake, ws=fake, nbytes=small):
        return lib.pbn_cloud_knn(vp(xyz) if xyz else None, n, k, 0.0, vp(idx) if idx else None, vp(d2) if d2 else None,
                                 vp(status) if status else None, vp(ws) if ws else None, nbytes, None)
    for bad in (dict(xyz=0), dict(idx=0), dict(d2=0), dict(status=0), dict(ws=0), dict(n=-1), dict(k=0), dict(k=33)):
        assert knn(**bad) == N.PBN_ERR_ARG, bad
    assert knn(nbytes=small - 1) == N.PBN_ERR_WORKSPACE
    assert knn(n=200000) == N.PBN_ERR_WORKSPACE
    t = (N.ctypes.c_float * 4)()
    assert lib.pbn_cloud_knn_timed(vp(fake), 100, 16, 0.0, vp(fake), vp(fake), vp(fake), vp(fake), small - 1, None,
                                   t) == N.PBN_ERR_WORKSPACE
    assert lib.pbn_cloud_knn_timed(vp(fake), 100, 16, 0.0, vp(fake), vp(fake), vp(fake), vp(fake), small, None,
                                   None) == N.PBN_ERR_ARG

    def normals(xyz=fake, n=100, idx=fake, k=16, view=fake, nl=fake):
        return lib.pbn_cloud_normals(vp(xyz) if xyz else None, n, vp(idx) if idx else None, k, vp(view) if view else None,
                                     vp(nl) if nl else None, None)
    for bad in (dict(xyz=0), dict(idx=0), dict(view=0), dict(nl=0), dict(n=-1), dict(k=0), dict(k=33)):
        assert normals(**bad) == N.PBN_ERR_ARG, bad


def test_cpu_tensors_are_refused():
    x = torch.zeros(8, 3)
    with pytest.raises(RuntimeError):
        mesh.knn_graph(x, k=4)
    with pytest.raises(RuntimeError):
        mesh.point_normals(x, torch.zeros(8, 4, dtype=torch.int32))
    with pytest.raises(RuntimeError):
        mesh.decode_points((np.zeros((8, 3), np.float32), np.zeros((8, 3), np.uint8)), device="cpu")


def test_knn_edges_drops_padding():
    idx = torch.tensor([[1, 2, -1], [0, -1, -1], [0, 1, -1]], dtype=torch.int32)
    e = mesh.knn_edges(idx)
    assert e.dtype == torch.int64 and e.tolist() == [[0, 1], [0, 2], [1, 0], [2, 0], [2, 1]]
    assert np.array_equal(cloud_ref.edges(idx.numpy()), e.numpy())


def _write_points(path, xyz, col, alpha):
    names = ["red", "green", "blue"] + (["alpha"] if alpha else [])
    vdt = np.dtype([(n, "<f4") for n in "xyz"] + [(n, "u1") for n in names])
    v = np.zeros(xyz.shape[0], vdt)
    for i, n in enumerate("xyz"):
        v[n] = xyz[:, i]
    for i, n in enumerate(names[:3]):
        v[n] = col[:, i]
    head = ["ply", "format binary_little_endian 1.0", "comment a scan", "element vertex %d" % xyz.shape[0]]
    head += ["property float %s" % n for n in "xyz"] + ["property uchar %s" % n for n in names] + ["end_header"]
    with open(path, "wb") as fh:
        fh.write(("\n".join(head) + "\n").encode("ascii"))
        fh.write(v.tobytes())


@pytest.mark.parametrize("alpha", [True, False])
def test_read_ply_points_round_trip_and_refusals(tmp_path, alpha):
    rng = np.random.default_rng(4)
    xyz = rng.normal(size=(37, 3)).astype(np.float32)
    col = rng.integers(0, 256, (37, 3)).astype(np.uint8)
    p = str(tmp_path / "cloud.ply")
    _write_points(p, xyz, col, alpha)
    x, c = mesh.read_ply_points(p)
    assert x.dtype == np.float32 and c.dtype == np.uint8
    assert np.array_equal(_bits(x), _bits(xyz)) and np.array_equal(c, col)
    with pytest.raises(ValueError):                          # read_ply keeps refusing a file without faces
        mesh.read_ply(p)
    raw = open(p, "rb").read()
    cases = {"ascii": raw.replace(b"binary_little_endian", b"ascii", 1),
             "double": raw.replace(b"property float x", b"property double x", 1),
             "extra": raw.replace(b"property uchar red", b"property float nx\nproperty uchar red", 1),
             "truncated": raw[:-3]}
    for name, data in cases.items():
        q = tmp_path / (name + ".ply")
        q.write_bytes(data)
        with pytest.raises(ValueError):
            mesh.read_ply_points(str(q))
    m = str(tmp_path / "mesh.ply")
    mesh.write_ply(m, xyz, col, rng.integers(0, 37, (5, 3)), alpha=alpha)
    with pytest.raises(ValueError):                          # a mesh belongs to read_ply
        mesh.read_ply_points(m)
