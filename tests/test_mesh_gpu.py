"""GPU tier of the mesh decode (csrc/mesh.hip through pbnet_amd.mesh).

* every fixture of tests/golden/mesh_*.npz (the reference's own outputs): nl bit for bit, the sup partition equal, and
  sup equal element by element where the generator recorded ids_exact; mesh_designed.npz (designed tie-free cases, the compiled
  segmentator's sup): element by element;
* a synthetic mesh of the bench scene's size (jitter, flat regions, coincident vertices) against tests/mesh_ref.py with
  the library's tie order: nl bit for bit, sup exactly; a second run bit-identical;
* error paths: bad indices raise, 0 faces is the identity, degenerate faces give valid ids."""
import glob
import os

import numpy as np
import pytest
import torch

import mesh_cases
import mesh_ref
from pbnet_amd import mesh

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURES = sorted(glob.glob(os.path.join(HERE, "golden", "mesh_*.npz")))
MESHES = [p for p in FIXTURES if not p.endswith(("mesh_point.npz", "mesh_designed.npz"))]
POINT = os.path.join(HERE, "golden", "mesh_point.npz")
DESIGNED = [p for p in FIXTURES if p.endswith("mesh_designed.npz")]


def _bits(t):
    return t.detach().cpu().numpy().view(np.uint32)


def _d(a, dtype=None):
    a = np.ascontiguousarray(a if dtype is None else np.asarray(a).astype(dtype))
    return torch.from_numpy(a).to(DEV)


@pytest.mark.parametrize("idx", [np.int32, np.int64], ids=["i32", "i64"])
@pytest.mark.parametrize("path", MESHES, ids=[os.path.basename(p)[:-4] for p in MESHES])
def test_fixture_parity(path, idx):
    g = np.load(path)
    xyz, faces = _d(g["xyz"]), _d(g["faces"], idx)
    nl = mesh.vertex_normals(xyz, faces)
    assert np.array_equal(_bits(nl), g["nl"].view(np.uint32))
    sup = mesh.segment_mesh(xyz, faces, float(g["k_thresh"]), int(g["seg_min_verts"]))
    assert sup.dtype == torch.int64 and sup.device.type == "cuda"
    s = sup.cpu().numpy()
    assert mesh_ref.same_partition(s, g["sup"])
    if bool(g["ids_exact"]):
        assert np.array_equal(s, g["sup"])
    # the decode_mesh path: raw vertices and colours in, the reference's arrays out
    dec = mesh.decode_mesh((g["vertices"], g["colours"], g["faces"].astype(idx)), device=DEV)
    assert np.array_equal(_bits(dec["xyz"]), g["xyz"].view(np.uint32))
    assert np.array_equal(_bits(dec["rgb"]), g["rgb"].view(np.uint32))
    assert np.array_equal(_bits(dec["nl"]), g["nl"].view(np.uint32))
    assert dec["face"].dtype == torch.int32 and np.array_equal(dec["face"].cpu().numpy(), g["faces"])
    assert torch.equal(dec["sup"], sup)


def test_point_fixture_parity():
    g = np.load(POINT)
    for idx in (np.int32, np.int64):
        sup = mesh.segment_point(_d(g["points"]), _d(g["normals"]), _d(g["edges"], idx), float(g["k_thresh"]),
                                 int(g["seg_min_verts"])).cpu().numpy()
        assert mesh_ref.same_partition(sup, g["sup"])
        if bool(g["ids_exact"]):
            assert np.array_equal(sup, g["sup"])
        assert np.array_equal(sup, mesh_ref.segment_point(g["points"], g["normals"], g["edges"], ties="asc"))


def test_designed_fixture_parity():
    """mesh_designed.npz: the compiled segmentator's sup on the designed tie-free cases, element by element, both index types."""
    assert len(DESIGNED) == 1
    g = np.load(DESIGNED[0])
    for name, mode, arrays, k, m, sup in mesh_cases.designed_cases(g):
        for idx in (np.int32, np.int64):
            if mode == "mesh":
                got = mesh.segment_mesh(_d(arrays[0]), _d(arrays[1], idx), k, m)
            else:
                got = mesh.segment_point(_d(arrays[0]), _d(arrays[1]), _d(arrays[2], idx), k, m)
            assert np.array_equal(got.cpu().numpy(), sup), (name, idx)


def bench_mesh(seed=0, n=402):
    """n x n height field (161 604 vertices, 321 602 faces at n = 402): jittered bumps, exactly flat regions, and a seam
    of coincident-coordinate vertices (the column exists twice; the faces right of it use the copy)."""
    rng = np.random.default_rng(seed)
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    x, y = i * 0.02, j * 0.02
    z = 0.15 * np.sin(x * 3.1) * np.cos(y * 2.3) + rng.normal(0, 0.002, x.shape)
    z[(x > 1.0) & (x < 3.0) & (y > 1.0) & (y < 4.0)] = 0.5                       # flat table top
    z[(x > 5.0) & (y > 5.0)] = 0.0                                               # flat floor
    v = np.stack([x, y, z], -1).reshape(-1, 3)
    idx = np.arange(n * n).reshape(n, n)
    a, b, c, d = idx[:-1, :-1], idx[1:, :-1], idx[1:, 1:], idx[:-1, 1:]
    f = np.concatenate([np.stack([a, b, c], -1).reshape(-1, 3), np.stack([a, c, d], -1).reshape(-1, 3)])
    seam = idx[n // 3]                                                           # column duplicated
    copy = np.arange(n * n, n * n + n)
    v = np.concatenate([v, v[seam]])
    right = (f // n > n // 3).any(axis=1, keepdims=True) & np.isin(f, seam)
    remap = np.full(n * n, -1)
    remap[seam] = copy
    f = np.where(right, remap[f], f)
    return v.astype(np.float32), f.astype(np.int32)


@pytest.fixture(scope="module")
def big():
    v, f = bench_mesh()
    assert v.shape[0] >= 161517 and f.shape[0] >= 300000
    _, counts = np.unique(v, axis=0, return_counts=True)
    assert counts.max() >= 2
    return v, f


def test_bench_sized_mesh_matches_restatement(big):
    v, f = big
    xyz, faces = _d(v), _d(f)
    nl = mesh.vertex_normals(xyz, faces)
    sup = mesh.segment_mesh(xyz, faces)
    want_nl = mesh_ref.decode_normals(v, f)
    assert np.array_equal(_bits(nl), want_nl.view(np.uint32))
    want = mesh_ref.segment_mesh(v, f, ties="asc")
    got = sup.cpu().numpy()
    print("bench-sized mesh: V=%d F=%d segments=%d" % (v.shape[0], f.shape[0], got.max() + 1))
    assert np.array_equal(got, want)
    # two runs are bit-identical
    nl2 = mesh.vertex_normals(xyz, faces)
    sup2 = mesh.segment_mesh(xyz, faces)
    assert torch.equal(nl.view(torch.int32), nl2.view(torch.int32))
    assert torch.equal(sup, sup2)


def test_bad_indices_raise():
    g = np.load(MESHES[0])
    xyz = _d(g["xyz"])
    n = xyz.shape[0]
    for idx in (np.int32, np.int64):
        for bad in (-1, n):
            f = g["faces"].astype(idx).copy()
            f[len(f) // 2, 1] = bad
            with pytest.raises(ValueError):
                mesh.vertex_normals(xyz, _d(f))
            with pytest.raises(ValueError):
                mesh.segment_mesh(xyz, _d(f))
            e = np.array([[0, 1], [1, bad]], idx)
            with pytest.raises(ValueError):
                mesh.segment_point(xyz, xyz, _d(e))
    f = g["faces"].astype(np.int64).copy()
    f[0, 0] = (1 << 32) + 1                    # an int64 index that would wrap to a valid int32
    with pytest.raises(ValueError):
        mesh.segment_mesh(xyz, _d(f))
    torch.cuda.synchronize()


def test_zero_faces_is_identity():
    xyz = _d(np.random.default_rng(0).normal(size=(37, 3)).astype(np.float32))
    for idx in (torch.int32, torch.int64):
        f = torch.zeros(0, 3, dtype=idx, device=DEV)
        assert torch.equal(mesh.segment_mesh(xyz, f).cpu(), torch.arange(37))
        assert torch.equal(mesh.vertex_normals(xyz, f).cpu(), torch.zeros(37, 3))
        e = torch.zeros(0, 2, dtype=idx, device=DEV)
        assert torch.equal(mesh.segment_point(xyz, xyz, e).cpu(), torch.arange(37))
    empty = torch.zeros(0, 3, dtype=torch.float32, device=DEV)
    assert mesh.segment_mesh(empty, torch.zeros(0, 3, dtype=torch.int64, device=DEV)).shape == (0,)


def test_degenerate_faces_give_valid_ids():
    """Zero-area faces (a repeated vertex, collinear corners, coincident corners): NaN segmentator normals, NaN weights
    sorted last.  The library's outcome is defined: ids 0..S-1, every id used, equal to mesh_ref's stable order."""
    v, f = bench_mesh(seed=1, n=60)
    f = f.astype(np.int64)
    v = np.concatenate([v, v[:3], [[0.5, 0.5, 0.5], [0.6, 0.6, 0.6], [0.7, 0.7, 0.7]]]).astype(np.float32)
    n0 = v.shape[0] - 6
    extra = np.array([[10, 10, 11], [n0, n0 + 1, 0], [n0 + 3, n0 + 4, n0 + 5], [500, 501, 500], [n0 + 2, 2, 7]])
    f = np.concatenate([f[:900], extra, f[900:]])
    sup = mesh.segment_mesh(_d(v), _d(f)).cpu().numpy()
    assert sup.min() == 0 and np.array_equal(np.unique(sup), np.arange(sup.max() + 1))
    assert np.array_equal(sup, mesh_ref.segment_mesh(v, f, ties="asc"))
    nl = mesh.vertex_normals(_d(v), _d(f)).cpu().numpy()
    assert np.isfinite(nl).all()
    assert np.array_equal(nl.view(np.uint32), mesh_ref.decode_normals(v, f).view(np.uint32))
