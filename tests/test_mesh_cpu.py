"""CPU tier of the mesh decode (pbnet_amd.mesh): the restatement tests/mesh_ref.py against the reference's recorded
outputs (tests/golden/mesh_*.npz, written by make_mesh_golden.py from decode_scannet.py's numpy normals and the compiled
segmentator), the PLY reader, and decode_mesh's host arithmetic.

mesh_designed.npz is of another kind: the designed S and W cases of tests/mesh_cases.py whose sup does not depend on the order of
tied weights, each with the compiled segmentator's sup: the reference's own word on `<=`, `<`, the float32 threshold and dot2 > 0.

sup: the fixtures are committed only when the reference's partition equals mesh_ref's under both tie orders (the
reference's std::sort leaves tied weights unordered); the ids are compared element by element where the generator
recorded ids_exact."""
import glob
import os

import numpy as np
import pytest
import torch

import mesh_cases
import mesh_ref
from pbnet_amd import mesh, scene_io

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURES = sorted(glob.glob(os.path.join(HERE, "golden", "mesh_*.npz")))
MESHES = [p for p in FIXTURES if not p.endswith(("mesh_point.npz", "mesh_designed.npz"))]
POINT = os.path.join(HERE, "golden", "mesh_point.npz")
DESIGNED = os.path.join(HERE, "golden", "mesh_designed.npz")


def test_fixture_set():
    names = sorted(os.path.basename(p)[:-4] for p in MESHES)
    assert names == ["mesh_flat", "mesh_oddities", "mesh_room"]
    assert os.path.exists(POINT)
    assert sorted(os.path.basename(p)[:-4] for p in FIXTURES) == ["mesh_designed", "mesh_flat", "mesh_oddities", "mesh_point", "mesh_room"]
    for p in FIXTURES:
        assert os.path.getsize(p) < 1 << 20


@pytest.mark.parametrize("path", MESHES, ids=[os.path.basename(p)[:-4] for p in MESHES])
def test_restatement_reproduces_mesh_fixture(path):
    g = np.load(path)
    nl = mesh_ref.decode_normals(g["xyz"], g["faces"])
    assert nl.dtype == np.float32
    assert np.array_equal(nl.view(np.uint32), g["nl"].view(np.uint32))
    for ties in ("asc", "desc"):
        sup = mesh_ref.segment_mesh(g["xyz"], g["faces"], float(g["k_thresh"]), int(g["seg_min_verts"]), ties=ties)
        assert mesh_ref.same_partition(sup, g["sup"]), ties
        if bool(g["ids_exact"]):
            assert np.array_equal(sup, g["sup"]), ties


def test_restatement_reproduces_point_fixture():
    g = np.load(POINT)
    for ties in ("asc", "desc"):
        sup = mesh_ref.segment_point(g["points"], g["normals"], g["edges"], float(g["k_thresh"]), int(g["seg_min_verts"]),
                                     ties=ties)
        assert mesh_ref.same_partition(sup, g["sup"]), ties
        if bool(g["ids_exact"]):
            assert np.array_equal(sup, g["sup"]), ties


def test_restatement_reproduces_designed_fixture():
    """Ids, not only partitions: the cases were recorded because both tie orders give one sup."""
    g = np.load(DESIGNED)
    assert len(g["names"]) >= 12
    for name, mode, arrays, k, m, sup in mesh_cases.designed_cases(g):
        segment = mesh_ref.segment_mesh if mode == "mesh" else mesh_ref.segment_point
        for ties in ("asc", "desc"):
            assert np.array_equal(segment(*arrays, k, m, ties=ties), sup), (name, ties)


def test_fixtures_cover_the_issue_cases():
    flat = np.load(os.path.join(HERE, "golden", "mesh_flat.npz"))
    assert np.all(flat["xyz"][:, 2] == flat["xyz"][0, 2])                         # perfectly flat
    w = mesh_ref.edge_weights(flat["xyz"], mesh_ref.segmentator_normals(flat["xyz"], flat["faces"]),
                              *mesh_ref.mesh_edges(flat["faces"]))
    assert np.unique(w).shape[0] < w.shape[0] // 100                             # many exactly tied weights
    odd = np.load(os.path.join(HERE, "golden", "mesh_oddities.npz"))
    f = odd["faces"]
    assert np.sum((f[:, 0] == f[:, 1]) | (f[:, 1] == f[:, 2]) | (f[:, 0] == f[:, 2])) == 1
    assert np.setdiff1d(np.arange(odd["xyz"].shape[0]), f).shape[0] >= 1         # unreferenced vertices
    _, counts = np.unique(odd["vertices"], axis=0, return_counts=True)
    assert counts.max() >= 2                                                     # coincident coordinates


def test_order_keys_are_total_and_put_nan_last():
    w = np.array([np.nan, 1.0, -0.0, 0.0, -1e-7, np.inf, 3e-8, -np.inf, -np.nan], np.float32)
    o = mesh_ref.edge_order(w)
    assert list(o[:6]) == [7, 4, 2, 3, 6, 1]
    assert list(o[6:7]) == [5] and sorted(o[7:]) == [0, 8]


def _write(tmp_path, index_type, alpha, n=50, f=80, seed=0):
    rng = np.random.default_rng(seed)
    xyz = rng.normal(size=(n, 3)).astype(np.float32)
    col = rng.integers(0, 256, (n, 3)).astype(np.uint8)
    faces = rng.integers(0, n, (f, 3))
    p = str(tmp_path / ("m_%s_%d.ply" % (index_type, alpha)))
    mesh.write_ply(p, xyz, col, faces, index_type=index_type, alpha=alpha)
    return p, xyz, col, faces


@pytest.mark.parametrize("index_type", ["int", "uint"])
@pytest.mark.parametrize("alpha", [True, False])
def test_read_ply_round_trip(tmp_path, index_type, alpha):
    p, xyz, col, faces = _write(tmp_path, index_type, alpha)
    head = open(p, "rb").read(400).split(b"end_header")[0].decode()
    assert ("property list uchar %s vertex_indices" % index_type) in head
    x, c, f = mesh.read_ply(p)
    assert x.dtype == np.float32 and c.dtype == np.uint8 and f.dtype == np.int64
    assert np.array_equal(x.view(np.uint32), xyz.view(np.uint32))
    assert np.array_equal(c, col)
    assert np.array_equal(f, faces)


def test_read_ply_rejects_what_it_does_not_read(tmp_path):
    p, *_ = _write(tmp_path, "int", True)
    raw = open(p, "rb").read()
    cases = {
        "ascii": raw.replace(b"binary_little_endian", b"ascii", 1),
        "big": raw.replace(b"binary_little_endian", b"binary_big_endian", 1),
        "double": raw.replace(b"property float x", b"property double x", 1),
        "extra": raw.replace(b"property uchar red", b"property float nx\nproperty uchar red", 1),
        "list_int": raw.replace(b"list uchar int", b"list int int", 1),
        "edge_elem": raw.replace(b"end_header", b"element edge 0\nproperty int vertex1\nend_header", 1),
        "truncated": raw[:-7],
    }
    bad = bytearray(raw)
    bad[raw.index(b"end_header\n") + len(b"end_header\n") + 50 * 16] = 4        # the first face says 4 corners
    cases["quad"] = bytes(bad)
    for name, data in cases.items():
        q = tmp_path / (name + ".ply")
        q.write_bytes(data)
        with pytest.raises(ValueError):
            mesh.read_ply(str(q))


def test_centre_and_scale_is_the_reference_arithmetic():
    """decode_scannet.py:62-70 (read_mesh_vertices_rgb), stated here as it is written there."""
    rng = np.random.default_rng(3)
    n = 100003
    x = (rng.normal(size=(n, 3)) * 3 + [1.5, -2.0, 0.7]).astype(np.float32)
    col = rng.integers(0, 256, (n, 3)).astype(np.uint8)
    vertices = np.zeros(shape=[n, 6], dtype=np.float32)
    vertices[:, 0] = x[:, 0]
    vertices[:, 1] = x[:, 1]
    vertices[:, 2] = x[:, 2]
    vertices[:, 3] = col[:, 0]
    vertices[:, 4] = col[:, 1]
    vertices[:, 5] = col[:, 2]
    want_xyz = vertices[:, :3] - vertices[:, :3].mean(0)
    want_rgb = vertices[:, 3:] / 127.5 - 1
    xyz, rgb = mesh.centre_and_scale(x, col)
    assert xyz.dtype == np.float32 and rgb.dtype == np.float32
    assert np.array_equal(xyz.view(np.uint32), want_xyz.view(np.uint32))
    assert np.array_equal(rgb.view(np.uint32), want_rgb.view(np.uint32))


def test_save_decoded_test_split_and_labelled(tmp_path):
    n = 40
    rng = np.random.default_rng(1)
    dec = {"xyz": rng.normal(size=(n, 3)).astype(np.float32), "rgb": rng.normal(size=(n, 3)).astype(np.float32),
           "nl": rng.normal(size=(n, 3)).astype(np.float32), "face": rng.integers(0, n, (70, 3)).astype(np.int32),
           "sup": rng.integers(0, 5, n).astype(np.int64)}
    mesh.save_decoded(str(tmp_path / "test"), "scene0707_00", dec)
    written = sorted(os.listdir(tmp_path / "test"))
    assert written == ["scene0707_00_%s.npy" % k for k in ("face", "nl", "rgb", "sup", "xyz")]
    for k, v in dec.items():
        got = np.load(scene_io.scene_path(str(tmp_path / "test"), "scene0707_00", k))
        assert got.dtype == scene_io.SCENE_ARRAYS[k][0] and np.array_equal(got, v)
    sem = rng.integers(0, 20, n).astype(np.float64)
    ins = rng.integers(-1, 4, n).astype(np.float64)
    mesh.save_decoded(str(tmp_path / "val"), "scene0011_00", dec, sem_label=sem, ins_label=ins)
    back = scene_io.load_scene(str(tmp_path / "val"), "scene0011_00")
    assert np.array_equal(back["sup"], dec["sup"]) and np.array_equal(back["sem_label"], sem)
    with pytest.raises(ValueError):
        mesh.save_decoded(str(tmp_path / "x"), "s", dec, sem_label=sem)


def test_cpu_tensors_are_refused():
    x = torch.zeros(4, 3)
    f = torch.zeros(2, 3, dtype=torch.int32)
    with pytest.raises(RuntimeError):
        mesh.vertex_normals(x, f)
    with pytest.raises(RuntimeError):
        mesh.segment_mesh(x, f)
    with pytest.raises(RuntimeError):
        mesh.segment_point(x, x, torch.zeros(2, 2, dtype=torch.int64))
