"""End to end on the GPU without a mesh: the vertices and colours of a fixture room (its faces are NOT used) go through
pbnet_amd.mesh.decode_points into SceneCache, a DeviceMerge validation batch and refine_instances with fixed proposals,
exactly as tests/test_mesh_e2e_gpu.py does for decode_mesh; every batch tensor and every refined output must equal the same
path fed the restatement's superpoints (tests/cloud_ref.py kNN -> tests/mesh_ref.py segment_point)."""
import os

import numpy as np
import pytest
import torch

import cloud_ref
import mesh_ref
from pbnet_amd import mesh
from test_mesh_e2e_gpu import DEV, _labels, _run

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
K = 16


@pytest.fixture(scope="module")
def decoded():
    g = np.load(os.path.join(HERE, "golden", "mesh_room.npz"))
    dec = mesh.decode_points((g["vertices"], g["colours"]), device=DEV, k=K, return_graph=True)
    xyz, rgb = mesh.centre_and_scale(g["vertices"], g["colours"])
    return (xyz, rgb) + cloud_ref.knn(xyz, K), {k: v.cpu().numpy() for k, v in dec.items()}


def test_decode_points_graph_and_superpoints_are_the_restatement(decoded):
    (xyz, rgb, idx, d2), d = decoded
    assert sorted(d) == ["d2", "idx", "nl", "rgb", "sup", "xyz"]
    assert np.array_equal(d["xyz"].view(np.uint32), xyz.view(np.uint32)) and np.array_equal(d["rgb"], rgb)
    assert np.array_equal(d["idx"], idx) and np.array_equal(d["d2"].view(np.uint32), d2.view(np.uint32))
    edges = mesh.knn_edges(torch.from_numpy(d["idx"])).numpy()
    assert np.array_equal(edges, cloud_ref.edges(idx))
    asc = mesh_ref.segment_point(xyz, d["nl"], edges, ties="asc")
    assert d["sup"].dtype == np.int64 and np.array_equal(d["sup"], asc)
    desc = mesh_ref.segment_point(xyz, d["nl"], edges, ties="desc")
    if mesh_ref.same_partition(asc, desc):                   # the partition allows the other tie order too
        assert mesh_ref.same_partition(d["sup"], desc)
    ref, gap, _ = cloud_ref.normals(xyz, idx)
    n = d["nl"].astype(np.float64)
    s = np.sign(np.einsum("ij,ij->i", ref, n))
    ok = gap >= 1e-3
    assert ok.mean() >= 0.99 and np.abs(n - s[:, None] * ref)[ok].max() <= 1e-6


def test_decode_points_feeds_validation_and_refinement(decoded, tmp_path):
    (xyz, rgb, idx, _), d = decoded
    sem, ins = _labels(d["xyz"].shape[0])
    ours = {k: d[k] for k in ("xyz", "rgb", "nl", "sup")}
    sup = mesh_ref.segment_point(xyz, d["nl"], cloud_ref.edges(idx), ties="asc")
    ref = {"xyz": xyz, "rgb": rgb, "nl": d["nl"], "sup": sup}
    b1, (c1, s1, i1, d1) = _run(dict(ours, sem_label=sem, ins_label=ins))
    b2, (c2, s2, i2, d2) = _run(dict(ref, sem_label=sem, ins_label=ins))
    assert set(b1) == set(b2)
    for k in b1:
        if torch.is_tensor(b1[k]):
            assert b1[k].dtype == b2[k].dtype and torch.equal(b1[k], b2[k]), k
        else:
            assert b1[k] == b2[k], k
    assert c1.shape[0] > 0
    assert torch.equal(c1, c2) and torch.equal(s1, s2) and torch.equal(i1, i2)
    for k in ("seg", "seg_refined"):
        assert torch.equal(d1[k], d2[k]), k
    # the dict goes through save_decoded unchanged, and a scan has no face file
    mesh.save_decoded(str(tmp_path), "scan0000_00", ours)
    assert sorted(os.listdir(tmp_path)) == ["scan0000_00_%s.npy" % k for k in ("nl", "rgb", "sup", "xyz")]
