"""End to end on the GPU for a raw scan: the fixture room's vertices, three times over with 2 mm of jitter and twenty points
50 m away (k = 16 < 20: their neighbours are each other), go through pbnet_amd.mesh.decode_points(pitch, outlier_ratio).
Its kept points (return_kept), given to decode_points as it stood before the keywords existed, must produce the same
bytes; both then run through SceneCache, a DeviceMerge validation batch and refine_instances exactly as
tests/test_cloud_e2e_gpu.py does; and carry_labels must give every raw point the label of raw_index's row."""
import os

import numpy as np
import pytest
import torch

import thin_ref
from pbnet_amd import mesh
from test_mesh_e2e_gpu import DEV, _labels, _run

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
K, PITCH, RATIO, N_FAR = 16, 0.03, 2.0, 20


@pytest.fixture(scope="module")
def scan():
    g = np.load(os.path.join(HERE, "golden", "mesh_room.npz"))
    rng = np.random.default_rng(3)
    v = g["vertices"]
    xyz = np.concatenate([v + rng.normal(scale=0.002, size=v.shape) for _ in range(3)] + [rng.uniform(50.0, 60.0, (N_FAR, 3))])
    colours = np.concatenate([g["colours"]] * 3 + [rng.integers(0, 256, (N_FAR, 3)).astype(np.uint8)])
    raw = (xyz.astype(np.float32), colours)
    dec = mesh.decode_points(raw, device=DEV, k=K, pitch=PITCH, outlier_ratio=RATIO, return_kept=True)
    d = {k: v.cpu().numpy() for k, v in dec.items()}
    plain = mesh.decode_points((d["kept_xyz"], d["kept_rgb"]), device=DEV, k=K)       # today's function on the kept points
    return raw, d, {k: v.cpu().numpy() for k, v in plain.items()}


def test_kept_points_decode_to_the_same_bytes(scan):
    (xyz, colours), d, plain = scan
    assert sorted(d) == ["count", "kept_rgb", "kept_xyz", "nl", "raw_index", "rgb", "sup", "xyz"]
    m = d["kept_xyz"].shape[0]
    assert 1000 < m < xyz.shape[0] // 2 and d["kept_rgb"].shape == (m, 3) and d["count"].shape == (m,)
    assert sorted(plain) == ["nl", "rgb", "sup", "xyz"]
    for k in ("xyz", "rgb", "nl", "sup"):
        got, want = d[k], plain[k]
        assert got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes(), k
    # the kept points are the restatement's: thinning, then the outlier mask over the device's graph of the thinned points
    th = thin_ref.thin(xyz, colours.astype(np.float32), PITCH)
    idx, d2 = mesh.knn_graph(torch.from_numpy(th["xyz"]).to(DEV), k=K)
    keep, _ = thin_ref.outlier(d2.cpu().numpy(), RATIO)
    assert np.array_equal(d["kept_xyz"].view(np.uint32), th["xyz"][keep].view(np.uint32))
    assert np.array_equal(d["kept_rgb"].view(np.uint32), th["rgb"][keep].view(np.uint32))
    assert np.array_equal(d["count"], th["count"][keep])
    assert np.array_equal(d["raw_index"], thin_ref.raw_index(th["inverse"], keep, idx.cpu().numpy()))
    assert not keep[th["inverse"][-N_FAR:]].any()           # the far points are gone ...
    assert np.all(d["raw_index"][-N_FAR:] == -1)             # ... and, among themselves, have nobody to speak for them


def test_raw_scan_feeds_validation_and_refinement_and_labels_come_back(scan):
    (xyz, _), d, plain = scan
    m = d["xyz"].shape[0]
    sem, ins = _labels(m)
    b1, (c1, s1, i1, d1) = _run(dict(d, sem_label=sem, ins_label=ins))          # SceneCache takes the dict with its extra keys
    b2, (c2, s2, i2, d2) = _run(dict(plain, sem_label=sem, ins_label=ins))
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
    # labels of the kept points back on the raw ones
    raw = d["raw_index"]
    assert raw.shape == (xyz.shape[0],) and raw.dtype == np.int32 and raw.max() == m - 1
    for labels in (torch.from_numpy(d["sup"]).to(DEV), torch.from_numpy(sem.astype(np.int32)).to(DEV),
                   torch.stack([torch.arange(m), torch.arange(m) % 7], 1).to(DEV)):
        got = mesh.carry_labels(labels, torch.from_numpy(raw).to(DEV)).cpu().numpy()
        host = labels.cpu().numpy()
        assert got.dtype == host.dtype and got.shape == (raw.shape[0],) + host.shape[1:]
        assert np.array_equal(got[raw >= 0], host[raw[raw >= 0]])
        assert np.all(got[raw < 0] == -1) and (raw < 0).sum() >= N_FAR
        if host.ndim == 1 and host.min() >= 0:
            assert np.array_equal(got == -1, raw < 0)        # -1 only where raw_index is -1
