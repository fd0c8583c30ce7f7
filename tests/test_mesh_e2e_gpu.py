"""End to end on the GPU: a fixture mesh goes through pbnet_amd.mesh.decode_mesh into SceneCache, a DeviceMerge
validation batch and refine_instances with fixed proposals; every batch tensor and every refined output must equal the
same path fed the reference's own nl / sup (tests/golden/mesh_*.npz, the fixtures whose ids the generator found exact)."""
import glob
import os
import types

import numpy as np
import pytest
import torch

from pbnet_amd import mesh
from pbnet_amd import postprocess as PP
from pbnet_amd.config import get_config
from pbnet_amd.loader import DeviceMerge, MergeDraws, SceneCache

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
HERE = os.path.dirname(os.path.abspath(__file__))
EXACT = sorted(p for p in glob.glob(os.path.join(HERE, "golden", "mesh_*.npz"))
               if not p.endswith(("mesh_point.npz", "mesh_designed.npz")) and bool(np.load(p)["ids_exact"]))


def _labels(n):
    i = np.arange(n)
    sem = (i // 37 % 20).astype(np.float64)
    ins = np.where(sem >= 2, i // 37, -100).astype(np.float64)
    return sem, ins


def _run(scene):
    name = "scene0000_00"
    cache = SceneCache({name: scene}, DEV, train=[name], val=[name])
    cfg = get_config(test=True)
    batch = DeviceMerge(cache, cfg, seed=5).val_merge([0], MergeDraws.draw_val(torch.Generator().manual_seed(5), 1))
    rows = int(batch["xyz_original"].shape[0])
    rng = np.random.default_rng(8)
    idx, off = [], [0]
    for p in range(7):
        members = np.unique(rng.integers(0, rows, int(rng.integers(rows // 8, rows // 3))))
        idx.append(np.stack([np.full(members.shape[0], p), members], 1))
        off.append(off[-1] + members.shape[0])
    proposals = (torch.from_numpy(np.concatenate(idx).astype(np.int64)).to(DEV),
                 torch.from_numpy(np.array(off, np.int32)).to(DEV), None, None)
    pred_sem = torch.from_numpy(rng.integers(2, 20, rows)).to(DEV)
    scores = torch.from_numpy(rng.uniform(0.05, 1.0, 7).astype(np.float32)).to(DEV)
    pcfg = types.SimpleNamespace(TEST_SCORE_THRESH=0.09, TEST_NPOINT_THRESH=20, TEST_NMS_THRESH=0.3)
    out = PP.refine_instances(pred_sem, proposals, scores, rows, batch["sup"], pcfg, return_debug=True)
    return batch, out


def test_fixtures_with_exact_ids_exist():
    assert any(os.path.basename(p) == "mesh_oddities.npz" for p in EXACT)


@pytest.mark.parametrize("path", EXACT, ids=[os.path.basename(p)[:-4] for p in EXACT])
def test_decode_mesh_feeds_validation_and_refinement(path):
    g = np.load(path)
    dec = mesh.decode_mesh((g["vertices"], g["colours"], g["faces"]), device=DEV)
    sem, ins = _labels(g["xyz"].shape[0])
    ours = {k: dec[k].cpu().numpy() for k in ("xyz", "rgb", "nl", "sup")}
    ref = {"xyz": g["xyz"], "rgb": g["rgb"], "nl": g["nl"], "sup": g["sup"]}
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
