#!/usr/bin/env python3
"""Golden vectors for the device batch construction (pbnet_amd/loader.py, csrc/augment.hip), produced IN THE BUILD
CONTAINER by the reference's own `Dataset.trainMerge` / `Dataset.valMerge` (datasets/scannetv2/dataset_preprocess.py),
imported from /root/reference and run on small synthetic scenes (pbnet_amd.synth.synth_room).

    python tests/golden/make_merge_golden.py        # writes tests/golden/merge_*.npz

Stubs, and why:
  * `SharedArray` is a dict: `SA.attach("shm://<scene>_<key>")` returns the scene's array (the reference's cfg.cache path).
  * `MinkowskiEngine.utils.sparse_quantize` / `sparse_collate` are replaced by this repository's first-occurrence voxeliser
    (`synth.voxelize_numpy`: floor(xyz / voxel) in float64, survivors in input order) -- the device path reproduces that
    convention, not MinkowskiEngine's internal choice of representative point.
Everything else -- dataAugment, elastic (scipy), crop, getCroppedInstLabel / getInstLabel, getInstanceInfo, the merge loops --
is the reference's own code.  `np.random.{rand,randn,randint,uniform}` are wrapped to record every draw, in order; the
stream is stored with the inputs and outputs, and `MergeDraws.replay` rebuilds it.

Each case also runs tests/merge_ref.py on the recorded draws, requires it to agree with the reference, and asserts that no
point lies within 1e-9 of a voxel or crop boundary (so the fixtures do not depend on float64 summation order).

Cases:
  merge_T1  train, mix-up, the crop loop taken (small max_crop_p / min_crop_p) and succeeding
  merge_T2  train, every one of the 5 tries fails (the last try's mask, un-offset xyz)
  merge_T3  train, the primary scene has no instances (its ins.max()+1 = -99 shifts the partner's labels)
  merge_V1  validation, batch_size_v 1
  merge_V2  validation, batch_size_v 2"""
import os
import sys
import types
from types import SimpleNamespace

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from pbnet_amd.synth import synth_room, voxelize_numpy          # noqa: E402
from pbnet_amd.loader import MergeDraws                        # noqa: E402
import merge_ref                                                # noqa: E402

SHM = {}
_sa = types.ModuleType("SharedArray")
_sa.attach = lambda name: SHM[name[len("shm://"):]]
sys.modules["SharedArray"] = _sa


def _sparse_quantize(coords, feats, quantization_size, return_index, return_inverse):
    q, first, inv = voxelize_numpy(coords, quantization_size)
    return q.astype(np.int32), feats[first], torch.from_numpy(first), torch.from_numpy(inv)


def _sparse_collate(coords, feats):
    c = [np.concatenate([np.full((len(q), 1), b, np.int32), q], 1) for b, q in enumerate(coords)]
    return torch.from_numpy(np.concatenate(c)), torch.from_numpy(np.concatenate(feats))


_me = types.ModuleType("MinkowskiEngine")
_me.utils = SimpleNamespace(sparse_quantize=_sparse_quantize, sparse_collate=_sparse_collate)
sys.modules["MinkowskiEngine"] = _me
import importlib.util                                          # noqa: E402
_spec = importlib.util.spec_from_file_location(                 # reference code, executed here only
    "dataset_preprocess", "/root/reference/datasets/scannetv2/dataset_preprocess.py")
DP = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(DP)

RECORD = []


def _wrap(name):
    real = getattr(np.random, name)

    def f(*a, **kw):
        v = real(*a, **kw)
        RECORD.append((name, np.array(v, np.float64)))
        return v
    return f


for _n in ("rand", "randn", "randint", "uniform"):
    setattr(np.random, _n, _wrap(_n))

VOXEL = 0.02
MARGIN = 1e-9


def scene(seed, n_boxes=3, room=(1.6, 1.3, 1.0), pitch=0.085):
    s = synth_room(seed=seed, pitch=pitch, room=room, n_boxes=n_boxes)
    rng = np.random.default_rng(seed + 77)
    sup = (np.floor(s["xyz"] / 0.3).astype(np.int64) @ np.array([1, 16, 256])).astype(np.int64)
    # a ScanNet-like raw scene: not min-normalised, labels with holes (the relabel loop has work to do)
    xyz = (s["xyz"] + rng.uniform(-2, 2, 3)).astype(np.float32)
    ins = s["ins"].copy()
    ins[ins >= 0] = ins[ins >= 0] * 2 + 1
    return dict(xyz=xyz, rgb=s["rgb"], sem_label=s["sem"], ins_label=ins, nl=s["normal"], sup=sup)


def dataset(scenes, names, max_crop_p, min_crop_p, batch_v=1):
    d = DP.Dataset.__new__(DP.Dataset)
    d.batch_size, d.batch_size_v, d.dataset_workers, d.cache, d.dist = len(names), batch_v, 0, True, False
    d.voxel_size, d.scale_size, d.min_crop_p, d.max_crop_p, d.mixup = VOXEL, 1, min_crop_p, max_crop_p, True
    d.full_scale = [128 * d.scale_size / 50.0, 512 * d.scale_size / 50.0]
    d.train_file_list = np.array(names)
    d.val_file_list = np.array(names)
    SHM.clear()
    for n, s in scenes.items():
        for k, v in s.items():
            SHM["%s_%s" % (n, k)] = v.copy()
    return d


def _np(v):
    return v.numpy() if torch.is_tensor(v) else np.asarray(v)


def run(case, kind, scenes, ids, max_crop_p=300000, min_crop_p=50000, seed=0, expect=None):
    names = sorted(scenes)
    cfg = SimpleNamespace(voxel_size=VOXEL, scale_size=1, max_crop_p=max_crop_p, min_crop_p=min_crop_p)
    for attempt in range(200):
        d = dataset(scenes, names, max_crop_p, min_crop_p, batch_v=len(ids))
        np.random.seed(seed + attempt)
        RECORD.clear()
        out = d.trainMerge(list(ids)) if kind == "train" else d.valMerge(list(ids))
        rec = MergeDraws.record_arrays(RECORD)
        draws = MergeDraws.replay(kind, rec["draw_kind"], rec["draw_shape"], rec["draw_val"], len(ids))
        m = merge_ref.Margins()
        fn = merge_ref.train_merge if kind == "train" else merge_ref.val_merge
        ref = fn(scenes, names, ids, draws, cfg, margins=m)
        if m.voxel < MARGIN or m.crop < MARGIN:
            continue
        if expect is not None and not expect(out, ref, draws):
            continue
        break
    else:
        raise SystemExit("%s: no seed met the case's conditions" % case)
    for k in ("xyz_voxel", "feat_voxel", "xyz_original", "sem", "ins", "inst_info", "instance_pointnum", "v2p_index"):
        a, b = _np(out[k]), ref[k]
        assert a.shape == b.shape and a.dtype == b.dtype, (case, k, a.shape, b.shape, a.dtype, b.dtype)
        if k in ("xyz_original", "inst_info"):
            ulp = np.spacing(np.abs(a).astype(np.float32))
            assert (np.abs(a - b) <= ulp).all(), (case, k)
        else:
            assert np.array_equal(a, b), (case, k)
    assert list(out["fn"]) == ref["fn"]
    save = dict(kind=np.array(kind), names=np.array(names), ids=np.asarray(ids, np.int64), voxel_size=VOXEL, scale_size=1,
                max_crop_p=max_crop_p, min_crop_p=min_crop_p, seed=seed + attempt,
                voxel_margin=m.voxel, crop_margin=m.crop, **rec)
    if kind == "train":
        save["crop_used"] = ref["crop_used"]
        save["crop_success"] = ref["crop_success"]
    for j, n in enumerate(names):
        for k, v in scenes[n].items():
            save["scene%d_%s" % (j, k)] = v
    for k in ("xyz_voxel", "feat_voxel", "xyz_original", "sem", "ins", "inst_info", "instance_pointnum", "v2p_index"):
        save["out_" + k] = _np(out[k])
    if kind == "val":
        save["out_sup"] = np.asarray(out["sup"])
    path = os.path.join(HERE, "merge_%s.npz" % case)
    np.savez_compressed(path, **save)
    print("%s: %d points, %d voxels, %d instances, seed %d, margins voxel %.2e crop %.2e, %d bytes"
          % (case, save["out_xyz_original"].shape[0], save["out_xyz_voxel"].shape[0], save["out_instance_pointnum"].size,
             seed + attempt, m.voxel, m.crop, os.path.getsize(path)))
    assert os.path.getsize(path) < 500 * 1024


def main():
    base = {"sceneA": scene(11), "sceneB": scene(12, n_boxes=4), "sceneC": scene(13, n_boxes=2)}
    n_one = max(s["xyz"].shape[0] for s in base.values())

    def cropped(out, ref, draws):
        return all(u > 1 for u in ref["crop_used"]) and out["xyz_original"].shape[0] < 2 * n_one

    run("T1", "train", base, [0, 2], max_crop_p=int(1.2 * n_one), min_crop_p=int(0.3 * n_one), seed=100, expect=cropped)

    def all_fail(out, ref, draws):
        return bool((ref["crop_used"] > 0).all() and not ref["crop_success"].any())
    run("T2", "train", base, [1], max_crop_p=int(1.2 * n_one), min_crop_p=int(1.15 * n_one), seed=300, expect=all_fail)

    small = {"sceneA": scene(11, pitch=0.11), "sceneB": scene(12, n_boxes=4, pitch=0.11), "sceneC": scene(13, n_boxes=2, pitch=0.11)}
    empty = dict(small)
    empty["sceneA"] = dict(small["sceneA"], ins_label=np.full_like(small["sceneA"]["ins_label"], -100))
    run("T3", "train", empty, [0, 1], seed=500,
        expect=lambda out, ref, draws: np.floor(draws.scenes[0].mix_u * 3) != 0)
    run("V1", "val", small, [1], seed=700)
    run("V2", "val", small, [0, 2], seed=900)


if __name__ == "__main__":
    main()
