"""GPU tier at scale: DeviceMerge.train_merge of four configs[1]-sized scenes with mix-up and generator draws against the
float64 restatement (tests/merge_ref.py) under the golden tolerances, bit-identical on a repeat, feeding one model_fn
training step; val_merge of two scenes into model_fn_eval; the no-crop and no-instance edges; on small scenes the merge
without mix-up, hand-edited draws that mix elastic and plain units, and the crop that runs out of triples."""
import numpy as np
import pytest
import torch

import merge_ref
from pbnet_amd.config import get_config
from pbnet_amd.loader import DeviceMerge, MergeDraws, SceneCache

DEV = torch.device("cuda:0")


@pytest.fixture(scope="module")
def big():
    scenes = merge_ref.synth_scenes(range(2, 8))
    names = sorted(scenes)
    return scenes, names, SceneCache(scenes, DEV, train=names, val=names)


def _draws(merge, cache, ids, seed):
    names = cache.train
    gen = torch.Generator().manual_seed(seed)

    def merged(i, mix_id):
        return cache.host[names[ids[i]]]["n"] + cache.host[names[mix_id]]["n"]
    return MergeDraws.draw_train(gen, len(ids), len(names), merged, merge.cfg.max_crop_p)


@pytest.mark.gpu
def test_train_merge_at_scale(big):
    scenes, names, cache = big
    cfg = get_config(batch_size=4)
    merge = DeviceMerge(cache, cfg, seed=7)
    ids = [0, 1, 2, 3]
    draws = _draws(merge, cache, ids, 11)
    got = merge.train_merge(ids, draws)
    assert merge.readbacks == 4
    assert got["xyz_original"].shape[0] > 4 * 150000
    want = merge_ref.train_merge(scenes, names, ids, draws, cfg)
    assert np.array_equal(merge.last_crop_used, want["crop_used"])
    merge_ref.assert_batch(merge_ref.to_numpy(got), want, "train x4")
    again = merge.train_merge(ids, draws)
    for k in merge_ref.OUT_KEYS:
        assert torch.equal(got[k], again[k]), k
    # one training step on the batch
    from pbnet_amd.network.PBNet import PBNet, model_fn
    torch.manual_seed(22)
    model = PBNet(cfg).to(DEV).train()
    loss, _, visual, _ = model_fn(got, model, 1, cfg, "train")
    assert torch.isfinite(loss) and np.isfinite(visual["loss"])
    loss.backward()


@pytest.mark.gpu
def test_train_merge_seeded_is_reproducible(big):
    _, _, cache = big
    cfg = get_config(batch_size=2)
    a = DeviceMerge(cache, cfg, seed=3).train_merge([4, 5])
    b = DeviceMerge(cache, cfg, seed=3).train_merge([4, 5])
    c = DeviceMerge(cache, cfg, seed=4).train_merge([4, 5])
    for k in merge_ref.OUT_KEYS:
        assert torch.equal(a[k], b[k]), k
    assert a["xyz_original"].shape != c["xyz_original"].shape or not torch.equal(a["xyz_original"], c["xyz_original"])


@pytest.mark.gpu
def test_val_merge_feeds_model_fn_eval(big):
    scenes, names, cache = big
    cfg = get_config(test=True)
    merge = DeviceMerge(cache, cfg, seed=5)
    draws = MergeDraws.draw_val(torch.Generator().manual_seed(5), 2)
    got = merge.val_merge([1, 4], draws)
    want = merge_ref.val_merge(scenes, names, [1, 4], draws, cfg)
    merge_ref.assert_batch(merge_ref.to_numpy(got), want, "val x2")
    assert got["fn"] == [names[i] for i in (1, 4, 1, 4, 1, 4)]
    assert torch.equal(got["sup"].cpu(), torch.from_numpy(scenes[names[4]]["sup"]))
    from pbnet_amd.network.PBNet import PBNet, model_fn_eval
    torch.manual_seed(22)
    model = PBNet(cfg).to(DEV).eval()
    with torch.no_grad():
        pred = model_fn_eval(got, model, 1, cfg, n_batch=len(got["fn"]))      # 3B copies (the reference hard-codes 3)
    assert pred["sem"].shape[0] == got["xyz_original"].shape[0]


@pytest.mark.gpu
def test_edges_no_crop_and_no_instances():
    scenes = merge_ref.synth_scenes([21, 22, 23], pitch=0.06)
    names = sorted(scenes)
    scenes[names[0]]["ins_label"][:] = -100
    scenes[names[1]]["ins_label"][:] = -100
    cache = SceneCache(scenes, DEV, train=names, val=names)
    cfg = get_config(batch_size=3)                  # max_crop_p 300000: these scenes never crop
    merge = DeviceMerge(cache, cfg, seed=9)
    ids = [0, 1, 2]
    draws = _draws(merge, cache, ids, 9)
    assert all(s.crop.shape[0] == 0 for s in draws.scenes)
    got = merge.train_merge(ids, draws)
    assert (merge.last_crop_used == 0).all()
    want = merge_ref.train_merge(scenes, names, ids, draws, cfg)
    merge_ref.assert_batch(merge_ref.to_numpy(got), want, "edges")
    # every scene without instances: inst_info all -100, no instance_pointnum, the -99 running offset of the reference
    merge2 = DeviceMerge(cache, cfg)
    d2 = _draws(merge2, cache, [0, 1], 12)
    for s in d2.scenes:
        s.mix_u = 0.5 / 3                          # partner = names[0]: no instances either
    got2 = merge2.train_merge([0, 1], d2)
    want2 = merge_ref.train_merge(scenes, names, [0, 1], d2, cfg)
    merge_ref.assert_batch(merge_ref.to_numpy(got2), want2, "no instances")
    assert got2["instance_pointnum"].numel() == 0 and (got2["inst_info"] == -100).all()


# ---- branches the generator's draws never take: no mix-up, mixed gates, a crop that runs out of triples -----------------------
@pytest.fixture(scope="module")
def small():
    scenes = merge_ref.synth_scenes([31, 32, 33, 34], pitch=0.06)
    names = sorted(scenes)
    return scenes, names, SceneCache(scenes, DEV, train=names, val=names)


def _draws_single(cache, ids, seed, max_crop_p):
    names = cache.train
    gen = torch.Generator().manual_seed(seed)
    return MergeDraws.draw_train(gen, len(ids), len(names), lambda i, mix_id: cache.host[names[ids[i]]]["n"], max_crop_p,
                                 mixup=False)


@pytest.mark.gpu
@pytest.mark.parametrize("crops", [False, True])
def test_train_merge_without_mixup(small, crops):
    """One unit per scene, each with the float32 pre-minimum; once under max_crop_p, once with the crop loop running."""
    scenes, names, cache = small
    n_min = min(cache.host[n]["n"] for n in names)
    cfg = get_config(batch_size=3, max_crop_p=n_min // 3, min_crop_p=n_min // 12) if crops else get_config(batch_size=3)
    merge = DeviceMerge(cache, cfg, seed=13, mixup=False)
    ids = [2, 0, 3]
    draws = _draws_single(cache, ids, 14, cfg.max_crop_p)
    assert all((s.crop.shape[0] > 0) == crops and s.partner is None for s in draws.scenes)
    got = merge.train_merge(ids, draws)
    want = merge_ref.train_merge(scenes, names, ids, draws, cfg, mixup=False)
    assert np.array_equal(merge.last_crop_used, want["crop_used"]) and (want["crop_used"] > 0).all() == crops
    merge_ref.assert_batch(merge_ref.to_numpy(got), want, "no mix-up, crop %s" % crops)
    assert got["fn"] == [names[i] for i in ids]


@pytest.mark.gpu
def test_train_merge_mixed_draws(small):
    """Elastic and non-elastic units in one call, a unit without scale, a unit without jitter and drawn angle."""
    scenes, names, cache = small
    cfg = get_config(batch_size=3)
    merge = DeviceMerge(cache, cfg, seed=15)
    ids = [1, 3, 0]
    draws = _draws(merge, cache, ids, 16)
    draws.scenes[0].primary.elastic_gate = 1.5                   # not elastic; its partner is
    draws.scenes[1].primary.scale = None
    draws.scenes[2].partner.jitter = None
    draws.scenes[2].partner.theta_u = None                       # the index-dependent default angle
    assert not draws.scenes[0].primary.elastic and draws.scenes[0].partner.elastic
    got = merge.train_merge(ids, draws)
    assert draws.scenes[0].primary.noise == [None, None] and draws.scenes[0].partner.noise[1] is not None
    want = merge_ref.train_merge(scenes, names, ids, draws, cfg)
    merge_ref.assert_batch(merge_ref.to_numpy(got), want, "mixed draws")


@pytest.mark.gpu
def test_train_merge_out_of_triples(small):
    """min_crop_p above max_crop_p: no try can succeed, five tries need at least five triples, the draws hold three."""
    scenes, names, cache = small
    n = cache.host[names[0]]["n"]
    cfg = get_config(batch_size=1, max_crop_p=n // 3, min_crop_p=n)
    merge = DeviceMerge(cache, cfg, seed=17, mixup=False)
    draws = _draws_single(cache, [0], 18, cfg.max_crop_p)
    assert draws.scenes[0].crop.shape[0] == 85
    draws.scenes[0].crop = draws.scenes[0].crop[:3]
    with pytest.raises(RuntimeError, match=r"crop triples ran out \(scenes \[0\], \[3\] drawn\)") as err:
        merge.train_merge([0], draws)
    assert "shrink levels" not in str(err.value)
