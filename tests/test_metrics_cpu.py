"""CPU tier of the validation meters (pbnet_amd/validate.py): the integer restatement against every golden count, the
meters' host arithmetic against the reference's float32 results, the 2^24 divergence, argument refusals, the reduction over
a gloo world of 2, and the log line of ValidationEpoch.finish().

Tolerance of the ratios: the reference forms each in float32 (a sum over K, one add of 1e-10, one division, one mean over K:
at most K + 3 roundings of 2^-24, 23 x 6e-8 = 1.4e-6 at K = 20), this package in float64 from the same integers: relative
2e-6.  A class with zero union compares as exactly 0.  Counts are integers: equality."""
import glob
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import metrics_ref as R
from pbnet_amd import validate as V
from pbnet_amd.config import get_config

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SEM_CASES = ["S1", "S2", "S3", "S4_K2", "S4_K13"]
RTOL = 2e-6


def load(name):
    return dict(np.load(os.path.join(GOLDEN, "metrics_%s.npz" % name)))


def scenes(g):
    off = np.concatenate([[0], np.cumsum(g["lens"])])
    return [(g["pred"][a:b].astype(np.int64), g["target"][a:b].astype(np.int64)) for a, b in zip(off[:-1], off[1:])]


def as_meter_counts(iut):
    """golden (intersection, union, target) -> the meter's (intersection, output, target)."""
    inter, union, tgt = (np.asarray(a, np.int64) for a in iut)
    return np.stack([inter, union - tgt + inter, tgt])


def close(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape
    assert np.array_equal(got == 0, want == 0)
    assert np.all(np.abs(got - want) <= RTOL * np.abs(want)), (got, want)


def test_fixtures_are_small_and_complete():
    files = sorted(glob.glob(os.path.join(GOLDEN, "metrics_*.npz")))
    assert [os.path.basename(f)[8:-4] for f in files] == sorted(SEM_CASES + ["M1"])
    assert all(os.path.getsize(f) < 244 * 1024 for f in files)
    for name in SEM_CASES:
        g = load(name)
        assert float(g["sum_f32"].max()) < 2 ** 24 and np.array_equal(g["sum_f32"], g["sum_counts"])


@pytest.mark.parametrize("name", SEM_CASES)
def test_restatement_equals_every_golden_count(name):
    g = load(name)
    K = int(g["K"])
    for s, (pred, target) in enumerate(scenes(g)):
        inter, out, tgt, conf = R.sem_counts(pred, target, K, int(g["ignore_index"]), confusion=True)
        assert np.array_equal(np.stack([inter, out + tgt - inter, tgt]), g["scene_counts"][s])
        assert np.array_equal(np.diag(conf), inter)
        # the reference's own sequence of torch operations, on CPU tensors
        ref = R.reference_form_torch(torch.from_numpy(pred), torch.from_numpy(target), K)
        assert np.array_equal(np.stack(ref), g["scene_f32"][s])


def test_s2_has_out_of_range_targets_that_still_count_their_prediction():
    g = load("S2")
    K = 20
    pred, target = (np.concatenate(x) for x in zip(*scenes(g)))
    odd = (target != -100) & ((target < 0) | (target >= K)) & (pred >= 0) & (pred < K)
    assert odd.sum() > 10
    _, out, _ = R.sem_counts(pred, target, K)
    _, out_wo, _ = R.sem_counts(pred[~odd], target[~odd], K)
    assert out.sum() == out_wo.sum() + odd.sum()


@pytest.mark.parametrize("name", SEM_CASES)
def test_semantic_meter_host_arithmetic(name):
    g = load(name)
    K = int(g["K"])
    m = V.SemanticMeter(K, device="cpu")
    for s in range(g["lens"].shape[0]):
        m.merge_(as_meter_counts(g["scene_counts"][s]))
        close(m.accuracy_val(), g["accuracy_val"][s])
    res = m.result()
    assert np.array_equal(np.stack([res["intersection"], res["union"], res["target"]]), g["sum_counts"])
    assert res["intersection"].dtype == np.int64 and res["iou_class"].dtype == np.float64
    for key in ("iou_class", "accuracy_class", "mIoU", "mAcc", "allAcc"):
        close(res[key], g[key])
    if name == "S1":
        assert g["sum_counts"][1][15] == 0 and res["iou_class"][15] == 0.0      # the absent class: 0 / 1e-10
    # merging a meter == merging its counts
    m2 = V.SemanticMeter(K, device="cpu").merge_(m)
    assert np.array_equal(m2.result()["intersection"], res["intersection"])


def test_mask_meter_host_arithmetic():
    g = load("M1")
    assert list(g["raised"]) == [False, False, False, True, False] and g["rows"].shape == (4, 8)
    off = np.concatenate([[0], np.cumsum(g["lens"])])
    m = V.MaskAccuracyMeter()
    k = 0
    for s, (a, b) in enumerate(zip(off[:-1], off[1:])):
        row = R.mask_row(g["pred"][a:b], g["gt"][a:b])
        if not g["raised"][s]:
            assert np.array_equal(row, g["rows"][k])
            k += 1
        m.merge_(row)
    res = m.result()
    assert res["scenes"] == 4 and res["skipped"] == 1 and res["n_nan"] == 0
    close(res["All_mask_acc"], g["All_mask_acc"])
    close(res["Fp_acc"], g["Fp_acc"])
    assert np.isnan(g["Tp_acc"]) and np.isnan(res["Tp_acc"])                     # the scene without positives: 0 / 0 upstream
    tot = g["rows"].sum(0)
    assert res["Tp_acc_pooled"] == tot[3] / tot[2] and res["All_mask_acc_pooled"] == tot[1] / tot[0]
    assert res["Fp_acc_pooled"] == 1.0 - tot[5] / tot[4]
    # without the poisoned scene the mean over scenes is a number again
    ok = V.MaskAccuracyMeter().merge_(g["rows"][[0, 1, 3]]).result()
    assert 0.5 < ok["Tp_acc"] < 1.0


def test_float32_sums_stall_at_2_pow_24_and_integers_do_not():
    ref = V.AverageMeter()                                     # tools/log.py:16-30 on the reference's float32 vectors
    ref.update(np.array([2 ** 24, 5], np.float32))
    ref.update(np.array([1, 1], np.float32))
    assert ref.sum[0] == 2 ** 24 and ref.sum[1] == 6           # the large class stopped growing
    m = V.SemanticMeter(2, device="cpu")
    m.merge_(np.array([[2 ** 24, 5]] * 3))
    m.merge_(np.array([[1, 1]] * 3))
    assert m.result()["intersection"].tolist() == [2 ** 24 + 1, 6]


def test_cpu_tensors_and_bad_class_counts_are_refused():
    p = torch.zeros(8, dtype=torch.int64)
    with pytest.raises(RuntimeError):
        V.SemanticMeter(20, device="cpu").update(p, p)
    with pytest.raises(RuntimeError):
        V.intersectionAndUnionGPU(p, p, 20)
    with pytest.raises(RuntimeError):
        V.MaskAccuracyMeter().update(torch.zeros(8), p)
    for K in (1, 65, 0):
        with pytest.raises(ValueError):
            V.SemanticMeter(K, device="cpu")
        with pytest.raises(ValueError):
            V.intersectionAndUnionGPU(p, p, K)


def test_c_abi_refuses_before_any_launch():
    """The argument checks run on the host before any launch: no GPU needed, the pointers are never dereferenced."""
    from pbnet_amd import _native as N
    lib, fake = N.lib(), 1 << 20
    sem = lambda n, K, pred=fake, tgt=fake, acc=fake, f=(1, 1): lib.pbn_sem_confusion(pred, f[0], tgt, f[1], n, K, -100, acc, None, None)  # noqa: E731
    assert sem(10, 1) == sem(10, 65) == sem(-1, 20) == N.PBN_ERR_ARG
    assert sem(10, 20, acc=None) == sem(10, 20, pred=None) == sem(10, 20, tgt=None) == N.PBN_ERR_ARG
    assert sem(10, 20, f=(2, 0)) == sem(10, 20, pred=fake + 4) == N.PBN_ERR_ARG
    assert sem(0, 20) == sem(0, 20, pred=None, tgt=None) == N.PBN_OK          # nothing to do, nothing launched
    mask = lambda n, dt=0, pred=fake, gt=fake, row=fake: lib.pbn_mask_accuracy(pred, dt, gt, 1, n, 0.5, row, None)  # noqa: E731
    assert mask(-1) == mask(4, dt=3) == mask(4, row=None) == mask(4, pred=None) == mask(4, gt=None) == N.PBN_ERR_ARG


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _reduce_worker(rank, world, port, out):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    g, gm = load("S1"), load("M1")
    sem = V.SemanticMeter(20, device="cpu", confusion=True)
    for s in range(rank, 5, world):                             # rank 0: scenes 0, 2, 4; rank 1: 1, 3
        sem.merge_(as_meter_counts(g["scene_counts"][s]), confusion=np.full((20, 20), s + 1))
    last = sem.accuracy_val()
    sem.all_reduce()
    mask = V.MaskAccuracyMeter().merge_(gm["rows"][rank::world])
    mask.gather_()
    res = sem.result()
    out[rank] = (np.stack([res["intersection"], res["union"], res["target"]]), res["confusion"][0, 0], last,
                 sem.accuracy_val(), mask.rows())
    dist.destroy_process_group()


def test_all_reduce_over_gloo_world_of_two():
    world = 2
    out = mp.Manager().dict()
    mp.spawn(_reduce_worker, args=(world, _free_port(), out), nprocs=world, join=True)
    g, gm = load("S1"), load("M1")
    for r in range(world):
        counts, conf00, last_before, last_after, rows = out[r]
        assert np.array_equal(counts, g["sum_counts"])
        assert conf00 == 1 + 2 + 3 + 4 + 5
        assert last_before == last_after                         # the last-update counts stay local
        assert np.array_equal(rows, np.concatenate([gm["rows"][0::2], gm["rows"][1::2]]))
    close(out[0][2], g["scene_counts"][4][0].sum() / (g["scene_counts"][4][2].sum() + 1e-10))


class _Log(object):
    def __init__(self):
        self.lines, self.scalars = [], []

    def info(self, line):
        self.lines.append(line)

    def add_scalar(self, tag, value, step):
        self.scalars.append((tag, float(value), step))


def test_validation_epoch_finish_formats_the_reference_line():
    g = load("S1")
    log = _Log()
    cfg = get_config()
    ve = V.ValidationEpoch(None, cfg, 4, logger=log, writer=log, device="cpu")
    assert not ve.cluster
    ve.semantic.merge_(as_meter_counts(g["sum_counts"]))
    out = ve.finish()
    want = "mIoU/mAcc/allAcc {:.4f}/{:.4f}/{:.4f}.".format(float(g["mIoU"]), float(g["mAcc"]), float(g["allAcc"]))
    assert log.lines == [want] and want == "mIoU/mAcc/allAcc 0.7748/0.8609/0.9208."
    assert [t for t, _, _ in log.scalars] == ["val/mIOU_eval", "val/mAcc_eval", "val/allACC_eval"]
    assert all(step == 4 for _, _, step in log.scalars)
    close(out["mIoU"], g["mIoU"])
    assert not {"All_mask_acc", "mask", "avgs", "mAP", "matches"} & set(out)
    with pytest.raises(ValueError, match="n_batch"):
        ve.step({"fn": ["a"] * 6})
