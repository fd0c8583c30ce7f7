"""GPU tier of the validation meters: csrc/metrics.hip through pbnet_amd/validate.py and, for the error paths, the C ABI.
Counts are integers: every comparison of counts is equality.  Ratios against the reference's float32 results: relative
2e-6 (see tests/test_metrics_cpu.py for where that bound comes from)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import metrics_ref as R
from pbnet_amd import _native as N
from pbnet_amd import validate as V
from test_metrics_cpu import SEM_CASES, as_meter_counts, close, load, scenes

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
PAIRS = [(torch.int64, torch.int64), (torch.int64, torch.int32), (torch.int32, torch.int64), (torch.int32, torch.int32)]
SCORE_DTYPES = [torch.float32, torch.bfloat16, torch.float16]


def dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV, dtype)


def raw_counts(pred, target, K, confusion=True, ignore=-100):
    acc = torch.zeros(3 * K, dtype=torch.int64, device=DEV)
    conf = torch.zeros(K * K, dtype=torch.int64, device=DEV) if confusion else None
    V._sem_confusion(pred, target, K, ignore, acc, conf)
    return acc.cpu().numpy().reshape(3, K), (conf.cpu().numpy().reshape(K, K) if confusion else None)


def labels(rng, n, K, odd=True):
    target = rng.integers(0, K, n)
    pred = np.where(rng.random(n) < 0.8, target, rng.integers(0, K, n))
    target[rng.random(n) < 0.2] = -100
    if odd and n > 8:
        for arr in (pred, target):
            at = rng.choice(n, max(1, n // 40), replace=False)
            arr[at] = np.array([-1, K, K + 3, -99, -100])[rng.integers(0, 5, at.shape[0])]
    return pred.astype(np.int64), target.astype(np.int64)


@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: "%s-%s" % (str(p[0])[6:], str(p[1])[6:]))
@pytest.mark.parametrize("name", SEM_CASES)
def test_counts_equal_golden(name, pair):
    g = load(name)
    K = int(g["K"])
    meter = V.SemanticMeter(K, confusion=True)
    conf_sum = np.zeros((K, K), np.int64)
    for s, (pred, target) in enumerate(scenes(g)):
        p, t = dev(pred, pair[0]), dev(target, pair[1])
        acc, conf = raw_counts(p, t, K)
        assert np.array_equal(np.stack([acc[0], acc[1] + acc[2] - acc[0], acc[2]]), g["scene_counts"][s])
        assert np.array_equal(np.diag(conf), acc[0])
        assert np.array_equal(conf, R.sem_counts(pred, target, K, confusion=True)[3])
        conf_sum += conf
        meter.update(p, t)
        assert torch.equal(p.cpu(), torch.from_numpy(pred).to(pair[0]))               # the kernel does not write pred
        close(meter.accuracy_val(), g["accuracy_val"][s])
    res = meter.result()                                                              # accumulation == the per-scene sum
    assert np.array_equal(np.stack([res["intersection"], res["union"], res["target"]]), g["sum_counts"])
    assert np.array_equal(res["confusion"], conf_sum)
    for key in ("iou_class", "accuracy_class", "mIoU", "mAcc", "allAcc"):
        close(res[key], g[key])


@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: "%s-%s" % (str(p[0])[6:], str(p[1])[6:]))
def test_views_at_every_element_offset_and_strided(pair):
    rng = np.random.default_rng(3)
    n, K = 4099, 20
    pred, target = labels(rng, n + 3, K)
    pb, tb = dev(pred, pair[0]), dev(target, pair[1])
    for op in range(4):
        for ot in range(4):
            m = n - (op + ot) % 3                                                   # lengths with every tail too
            acc, conf = raw_counts(pb[op:op + m], tb[ot:ot + m], K)
            want = R.sem_counts(pred[op:op + m], target[ot:ot + m], K, confusion=True)
            assert np.array_equal(acc, np.stack(want[:3])) and np.array_equal(conf, want[3]), (op, ot)
    acc, conf = raw_counts(pb[1::2], tb[::2][:pb[1::2].shape[0]], K)                 # non-contiguous inputs
    want = R.sem_counts(pred[1::2], target[::2][:pred[1::2].shape[0]], K, confusion=True)
    assert np.array_equal(acc, np.stack(want[:3])) and np.array_equal(conf, want[3])
    acc2, _ = raw_counts(pb[:4096].view(64, 64), tb[:4096].view(64, 64), K)          # any shape: flattened
    assert np.array_equal(acc2, np.stack(R.sem_counts(pred[:4096], target[:4096], K)))


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257, 1000003, 3 * 161517])
def test_sizes_against_restatement(n):
    rng = np.random.default_rng(n + 1)
    for K, pair in ((20, PAIRS[0]), (2, PAIRS[3]), (32, PAIRS[1]), (33, PAIRS[2]), (64, PAIRS[0])):
        if n > 100000 and K in (2, 33):
            continue
        pred, target = labels(rng, n, K)
        acc, conf = raw_counts(dev(pred, pair[0]), dev(target, pair[1]), K)
        want = R.sem_counts(pred, target, K, confusion=True)
        assert np.array_equal(acc, np.stack(want[:3])) and np.array_equal(conf, want[3]), (n, K)
        acc_only, _ = raw_counts(dev(pred, pair[0]), dev(target, pair[1]), K, confusion=False)
        assert np.array_equal(acc_only, acc)
    if 0 < n < 100000:                                                               # against the reference's own op sequence
        pred, target = labels(rng, n, 20)
        ref = R.reference_form_torch(dev(pred, torch.int64), dev(target, torch.int64), 20)
        acc, _ = raw_counts(dev(pred, torch.int64), dev(target, torch.int64), 20)
        assert np.array_equal(np.stack([acc[0], acc[1] + acc[2] - acc[0], acc[2]]), np.stack(ref).astype(np.int64))


def test_an_ignore_value_inside_the_class_range_follows_the_reference():
    """mIOU.py:24 writes the ignore value INTO output: with ignore_index = 5 those points land in bin 5 of output and of
    intersection.  Nobody configures that, but the restatement of the masked write covers it."""
    rng = np.random.default_rng(8)
    pred, target = labels(rng, 5000, 20, odd=False)
    target[target == -100] = 5
    acc, _ = raw_counts(dev(pred, torch.int64), dev(target, torch.int64), 20, confusion=False, ignore=5)
    ref = R.reference_form_torch(dev(pred, torch.int64), dev(target, torch.int64), 20, ignore_index=5)
    assert np.array_equal(np.stack([acc[0], acc[1] + acc[2] - acc[0], acc[2]]), np.stack(ref).astype(np.int64))


def test_counters_between_sentinels_and_added_not_written():
    K, mark = 20, 0x5A5A5A5A5A5A5A5A
    rng = np.random.default_rng(5)
    pred, target = labels(rng, 70001, K)
    buf = torch.full((8 + 3 * K + 8 + K * K + 8,), mark, dtype=torch.int64, device=DEV)
    acc, conf = buf[8:8 + 3 * K], buf[16 + 3 * K:16 + 3 * K + K * K]
    acc.fill_(7)
    conf.fill_(11)
    V._sem_confusion(dev(pred, torch.int32), dev(target, torch.int64), K, -100, acc, conf)
    h = buf.cpu().numpy()
    want = R.sem_counts(pred, target, K, confusion=True)
    assert np.array_equal(h[8:8 + 3 * K], np.concatenate(want[:3]) + 7)
    assert np.array_equal(h[16 + 3 * K:16 + 3 * K + K * K], want[3].reshape(-1) + 11)
    for a, b in ((0, 8), (8 + 3 * K, 16 + 3 * K), (16 + 3 * K + K * K, h.shape[0])):
        assert (h[a:b] == mark).all()
    row = torch.full((3, 8), mark, dtype=torch.int64, device=DEV)
    s, g = torch.rand(70001, device=DEV), torch.randint(0, 2, (70001,), device=DEV)
    rc = N.lib().pbn_mask_accuracy(s.data_ptr(), 0, g.data_ptr(), 1, 70001, 0.5, row[1].data_ptr(), N.current_stream())
    assert rc == 0
    h = row.cpu().numpy()
    assert (h[0] == mark).all() and (h[2] == mark).all()
    assert np.array_equal(h[1], R.mask_row(s.cpu().numpy(), g.cpu().numpy()))          # written, not added


def test_identical_on_two_runs_and_on_a_side_stream():
    K = 20
    rng = np.random.default_rng(6)
    pred, target = labels(rng, 3 * 161517, K)
    p, t = dev(pred, torch.int64), dev(target, torch.int64)
    first = raw_counts(p, t, K)
    second = raw_counts(p, t, K)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        third = raw_counts(p, t, K)
    torch.cuda.current_stream().wait_stream(side)
    for other in (second, third):
        assert np.array_equal(first[0], other[0]) and np.array_equal(first[1], other[1])
    assert np.array_equal(first[0], np.stack(R.sem_counts(pred, target, K)))


def test_update_neither_synchronises_nor_allocates():
    K = 20
    rng = np.random.default_rng(7)
    pred, target = labels(rng, 100003, K)
    p, t = dev(pred, torch.int64), dev(target, torch.int64)
    s, g = torch.rand(50000, 1, device=DEV), torch.randint(0, 2, (50000,), device=DEV)
    big_s, big_g = torch.rand(90000, device=DEV).bfloat16(), torch.randint(0, 2, (90000,), device=DEV)
    sem, mask = V.SemanticMeter(K, confusion=True), V.MaskAccuracyMeter()
    sem.update(p, t)
    mask.update(s, g)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        try:
            torch.ones(1, device=DEV).item()
            honoured = False
        except RuntimeError:
            honoured = True
        allocs = torch.cuda.memory_stats()["allocation.all.allocated"]
        sem.update(p[1:], t[1:])
        mask.update(s, g)
        mask.update(big_s, big_g)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    if not honoured:
        print("this ROCm build does not honour set_sync_debug_mode('error'): the no-synchronisation assertion was not made")
    assert torch.cuda.memory_stats()["allocation.all.allocated"] == allocs           # no allocation after the first call
    a = np.stack(R.sem_counts(pred, target, K)) + np.stack(R.sem_counts(pred[1:], target[1:], K))
    assert np.array_equal(sem.result()["intersection"], a[0]) and np.array_equal(sem.result()["target"], a[2])
    assert mask.rows().shape == (3, 8)


@pytest.mark.parametrize("dtype", SCORE_DTYPES, ids=lambda d: str(d)[6:])
def test_mask_rows_equal_golden(dtype):
    g = load("M1")
    off = np.concatenate([[0], np.cumsum(g["lens"])])
    meter = V.MaskAccuracyMeter(capacity=2)                                          # grows twice on the way
    for a, b in zip(off[:-1], off[1:]):
        score = dev(g["pred"][a:b], dtype).view(-1, 1)
        assert torch.equal(score.float().cpu().view(-1), torch.from_numpy(g["pred"][a:b]))   # the fixture is exact in `dtype`
        keep = score.clone()
        meter.update(score, dev(g["gt"][a:b], torch.int64))
        assert torch.equal(score, keep)                                              # pred_mask is not binarised in place
    assert np.array_equal(meter.rows(), g["rows"])
    res = meter.result()
    assert res["scenes"] == 4 and res["skipped"] == 1 and res["n_nan"] == 0
    close(res["All_mask_acc"], g["All_mask_acc"])
    close(res["Fp_acc"], g["Fp_acc"])
    assert np.isnan(res["Tp_acc"]) and np.isnan(g["Tp_acc"])
    assert 0.5 < res["Tp_acc_pooled"] < 1.0


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 65536, 65537, 300001])
def test_mask_sizes_offsets_nan_and_threshold_edges(n):
    rng = np.random.default_rng(n)
    score = rng.random(n + 3).astype(np.float32)
    edge = np.array([0.5, np.nextafter(np.float32(0.5), np.float32(0)), np.nextafter(np.float32(0.5), np.float32(1)), np.nan,
                     0.0, 1.0, -np.inf, np.inf], np.float32)
    at = rng.choice(n + 3, min(n + 3, 64), replace=False)
    score[at] = edge[np.arange(at.shape[0]) % edge.shape[0]]
    gt = rng.integers(0, 2, n + 3)
    gt[rng.choice(n + 3, max(1, n // 50), replace=False)] = -1                          # an unmutated ignore row agrees with nothing
    for dtype in SCORE_DTYPES:
        sb = dev(score, dtype)
        for gdt in (torch.int64, torch.int32):
            gb = dev(gt, gdt)
            for o in range(4 if n < 70000 else 2):
                meter = V.MaskAccuracyMeter()
                meter.update(sb[o:o + n], gb[(o + 1) % 4:(o + 1) % 4 + n])
                want = R.mask_row(sb[o:o + n].float().cpu().numpy(), gt[(o + 1) % 4:(o + 1) % 4 + n])
                assert np.array_equal(meter.rows()[0], want), (n, dtype, gdt, o)
    meter = V.MaskAccuracyMeter()
    meter.update(dev(score, torch.float32)[::2], dev(gt, torch.float32)[::2])          # strided, float targets: converted
    assert np.array_equal(meter.rows()[0], R.mask_row(score[::2], gt[::2]))


def test_shim_returns_the_reference_tensors_and_writes_in_place():
    g = load("S2")
    K = int(g["K"])
    for s, (pred, target) in enumerate(scenes(g)):
        output, tgt = dev(pred, torch.int64), dev(target, torch.int64)
        inter, union, area_t = V.intersectionAndUnionGPU(output, tgt, K, -100)
        for got, want in zip((inter, union, area_t), g["scene_f32"][s]):
            assert got.dtype == torch.float32 and got.device == output.device
            assert torch.equal(got.cpu(), torch.from_numpy(want))
        ign = target == -100
        assert ign.any() and (output.cpu().numpy()[ign] == -100).all()
        assert np.array_equal(output.cpu().numpy()[~ign], pred[~ign])
    m = V.SemanticMeter(K)
    m.merge_(as_meter_counts(g["sum_counts"]))                                        # host counts into device counters
    assert np.array_equal(m.result()["union"], g["sum_counts"][1])


def test_refused_arguments_write_nothing():
    K, mark = 20, 0x1234567
    lib = N.lib()
    p = torch.zeros(100, dtype=torch.int64, device=DEV)
    acc = torch.full((3 * 64 + 64 * 64,), mark, dtype=torch.int64, device=DEV)
    st = N.current_stream()

    def sem(pred, target, n, k, a, f=(1, 1)):
        return lib.pbn_sem_confusion(pred, f[0], target, f[1], n, k, -100, a, None, st)
    assert sem(p.data_ptr(), p.data_ptr(), 100, 1, acc.data_ptr()) == N.PBN_ERR_ARG
    assert sem(p.data_ptr(), p.data_ptr(), 100, 65, acc.data_ptr()) == N.PBN_ERR_ARG
    assert sem(p.data_ptr(), p.data_ptr(), -1, K, acc.data_ptr()) == N.PBN_ERR_ARG
    assert sem(None, p.data_ptr(), 100, K, acc.data_ptr()) == N.PBN_ERR_ARG
    assert sem(p.data_ptr(), None, 100, K, acc.data_ptr()) == N.PBN_ERR_ARG
    assert sem(p.data_ptr(), p.data_ptr(), 100, K, None) == N.PBN_ERR_ARG
    assert sem(p.data_ptr(), p.data_ptr(), 100, K, acc.data_ptr(), f=(1, 7)) == N.PBN_ERR_ARG
    assert sem(p.data_ptr(), p.data_ptr(), 0, K, acc.data_ptr()) == N.PBN_OK          # n == 0: PBN_OK, writes nothing
    row = acc[:8]
    s = torch.zeros(100, device=DEV)
    assert lib.pbn_mask_accuracy(s.data_ptr(), 5, p.data_ptr(), 1, 100, 0.5, row.data_ptr(), st) == N.PBN_ERR_ARG
    assert lib.pbn_mask_accuracy(s.data_ptr(), 0, p.data_ptr(), 1, -1, 0.5, row.data_ptr(), st) == N.PBN_ERR_ARG
    assert lib.pbn_mask_accuracy(None, 0, p.data_ptr(), 1, 100, 0.5, row.data_ptr(), st) == N.PBN_ERR_ARG
    assert lib.pbn_mask_accuracy(s.data_ptr(), 0, p.data_ptr(), 1, 100, 0.5, None, st) == N.PBN_ERR_ARG
    torch.cuda.synchronize()
    assert (acc.cpu().numpy() == mark).all()
    assert lib.pbn_mask_accuracy(None, 0, None, 1, 0, 0.5, row.data_ptr(), st) == N.PBN_OK   # n == 0: a zero row
    assert (acc.cpu().numpy()[:8] == 0).all() and (acc.cpu().numpy()[8:] == mark).all()
    with pytest.raises(TypeError):
        V.SemanticMeter(K).update(p.float(), p)
    with pytest.raises(ValueError):
        V.SemanticMeter(K).update(p[:50], p)
