"""CPU tier: the association-log record (evaluate.decode_association_log) and evaluate.matches_from_table against the golden
vectors of the reference's tools/eval.py.  The log is packed by tests/ap_record_ref.py from tables that np.unique / np.bincount
build; rows, confidence bits, pairs and the AP tensor must match the golden exactly (the comparisons of tests/test_eval_gpu.py)."""
import glob
import os

import numpy as np
import pytest

import ap_record_ref as R
from pbnet_amd import evaluate as E

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = sorted(glob.glob(os.path.join(HERE, "golden", "eval_E*.npz")))


def sorted_rows(a):
    return a[np.lexsort(a.T[::-1])] if a.shape[0] else a


def flat(rec):
    """SceneMatches -> the golden's flat tables (class-major rows, pairs sorted)."""
    go = np.lexsort((rec.gt_id, rec.gt_class))
    po = np.lexsort((rec.pred_id, rec.pred_class))
    gt_rows = np.stack([rec.gt_class, rec.gt_id, rec.gt_vert], 1)[go].reshape(-1, 3)
    pred_rows = np.stack([rec.pred_class, rec.pred_id, rec.pred_vert, rec.pred_void], 1)[po].reshape(-1, 4)
    q, g = np.nonzero(rec.inter)
    pairs = np.stack([rec.pred_id[q], rec.gt_id[g], rec.inter[q, g]], 1).reshape(-1, 3)
    return gt_rows, pred_rows, np.asarray(rec.pred_conf, np.float32)[po], sorted_rows(pairs)


def same_ap(a, b):
    return np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(np.nan_to_num(a, nan=-1.0), np.nan_to_num(b, nan=-1.0))


def check_scene(rec, g, s):
    gt_rows, pred_rows, conf, pairs = flat(rec)
    assert np.array_equal(gt_rows, g["s%d_gt_rows" % s])
    assert np.array_equal(pred_rows, g["s%d_pred_rows" % s])
    assert np.array_equal(conf.view(np.int32), g["s%d_pred_conf" % s].view(np.int32))
    assert np.array_equal(pairs, sorted_rows(g["s%d_pairs" % s]))


def check_epoch(matches, g):
    ap = E.evaluate_matches(matches)
    assert same_ap(ap, g["ap"])
    avgs = E.compute_averages(ap)
    assert np.array_equal(np.array([avgs["all_ap"], avgs["all_ap_50%"], avgs["all_ap_25%"]], np.float64), g["avg"],
                          equal_nan=True)


def finish_epoch(matches, dropped, g, names):
    """Every scene with predictions is checked from the log.  A golden scene WITHOUT predictions (eval_E2 has one) is a
    header-only record: the log reports it and keeps none of its tables, as train.py:217-219 skips such a scene.  tools/eval.py,
    which made the golden AP, counts that scene's ground truth as misses, so for the AP comparison its prediction-free entry is
    built from the host tables through matches_from_table and put back in scene order."""
    empty = [names[s] for s in range(len(names)) if g["s%d_label" % s].shape[0] == 0]
    assert dropped == empty and list(matches) == [n for n in names if n not in empty]
    full = {}
    for s, name in enumerate(names):
        if name in empty:
            t = golden_scene(g, s)
            full[name] = E.matches_from_table(name, t["inter_all"], t["uid"], t["counts"], t["label_id"], t["conf"])
        else:
            assert matches[name].scene == name
            full[name] = matches[name]
        check_scene(full[name], g, s)
    check_epoch(full, g)


def golden_scene(g, s):
    inter, uid, counts = R.tables(g["s%d_mask" % s], g["s%d_gt" % s])
    return dict(n_pts=int(g["s%d_gt" % s].shape[0]), inter_all=inter, uid=uid, counts=counts, label_id=g["s%d_label" % s],
                conf=g["s%d_conf" % s])


@pytest.mark.parametrize("path", CASES, ids=[os.path.basename(p)[:-4] for p in CASES])
def test_packed_log_decodes_to_the_golden(path):
    g = np.load(path)
    n = int(g["n_scenes"])
    names = ["scene%04d_00" % s for s in range(n)]
    matches, dropped = E.decode_association_log(R.pack_log([golden_scene(g, s) for s in range(n)]), names)
    finish_epoch(matches, dropped, g, names)


@pytest.mark.parametrize("path", CASES, ids=[os.path.basename(p)[:-4] for p in CASES])
def test_matches_from_table_gives_the_golden_rows(path):
    g = np.load(path)
    matches = {}
    for s in range(int(g["n_scenes"])):
        t = golden_scene(g, s)
        rec = E.matches_from_table("scene%04d_00" % s, t["inter_all"], t["uid"], t["counts"], t["label_id"], t["conf"])
        check_scene(rec, g, s)
        matches[rec.scene] = rec
    check_epoch(matches, g)


def test_header_only_record_is_dropped_and_reported():
    g = np.load(CASES[0])
    empty = dict(n_pts=500, inter_all=np.zeros((0, 2), np.int64), uid=np.array([0, 3001]), counts=np.array([400, 100]),
                 label_id=np.zeros(0, np.int64), conf=np.zeros(0, np.float32))
    log = R.pack_log([golden_scene(g, 0), empty, golden_scene(g, 1)])
    assert log.shape[0] == R.pack_log([golden_scene(g, 0)]).shape[0] + R.HEADER + R.pack_log([golden_scene(g, 1)]).shape[0]
    matches, dropped = E.decode_association_log(log, ["a", "none", "b"])
    assert dropped == ["none"] and list(matches) == ["a", "b"]
    check_scene(matches["a"], g, 0)
    check_scene(matches["b"], g, 1)
    assert E.decode_association_log(np.zeros(0, np.int32), []) == ({}, [])


@pytest.mark.parametrize("bit", [bit for bit, _ in E.AP_STATUS])
def test_each_status_bit_raises_with_the_scene_name(bit):
    g = np.load(CASES[0])
    log = R.pack_log([golden_scene(g, 0), dict(golden_scene(g, 1), status=bit)])
    with pytest.raises(ValueError) as err:
        E.decode_association_log(log, ["fine_scene", "bad_scene"])
    text = dict(E.AP_STATUS)[bit]
    assert "bad_scene" in str(err.value) and text in str(err.value) and "fine_scene" not in str(err.value)


def test_a_damaged_log_is_refused():
    g = np.load(CASES[0])
    log = R.pack_log([golden_scene(g, 0)])
    with pytest.raises(ValueError):
        E.decode_association_log(log[:-1], ["a"])
    bad = log.copy()
    bad[0] = 7
    with pytest.raises(ValueError):
        E.decode_association_log(bad, ["a"])


def test_config_key_is_off_by_default():
    from pbnet_amd.config import get_config
    assert get_config().device_ap is False and get_config().device_post is False
