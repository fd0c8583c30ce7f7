"""CPU tier: tests/ap_table_ref.py, the numpy restatement the device AP table is checked against, is itself checked here: on the
reference's golden epochs it must give evaluate_matches(decode_association_log(...)) and the golden's reference-made AP bit for
bit, NaN pattern included; on crafted and random logs it must agree with the host evaluator, and the crafted rules must come out
as tools/eval.py:27-190 states them."""
import numpy as np
import pytest

import ap_table_cases as C
import ap_table_ref as T
from pbnet_amd import evaluate as E


def same_bits(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and \
        np.array_equal(a[~np.isnan(a)].view(np.int32), b[~np.isnan(b)].view(np.int32))


def host_ap(words, n):
    matches, _, _ = E.decode_association_log(words, ["s%d" % i for i in range(n)], on_status="skip")
    return E.evaluate_matches(matches)


def test_constants_are_the_evaluators():
    assert T.CLASS_IDS == tuple(int(c) for c in E.VALID_CLASS_IDS) and T.MIN_REGION == E.MIN_REGION_SIZE
    assert np.array_equal(T.OVERLAPS, E.OVERLAPS) and (T.MAGIC, T.HEADER) == (E.AP_RECORD_MAGIC, E.AP_RECORD_HEADER)


@pytest.mark.parametrize("path", C.GOLDEN, ids=C.GOLDEN_IDS)
def test_restatement_gives_the_golden_ap(path):
    scenes, golden = C.golden_scenes(path)
    words = C.pack(scenes)
    ref = T.evaluate_logs([words])
    assert ref["malformed"] is None and ref["directory"].shape[0] == len(scenes)
    assert same_bits(ref["ap"], host_ap(words, len(scenes)))
    assert same_bits(ref["ap"], golden)


@pytest.mark.parametrize("seed", [1, 2])
def test_restatement_agrees_with_the_host_evaluator_on_random_epochs(seed):
    scenes = C.random_scenes(seed)
    words = C.pack(scenes)
    ref = T.evaluate_logs([words])
    assert same_bits(ref["ap"], host_ap(words, len(scenes)))
    assert int(ref["cells"][:, :, 0].sum()) > 0 and int(ref["cells"][:, :, 3].max()) <= 16      # 16 distinct scores: ties


def test_crafted_rules():
    scenes = C.crafted_scenes()
    words = C.pack(scenes)
    ref = T.evaluate_logs([words])
    assert same_bits(ref["ap"], host_ap(words, len(scenes)))
    entries, cells, ap = ref["entries"], ref["cells"], ref["ap"][0]
    bits = lambda v: int(np.float32(v).view(np.int32))                                                 # noqa: E731
    # the second hit is a false positive at the lower score and stays unvisited: at 0.25 it then takes the other instance
    assert entries[C.CHAIR][C.O25] == sorted([(bits(0.8), 0), (bits(0.9), 1), (bits(0.8), 1)])
    # from 0.5 on it is lonely and its instance is missed (the BED record's chair instance is the other miss)
    assert entries[C.CHAIR][C.O50] == [(bits(0.8), 0), (bits(0.9), 1)] and cells[C.CHAIR, C.O50, 2] == 2
    assert cells[C.CHAIR, C.O25, 2] == 1
    # equal scores of a true and a false positive: one distinct score
    assert entries[C.SOFA][C.O50] == [(bits(0.5), 0), (bits(0.5), 1)] and cells[C.SOFA, C.O50, 3] == 1
    assert entries[C.SOFA][C.O25] == [(bits(0.5), 0), (bits(0.5), 1)]
    # IoU exactly at the threshold is not above it; one step lower it is
    for cls, at, lower in ((C.TABLE, C.O50, C.O25), (C.DOOR, C.O60, C.O55), (C.CABINET, C.O70, C.O65)):
        assert cells[cls, at, 1] == 0 and cells[cls, at, 2] == 1 and cells[cls, lower, 1] == 1 and cells[cls, lower, 2] == 0
    # the ignore ratio equal to the threshold keeps the false positive
    assert entries[C.BED][C.O50] == [(bits(0.3), 0)] and entries[C.BED][C.O25] == [] and entries[C.BED][C.O55] == [(bits(0.3), 0)]
    # only a too-small instance above the threshold: nothing, and no ground truth that counts
    assert cells[6].sum() == 0 and np.isnan(ap[6]).all() and ref["flags"][0, 6] == 0 and ref["flags"][1, 6] == 1
    # dropped predictions: the instance is missed, nothing is predicted
    assert cells[7, :, 0].sum() == 0 and (cells[7, :, 2] == 1).all() and ref["flags"][1, 7] == 0 and (ap[7] == 0).all()
    assert ref["flags"][:, 8].tolist() == [1, 0] and (ap[8] == 0).all()                  # instances, no prediction
    assert ref["flags"][:, 9].tolist() == [0, 1] and np.isnan(ap[9]).all()               # predictions only
    assert ref["flags"][:, 10].tolist() == [1, 1] and cells[10, :, 0].sum() == 0 and (ap[10] == 0).all()
    # the directory names the record with status bits and the header-only one
    assert ref["directory"][-2:, 1:].tolist() == [[9, 4, 1], [10, 0, 0]]


def test_wide_records():
    """Past 64 predictions and 64 columns: the restatement against the host evaluator, and the hand-derived entries of the record
    whose hits lie in three different 64s."""
    scenes = C.wide_random_scenes(21) + [C.wide_scene(), C.many_columns_scene()]
    assert max(s["label_id"].shape[0] for s in scenes[:6]) > 128 and min(s["uid"].shape[0] for s in scenes[:6]) > 64
    words = C.pack(scenes)
    ref = T.evaluate_logs([words])
    assert same_bits(ref["ap"], host_ap(words, len(scenes)))
    only = T.evaluate_logs([C.pack([C.wide_scene()])])
    bits = lambda v: int(np.float32(v).view(np.int32))                                                 # noqa: E731
    assert only["entries"][C.CHAIR][C.O50] == [(bits(0.5), 0), (bits(0.6), 0), (bits(0.7), 1)]
    assert only["entries"][C.CHAIR][C.O25] == [(bits(0.5), 0), (bits(0.6), 0), (bits(0.7), 1), (bits(0.7), 1)]
    assert only["cells"][C.CHAIR, C.O50].tolist() == [3, 1, 1, 3] and only["cells"][C.CHAIR, C.O25].tolist() == [4, 2, 0, 3]
    many = T.evaluate_logs([C.pack([C.many_columns_scene()])])
    assert many["cells"][17, C.O50].tolist() == [1, 1, 0, 1] and many["cells"][17, 8].tolist() == [1, 0, 1, 1]


def test_truncated_log_stops_the_walk():
    words = C.pack(C.crafted_scenes()[:2])
    assert T.evaluate_logs([words[:-1]])["malformed"] == C.pack(C.crafted_scenes()[:1]).shape[0]
    with pytest.raises(ValueError):
        E.decode_association_log(words[:-1], ["a", "b"])
