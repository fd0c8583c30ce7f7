"""GPU tier: the device AP table (csrc/apeval.hip, evaluate.APTable) on host-packed association logs against
tests/ap_table_ref.py (itself pinned to the host evaluator and the reference's goldens by tests/test_ap_table_ref_cpu.py).

Bounds: `cells` and `flags` are integers and exact; the NaN pattern is exact; every AP cell is within ONE float32 ulp.  That margin
is derived: the device and numpy sum the same float64 terms in possibly different order, the sums differ by at most ~n * 2^-53
relative, and after rounding to float32 that is the same value or its neighbour."""
import numpy as np
import pytest
import torch

import ap_table_cases as C
import ap_table_ref as T
from pbnet_amd import _native as N
from pbnet_amd import evaluate as E

pytestmark = pytest.mark.gpu


def run_table(logs, rec_cap=64, entry_cap=None, names=None):
    """The table over host-packed logs (int32 word arrays), added in turn; (result of finish(), the APTable, raw output bytes)."""
    dev = torch.device("cuda:0")
    table = E.APTable(rec_cap, entry_cap, device=dev)
    for i, words in enumerate(logs):
        n_rec = len(T.walk(words)[0])
        state = torch.tensor([words.shape[0], words.shape[0], n_rec, 0, -1, 0, 0, 0], dtype=torch.int32, device=dev)
        dev_words = torch.from_numpy(np.ascontiguousarray(np.concatenate([words, np.zeros(1, np.int32)]))).to(dev)
        table.add_words(dev_words, state, int(words.shape[0]), (names[i] if names else ["log%d_%d" % (i, j) for j in range(n_rec)]))
    result = table.finish()
    return result, table, table.out.cpu().numpy().tobytes()


def ulps(a, b):
    """Distance in float32 steps between equal-shaped arrays without NaN."""
    key = lambda x: np.where(x.view(np.int32) < 0, np.int32(-2 ** 31) - x.view(np.int32), x.view(np.int32)).astype(np.int64)   # noqa: E731
    return np.abs(key(np.ascontiguousarray(a, np.float32)) - key(np.ascontiguousarray(b, np.float32)))


def check_against(result, table, ref, golden_ap=None):
    ap, _, _, cells = result
    assert np.array_equal(cells, ref["cells"])
    assert np.array_equal(table.flags, ref["flags"])
    assert np.array_equal(table.directory, ref["directory"])
    for want in [ref["ap"]] + ([] if golden_ap is None else [golden_ap]):
        assert ap.shape == want.shape and ap.dtype == np.float32
        assert np.array_equal(np.isnan(ap), np.isnan(want))
        live = ~np.isnan(want)
        assert int(ulps(ap[live], want[live]).max(initial=0)) <= 1


@pytest.mark.parametrize("path", C.GOLDEN, ids=C.GOLDEN_IDS)
def test_goldens(path):
    scenes, golden = C.golden_scenes(path)
    words = C.pack(scenes)
    result, table, _ = run_table([words])
    check_against(result, table, T.evaluate_logs([words]), golden)
    assert result[1] == [] and result[2] == []


def test_crafted_rules():
    """One record per rule (tests/ap_table_cases.crafted_scenes; the rules' expected entries are asserted on the restatement by
    tests/test_ap_table_ref_cpu.py): second hits, ties, IoU and ignore ratio exactly at a threshold, too-small instances, dropped
    predictions, the three empty-cell values, and the records that are left out."""
    words = C.pack(C.crafted_scenes())
    names = ["rule%d" % i for i in range(11)]
    (ap, dropped, failed, cells), table, _ = run_table([words], names=[names])
    check_against((ap, dropped, failed, cells), table, T.evaluate_logs([words]))
    assert dropped == ["rule10"] and failed == [("rule9", ["a ground-truth id is negative or >= id_cap"])]
    assert table.directory[-2:, 1:].tolist() == [[9, 4, 1], [10, 0, 0]]
    assert cells[C.CHAIR, C.O25].tolist() == [3, 2, 1, 2] and cells[C.CHAIR, C.O50].tolist() == [2, 1, 2, 2]
    assert cells[C.SOFA, C.O50].tolist() == [2, 1, 0, 1]
    assert (ap[0, 8] == 0).all() and np.isnan(ap[0, 9]).all() and (ap[0, 10] == 0).all() and table.flags[:, 10].tolist() == [1, 1]


def test_truncated_log_raises():
    words = C.pack(C.crafted_scenes()[:2])
    with pytest.raises(ValueError, match="word %d" % C.pack(C.crafted_scenes()[:1]).shape[0]):
        run_table([words[:-1]])


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_random_epochs(seed):
    words = C.pack(C.random_scenes(seed))
    result, table, _ = run_table([words])
    check_against(result, table, T.evaluate_logs([words]))


def test_wide_records():
    """Records past the 64-wide steps of the matching wave: 130-200 predictions (several ballots: a first hit in one, later hits in
    the next, a prediction visited in one ballot met again by a later instance) and 100-150 columns (several strides of the lonely
    scan and of the row sums), plus the record of tests/ap_table_cases.wide_scene, whose entries are derived by hand."""
    scenes = C.wide_random_scenes(21) + [C.wide_scene()]
    words = C.pack(scenes)
    result, table, _ = run_table([words], entry_cap=12 * sum(s["label_id"].shape[0] for s in scenes))
    check_against(result, table, T.evaluate_logs([words]))
    (ap, _, _, cells), table, _ = run_table([C.pack([C.wide_scene()])])
    assert cells[C.CHAIR, C.O50].tolist() == [3, 1, 1, 3] and cells[C.CHAIR, C.O25].tolist() == [4, 2, 0, 3]


def test_columns_beyond_the_lds_classes():
    """A record with more columns than a matching wave keeps classes for in LDS, the instances in the last columns."""
    words = C.pack([C.many_columns_scene()] + C.random_scenes(4, n_records=3))
    result, table, _ = run_table([words])
    check_against(result, table, T.evaluate_logs([words]))
    assert result[3][17, C.O50].tolist() == [1, 1, 0, 1] and result[3][17, 8].tolist() == [1, 0, 1, 1]


def test_record_with_too_many_predictions_raises():
    words = C.pack(C.crafted_scenes()[:1] + [C.too_many_predictions_scene()])
    with pytest.raises(ValueError, match="word %d of log 1 has more than 65535 predictions" % C.pack(C.crafted_scenes()[:1]).shape[0]):
        run_table([words], entry_cap=1 << 17)
    result, table, _ = run_table([C.pack([C.too_many_predictions_scene(65535)])], entry_cap=1 << 17)   # the largest record that is served
    assert int(result[3].sum()) == 0 and result[1] == [] and table.directory.tolist() == [[0, 0, 0, 65535]]


def test_overflow_is_answered_with_the_wanted_capacity():
    """evaluate.ap_table_of_logs, the form behind ValidationEpoch and the serving front: capacities that are too small cost a
    second pass over the logs, not the epoch."""
    dev = torch.device("cuda:0")
    scenes = C.random_scenes(5, n_records=12)
    words = C.pack(scenes)
    log = E.AssociationLog(1, 1, log_words=int(words.shape[0]), device=dev)
    log.log.copy_(torch.from_numpy(words))
    log.state[:4] = torch.tensor([words.shape[0], words.shape[0], 12, 0], dtype=torch.int32)
    log.names = ["s%d" % i for i in range(12)]
    ref = T.evaluate_logs([words])
    for rec_cap, entry_cap in ((12, 64), (3, 64), (12, 1000), (None, None)):
        ap, dropped, failed, cells, table = E.ap_table_of_logs([log], rec_cap=rec_cap, entry_cap=entry_cap)
        check_against((ap, dropped, failed, cells), table, ref)
        assert table.rec_cap >= 12 and table.entry_cap >= int(ref["cells"][:, :, 0].sum())


def test_cell_above_the_lds_segment():
    """Many records of one class: the largest cell exceeds pbn_ap_table_lds_entries(), so it is sorted and integrated in global
    memory, next to cells that stay in LDS."""
    words = C.pack(C.random_scenes(7, n_records=200, one_class=True) + C.random_scenes(8, n_records=5))
    ref = T.evaluate_logs([words])
    lds = N.lib().pbn_ap_table_lds_entries()
    assert int(ref["cells"][:, :, 0].max()) > lds > int(ref["cells"][:, :, 0][ref["cells"][:, :, 0] > 0].min())
    result, table, _ = run_table([words], rec_cap=256)
    check_against(result, table, ref)


def test_two_logs_equal_their_concatenation_and_runs_repeat():
    a, b = C.random_scenes(11, n_records=9), C.random_scenes(12, n_records=7) + C.crafted_scenes()
    split = [C.pack(a), C.pack(b)]
    whole = C.pack(a + b)
    r1, t1, bytes1 = run_table(split)
    r2, t2, bytes2 = run_table([whole])
    r3, t3, bytes3 = run_table(split)
    check_against(r1, t1, T.evaluate_logs([whole]))
    words = lambda raw: np.frombuffer(raw, np.int32)                                                   # noqa: E731
    # the scalar block counts logs, the last log's first record and the largest log's prediction rows: all else is the same bytes
    assert np.array_equal(words(bytes1)[N.AP_TABLE_SCALARS:], words(bytes2)[N.AP_TABLE_SCALARS:])
    same = [0, 1, 2, 4, 5, 6, 7, 8, 9]
    assert words(bytes1)[same].tolist() == words(bytes2)[same].tolist()
    assert bytes1 == bytes3                                             # determinism: two runs, the same bytes
    again = t1.finish()                                                 # and a second finish of the same table
    assert t1.out.cpu().numpy().tobytes() == bytes1 and np.array_equal(again[3], r1[3])


def test_capacity_overflow_is_reported_and_corrupts_nothing():
    scenes = C.random_scenes(5, n_records=12)
    words = C.pack(scenes)
    ref = T.evaluate_logs([words])
    wanted = int(ref["cells"][:, :, 0].sum())
    preds = sum(s["label_id"].shape[0] for s in scenes)
    assert wanted // 2 > preds
    with pytest.raises(RuntimeError, match="wanted %d entries" % wanted):
        run_table([words], entry_cap=wanted // 2)                      # room for the prediction rows, not for the entries
    with pytest.raises(RuntimeError, match="%d prediction rows" % preds):
        run_table([words], entry_cap=preds - 1)
    with pytest.raises(RuntimeError, match="wanted 12 records"):
        run_table([words], rec_cap=5)
    # guard words behind a workspace that is exactly as large as asked for stay untouched by an overflowing epoch
    dev = torch.device("cuda:0")
    table = E.APTable(5, wanted // 2, device=dev)
    guarded = torch.full((table.ws_bytes + 4096,), 0x5a, dtype=torch.uint8, device=dev)
    table.ws = guarded[:table.ws_bytes]
    table.reset()
    state = torch.tensor([words.shape[0], words.shape[0], 12, 0, -1, 0, 0, 0], dtype=torch.int32, device=dev)
    table.add_words(torch.from_numpy(words).to(dev), state, int(words.shape[0]), ["s%d" % i for i in range(12)])
    with pytest.raises(RuntimeError):
        table.finish()
    assert bool((guarded[table.ws_bytes:] == 0x5a).all())
    # and the same epoch with room gives the reference
    result, table, _ = run_table([words], rec_cap=12, entry_cap=wanted)
    check_against(result, table, ref)


def test_overflowed_log_is_refused():
    words = C.pack(C.crafted_scenes()[:1])
    dev = torch.device("cuda:0")
    table = E.APTable(4, device=dev)
    state = torch.tensor([words.shape[0], 12345, 1, 1, -1, 0, 0, 0], dtype=torch.int32, device=dev)
    table.add_words(torch.from_numpy(words).to(dev), state, int(words.shape[0]), ["a"])
    with pytest.raises(RuntimeError, match="12345 words"):
        table.finish()
