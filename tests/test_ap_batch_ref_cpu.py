"""CPU tier: the numpy restatement of the batched AP association (tests/ap_batch_ref.py) against the per-scene statement
(ap_record_ref.tables + pack_log on the densified labels), the decoder's two status modes, and the AP that comes out of the
decoded records.  Ground truth and predictions are the golden scenes of the reference's tools/eval.py; their recorded masks may
overlap, so labels are made disjoint by "lowest mask index wins"."""
import glob
import os

import numpy as np
import pytest

import ap_batch_ref as B
import ap_record_ref as R
from pbnet_amd import evaluate as E

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = sorted(glob.glob(os.path.join(HERE, "golden", "eval_E*.npz")))
IDS = [os.path.basename(p)[:-4] for p in CASES]


def golden_batch(g):
    """The golden's scenes as one merged forward: dict(point_starts, point_instance, n_keep, scores [B, P], semantic_id [B, P], ids)."""
    n = int(g["n_scenes"])
    labels = [B.disjoint_labels(g["s%d_mask" % s]) if g["s%d_label" % s].shape[0] else np.full(g["s%d_gt" % s].shape[0], -100, np.int32)
              for s in range(n)]
    keep = [int(g["s%d_label" % s].shape[0]) for s in range(n)]
    p = max(sum(keep), 1)
    scores, sid = np.zeros((n, p), np.float32), np.full((n, p), -1, np.int64)
    for s in range(n):
        scores[s, :keep[s]], sid[s, :keep[s]] = g["s%d_conf" % s], g["s%d_label" % s]
    starts = np.concatenate([[0], np.cumsum([l.shape[0] for l in labels])]).tolist()
    return dict(point_starts=starts, point_instance=np.concatenate(labels), n_keep=keep, scores=scores, semantic_id=sid,
                ids=np.concatenate([g["s%d_gt" % s] for s in range(n)]).astype(np.int64), labels=labels)


def batched_log(b, log_words=1 << 17, **kw):
    n = len(b["n_keep"])
    args = dict(point_starts=b["point_starts"], point_instance=b["point_instance"], n_keep=b["n_keep"], post_status=[0] * n,
                scores=b["scores"], semantic_id=b["semantic_id"], tags=list(range(n)), u_cap=1024, id_cap=65536,
                log_words=log_words, ids=b["ids"])
    args.update(kw)
    return B.assoc_batch(**args)


def per_scene_records(g, b):
    out = []
    for s in range(len(b["n_keep"])):
        k = b["n_keep"][s]
        inter, uid, counts = R.tables(B.densify(b["labels"][s], k), g["s%d_gt" % s])
        out.append(dict(n_pts=int(g["s%d_gt" % s].shape[0]), inter_all=inter, uid=uid, counts=counts, label_id=g["s%d_label" % s],
                        conf=g["s%d_conf" % s]))
    return out


@pytest.mark.parametrize("path", CASES, ids=IDS)
def test_restatement_equals_the_per_scene_statement(path):
    g = np.load(path)
    b = golden_batch(g)
    state, log = batched_log(b)
    want = R.pack_log(per_scene_records(g, b))
    assert state.tolist()[:4] == [want.shape[0], want.shape[0], len(b["n_keep"]), 0]
    assert np.array_equal(log[:want.shape[0]], want) and not log[want.shape[0]:].any()
    assert state[4] == want.shape[0] - R.pack_log(per_scene_records(g, b)[-1:]).shape[0]


def test_restatement_overflow_is_sticky_and_wanted_exact():
    g = np.load(CASES[2])                                        # three scenes with predictions
    b = golden_batch(g)
    recs = [R.pack_log([r]) for r in per_scene_records(g, b)]
    assert len(recs) >= 3
    sizes = [r.shape[0] for r in recs]
    state, log = batched_log(b, log_words=sizes[0] + sizes[1] - 1)
    assert state.tolist()[:5] == [sizes[0], sum(sizes), 1, 1, -1]
    assert np.array_equal(log[:sizes[0]], recs[0]) and not log[sizes[0]:].any()


def test_restatement_ignores_labels_outside_the_kept_range():
    g = np.load(CASES[0])
    b = golden_batch(g)
    k0 = b["n_keep"][0]
    assert k0 >= 2
    fewer = dict(b, n_keep=[k0 - 1] + b["n_keep"][1:])           # the last instance's label is now >= n_keep: it counts for nothing
    _, log = batched_log(fewer)
    recs = per_scene_records(g, b)
    recs[0] = dict(recs[0], inter_all=recs[0]["inter_all"][:k0 - 1], label_id=recs[0]["label_id"][:k0 - 1],
                   conf=recs[0]["conf"][:k0 - 1])
    want = R.pack_log(recs)
    assert np.array_equal(log[:want.shape[0]], want)


def test_restatement_encodes_like_the_host_form():
    rng = np.random.default_rng(3)
    ins = rng.integers(-1, 6, 500).astype(np.int64)
    sem = rng.integers(0, 20, 500).astype(np.int64)
    sem[rng.random(500) < 0.2] = -100
    ids, status = B.encode_scene(sem, ins, 8)
    assert status == 0 and np.array_equal(ids, E.encode_gt_ids(sem, ins))
    ins[7] = 8
    assert B.encode_scene(sem, ins, 8)[1] == B.INSTANCE_CAP
    sem[np.nonzero(ins == 2)[0][0]] = 20
    assert B.encode_scene(sem, ins, 8)[1] == B.INSTANCE_CAP | B.SEMANTIC_RANGE


@pytest.mark.parametrize("path", CASES, ids=IDS)
def test_decoder_modes(path):
    g = np.load(path)
    b = golden_batch(g)
    n = len(b["n_keep"])
    names = ["scene%04d_00" % s for s in range(n)]
    state, log = batched_log(b)
    clean = E.decode_association_log(log[:state[0]], names)
    assert len(clean) == 2 and E.decode_association_log(log[:state[0]], names, on_status="raise")[1] == clean[1]
    matches, dropped, failed = E.decode_association_log(log[:state[0]], names, on_status="skip")
    assert list(matches) == list(clean[0]) and dropped == clean[1] and failed == []
    bad = next(s for s in range(n) if b["n_keep"][s])
    state, log = batched_log(b, post_status=[B.ID_RANGE | 1 if s == bad else 0 for s in range(n)])
    with pytest.raises(ValueError) as err:
        E.decode_association_log(log[:state[0]], names)
    assert names[bad] in str(err.value)
    matches, dropped, failed = E.decode_association_log(log[:state[0]], names, on_status="skip")
    assert [f[0] for f in failed] == [names[bad]] and len(failed[0][1]) == 2 and "id_cap" in " ".join(failed[0][1])
    assert names[bad] not in matches and names[bad] not in dropped
    assert list(matches) == [s for s in clean[0] if s != names[bad]] and dropped == clean[1]
    with pytest.raises(ValueError):
        E.decode_association_log(log[:state[0]], names, on_status="ignore")


@pytest.mark.parametrize("path", CASES, ids=IDS)
def test_ap_of_the_decoded_records_equals_the_per_scene_association(path, monkeypatch):
    """evaluate_matches on the decoded batched records against evaluate_matches on assign_instances_for_scan of the same dense
    masks.  This tier has no device, so the one device pass inside assign_instances_for_scan (overlap_table) is replaced by its
    host statement ap_record_ref.tables; tests/test_ap_batch_gpu.py makes the comparison through the device pass."""
    def host_table(masks, gt_ids, device=None):
        inter, uid, _ = R.tables(masks, gt_ids)
        return inter, uid
    monkeypatch.setattr(E, "overlap_table", host_table)
    g = np.load(path)
    b = golden_batch(g)
    n = len(b["n_keep"])
    names = ["scene%04d_00" % s for s in range(n)]
    state, log = batched_log(b)
    matches, dropped = E.decode_association_log(log[:state[0]], names)
    want = {}
    for s in range(n):
        if b["n_keep"][s] == 0:
            continue
        pred = dict(conf=g["s%d_conf" % s], label_id=g["s%d_label" % s], mask=B.densify(b["labels"][s], b["n_keep"][s]))
        want[names[s]] = E.assign_instances_for_scan(names[s], pred, g["s%d_gt" % s])
    assert list(matches) == list(want) and dropped == [names[s] for s in range(n) if b["n_keep"][s] == 0]
    for name in want:
        for field in E.SceneMatches.__slots__:
            x, y = getattr(matches[name], field), getattr(want[name], field)
            assert (x == y) if isinstance(x, str) else np.array_equal(np.asarray(x), np.asarray(y)), (name, field)
    a, w = E.evaluate_matches(matches), E.evaluate_matches(want)
    assert np.array_equal(np.isnan(a), np.isnan(w)) and np.array_equal(np.nan_to_num(a, nan=-1.0), np.nan_to_num(w, nan=-1.0))
