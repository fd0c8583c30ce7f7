"""Logs for the AP-table tests, as lists of tests/ap_record_ref.pack_record keyword dicts: the reference's golden epochs, crafted
records that each exercise one rule of tools/eval.py:27-190, and seeded random epochs with ties everywhere."""
import glob
import os

import numpy as np

import ap_record_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = sorted(glob.glob(os.path.join(HERE, "golden", "eval_E*.npz")))
GOLDEN_IDS = [os.path.basename(p)[:-4] for p in GOLDEN]
CABINET, BED, CHAIR, SOFA, TABLE, DOOR = 0, 1, 2, 3, 4, 5          # class indices; their NYU40 ids are index + 3
O50, O55, O60, O65, O70, O25 = 0, 1, 2, 3, 4, 9                    # overlap indices of 0.5, 0.55, 0.6, 0.65, 0.7 and 0.25


def scene(uid, counts, label_id, conf, inter, status=0, n_pts=None):
    inter = np.asarray(inter, np.int64).reshape(len(label_id), len(uid))
    return dict(n_pts=int(np.sum(counts)) if n_pts is None else n_pts, inter_all=inter, uid=np.asarray(uid, np.int64),
                counts=np.asarray(counts, np.int64), label_id=np.asarray(label_id, np.int64),
                conf=np.asarray(conf, np.float32), status=status)


def golden_scenes(path):
    """(scenes, golden ap) of one eval_E*.npz.  A golden scene WITHOUT predictions would be a header-only record, which the log
    drops, while tools/eval.py -- which made the golden AP -- counts its ground truth as misses: it is packed with one
    non-benchmark prediction of no vertices instead, which is dropped as a prediction and keeps the scene."""
    g = np.load(path)
    scenes = []
    for s in range(int(g["n_scenes"])):
        inter, uid, counts = R.tables(g["s%d_mask" % s], g["s%d_gt" % s])
        label, conf = g["s%d_label" % s], g["s%d_conf" % s]
        if label.shape[0] == 0:
            inter, label, conf = np.zeros((1, uid.shape[0]), np.int64), np.zeros(1, np.int64), np.zeros(1, np.float32)
        scenes.append(dict(n_pts=int(g["s%d_gt" % s].shape[0]), inter_all=inter, uid=uid, counts=counts, label_id=label, conf=conf))
    return scenes, g["ap"]


def crafted_scenes():
    """One record per rule; the classes keep the rules apart.  Column 0 is the unannotated id 0 throughout."""
    return [
        # CHAIR: two predictions over instance 5001 -- the second is a false positive at the lower score and stays unvisited,
        # so at 0.25 it still takes instance 5002 (IoU 400/1200 and 200/700); from 0.5 on it is lonely and 5002 is missed
        scene([0, 5001, 5002], [50, 1000, 300], [5, 5], [0.9, 0.8], [[0, 900, 0], [0, 400, 200]]),
        # SOFA: equal scores shared by a true positive (IoU 1) and a false positive (IoU 100/220: a second hit at 0.25, lonely
        # with ignore ratio 1/6 from 0.5 on)
        scene([0, 6001], [400, 200], [6, 6], [0.5, 0.5], [[0, 200], [20, 100]]),
        # TABLE / DOOR / CABINET: IoU exactly 1/2, 3/5 and 7/10 -- not above 0.5, 0.6000000000000001 and 0.7000000000000002
        scene([0, 3001, 7001, 8001], [300, 850, 150, 400], [7, 8, 3], [0.7, 0.6, 0.4],
              [[50, 0, 100, 0], [100, 0, 0, 300], [150, 700, 0, 0]]),
        # BED: the ignore ratio 100 / 200 equals the threshold 0.5: `<=` keeps the false positive there and above, not at 0.25;
        # the void is id 0 and the non-benchmark id 2001, the other half lies in an instance of another class
        scene([0, 2001, 4001, 5001], [60, 60, 500, 400], [4], [0.3], [[60, 40, 0, 100]]),
        # class 9 (index 6): the only overlap is a 90-vertex instance: not lonely, and the instance does not count: nothing
        scene([0, 9001], [10, 90], [9], [0.6], [[10, 90]]),
        # class 10 (index 7): a 99-vertex prediction and a non-benchmark label are dropped, the instance is missed
        scene([0, 10001], [900, 300], [10, 2], [0.9, 0.9], [[0, 99], [500, 200]]),
        # class 11 (index 8): instances without any prediction: 0.0
        scene([0, 11001], [200, 400], [2], [0.2], [[150, 0]]),
        # class 12 (index 9): predictions only: NaN
        scene([0, 5003], [300, 50], [12], [0.4], [[300, 0]]),
        # class 14 (index 10): an instance and a kept prediction wholly in the void: both flags and no entry: 0.0
        scene([0, 14001], [300, 400], [14], [0.4], [[300, 0]]),
        # a record with status bits and a header-only record: left out, and named in the directory
        scene([0, 5001], [10, 1000], [5], [0.95], [[0, 1000]], status=4),
        scene([0, 5001], [10, 1000], [], [], np.zeros((0, 2))),
    ]


SCORES = np.linspace(0.05, 0.95, 16).astype(np.float32)            # 16 distinct float32 scores: ties everywhere


def random_scenes(seed, n_records=40, max_keep=64, max_gt=48, classes=(3, 4, 5, 6), one_class=False, min_keep=1, min_gt=2):
    rng = np.random.RandomState(seed)
    scenes = []
    for _ in range(n_records):
        ng, nk = int(rng.randint(min_gt, max_gt + 1)), int(rng.randint(min_keep, max_keep + 1))
        kinds = rng.choice(classes[:1] if one_class else classes + (1, 2), ng)           # 1 / 2: wall / floor, void columns
        uid = np.sort(np.unique(np.concatenate([[0], kinds * 1000 + rng.randint(1, 400, ng)])))
        ng = uid.shape[0]
        counts = rng.choice([40, 99, 100, 150, 300, 600], ng)
        label = rng.choice(classes[:1] if one_class else classes + (2, 13), nk)
        inter = np.zeros((nk, ng), np.int64)
        for q in range(nk):
            for g in rng.choice(ng, min(ng, int(rng.randint(1, 4))), replace=False):
                inter[q, g] = int(counts[g] * rng.choice([0.2, 0.5, 0.6, 0.75, 0.9, 1.0]))
            if rng.rand() < 0.3:
                inter[q, 0] += int(rng.randint(1, 200))
        counts[0] = max(counts[0], int(inter[:, 0].max()))
        scenes.append(scene(uid, counts, label, rng.choice(SCORES, nk), inter))
    return scenes


def wide_random_scenes(seed):
    """Records past 64 on both axes (130-200 predictions, 100-150 columns, two classes so that same-class hits are common): a
    matching wave scans its predictions in several ballots and its columns in several strides."""
    return random_scenes(seed, n_records=6, max_keep=200, max_gt=150, classes=(3, 4), min_keep=130, min_gt=100)


def wide_scene():
    """200 predictions x 80 columns, the rules of the greedy loop ACROSS the 64-wide ballots and column strides.  Chair instance
    5001 (column 70, 1000 vertices) is hit with IoU >= 2/3 by rows 10, 70 and 130 -- one per ballot: row 10 takes it, rows 70
    and 130 are false positives at min(best, conf) and stay unvisited; row 70 then takes instance 5006 (column 75) at 0.25 only
    (IoU 350/1250).  Row 190 overlaps only the 90-vertex instance 5009 (column 78): not lonely, nothing emitted.  Every other row
    is a non-benchmark prediction in the void."""
    nk, ng = 200, 80
    uid = np.array([0] + list(range(1001, 1070)) + list(range(5001, 5011)), np.int64)
    counts = np.full(ng, 50, np.int64)
    counts[0], counts[70], counts[75], counts[78] = 40000, 1000, 350, 90
    label, conf, inter = np.full(nk, 2, np.int64), np.full(nk, 0.25, np.float32), np.zeros((nk, ng), np.int64)
    inter[:, 0] = 150
    for row, c in ((10, 0.5), (70, 0.7), (130, 0.6)):
        label[row], conf[row], inter[row, 0], inter[row, 70] = 5, c, 0, 900
    inter[70, 75] = 350
    label[190], conf[190], inter[190, 0], inter[190, 78] = 5, 0.8, 20, 90
    return scene(uid, counts, label, conf, inter)


def many_columns_scene(n_columns=4200):
    """Two predictions x 4200 columns, the instances in the last columns: 39001 (1000 vertices, hit with IoU 0.9 by row 0) and the
    90-vertex 39002, the only overlap of row 1 besides the void (not lonely, nothing emitted)."""
    void = np.concatenate([np.arange(k * 1000, k * 1000 + 1000) for k in (1, 2, 13, 15, 17, 18, 19, 20)])[:n_columns - 3]
    uid = np.concatenate([[0], void, [39001, 39002]]).astype(np.int64)
    counts = np.full(n_columns, 10, np.int64)
    counts[-2], counts[-1] = 1000, 90
    inter = np.zeros((2, n_columns), np.int64)
    inter[0, -2], inter[1, -1], inter[1, 0] = 900, 90, 20
    return scene(uid, counts, [39, 39], [0.9, 0.8], inter)


def too_many_predictions_scene(n_keep=65536):
    """One column and one prediction more than a record may hold for the device table."""
    return scene([0], [10], np.full(n_keep, 2, np.int64), np.zeros(n_keep, np.float32), np.zeros((n_keep, 1), np.int64))


def pack(scenes, first_tag=0):
    return R.pack_log([dict(s, tag=first_tag + i) for i, s in enumerate(scenes)])
