"""CPU tier of the scene summary: the numpy restatement of pbn_scene_summary's contract (tests/scene_summary_ref.py) against a
brute-force loop over points and instances in Python numbers, on every shared case (tests/scene_summary_cases.py); the copy order
of the float32 additions on the order-sensitive triple; copies = 1 against numpy's own first-maximum argmax."""
import math

import numpy as np
import pytest

import scene_summary_cases as C
import scene_summary_ref as R

CASES = C.cases()


def _brute_fold(case):
    starts, copies, k = case["point_starts"], case["copies"], case["n_cls"]
    out = np.zeros(starts[-1], dtype=np.int32)
    for j in range(len(starts) - 1):
        n = starts[j + 1] - starts[j]
        for i in range(n):
            best, arg = -math.inf, 0
            for c in range(k):
                s = np.float32(case["scores"][copies * starts[j] + i, c])
                for m in range(1, copies):
                    with np.errstate(invalid="ignore", over="ignore"):
                        s = np.float32(s + case["scores"][copies * starts[j] + m * n + i, c])
                if s > best:
                    best, arg = float(s), c
            out[starts[j] + i] = arg
    return out


def _brute_instance(case, sem_fold, j, k):
    """(class, count, box, centre) of instance k of scene j from a scan over the scene: np.bincount, min / max / mean of the
    quantised values in Python integers."""
    p0, p1 = case["point_starts"][j], case["point_starts"][j + 1]
    rows = [i for i in range(p0, p1) if case["point_instance"][i] == k]
    hist = np.bincount(sem_fold[rows], minlength=case["n_cls"]) if rows else np.zeros(case["n_cls"], dtype=np.int64)
    cls = int(np.argmax(hist))
    box = centre = None
    if case["xyz"] is not None:
        good = [i for i in rows if all(abs(float(v)) < 32768.0 for v in case["xyz"][i])]      # NaN compares false
        if good:
            pts = case["xyz"][good]
            box = [float(pts[:, d].min()) for d in range(3)] + [float(pts[:, d].max()) for d in range(3)]
            q = [[int(np.rint(np.float32(v) * np.float32(65536.0))) for v in row] for row in pts]
            centre = [np.float32(float(sum(r[d] for r in q)) / float(len(good)) / 65536.0) for d in range(3)]
        else:
            box, centre = [math.nan] * 6, [math.nan] * 3
    return cls, int(hist[cls]), box, centre


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_restatement_equals_brute_force(case):
    got = R.summarize(case["scores"], case["point_starts"], case["copies"], case["point_instance"], case["n_keep"], case["n_prop"],
                      case["xyz"], case["labels"])
    sem_fold = _brute_fold(case)
    assert np.array_equal(got["sem_fold"], sem_fold)
    b, p = len(case["n_keep"]), case["n_prop"]
    assert got["class_vote"].shape == (b, p) and got["class_points"].shape == (b, p) and got["status"].shape == (b,)
    kept = R.kept_counts(case["n_keep"], p)
    for j in range(b):
        status = 0
        inst = case["point_instance"][case["point_starts"][j]:case["point_starts"][j + 1]]
        if any(v != C.NO_LABEL and not 0 <= v < kept[j] for v in inst):
            status |= R.STATUS_INSTANCE
        if case["xyz"] is not None:
            pts = case["xyz"][case["point_starts"][j]:case["point_starts"][j + 1]]
            if any(not abs(float(v)) < 32768.0 for v in pts.reshape(-1)):
                status |= R.STATUS_COORD
        for k in range(kept[j]):
            cls, count, box, centre = _brute_instance(case, sem_fold, j, k)
            inside = cls < len(case["labels"])
            status |= 0 if inside else R.STATUS_CLASS
            assert got["class_vote"][j, k] == (case["labels"][cls] if inside else -1) and got["class_points"][j, k] == count
            if box is not None:
                assert np.array_equal(got["box"][j, k], np.array(box, dtype=np.float32), equal_nan=True)
                assert np.array_equal(got["centroid"][j, k], np.array(centre, dtype=np.float32), equal_nan=True)
        assert got["status"][j] == status
        assert (got["class_vote"][j, kept[j]:] == -1).all() and (got["class_points"][j, kept[j]:] == 0).all()
        if case["xyz"] is not None:
            assert (got["box"][j, kept[j]:] == 0).all() and (got["centroid"][j, kept[j]:] == 0).all()
        else:
            assert got["box"] is None and got["centroid"] is None


def test_copy_order_is_what_the_restatement_fixes():
    big, one = np.float32(1e8), np.float32(1.0)
    assert (big + one) + -big == 0 and (big + -big) + one == 1          # the triple is order-sensitive in float32
    rows = np.zeros((3, 2), dtype=np.float32)
    rows[:, 0] = [1e8, 1.0, -1e8]                   # in copy order: 0
    rows[:, 1] = [0.5, 0.0, 0.0]
    assert R.fold_labels(rows, [0, 1], 3)[0] == 1
    rows[:, 0] = [1e8, -1e8, 1.0]                   # the same three numbers, another copy order: 1
    assert R.fold_labels(rows, [0, 1], 3)[0] == 0
    case = [c for c in CASES if c["name"] == "copy order"][0]
    assert (R.fold_labels(case["scores"], case["point_starts"], 3) == 1).all()


def test_one_copy_is_numpys_first_maximum():
    rng = np.random.default_rng(7)
    scores = (rng.integers(-5, 6, size=(500, 20)) / 4.0).astype(np.float32)     # many ties
    assert (np.sort(scores, 1)[:, -1] == np.sort(scores, 1)[:, -2]).any()
    assert np.array_equal(R.fold_labels(scores, [0, 200, 200, 500], 1), scores.argmax(1).astype(np.int32))


def test_kept_counts_are_clamped_to_the_table():
    assert R.kept_counts([3, 5, 2], 6) == [3, 3, 0] and R.kept_counts([-1, 2], 4) == [0, 2]
