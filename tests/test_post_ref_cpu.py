"""CPU tier: tests/post_ref.py (the numpy restatement of the post-processing under the device tie rule: score descending,
lower survivor index first among equal scores) against the four recorded goldens, and the rank-by-counting order of
csrc/post.hip's k_post_nms against np.lexsort.

Every golden holds one tied pair among its survivors (positions 0 and 1).  P1, P2 and P3 reproduce as recorded under the device
rule.  P4 does not: its tied pair (proposals 2 and 3, score 0.6217706) overlaps above the NMS threshold, the recording numpy's
unstable argsort walked the higher index first and picked survivor 1, the device rule picks survivor 0.  That is the sort of the
numpy build, not a defect: P4 is compared as recorded on `out_pointnum` and `out_cross_ious` (which do not depend on the order)
and its recorded pick is shown to be exactly the other order of that one pair."""
import glob
import os

import numpy as np
import pytest

import post_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = sorted(glob.glob(os.path.join(HERE, "golden", "post_P*.npz")))
AS_RECORDED = ("post_P1", "post_P2", "post_P3")
ORDER_FREE_KEYS = ("out_pointnum", "out_cross_ious")


def test_there_are_four_goldens():
    assert [os.path.basename(p)[:-4] for p in CASES] == ["post_P1", "post_P2", "post_P3", "post_P4"]


@pytest.mark.parametrize("path", CASES, ids=[os.path.basename(p)[:-4] for p in CASES])
def test_golden_through_the_restatement(path):
    g = np.load(path)
    got = R.refine_golden(g)
    name = os.path.basename(path)[:-4]
    keys = R.GOLDEN_KEYS if name in AS_RECORDED else ORDER_FREE_KEYS
    for key in keys:
        want = g[key]
        assert got[R.GOLDEN_KEYS[key]].dtype == want.dtype and np.array_equal(got[R.GOLDEN_KEYS[key]], want), (name, key)
    assert got["status"] == 0
    # one tied pair among the survivors in every golden
    s = g["in_clt"].reshape(-1)[got["rows"]]
    assert s.shape[0] - np.unique(s).shape[0] == 1


def test_p1_needs_lower_index_first():
    g = np.load(CASES[0])
    got = R.refine_golden(g)
    assert np.array_equal(got["pick"], [7, 0, 1, 3]) and got["keep"].shape[0] == 0      # every picked cluster vanishes
    s = g["in_clt"].reshape(-1)[got["rows"]]
    reversed_stable = np.argsort(s, kind="stable")[::-1]
    assert list(reversed_stable[:3]) == [7, 1, 0]                                       # the other rule walks 1 before 0


def test_p4_recorded_pick_is_the_other_order_of_its_tied_pair():
    g = np.load(CASES[3])
    got = R.refine_golden(g)
    s = g["in_clt"].reshape(-1)[got["rows"]]
    assert s[0] == s[1] and got["cross_ious"][0, 1] > np.float32(float(g["nms_t"]))
    assert np.array_equal(got["pick"], [0]) and np.array_equal(g["out_pick"], [1])


def test_rank_by_counting_equals_lexsort():
    rng = np.random.default_rng(7)
    for trial in range(200):
        n = int(rng.integers(1, 140))
        s = rng.random(n).astype(np.float32)
        n_tied = int(rng.integers(0, n + 1))                     # forced ties: copies of a few values, up to all equal
        if n_tied:
            s[rng.permutation(n)[:n_tied]] = rng.choice(s, size=max(1, n_tied // 3))[rng.integers(0, max(1, n_tied // 3), n_tied)]
        rank = R.rank_by_counting(s)
        assert sorted(rank) == list(range(n))                    # a permutation: exact and stable
        assert np.array_equal(R.order_from_rank(rank), np.lexsort((np.arange(n), -s)))
