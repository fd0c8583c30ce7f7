"""CPU tier: the designed grouping inputs of tests/cluster_cases.py are valid (every precondition holds, the C oracle and the
brute force agree on them bit for bit) and sharp (each deliberately wrong variant of the specification in tests/cluster_mutants.py
differs from the specification on at least one case).  The kill matrix is printed (pytest -s shows it)."""
import functools

import numpy as np
import pytest

from oracle import pb_cluster_ref as oracle
import cluster_cases as CC
import cluster_mutants as CM

KEYS = ("cluster_id", "cluster_num", "den_queue", "clt_sem")


def _same(a, b):
    return all(np.array_equal(a[k], b[k]) for k in KEYS) and a["center"].shape == b["center"].shape and \
        np.array_equal(a["center"].view(np.int32), b["center"].view(np.int32))


@pytest.mark.parametrize("name", [c["name"] for c in CC.cases() if c["precondition"] is not None])
def test_precondition_holds(name):
    c = CC.case(name)
    c["precondition"](c)


def test_preconditions_fail_loudly_when_the_cell_size_changes():
    """The same inputs under another cell size (a radius of 0.05 instead of 0.04) no longer have the designed cells."""
    for name in ("A_single_edges", "B_seam", "G_piles_m64"):
        c = dict(CC.case(name), radius=0.05)
        with pytest.raises(AssertionError):
            c["precondition"](c)


@pytest.mark.parametrize("name", CC.NAMES)
def test_oracle_equals_bruteforce(name):
    c = CC.case(name)
    want = CC.reference(name)
    got = CC.run(oracle.binary_cluster, c)
    for k in KEYS:
        assert np.array_equal(got[k], want[k]), k
    assert np.array_equal(got["center"].view(np.int32), want["center"].view(np.int32)), "centre bits"
    assert want["cluster_id"].shape[0] == c["off"].shape[0] and want["cluster_num"].shape == c["seg"].shape


def test_designed_outcomes():
    """What the families were built to produce, read off the brute force."""
    a = CC.case("A_single_edges")
    ref = CC.reference("A_single_edges")
    assert ref["cluster_num"].tolist() == [a["design"]["expect_clusters"]]          # every structure is ONE component
    for s in a["design"]["structures"]:
        assert len(set(ref["cluster_id"][list(s["index"].values())])) == 1
    b = CC.case("B_seam")
    ref = CC.reference("B_seam")
    ga, gb, loner = b["design"]["far_groups"]
    assert len(set(ref["cluster_id"][ga])) == 1 and len(set(ref["cluster_id"][gb])) == 1
    assert ref["cluster_id"][ga[0]] != ref["cluster_id"][gb[0]] and ref["cluster_id"][loner[0]] == -1
    assert (ref["den_queue"][ga] == 4).all() and ref["den_queue"][loner[0]] == 0
    for m in b["design"]["motifs"]:
        ids = ref["cluster_id"][list(m["index"].values())]
        assert len(set(ids)) == 1 and ids[0] >= 0, m["kind"]                         # joined (or adopted) across the seam
    for c in CC.cases():
        if c["family"] == "C":
            k = int(CC.reference(c["name"])["cluster_num"].sum())
            assert 8 <= k <= 2000, (c["name"], k)                                    # neither one giant nor all singletons
    for m in (0, 1, 63, 64, 65):
        g = CC.case("G_piles_m%d" % m)
        den = CC.reference(g["name"])["den_queue"]
        for k, idx in zip((64, 63, 65, 129), g["design"]["piles"]):
            half = k // 2                                                                # pile 0: only the coincident half is AT r
            assert (den[idx[half:]] == (k - 1 if k == 64 else k)).all() and (den[idx[:half]] == k).all()
    e = CC.reference("E_interleaved_members")
    assert sorted(np.bincount(e["cluster_id"]).tolist()) == [1, 16, 17, 32, 33, 128, 256, 257, 600]
    for name in ("E_huge", "E_tiny"):
        r = CC.reference(name)
        assert r["cluster_num"].sum() >= 1 and 40 <= r["den_queue"].max() < len(r["den_queue"]) - 1
    f = CC.reference("F_lattice_noise")
    assert (f["cluster_id"] >= 0).sum() > (CC.reference("F_lattice_noise_off")["cluster_id"] >= 0).sum()


@functools.lru_cache(maxsize=None)
def _kills(mutant):
    return tuple(c["name"] for c in CC.cases() if not _same(CC.run(functools.partial(CM.binary_cluster, mutant=mutant), c),
                                                            CC.reference(c["name"])))


@pytest.mark.parametrize("name", CC.NAMES)
def test_mutant_harness_restates_the_specification(name):
    assert _same(CC.run(functools.partial(CM.binary_cluster, mutant=None), CC.case(name)), CC.reference(name))


@pytest.mark.parametrize("mutant", CM.MUTANTS)
def test_mutant_is_killed(mutant):
    killed_by = _kills(mutant)
    print("\nKILL %-22s %2d/%d cases: %s" % (mutant, len(killed_by), len(CC.NAMES), " ".join(killed_by)))
    assert killed_by, "mutant %s survives the whole case set: the set is too weak" % mutant
