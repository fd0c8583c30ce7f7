"""CPU tier of the label vote: the numpy restatement (tests/vote_ref.py) against a Counter per row on every designed case
(tests/vote_cases.py), the host argument checks of pbnet_amd.mesh, and for every named mistake of the restatement a
designed case that tells it from the contract -- so the GPU tier, which pins the device to the restatement bit for bit on
the same cases, would catch that mistake in the kernels."""
import numpy as np
import pytest
import torch

import thin_ref
import vote_cases as C
import vote_ref as R
from pbnet_amd import mesh

DTYPES = {"sem_label": np.int64, "ins_label": np.int64, "votes": np.int32, "members": np.int32, "old_id": np.int64}


def same_vote(a, b):
    return sorted(a) == sorted(b) and all(a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and
                                          np.array_equal(a[k], b[k]) for k in a)


def _want(name, **kw):
    rows, sem, ins, m, nc = C.VOTE[name]
    return R.vote(rows, sem, ins, m, nc, **kw)


@pytest.mark.parametrize("name", sorted(C.VOTE))
def test_restatement_is_the_counter_per_row(name):
    rows, sem, ins, m, nc = C.VOTE[name]
    for compact in (True, False):
        got = R.vote(rows, sem, ins, m, nc, compact=compact)
        assert same_vote(got, R.vote_loop(rows, sem, ins, m, nc, compact=compact))
        assert sorted(got) == sorted(DTYPES) and all(got[k].dtype == DTYPES[k] for k in got)
        assert all(got[k].shape == (m,) for k in ("sem_label", "ins_label", "votes", "members"))
        assert got["members"].sum() == (rows >= 0).sum() and np.all(got["votes"] <= got["members"])
        assert np.array_equal(got["members"] == 0, got["votes"] == 0)
        live = got["ins_label"][got["ins_label"] >= 0]
        if compact:                                          # ids 0..I'-1, every one used, old ids ascending
            assert np.array_equal(np.unique(live), np.arange(got["old_id"].shape[0]))
            assert np.all(np.diff(got["old_id"]) > 0)
        else:
            assert got["old_id"].shape == (0,)


def test_room_scan_restatement_is_the_counter_per_row():
    xyz, sem, ins = C.room_scan()
    rows = thin_ref.thin(xyz, None, 0.05)["inverse"]
    got = R.vote(rows, sem, ins)
    assert same_vote(got, R.vote_loop(rows, sem, ins))
    assert 0.5 < (got["votes"] == got["members"]).mean() < 1.0          # border cells exist, and are the minority
    assert got["old_id"].tolist() == [0, 1, 7]


def test_cases_have_the_shapes_they_were_designed_for():
    for n in (63, 64, 65, 255, 256, 257):
        assert _want("row%d" % n)["members"].tolist() == [n]
    rows, sem, ins, m, _ = C.VOTE["walk300"]
    in1 = rows == 1
    assert np.unique(np.stack([sem[in1], ins[in1]], 1), axis=0).shape[0] == 300
    assert _want("walk300")["votes"].tolist() == [4, 3, 5]
    assert _want("n0")["members"].tolist() == [0] * 5 and _want("n0")["sem_label"].tolist() == [-100] * 5
    assert _want("m0")["sem_label"].shape == (0,) and _want("m0")["old_id"].shape == (0,)
    t2 = _want("tie2")
    assert (t2["sem_label"][0], t2["votes"][0], t2["members"][0]) == (5, 2, 5) and t2["old_id"].tolist() == [2, 3]
    t3 = _want("tie3")
    assert t3["sem_label"].tolist() == [4, 3] and t3["old_id"].tolist() == [2, 3] and t3["votes"].tolist() == [3, 2]
    au = _want("all_unannotated")
    assert au["sem_label"].tolist() == [-100] * 3 and au["ins_label"].tolist() == [-100] * 3 and au["votes"].sum() == 40
    am = _want("all_minus1")
    assert am["members"].tolist() == [0] * 4 and am["old_id"].shape == (0,)
    g = _want("gaps")
    assert g["members"].tolist() == [0, 7, 0, 0, 3, 0, 0, 1, 0, 0] and g["ins_label"].tolist() == [-100, 1, -100, -100, 0, -100,
                                                                                                  -100, 2, -100, -100]
    ni = _want("no_ins")
    assert ni["ins_label"].tolist() == [0, 0, 0, 0, -100] and ni["old_id"].tolist() == [0]
    e = _want("extremes", compact=False)
    assert e["sem_label"].tolist() == [1022, 0] and e["ins_label"].tolist() == [C.INS_TOP, C.INS_TOP]
    assert _want("extremes")["old_id"].tolist() == [C.INS_TOP]
    v = _want("vanish")
    assert v["ins_label"].tolist() == [-100] * 3 and v["old_id"].shape == (0,) and v["sem_label"].tolist() == [0, 1, -100]
    b = _want("border", compact=False)
    assert (b["sem_label"][0], b["ins_label"][0], b["votes"][0], b["members"][0]) == (1, 5, 3, 7)


@pytest.mark.parametrize("name", sorted(C.VOTE_RAISES))
def test_restatement_refuses(name):
    with pytest.raises(ValueError):
        R.vote(*C.VOTE_RAISES[name])


def _differs(wrong):
    return [n for n in sorted(C.VOTE) if not same_vote(_want(n), _want(n, wrong=wrong))]


@pytest.mark.parametrize("wrong,must", [("ties_high", "tie2"), ("ties_high", "tie3"), ("unannotated_first", "unannotated_tie"),
                                        ("unannotated_out", "unannotated_majority"), ("separate", "border"),
                                        ("minus_one_row0", "minus1"), ("first_appearance", "descending_ids"), ("ge", "tie2"),
                                        ("ge", "tie3")])
def test_mistakes_are_told_apart(wrong, must):
    assert wrong in R.WRONG and must in _differs(wrong)


def test_the_separate_vote_invents_a_pair():
    """On the border cell the two independent votes give (2, 5): a pair that no raw point of the row carries."""
    rows, sem, ins, m, nc = C.VOTE["border"]
    got = R.vote(rows, sem, ins, m, nc, compact=False, wrong="separate")
    pair = (int(got["sem_label"][0]), int(got["ins_label"][0]))
    assert pair == (2, 5) and pair not in set(zip(sem[rows == 0].tolist(), ins[rows == 0].tolist()))


# -------------------------------------------------------------------------------------------------- host argument checks
def test_host_argument_checks():
    """Refused on the host, before the library or a device is touched (the tensors here live on the CPU, which the device
    entry point refuses last)."""
    i32 = lambda *v: torch.tensor(v, dtype=torch.int32)
    with pytest.raises(TypeError):
        mesh.vote_labels(torch.zeros(3, dtype=torch.int64), i32(0, 0, 0))
    with pytest.raises(TypeError):
        mesh.vote_labels(i32(0, 0, 0), torch.zeros(3))
    with pytest.raises(TypeError):
        mesh.vote_labels(i32(0, 0, 0), i32(0, 0, 0), torch.zeros(3, 1, dtype=torch.int32))
    with pytest.raises(ValueError):
        mesh.vote_labels(i32(0, 0, 0), i32(0, 0))
    for nc in (0, 1024):
        with pytest.raises(ValueError, match="n_classes"):
            mesh.vote_labels(i32(0, 0), i32(0, 0), n_classes=nc)
    with pytest.raises(ValueError):
        mesh.vote_labels(i32(0, 0), i32(0, 0), m=-1)
    with pytest.raises(RuntimeError):
        mesh.vote_labels(i32(0, 0), i32(0, 0), m=1)          # a CPU tensor: no CPU path
    src = (np.zeros((4, 3), np.float32), np.zeros((4, 3), np.uint8))
    with pytest.raises(ValueError, match="both"):
        mesh.decode_points(src, sem_label=np.zeros(4))
    with pytest.raises(ValueError, match="both"):
        mesh.decode_points(src, ins_label=np.zeros(4))
    with pytest.raises(ValueError, match="integer"):
        mesh.decode_points(src, sem_label=np.array([0.0, 1.5, 2.0, 3.0]), ins_label=np.zeros(4))
    with pytest.raises(ValueError, match="integer"):
        mesh.decode_points(src, sem_label=np.zeros(4), ins_label=np.array([0.0, np.nan, 2.0, 3.0]))
    with pytest.raises(ValueError, match="shape"):
        mesh.decode_points(src, sem_label=np.zeros(5), ins_label=np.zeros(5))
    with pytest.raises(TypeError):
        mesh.decode_points(src, sem_label=np.zeros(4, bool), ins_label=np.zeros(4))


def test_library_refuses_bad_arguments_before_any_launch():
    """pbn_cloud_vote_labels checks its sizes on the host (the pointers are never dereferenced)."""
    from pbnet_amd import _native as N
    lib, vp, fake, big = N.lib(), N.c_vp, 1 << 20, 1 << 30

    def call(n=8, m=4, nc=20, ws=big):
        return lib.pbn_cloud_vote_labels(vp(fake), vp(fake), None, n, m, nc, vp(fake), vp(fake), vp(fake), vp(fake), vp(fake),
                                         vp(fake), vp(fake), ws, None)
    for kw in (dict(n=-1), dict(m=-1), dict(nc=0), dict(nc=1024), dict(n=(1 << 28) + 1), dict(m=(1 << 28) + 1)):
        assert call(**kw) == N.PBN_ERR_ARG
    assert call(ws=16) == N.PBN_ERR_WORKSPACE
    assert lib.pbn_cloud_vote_labels(None, vp(fake), None, 8, 4, 20, vp(fake), vp(fake), vp(fake), vp(fake), vp(fake), None,
                                     vp(fake), big, None) == N.PBN_ERR_ARG
    assert 0 < lib.pbn_cloud_vote_workspace_bytes(1000, 10) < lib.pbn_cloud_vote_workspace_bytes(100000, 10)
    assert lib.pbn_cloud_vote_workspace_bytes(-1, 4) == 0 and lib.pbn_cloud_vote_workspace_bytes(4, (1 << 28) + 1) == 0


def test_save_decoded_writes_the_dicts_labels_and_no_bookkeeping(tmp_path):
    import os
    from pbnet_amd import scene_io
    n = 12
    rng = np.random.default_rng(2)
    dec = {"xyz": rng.normal(size=(n, 3)).astype(np.float32), "rgb": rng.normal(size=(n, 3)).astype(np.float32),
           "nl": rng.normal(size=(n, 3)).astype(np.float32), "sup": rng.integers(0, 3, n),
           "sem_label": rng.integers(0, 20, n), "ins_label": np.where(np.arange(n) % 3, np.arange(n) % 2, -100),
           "votes": np.ones(n, np.int32), "members": np.ones(n, np.int32), "ins_old_id": np.array([4, 9]),
           "raw_index": np.arange(40, dtype=np.int32) % n, "count": np.ones(n, np.int32)}
    mesh.save_decoded(str(tmp_path), "scan", dec)
    assert sorted(os.listdir(tmp_path)) == ["scan_%s.npy" % k for k in ("ins_label", "nl", "rgb", "sem_label", "sup", "xyz")]
    back = scene_io.load_scene(str(tmp_path), "scan", with_mesh=False)
    assert back["sem_label"].dtype == np.float64 and np.array_equal(back["sem_label"], dec["sem_label"])
    assert back["ins_label"].dtype == np.float64 and np.array_equal(back["ins_label"], dec["ins_label"])
