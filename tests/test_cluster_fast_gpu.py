"""GPU tier: the HP-only grouping mode (pbn_binary_cluster flags bit 2, ``cluster_device(need_den=False)``) that
PBNet.forward uses.  The neighbour count may stop once it reaches min_pts; every output the forward consumes must be
bit-identical to the exact mode, and ``den`` must be min(exact count, min_pts).  The reference-shaped shims keep the
exact count."""
import glob
import os

import numpy as np
import pytest
import torch

from oracle import pb_cluster_ref as oracle
from pbnet_amd import pbnet_ops
from test_cluster_gpu import _scene_groups

pytestmark = pytest.mark.gpu

GOLDEN = sorted(glob.glob(os.path.join(os.path.dirname(__file__), "golden", "cluster_*.npz")))
DEV = "cuda:0"


def _general(sem, seg):
    start = np.concatenate([[0], np.cumsum(seg)])
    return any(len(np.unique(np.asarray(sem)[a:b])) > 1 for a, b in zip(start[:-1], start[1:]))


def _both(off, org, sem, seg, radius, min_pts, nv=True, pad=0):
    """Run the exact and the HP-only mode on the same input; `pad` > 0 runs both in capacity mode over that many extra
    garbage rows.  Returns two dicts of host arrays over the rows that exist."""
    sem = np.asarray(sem, np.int32)
    seg = np.asarray(seg, np.int32)
    general = _general(sem, seg)
    n = len(off)
    off = np.asarray(off, np.float32)
    org = np.asarray(org, np.float32)
    if pad:
        rng = np.random.default_rng(1)
        junk3 = rng.normal(0, 50, (pad, 3)).astype(np.float32)
        junk3[::7] = np.nan
        off = np.concatenate([off, junk3])
        org = np.concatenate([org, junk3[::-1]])
        sem = np.concatenate([sem, np.full(pad, 77, np.int32)])
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    out = []
    for need_den in (True, False):
        res = pbnet_ops.cluster_device(t(off), t(org), t(sem), t(seg), radius, min_pts, nv_flag=nv, general_sem=general,
                                       capacity=bool(pad), need_den=need_den)
        c = int(res.n_clusters.item())
        assert c >= 0
        out.append(dict(n_clusters=c, cluster_id=res.cluster_id[:n].cpu().numpy(), cluster_num=res.cluster_num.cpu().numpy(),
                        den=res.den[:n].cpu().numpy(), centers=res.centers[:3 * c].cpu().numpy().view(np.int32),
                        clt_sem=res.clt_sem[:c].cpu().numpy(), member_start=res.member_start[:c + 1].cpu().numpy(),
                        member_idx=res.member_idx[:int(res.member_start[c].item())].cpu().numpy()))
    return out


def _assert_hp_only_equals_exact(exact, fast, min_pts):
    for k in ("n_clusters", "cluster_id", "cluster_num", "centers", "clt_sem", "member_start", "member_idx"):
        assert np.array_equal(np.asarray(fast[k]), np.asarray(exact[k])), k
    assert np.array_equal(fast["den"], np.minimum(exact["den"], min_pts)), "den"


@pytest.mark.parametrize("path", GOLDEN, ids=[os.path.basename(p)[8:-4] for p in GOLDEN])
def test_golden_hp_only_equals_exact(path):
    g = dict(np.load(path))
    exact, fast = _both(g["off"], g["org"], g["sem"], g["seg"], float(g["radius"]), int(g["min_pts"]), nv=bool(g["nv_flag"]))
    assert np.array_equal(exact["den"], g["den_queue"])        # the exact mode still counts exactly
    assert np.array_equal(exact["cluster_id"], g["cluster_id"])
    _assert_hp_only_equals_exact(exact, fast, int(g["min_pts"]))


@pytest.mark.parametrize("path", GOLDEN[::4], ids=[os.path.basename(p)[8:-4] for p in GOLDEN[::4]])
def test_capacity_mode_hp_only_equals_exact(path):
    g = dict(np.load(path))
    n = g["off"].shape[0]
    exact, fast = _both(g["off"], g["org"], g["sem"], g["seg"], float(g["radius"]), int(g["min_pts"]), nv=bool(g["nv_flag"]),
                        pad=n // 3 + 100)
    assert np.array_equal(exact["den"], g["den_queue"])
    _assert_hp_only_equals_exact(exact, fast, int(g["min_pts"]))


def test_all_class_groups_hp_only():
    off, org, sem, seg = _scene_groups(seed=7, pitch=0.04, room=(3.0, 2.4, 2.0), n_boxes=20)
    assert len(seg) == 54
    exact, fast = _both(off, org, sem, seg, 0.04, 31)
    _assert_hp_only_equals_exact(exact, fast, 31)
    assert (exact["den"] > 31).any() and (exact["den"] < 31).any()     # both sides of the threshold are exercised


def test_full_size_scene_hp_only():
    off, org, sem, seg = _scene_groups(seed=2, pitch=0.0225, room=(4.0, 3.2, 2.6), n_boxes=12, copies=3)
    exact, fast = _both(off, org, sem, seg, 0.04, 31)
    want = oracle.binary_cluster(off, org, sem, seg, 0.04, 31)
    assert np.array_equal(exact["den"], want["den_queue"])
    _assert_hp_only_equals_exact(exact, fast, 31)


@pytest.mark.parametrize("min_pts", [0, 1, 31, 200])
def test_far_away_and_clamped_coordinates_hp_only(min_pts):
    """Clamped border cells collect points that are far apart: they keep the pairwise tests in both modes."""
    rng = np.random.default_rng(5)
    P = np.concatenate([rng.normal(0, 0.01, (80, 3)) + [-1500.0, 2000.0, -3.0], rng.normal(0, 0.01, (90, 3)) + [1e4, -1e4, 1e4],
                        rng.normal(0, 0.01, (70, 3)), rng.normal(0, 0.002, (60, 3)),
                        rng.uniform(-3e3, 3e3, (50, 3)) + [0.0, 0.0, 5e4]]).astype(np.float32)
    sem = np.full(len(P), 17)
    exact, fast = _both(P, P, sem, [len(P)], 0.04, min_pts)
    want = oracle.binary_cluster(P, P, sem, [len(P)], 0.04, min_pts)
    assert np.array_equal(exact["den"], want["den_queue"])
    assert np.array_equal(exact["cluster_id"], want["cluster_id"])
    _assert_hp_only_equals_exact(exact, fast, min_pts)


def test_shims_keep_the_exact_count(golden_dir):
    """pbnet_ops.cluster and PB_lib.binary_cluster return den_queue: they run the exact mode."""
    from pbnet_amd import PB_lib
    g = dict(np.load(os.path.join(golden_dir, "cluster_G6.npz")))
    off, org = torch.from_numpy(g["off"]), torch.from_numpy(g["org"])
    sem, seg = torch.from_numpy(g["sem"]).long(), torch.from_numpy(g["seg"])
    want = oracle.binary_cluster(g["off"], g["org"], g["sem"], g["seg"], 0.04, 31)
    assert (want["den_queue"] > 31).any()
    _, _, den, _ = pbnet_ops.cluster(off, org, sem, seg, 0.04, 31, len(seg))
    assert np.array_equal(den.numpy(), want["den_queue"] + 1)
    n = off.shape[0]
    x, y, z = (off[:, k].contiguous() for k in range(3))
    xo, yo, zo = (org[:, k].contiguous() for k in range(3))
    den_q = torch.zeros(n, dtype=torch.int32)
    mapper = torch.cat([torch.arange(int(k)) for k in seg]).int()
    PB_lib.binary_cluster(x, y, z, x.abs() + y.abs() + z.abs(), mapper, xo, yo, zo, sem.int(), seg, torch.ones(18) * 0.04,
                          (torch.ones(18) * 31).int(), torch.full((n,), -1, dtype=torch.int32),
                          torch.zeros(len(seg), dtype=torch.int32), den_q, torch.zeros(n, dtype=torch.float32),
                          torch.zeros(n, dtype=torch.int32), len(seg), 0.05, True)
    assert np.array_equal(den_q.numpy(), want["den_queue"])
