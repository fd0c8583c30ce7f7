"""GPU tier: the HIP grouping pipeline against the brute-force statement of the specification (tests/bruteforce_cluster.py) on the
designed inputs of tests/cluster_cases.py -- one family per cell-driven branch of csrc/cluster.hip -- in four call modes: exact,
HP-only (need_den=False), capacity (garbage rows behind the points that exist) and the general (component, class) path forced on
single-class inputs.  No tolerances: the arithmetic contract fixes every bit, centre bits included."""
import numpy as np
import pytest
import torch

import cluster_cases as CC
from pbnet_amd import _native as N
from pbnet_amd import pbnet_ops

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
MODES = ("exact", "hp_only", "capacity", "general")
PARAMS = [(c["name"], m) for c in CC.cases() for m in MODES if not (m == "general" and CC.is_general(c))]


def _device_run(c, mode):
    n = c["off"].shape[0]
    off, org, sem = c["off"], c["org"], c["sem"]
    if mode == "capacity":
        pad = n // 3 + 100
        rng = np.random.default_rng(1)
        junk3 = rng.normal(0, 50, (pad, 3)).astype(np.float32)
        junk3[::7] = np.nan
        off = np.concatenate([off, junk3])
        org = np.concatenate([org, junk3[::-1]])
        sem = np.concatenate([sem, np.full(pad, 77, np.int32)])      # an invalid class id: must never be looked at
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    res = pbnet_ops.cluster_device(t(off), t(org), t(sem), t(c["seg"]), c["radius"], c["min_pts"], para_f=c["para_f"],
                                   nv_flag=c["nv_flag"], general_sem=CC.is_general(c) or mode == "general",
                                   capacity=mode == "capacity", need_den=mode != "hp_only")
    k = int(res.n_clusters.item())
    assert k >= 0
    return dict(n_clusters=k, cluster_id=res.cluster_id[:n].cpu().numpy(), cluster_num=res.cluster_num.cpu().numpy(),
                den=res.den[:n].cpu().numpy(), center=res.centers[:3 * k].cpu().numpy().reshape(k, 3),
                clt_sem=res.clt_sem[:k].cpu().numpy(), member_start=res.member_start[:k + 1].cpu().numpy(),
                member_idx=res.member_idx.cpu().numpy())


@pytest.mark.parametrize("name,mode", PARAMS, ids=["%s-%s" % p for p in PARAMS])
def test_hip_equals_bruteforce(name, mode):
    c = CC.case(name)
    want = CC.reference(name)
    got = _device_run(c, mode)
    k = want["center"].shape[0]
    assert got["n_clusters"] == k
    for key in ("cluster_id", "cluster_num", "clt_sem"):
        assert np.array_equal(got[key], want[key]), key
    count = want["den_queue"]
    assert np.array_equal(got["den"], np.minimum(count, c["min_pts"]) if mode == "hp_only" else count), "den"
    assert np.array_equal(got["center"].view(np.int32), want["center"].view(np.int32)), "centre bits"
    ms = got["member_start"]
    assert ms[0] == 0 and ms[k] == (want["cluster_id"] >= 0).sum()
    for j in range(k):                                               # members CSR == nonzero(cluster_id == j), in index order
        assert np.array_equal(got["member_idx"][ms[j]:ms[j + 1]], np.nonzero(want["cluster_id"] == j)[0]), j


def test_too_many_segments_is_an_argument_error_and_writes_nothing():
    """65536 segments do not fit the 16-bit segment field of the cell key: PBN_ERR_ARG, every output untouched."""
    n, b = 8, CC.N_SEG_TOO_MANY
    i32 = dict(dtype=torch.int32, device=DEV)
    xyz = torch.rand(n, 3, device=DEV)
    sem = torch.full((n,), 17, **i32)
    seg = torch.zeros(b, **i32)
    seg[b - 1] = n
    mark = 0x5A5A5A5A
    outs = dict(cluster_id=torch.full((n,), mark, **i32), cluster_num=torch.full((b,), mark, **i32), den=torch.full((n,), mark, **i32),
                centers=torch.full((3 * n,), 123.25, device=DEV), clt_sem=torch.full((n,), mark, **i32),
                n_clusters=torch.full((1,), mark, **i32), member_start=torch.full((n + 1,), mark, **i32),
                member_idx=torch.full((n,), mark, **i32))
    lib = N.lib()
    ws_bytes = lib.pbn_cluster_workspace_bytes(n, b, 0)
    ws = torch.full((max(ws_bytes, 1),), 0x5A, dtype=torch.uint8, device=DEV)
    rc = lib.pbn_binary_cluster(N.ptr(xyz), N.ptr(xyz), N.ptr(sem), N.ptr(seg), n, b, 0.04, 2, 0.05, 1, 0, N.ptr(outs["cluster_id"]),
                                N.ptr(outs["cluster_num"]), N.ptr(outs["den"]), N.ptr(outs["centers"]), N.ptr(outs["clt_sem"]),
                                N.ptr(outs["n_clusters"]), N.ptr(outs["member_start"]), N.ptr(outs["member_idx"]), N.ptr(ws), ws_bytes,
                                N.current_stream())
    torch.cuda.synchronize()
    assert rc == N.PBN_ERR_ARG
    for key, v in outs.items():
        assert bool((v == (123.25 if key == "centers" else mark)).all()), key
    assert bool((ws == 0x5A).all())
    with pytest.raises(RuntimeError, match="PBN_ERR_ARG"):
        pbnet_ops.cluster_device(xyz, xyz, sem, seg, 0.04, 2)
    # one segment fewer is served: 65535 segments, the points in the last one
    ok = pbnet_ops.cluster_device(xyz, xyz, sem, seg[1:].contiguous(), 0.04, 2)
    assert int(ok.n_clusters.item()) >= 0 and ok.cluster_num.shape[0] == b - 1
