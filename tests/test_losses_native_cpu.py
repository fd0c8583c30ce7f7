"""CPU tier of the native losses (csrc/losses.hip, pbnet_amd/losses.py): the float64 twin that serves as gradient reference
agrees with the oracle, and the three C entries exist, size their workspace and refuse bad arguments on the host."""
import numpy as np
import pytest

import loss_grad_ref as G
from pbnet_amd import _native as N
from pbnet_amd.config import get_config
from test_losses import TOL, _case

NAMES = ("pbn_losses_workspace_bytes", "pbn_losses_forward", "pbn_losses_backward")


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_float64_twin_agrees_with_oracle(seed):
    c, mine = _case(seed), G.case(seed)
    assert set(c) == set(mine) and all(np.array_equal(c[k], mine[k]) for k in c)      # the GPU tier's inputs are _case's
    cfg = get_config()
    want = G.oracle_terms(c, cfg.fg_thresh, cfg.bg_thresh)
    before = c["gt_mask"].copy()
    got, grads = G.twin(c, cfg.fg_thresh, cfg.bg_thresh)
    assert np.array_equal(c["gt_mask"], before)
    for k in G.TERMS:
        print("%s: twin %.9f oracle %.9f" % (k, got[k], want[k]))
        assert abs(got[k] - want[k]) <= TOL * max(1.0, abs(want[k])), k
    assert all(g is not None and np.isfinite(g).all() for g in grads.values())
    # zero-norm prediction rows: the norm's gradient is 0 there, what is left is -g^ / 1e-8 / (n_valid + 1e-6)
    assert np.abs(grads["offset"][:5]).max() > 1e3
    point_only, _ = G.twin(c, cfg.fg_thresh, cfg.bg_thresh, clustered=False)
    assert set(point_only) == {"semantic_loss", "offset_norm_loss", "offset_dir_loss", "loss"}


def test_signatures_hold_the_loss_entries():
    assert all(n in N.SIGNATURES for n in NAMES)
    lib = N.lib()
    assert all(hasattr(lib, n) for n in NAMES)


def test_workspace_query_is_positive_and_monotone():
    q = N.lib().pbn_losses_workspace_bytes
    sizes = [0, 1, 255, 257, 5000, 70001, 1200000, 5000000]
    for fixed in (0, 3000):
        pts = [q(n, fixed, fixed) for n in sizes]
        rows = [q(fixed, n, fixed) for n in [-1] + sizes]
        prop = [q(fixed, fixed, n) for n in sizes]
        for seq in (pts, rows, prop):
            assert seq[0] > 0 and all(a <= b for a, b in zip(seq, seq[1:])), seq
    assert q(70001, 3000, 9) > q(1, 0, 0)
    assert q(-1, 0, 0) == 0 and q(0, 0, -1) == 0


def test_forward_refuses_bad_arguments_before_any_launch():
    """Every check runs on the host before a launch: the pointers below are never dereferenced."""
    lib = N.lib()
    vp = N.c_vp
    fake = 1 << 20                                    # 16-byte aligned, never touched
    need = lib.pbn_losses_workspace_bytes(1000, 300, 9)

    def call(sem=fake, sem_dt=0, ld=20, n=1000, k=20, mask_dt=0, gt_mask=fake, rows=300, clt_dt=0, prop=9, off_dt=0, ws=fake,
             ws_bytes=need, terms=fake):
        return lib.pbn_losses_forward(vp(sem), sem_dt, ld, vp(fake), vp(fake), off_dt, vp(fake), vp(fake), vp(fake), n, k,
                                      vp(fake), mask_dt, vp(gt_mask), vp(fake), rows, vp(fake), 7, vp(fake), clt_dt, prop, 0.95,
                                      0.2, vp(fake), vp(terms), vp(fake), vp(fake), vp(ws), ws_bytes, None)

    assert call(sem=None) == N.PBN_ERR_ARG
    assert call(gt_mask=None) == N.PBN_ERR_ARG
    assert call(terms=None) == N.PBN_ERR_ARG
    assert call(ws=None) == N.PBN_ERR_ARG
    assert call(n=-1) == N.PBN_ERR_ARG
    assert call(prop=-1) == N.PBN_ERR_ARG
    assert call(k=1) == N.PBN_ERR_ARG and call(k=65, ld=65) == N.PBN_ERR_ARG
    assert call(ld=19) == N.PBN_ERR_ARG                                  # rows would overlap
    assert call(sem=fake + 2) == N.PBN_ERR_ARG                           # float32 logits at an odd half-word
    for bad in (dict(sem_dt=3), dict(off_dt=-1), dict(mask_dt=7), dict(clt_dt=3)):
        assert call(**bad) == N.PBN_ERR_UNSUPPORTED, bad
    assert call(ws_bytes=need - 256) == N.PBN_ERR_WORKSPACE
    assert call(ws_bytes=0) == N.PBN_ERR_WORKSPACE
    # below cluster_epoch (rows < 0) the mask / proposal arguments are not looked at, and the workspace is smaller
    assert call(rows=-1, mask_dt=7, gt_mask=None, ws_bytes=lib.pbn_losses_workspace_bytes(1000, -1, 0) - 256) == N.PBN_ERR_WORKSPACE
