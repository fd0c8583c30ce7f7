"""GPU tier: the rows a caller expects per level are an ARGUMENT of the capacity-form U-Net forward (pbn_unet_forward_dev's
rows_expected; csrc/executor.hip hands them to every launch as ConvHints) -- no state between calls.

One synthetic blob of about 28 000 voxels after de-duplication under a MinkUNet14A plan, fp32 and bf16.  Level capacities are
the exact counts x 1.25 rounded up to 256: level 0 then has a capacity above the wave family's 30 000-row limit and expected
rows below it, the smallest shape at which the expectation changes the kernel family of a launch.

(a) rows_expected = the exact counts against pbn_unet_forward at the exact sizes, on the rows that exist.
    Observed once at the parent commit, where the expectation went through the thread-local setter pbn_unet_set_rows_hint:
    bit equality in fp32 and in bf16 (max |diff| 0 over 28 113 rows; the same run with the capacities as expectation
    differed from the exact forward by 2.9e-6 in fp32 and 2.0e-3 in bf16, so the expectation does decide kernels here).
    Asserted here: bit equality.
(b) rows_expected = NULL against rows_expected = the capacities: bit for bit (NULL means "choose by the capacities")."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from pbnet_amd import _native as N
from pbnet_amd import planned
from pbnet_amd.MinkowskiEngine.conv import SPLITK_WORKSPACE_BYTES
from pbnet_amd.network.mink_unet import alloc_arena, input_slab

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_unet_plan_golden as G  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
WAVE_MAX_ROWS = 30000               # csrc/spconv_wave.hip: wave_family_wanted


def _blob():
    """Integer points of a ball (27 000 .. 29 000 of them) in a fixed shuffled order, the first 500 once more at the end."""
    r = np.arange(-19, 20)
    x, y, z = np.meshgrid(r, r, r, indexing="ij")
    keep = x * x + y * y + z * z <= 355
    pts = np.stack([x[keep], y[keep], z[keep]], 1).astype(np.int32) + 24
    pts = pts[np.random.RandomState(11).permutation(len(pts))]
    coords = np.concatenate([np.zeros((len(pts), 1), np.int32), pts], 1)
    return np.concatenate([coords, coords[:500]], 0), len(pts)


def _forward_dev(lib, plan, n_rows, counts_dev, rows_expected, slab, cin_p, tables, arena, nbytes, dt, ws):
    vp = ctypes.c_void_p
    hint = None if rows_expected is None else (ctypes.c_int32 * 5)(*rows_expected)
    return lib.pbn_unet_forward_dev(plan["ops"], plan["n_ops"], plan["bufs"], plan["n_bufs"], n_rows, vp(counts_dev.data_ptr()), hint,
                                    vp(slab.data_ptr()), cin_p, *tables, vp(arena.data_ptr()), nbytes, N.DT[dt],
                                    vp(ws.data_ptr()), ws.numel(), N.current_stream())


def run_case(dt):
    """One forward per form: the output rows that exist of 'exact' (pbn_unet_forward at the exact sizes) and of the capacity
    form with rows_expected = the exact counts ('expect'), NULL ('none') and the capacities ('caps')."""
    lib = N.lib()
    coords_np, n_unique = _blob()
    n_in = len(coords_np)
    cap0 = -(-int(n_unique * 1.25) // 256) * 256
    assert 27000 <= n_unique <= 29000 and n_unique < WAVE_MAX_ROWS < cap0 and n_in <= cap0
    coords = torch.zeros(cap0, 4, dtype=torch.int32, device=DEV)
    coords[:n_in] = torch.from_numpy(coords_np).to(DEV)
    n_dev = torch.tensor([n_in], dtype=torch.int32, device=DEV)
    lin = planned._Lineage(coords, cap0, n_dev, DEV)
    exact = [int(v) for v in lin.counts.tolist()]
    assert exact[0] == n_unique
    caps = [-(-int(v * 1.25) // 256) * 256 for v in exact]
    assert caps[0] == cap0
    net = G.build("MinkUNet14A").to(DEV)
    plan = net._plan(dt)
    cin_p = plan["cin_p"]
    feats = torch.randn(n_in, G.CIN, generator=torch.Generator().manual_seed(13)).to(DEV, dt)
    slab = input_slab(feats, cin_p, lin.perm, lin.unique_index, cap0, lin.counts)
    ws = torch.empty(SPLITK_WORKSPACE_BYTES, dtype=torch.uint8, device=DEV)
    tables = lin.tables()
    out = {}
    arena, nbytes, offs, n_rows = alloc_arena(plan["bufs"], plan["n_bufs"], exact, dt, DEV)
    vp = ctypes.c_void_p
    N.check(lib.pbn_unet_forward(plan["ops"], plan["n_ops"], plan["bufs"], plan["n_bufs"], n_rows, vp(slab.data_ptr()), cin_p,
                                 *tables, vp(arena.data_ptr()), nbytes, N.DT[dt], vp(ws.data_ptr()), ws.numel(),
                                 N.current_stream()), "pbn_unet_forward")
    out["exact"] = net._output_rows(plan, arena, offs, exact[0], dt).clone()
    for name, expected in (("expect", exact), ("none", None), ("caps", caps)):
        arena, nbytes, offs, n_rows = alloc_arena(plan["bufs"], plan["n_bufs"], caps, dt, DEV)
        N.check(_forward_dev(lib, plan, n_rows, lin.counts, expected, slab, cin_p, tables, arena, nbytes, dt, ws),
                "pbn_unet_forward_dev")
        out[name] = net._output_rows(plan, arena, offs, caps[0], dt)[:exact[0]].clone()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out["exact"].float()).all()) and float(out["exact"].float().abs().max()) > 0
    return out


@pytest.fixture(scope="module", params=[torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def forms(request):
    with torch.no_grad():
        return run_case(request.param)


def test_expected_rows_against_the_exact_forward(forms):
    diff = (forms["expect"].float() - forms["exact"].float()).abs().max().item()
    print("rows_expected = exact counts vs pbn_unet_forward at exact sizes: max |diff| %.3e, bit-equal %s" % (
        diff, torch.equal(forms["expect"], forms["exact"])))
    assert torch.equal(forms["expect"], forms["exact"])
    # ... and the expectation is what decides it: chosen by the capacities, level 0 leaves the wave family and the sums reorder
    assert not torch.equal(forms["caps"], forms["exact"])


def test_null_means_choose_by_the_capacities(forms):
    assert torch.equal(forms["none"], forms["caps"])
