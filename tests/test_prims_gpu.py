"""GPU tier: fill_ranges, scan_exclusive_i32, scan_exclusive_i32_chained and radix_sort_u32 on their own (csrc/selftest.hip
calls them as the stages do) on the designed inputs of tests/prims_cases.py, against the plain numpy statement
tests/prims_ref.py.  All integers and bytes: no tolerance.  Every buffer carries canaries around what may be written.  The
file's wall time is printed by its last test (pytest -s)."""
import time

import numpy as np
import pytest
import torch

import prims_cases as PC
from pbnet_amd import selftest as S

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
CANARY = -1515870811                                             # 0xA5A5A5A5
T0 = [None]


@pytest.fixture(autouse=True, scope="module")
def _wall_clock():
    T0[0] = time.perf_counter()
    yield


def _dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)                 # a copy: the cases are read-only


# ---- scans -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", PC.SCAN_NAMES)
def test_scan_equals_reference(name):
    c = PC.scan_case(name)
    n = c["n"]
    # out holds n results, then the canary (or the total, in the adjacent variant), then one more canary
    src = torch.full((n + 2,), CANARY, dtype=torch.int32, device=DEV)
    src[:n] = _dev(c["in"])
    out = src if c["alias"] else torch.full((n + 2,), CANARY, dtype=torch.int32, device=DEV)
    if c["nototal"]:
        total = None
    elif c["adjacent"]:
        total = out[n:n + 1]
    else:
        total = torch.full((3,), CANARY, dtype=torch.int32, device=DEV)[1:2]      # non-zero before the call, n = 0 included
    status, _ = S.scan(src, out, n, chained=c["chained"], total=total)
    torch.cuda.synchronize()
    st = int(status.item())
    assert st & S.SCAN_CHAIN_SPIN == 0, "a workgroup of the chained scan gave up waiting"
    assert st == 0
    got = out.cpu().numpy()
    assert np.array_equal(got[:n], c["out"]), "first difference at %d of %d" % (int(np.argmax(got[:n] != c["out"])), n)
    if total is not None:
        assert int(total.item()) == c["total"]
    assert got[n + 1] == CANARY and (c["adjacent"] or got[n] == CANARY)
    if not c["alias"]:
        assert np.array_equal(src.cpu().numpy()[:n], c["in"]) and (src[n:] == CANARY).all()


# ---- sort ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", PC.SORT_NAMES)
def test_sort_equals_reference(name):
    c = PC.sort_case(name)
    n = c["n"]
    keys, vals = _dev(c["keys"].view(np.int32)), _dev(c["vals"])
    first = None
    ws = None
    for call in range(2):                                        # the second call goes into the used workspace as it is
        keys_out, vals_out, status, ws = S.sort_u32(keys, vals, ws=ws)
        torch.cuda.synchronize()
        st = int(status.item())
        assert st & S.SORT_SPIN == 0, "a workgroup of the sort gave up waiting"
        assert st == 0
        k, v = keys_out.cpu().numpy().view(np.uint64), vals_out.cpu().numpy()
        assert np.array_equal(v, c["vals_out"]), "call %d: not the stable order" % call
        assert np.array_equal(k, c["keys_out"]), "call %d: keys (low words sorted, high words 0)" % call
        assert n == 0 or int(k.max()) < 1 << 32
        if first is None:
            first = (k.tobytes(), v.tobytes())
        else:
            assert first == (k.tobytes(), v.tobytes()), "the second call into the same workspace differs"
    assert np.array_equal(keys.cpu().numpy(), c["keys"].view(np.int32)) and np.array_equal(vals.cpu().numpy(), c["vals"])


# ---- fill ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", PC.FILL_NAMES)
def test_fill_equals_reference(name):
    buf = torch.full((PC.FILL_BYTES,), PC.FILL_PRESET, dtype=torch.uint8, device=DEV)
    assert buf.data_ptr() % 16 == 0                              # offsets are alignments
    S.fill(buf, PC.FILL_CASES[name])
    torch.cuda.synchronize()
    got, want = buf.cpu().numpy(), PC.fill_reference(name)
    assert np.array_equal(got, want), "bytes differ at %s .." % np.flatnonzero(got != want)[:8]


def test_wall_time():
    print("\ntests/test_prims_gpu.py: %.2f s wall for %d scan, %d sort and %d fill cases" % (
        time.perf_counter() - T0[0], len(PC.SCAN_NAMES), len(PC.SORT_NAMES), len(PC.FILL_NAMES)))
