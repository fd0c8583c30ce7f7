"""The shared device primitives on their own (csrc/selftest.hip): the range fill, the two exclusive scans and the 32-bit
radix sort, called exactly as the stages call them.  These wrappers check arguments, size the workspace and raise on a
non-zero return; they compute nothing.  tests/test_prims_gpu.py holds the designed cases, tests/prims_ref.py the statement."""
import ctypes

import torch

from . import _native as N

SCAN, SCAN_CHAINED, SORT = 0, 1, 2          # `what` of pbn_selftest_workspace_bytes
SCAN_TILE, SCAN_THREADS = 2048, 256         # csrc/pbn_common.h: elements per workgroup of a scan, its threads
SCAN_CHAIN_SPIN = 16                        # csrc/pbn_common.h: a workgroup of the chained scan gave up waiting
SORT_SPIN = 8                               # csrc/sort_dev.h SCAN_SORT_SPIN: a workgroup of the sort gave up waiting
MAX_RANGES = 64                             # ranges of one fill call
MAX_N = 1 << 28


def sort_tile():
    """Keys per workgroup of a digit pass in the library that is loaded."""
    return int(N.lib().pbn_selftest_sort_tile())


def workspace(what, n, dev):
    if what not in (SCAN, SCAN_CHAINED, SORT):
        raise ValueError("selftest.workspace: unknown primitive %r" % (what,))
    nbytes = N.lib().pbn_selftest_workspace_bytes(what, int(n))
    if nbytes == 0:
        raise ValueError("selftest.workspace: %r elements are outside 0..2^28" % (n,))
    return torch.empty(nbytes, dtype=torch.uint8, device=dev)


def _check_i32(name, t, n):
    N.require_cuda(t)
    if t.dtype != torch.int32 or t.dim() != 1 or not t.is_contiguous() or t.numel() < n:
        raise TypeError("%s must be a contiguous int32 vector of at least %d elements, got %s %s" % (name, n, t.dtype, tuple(t.shape)))
    return t


def _check_ws(ws, what, n, dev):
    if ws is None:
        return workspace(what, n, dev)
    N.require_cuda(ws)
    if ws.dtype != torch.uint8 or not ws.is_contiguous():
        raise TypeError("workspace must be a contiguous uint8 tensor")
    return ws


def fill(buf, ranges):
    """One fill_ranges call on `buf` (uint8, device): ranges = [(offset, nbytes, value)], offset None = a null pointer."""
    N.require_cuda(buf)
    if buf.dtype != torch.uint8 or buf.dim() != 1 or not buf.is_contiguous():
        raise TypeError("fill: buf must be a contiguous uint8 vector")
    k = len(ranges)
    if k > MAX_RANGES:
        raise ValueError("fill: %d ranges, at most %d" % (k, MAX_RANGES))
    off, cnt, val = (N.c_i64 * max(k, 1))(), (N.c_i64 * max(k, 1))(), (ctypes.c_uint8 * max(k, 1))()
    for i, (o, b, v) in enumerate(ranges):
        o, b, v = (-1 if o is None else int(o)), int(b), int(v)
        if b < 0 or not 0 <= v <= 255 or o < -1 or (o >= 0 and o + b > buf.numel()):
            raise ValueError("fill: range %d (%r, %r, %r) does not lie in a buffer of %d bytes" % (i, o, b, v, buf.numel()))
        off[i], cnt[i], val[i] = o, b, v
    N.check(N.lib().pbn_selftest_fill(N.ptr(buf), off, cnt, val, k, N.current_stream()), "pbn_selftest_fill")


def scan(inp, out, n, chained=False, total=None, status=None, ws=None):
    """out[:n] = exclusive prefix sums of inp[:n]; total (an int32 tensor of one element, or None) gets the sum.  inp and out
    may be the same tensor and total may be out[n:n + 1]: the addresses go through as they are.  Returns (status, ws); status
    is an int32 [1] tensor, zeroed here unless given."""
    n = int(n)
    if not 0 <= n <= MAX_N:
        raise ValueError("scan: n = %d is outside 0..2^28" % n)
    _check_i32("inp", inp, n)
    _check_i32("out", out, n)
    if total is not None:
        _check_i32("total", total, 1)
    dev = inp.device
    if status is None:
        status = torch.zeros(1, dtype=torch.int32, device=dev)
    _check_i32("status", status, 1)
    what = SCAN_CHAINED if chained else SCAN
    ws = _check_ws(ws, what, n, dev)
    N.check(N.lib().pbn_selftest_scan(N.ptr(inp), N.ptr(out), n, int(bool(chained)), N.ptr(total), N.ptr(status), N.ptr(ws),
                                      ws.numel(), N.current_stream()), "pbn_selftest_scan")
    return status, ws


def sort_u32(keys, vals, ws=None):
    """Stable sort of (keys[i], vals[i]) by key.  keys: int32 holding the 32 key bits, vals: int32.  Returns keys_out (int64:
    the 64-bit words of the sort's output buffer), vals_out, status (int32 [1], zeroed here) and the workspace, which a second
    call may be given as it is."""
    n = int(keys.numel())
    if n > MAX_N:
        raise ValueError("sort_u32: %d keys, at most 2^28" % n)
    _check_i32("keys", keys, n)
    _check_i32("vals", vals, n)
    if vals.numel() != n:
        raise ValueError("sort_u32: %d values for %d keys" % (vals.numel(), n))
    dev = keys.device
    keys_out = torch.empty(n, dtype=torch.int64, device=dev)
    vals_out = torch.empty(n, dtype=torch.int32, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    ws = _check_ws(ws, SORT, n, dev)
    N.check(N.lib().pbn_selftest_sort_u32(N.ptr(keys), N.ptr(vals), n, N.ptr(keys_out), N.ptr(vals_out), N.ptr(status), N.ptr(ws),
                                          ws.numel(), N.current_stream()), "pbn_selftest_sort_u32")
    return keys_out, vals_out, status, ws
