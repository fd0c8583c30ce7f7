"""Plain numpy statements of the shared device primitives (csrc/common.hip fill_ranges, scan_exclusive_i32 and its chained
form; csrc/sort.hip radix_sort_u32), all on the host in int64 / uint64.  Nothing here knows about tiles, windows or digits:
that is tests/prims_mutants.py, which must agree with these on every designed case."""
import numpy as np

INT32_MIN, INT32_MAX = -(1 << 31), (1 << 31) - 1


def scan(x):
    """Exclusive prefix sums of an int32 vector: (out int32 [n], total).  The running sums must fit int32 (asserted)."""
    x = np.asarray(x, np.int32)
    incl = np.cumsum(x.astype(np.int64))
    if len(x):
        assert INT32_MIN <= incl.min() and incl.max() <= INT32_MAX, "a running sum leaves int32"
    out = np.zeros(len(x), np.int64)
    out[1:] = incl[:-1]
    return out.astype(np.int32), int(incl[-1]) if len(x) else 0


def sort(keys, vals):
    """Stable sort of (key, value) pairs by the 32-bit key: (keys_out uint64 [n], vals_out int32 [n])."""
    keys = np.asarray(keys, np.uint32)
    vals = np.asarray(vals, np.int32)
    order = np.argsort(keys, kind="stable")
    return keys[order].astype(np.uint64), vals[order]


def fill(buf, ranges):
    """`buf` (uint8) after the ranges [(offset, nbytes, value)] were filled in list order; offset None = a null pointer."""
    out = np.array(buf, np.uint8, copy=True)
    for off, nbytes, value in ranges:
        if off is None or nbytes == 0:
            continue
        assert 0 <= off and off + nbytes <= len(out)
        out[off:off + nbytes] = value
    return out


def order_key(w):
    """csrc/mesh.hip / orient.hip order_key of float32 values: ascending as unsigned, NaN last, -0 ties with +0."""
    w = np.asarray(w, np.float32)
    b = w.view(np.uint32).copy()
    b[w == 0] = 0
    k = np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000)).astype(np.uint32)
    k[np.isnan(w)] = 0xffffffff
    return k
