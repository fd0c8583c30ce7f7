"""The specification of the coordinate pyramid (include/pbnet_hip.h: pbn_prepare_layout; csrc/pyramid.hip) in plain numpy, and the
helpers that read a prepared arena back.  reference() returns every array of the contract in its EXACT device form: the contract
fixes the order of every level (Z-order of the file comment of pyramid.hip; parents numbered by first child), so the sorted
pipeline is compared element for element; canonical() is the order-free form for pipelines with another row order (the hash-table
pipeline's curve has another origin; pbn_coords_build keeps the external order).

Nothing here shares code with the kernels: floor is np.floor_divide, the interleave is a bit loop, lookups are searches in packed
64-bit coordinate keys.  The GPU helpers (_prepare, _view, _arrays) import torch lazily, so the CPU tier needs no device."""
import ctypes

import numpy as np

DEV = "cuda:0"
MAX_KEY_BITS = 44                   # the widest digit plan: 4 digits of 11 bits
LO, HI = -32768, 32767              # the packable coordinate range; batch indices are 0..65534


# ---- the specification ---------------------------------------------------------------------------------------------------------
def kernel_offsets(ksize, x_fastest=1):
    """Conventions C1/C2 of oracle/sparse_ref.py: entry k of a cube -> (dx, dy, dz); odd sizes centred; x fastest (C1) or, with
    x_fastest = 0, z fastest."""
    c0 = ksize // 2 if ksize % 2 else 0
    out = []
    for slow in range(ksize):
        for mid in range(ksize):
            for fast in range(ksize):
                out.append((fast - c0, mid - c0, slow - c0) if x_fastest else (slow - c0, mid - c0, fast - c0))
    return np.array(out, np.int64)


def pack_key(c):
    """[n,4] in-range coordinates -> one uint64 per row, injective."""
    c = np.asarray(c, np.int64)
    u = lambda a: a.astype(np.uint64)
    return (u(c[:, 0]) << np.uint64(48)) | (u(c[:, 1] - LO) << np.uint64(32)) | (u(c[:, 2] - LO) << np.uint64(16)) | u(c[:, 3] - LO)


def interleave3(x, y, z, e):
    """Bit i of x, y, z -> bits 3i, 3i + 1, 3i + 2."""
    key = np.zeros(len(x), np.uint64)
    for i in range(e):
        for a, v in enumerate((x, y, z)):
            key |= ((v.astype(np.uint64) >> np.uint64(i)) & np.uint64(1)) << np.uint64(3 * i + a)
    return key


def sort_plan(nbits):
    """(passes, digit bits) of the LSD sort for a key of nbits bits: up to 33 bits min(3, ceil(nbits / 8)) digits, up to 44 bits
    four; each digit as narrow as that allows, at least 8 bits.  None: no plan holds the key."""
    if nbits > MAX_KEY_BITS:
        return None
    passes = min(3, -(-nbits // 8)) if nbits <= 33 else 4
    return passes, max(8, -(-nbits // passes))


def _first_occurrence_ids(keys):
    """ids numbering the distinct keys in the order of their first occurrence; (first row of every id, id of every row)."""
    _, first, inv = np.unique(keys, return_index=True, return_inverse=True)
    order = np.argsort(first, kind="stable")
    rank = np.empty(len(order), np.int64)
    rank[order] = np.arange(len(order))
    return first[order], rank[inv.reshape(-1)]


def _lookup(level_coords, query):
    """row of every query coordinate in level_coords, -1 when absent or outside the coordinate range."""
    ok = ((query[:, 1:] >= LO) & (query[:, 1:] <= HI)).all(1)
    keys = pack_key(level_coords)
    order = np.argsort(keys, kind="stable")
    want = pack_key(np.where(ok[:, None], query, 0))
    pos = np.minimum(np.searchsorted(keys[order], want), len(keys) - 1)
    return np.where(ok & (keys[order][pos] == want), order[pos], -1).astype(np.int32)


def reference(coords, n_valid=None, x_fastest=1, want_k5=1):
    coords = np.asarray(coords, np.int64).reshape(-1, 4)
    c_in = coords if n_valid is None else coords[:n_valid]
    n = len(c_in)
    out = {"nbits": 0, "plan": None, "e": 0, "origin": None}
    if n == 0:
        out.update(counts=np.zeros(5, np.int32), n_unique=np.zeros(1, np.int32), unique_index=np.zeros(0, np.int64),
                   inverse=np.zeros(0, np.int64), perm=np.zeros(0, np.int64), inv_perm=np.zeros(0, np.int64),
                   ucoords=np.zeros((0, 4), np.int32))
        for l in range(5):
            out["coords%d" % l] = np.zeros((0, 4), np.int32)
            out["k3_%d" % l] = np.zeros((0, 27), np.int32)
        for l in range(4):
            out["parent_row%d" % l] = out["child_k%d" % l] = np.zeros(0, np.int32)
            out["nbr_down%d" % l] = out["up%d" % l] = np.zeros((0, 8), np.int32)
        if want_k5:
            out["k5"] = np.zeros((0, 125), np.int32)
        return out
    assert (c_in[:, 0] >= 0).all() and (c_in[:, 0] < 65535).all() and (c_in[:, 1:] >= LO).all() and (c_in[:, 1:] <= HI).all()
    # de-duplication: first occurrence wins, survivors in ascending input order
    first, inverse = _first_occurrence_ids(pack_key(c_in))
    uc = c_in[first]
    n1 = len(uc)
    # Z-order
    b_min = int(uc[:, 0].min())
    origin = np.floor_divide(uc[:, 1:].min(0), 16) * 16
    ext = int((uc[:, 1:].max(0) - origin).max())
    e = max(1, ext.bit_length())
    nbits = 3 * e + int(uc[:, 0].max() - b_min).bit_length()
    rel = uc[:, 1:] - origin
    zkey = ((uc[:, 0] - b_min).astype(np.uint64) << np.uint64(3 * e)) | interleave3(rel[:, 0], rel[:, 1], rel[:, 2], e)
    perm = np.argsort(zkey, kind="stable")
    inv_perm = np.empty(n1, np.int64)
    inv_perm[perm] = np.arange(n1)
    out.update(nbits=nbits, plan=sort_plan(nbits), e=e, origin=origin, b_min=b_min, zkeys=zkey[perm],
               n_unique=np.array([n1], np.int32), unique_index=first.astype(np.int64), inverse=inverse.astype(np.int64),
               perm=perm.astype(np.int64), inv_perm=inv_perm, ucoords=uc.astype(np.int32))
    # levels: floor(c / 2^l) * 2^l, rows numbered in the order of their first child
    levels = [uc[perm]]
    for l in range(1, 5):
        fine = levels[-1]
        s = 1 << l
        pc = fine.copy()
        pc[:, 1:] = np.floor_divide(fine[:, 1:], s) * s
        first_child, parent = _first_occurrence_ids(pack_key(pc))
        par = np.floor_divide(fine[:, 1:], s // 2) % 2
        ck = par[:, 0] + 2 * par[:, 1] + 4 * par[:, 2]
        nbr_down = np.full((len(first_child), 8), -1, np.int32)
        nbr_down[parent, ck] = np.arange(len(fine))
        up = np.full((len(fine), 8), -1, np.int32)
        up[np.arange(len(fine)), ck] = parent
        out["parent_row%d" % (l - 1)] = parent.astype(np.int32)
        out["child_k%d" % (l - 1)] = ck.astype(np.int32)
        out["nbr_down%d" % (l - 1)] = nbr_down
        out["up%d" % (l - 1)] = up
        levels.append(pc[first_child])
    out["counts"] = np.array([len(c) for c in levels], np.int32)
    # kernel maps: entry k of row r = row of coordinate(r) + offset_k * stride in the same level (batch included)
    jobs = [("k3_%d" % l, l, 3) for l in range(5)] + ([("k5", 0, 5)] if want_k5 else [])
    for l, c in enumerate(levels):
        out["coords%d" % l] = c.astype(np.int32)
    for name, l, ksize in jobs:
        offs = kernel_offsets(ksize, x_fastest) * (1 << l)
        c = levels[l]
        q = np.repeat(c, len(offs), axis=0)
        q[:, 1:] += np.tile(offs, (len(c), 1))
        out[name] = _lookup(c, q).reshape(len(c), len(offs))
    return out


ARRAYS = tuple(["counts", "n_unique", "unique_index", "inverse", "perm", "inv_perm", "ucoords", "k5"] +
               ["coords%d" % l for l in range(5)] + ["k3_%d" % l for l in range(5)] +
               ["%s%d" % (k, l) for k in ("parent_row", "child_k", "nbr_down", "up") for l in range(4)])


def contract(ref):
    """The arrays of the contract out of a reference() result (without nbits, plan, ...)."""
    return {k: ref[k] for k in ARRAYS if k in ref}


# ---- order-free form -------------------------------------------------------------------------------------------------------------
def _pk(c):
    """[n,4] coordinates -> one int64 per row (order-preserving per field)."""
    c = c.astype(np.int64)
    return (c[:, 0] << 48) | ((c[:, 1] + 32768) << 32) | ((c[:, 2] + 32768) << 16) | (c[:, 3] + 32768)


def canonical(a):
    """The same contract with every row REFERENCE replaced by the coordinate key of the row it names, and the rows of every
    level put in coordinate-key order: equal for any two Z-orders of the same lineage.  (The origin of the Z-order curve is an
    implementation choice: the hash pipeline interleaves x + 32768, pyramid.hip x - box minimum rounded to 16; both keep the
    children of a voxel contiguous, and convolution results do not depend on the row order.)"""
    out = {k: a[k] for k in ("counts", "n_unique", "unique_index", "inverse", "ucoords")}
    keys = [_pk(a["coords%d" % l]) for l in range(5)]
    order = [np.argsort(k, kind="stable") for k in keys]
    ref = lambda l, idx: np.where(idx >= 0, keys[l][np.maximum(idx, 0)], -1)           # row ids of level l -> coordinate keys
    assert np.array_equal(a["inv_perm"][a["perm"]], np.arange(len(a["perm"])))
    for l in range(5):
        out["coords%d" % l] = a["coords%d" % l][order[l]]
        out["k3_%d" % l] = ref(l, a["k3_%d" % l])[order[l]]
    if "k5" in a:
        out["k5"] = ref(0, a["k5"])[order[0]]
    for l in range(4):
        out["parent_row%d" % l] = ref(l + 1, a["parent_row%d" % l])[order[l]]
        out["child_k%d" % l] = a["child_k%d" % l][order[l]]
        out["nbr_down%d" % l] = ref(l, a["nbr_down%d" % l])[order[l + 1]]
        out["up%d" % l] = ref(l + 1, a["up%d" % l])[order[l]]
    return out


def _is_z_ordered(a):
    """Children of a voxel are contiguous at every level and parents are numbered in the order of their first child."""
    for l in range(4):
        p = a["parent_row%d" % l]
        if len(p) and not (p[0] == 0 and np.all(np.diff(p) >= 0) and np.all(np.diff(p) <= 1)):
            return False
    return True


# ---- reading a prepared arena back (GPU tier) ------------------------------------------------------------------------------------
def _prepare(coords, which, n_dev=None, want_k5=1, x_fastest=None, into=None):
    """One prepare call on device coordinates; into = (arena, layout) of an earlier call re-uses them as they are."""
    import torch
    from pbnet_amd import _native as N
    from pbnet_amd.MinkowskiEngine import conventions as CV
    lib = N.lib()
    n = int(coords.shape[0])
    xf = int(CV.X_FASTEST) if x_fastest is None else int(x_fastest)
    if into is None:
        P = N.PrepareLayout()
        nbytes = lib.pbn_coords_prepare_bytes(n, want_k5, ctypes.byref(P))
        arena = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    else:
        arena, P = into
        nbytes = arena.numel()
    fn = lib.pbn_coords_prepare_hash if which == "hash" else lib.pbn_coords_prepare_dev
    if which == "sorted" and n_dev is None:
        rc = lib.pbn_coords_prepare(N.ptr(coords), n, want_k5, xf, N.ptr(arena), nbytes, ctypes.byref(P), N.current_stream())
    else:
        rc = fn(N.ptr(coords), None if n_dev is None else N.ptr(n_dev), n, want_k5, xf, N.ptr(arena), nbytes,
                ctypes.byref(P), N.current_stream())
    N.check(rc, "prepare " + which)
    torch.cuda.synchronize()
    return arena, P


def _view(arena, off, count, dtype):
    import torch
    nb = count * torch.empty(0, dtype=dtype).element_size()
    return arena[off:off + nb].view(dtype).cpu().numpy()


def _arrays(arena, P, n, n_in=None):
    """Every output of the contract (include/pbnet_hip.h: pbn_prepare_layout), cut to its meaningful extent."""
    import torch
    L = P.pyramid
    counts = _view(arena, L.counts, 5, torch.int32)
    out = {"counts": counts.copy(), "n_unique": _view(arena, P.n_unique, 1, torch.int32).copy()}
    if counts[0] < 0:
        return out
    n1 = int(counts[0])
    out["unique_index"] = _view(arena, P.unique_index, n, torch.int64)[:n1]
    out["inverse"] = _view(arena, P.inverse, n, torch.int64)[:n if n_in is None else n_in]      # one entry per INPUT row
    out["perm"] = _view(arena, P.perm, n, torch.int64)[:n1]
    out["inv_perm"] = _view(arena, P.inv_perm, n, torch.int64)[:n1]
    out["ucoords"] = _view(arena, P.ucoords, n * 4, torch.int32).reshape(n, 4)[:n1]
    for l in range(5):
        nl = int(counts[l])
        out["coords%d" % l] = _view(arena, L.coords[l], n * 4, torch.int32).reshape(n, 4)[:nl]
        out["k3_%d" % l] = _view(arena, L.k3[l], n * 27, torch.int32).reshape(n, 27)[:nl]
    if L.k5 >= 0:                                                                                # -1: laid out without a k = 5 map
        out["k5"] = _view(arena, L.k5, n * 125, torch.int32).reshape(n, 125)[:n1]
    for l in range(4):
        nf, nc = int(counts[l]), int(counts[l + 1])
        out["parent_row%d" % l] = _view(arena, L.parent_row[l], n, torch.int32)[:nf]
        out["child_k%d" % l] = _view(arena, L.child_k[l], n, torch.int32)[:nf]
        out["nbr_down%d" % l] = _view(arena, L.nbr_down[l], n * 8, torch.int32).reshape(n, 8)[:nc]
        out["up%d" % l] = _view(arena, L.up[l], n * 8, torch.int32).reshape(n, 8)[:nf]
    return out
