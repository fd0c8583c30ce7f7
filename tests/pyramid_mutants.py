"""A second statement of the coordinate pyramid, written the way csrc/pyramid.hip works (shifts and masks, "first row of its
voxel" by comparison with the previous sorted row, level numbering by a running count, top maps by search in shifted Z-order keys,
maps of levels 1 and 0 derived top-down from the parent level) with one switch per deliberate mistake.  With mutant=None it must
equal tests/pyramid_ref.reference exactly on every designed case (tests/test_pyramid_cases_cpu.py); a mutant that equals the
specification on every case shows that the case set is too weak."""
import numpy as np

import pyramid_ref as PR

MUTANTS = ("trunc_div", "flag_ignores_batch", "lookup_ignores_batch", "child_k_reversed", "offsets_flipped", "derive_div2",
           "last_occurrence", "raw_origin", "absent_child_zero", "no_box_limit", "parents_by_coord_key", "plan_drops_top_digit",
           "level_key_drops_batch")


def _spread3(v):
    x = v.astype(np.uint64) & np.uint64(0xffff)
    for s, m in ((32, 0x00ff00000000ffff), (16, 0x00ff0000ff0000ff), (8, 0xf00f00f00f00f00f), (4, 0x30c30c30c30c30c3),
                 (2, 0x9249249249249249)):
        x = (x | (x << np.uint64(s))) & np.uint64(m)
    return x


def _zkey(b, xyz, e):
    return (b.astype(np.uint64) << np.uint64(3 * e)) | _spread3(xyz[:, 0]) | (_spread3(xyz[:, 1]) << np.uint64(1)) | \
        (_spread3(xyz[:, 2]) << np.uint64(2))


def _offset(k, ksize, x_fastest):
    c0 = ksize // 2 if ksize & 1 else 0
    a, b, c = k % ksize - c0, (k // ksize) % ksize - c0, k // (ksize * ksize) - c0
    return (a, b, c) if x_fastest else (c, b, a)


def reference(coords, n_valid=None, x_fastest=1, want_k5=1, mutant=None):
    assert mutant is None or mutant in MUTANTS
    coords = np.asarray(coords, np.int64).reshape(-1, 4)
    c_in = coords if n_valid is None else coords[:n_valid]
    n = len(c_in)
    if n == 0:
        return PR.contract(PR.reference(c_in, None, x_fastest, want_k5))            # nothing to get wrong
    # 1. de-duplication: rows grouped by a stable sort of the packed coordinate; the group's first (smallest) input row survives
    pk = PR.pack_key(c_in)
    order = np.argsort(pk, kind="stable")
    start = np.ones(n, bool)
    start[1:] = pk[order][1:] != pk[order][:-1]
    group = np.cumsum(start) - 1
    if mutant == "last_occurrence":
        end = np.ones(n, bool)
        end[:-1] = start[1:]
        winner = order[end]
    else:
        winner = order[start]
    uidx = np.sort(winner)
    newid = np.empty(len(winner), np.int64)
    newid[np.argsort(winner, kind="stable")] = np.arange(len(winner))
    inverse = np.empty(n, np.int64)
    inverse[order] = newid[group]
    uc = c_in[uidx]
    n1 = len(uc)
    # 2. keys and sort
    b0 = uc[:, 0].min()
    mins, maxs = uc[:, 1:].min(0), uc[:, 1:].max(0)
    origin = mins if mutant == "raw_origin" else mins & ~15
    ext = int((maxs - origin).max())
    e = ext.bit_length() if ext > 0 else 1
    nbits = 3 * e + int(uc[:, 0].max() - b0).bit_length()
    keys = _zkey(uc[:, 0] - b0, uc[:, 1:] - origin, e)
    skey = keys
    if mutant == "plan_drops_top_digit" and nbits <= PR.MAX_KEY_BITS:
        dbits = PR.sort_plan(nbits)[1]
        skey = keys & np.uint64((1 << ((nbits // dbits) * dbits)) - 1)               # the digits that fit BELOW nbits
    perm = np.argsort(skey, kind="stable")                                            # a stable LSD sort of those digits
    inv_perm = np.empty(n1, np.int64)
    inv_perm[perm] = np.arange(n1)
    key_s, c0 = keys[perm], uc[perm]
    out = dict(n_unique=np.array([n1], np.int32), unique_index=uidx, inverse=inverse, perm=perm, inv_perm=inv_perm,
               ucoords=uc.astype(np.int32), coords0=c0.astype(np.int32))
    # 3. levels from the sorted rows
    down = (lambda v, l: (np.abs(v) >> l) * np.sign(v)) if mutant == "trunc_div" else (lambda v, l: v >> l)
    prev = np.roll(c0, 1, axis=0)
    ids, firsts = [np.arange(n1)], [np.ones(n1, bool)]
    for l in range(1, 5):
        f = (down(c0[:, 1:], l) != down(prev[:, 1:], l)).any(1)
        if mutant != "flag_ignores_batch":
            f |= c0[:, 0] != prev[:, 0]
        f[0] = True
        firsts.append(f)
        ids.append(np.cumsum(f) - 1)
    # key of a level-l voxel: the row's key without the 3 * l lowest bits -- of its SPATIAL part only: a box narrower than 2^l holds
    # one level-l voxel per batch (the origin is a multiple of 16), and the batch bits stay
    kshift = (lambda l: 3 * l) if mutant == "level_key_drops_batch" else (lambda l: 3 * min(l, e))
    lcoords, lkeys = [c0], [key_s]
    for l in range(1, 5):
        c = c0[firsts[l]].copy()
        c[:, 1:] = down(c[:, 1:], l) << l
        lcoords.append(c)
        lkeys.append(key_s[firsts[l]] >> np.uint64(kshift(l)))
    if mutant == "parents_by_coord_key":
        for l in range(1, 5):
            rank = np.empty(len(lcoords[l]), np.int64)
            o = np.argsort(PR.pack_key(np.clip(lcoords[l], [0, PR.LO, PR.LO, PR.LO], None)), kind="stable")
            rank[o] = np.arange(len(o))
            ids[l] = rank[ids[l]]
            lcoords[l], lkeys[l] = lcoords[l][o], lkeys[l][o]
    out["counts"] = np.array([len(c) for c in lcoords], np.int32)
    nbr_down = []
    for l in range(1, 5):
        rows = ids[l - 1][firsts[l - 1]]                                   # the rows of level l - 1, through their first sorted row
        par = ids[l][firsts[l - 1]]
        cc = c0[firsts[l - 1]][:, 1:]
        bit = (cc >> (l - 1)) & 1
        ck = bit[:, 2] + 2 * bit[:, 1] + 4 * bit[:, 0] if mutant == "child_k_reversed" else bit[:, 0] + 2 * bit[:, 1] + 4 * bit[:, 2]
        nfine, ncoarse = len(lcoords[l - 1]), len(lcoords[l])
        parent_row, child_k = np.zeros(nfine, np.int32), np.zeros(nfine, np.int32)
        parent_row[rows], child_k[rows] = par, ck
        nd = np.full((ncoarse, 8), 0 if mutant == "absent_child_zero" else -1, np.int32)
        nd[par, ck] = rows
        up = np.full((nfine, 8), -1, np.int32)
        up[rows, ck] = par
        out["coords%d" % l] = lcoords[l].astype(np.int32)
        out.update({"parent_row%d" % (l - 1): parent_row, "child_k%d" % (l - 1): child_k, "nbr_down%d" % (l - 1): nd,
                    "up%d" % (l - 1): up})
        nbr_down.append(nd)
    # 4. maps.  levels 2..4: search for the shifted key of coordinate + offset among the level's keys
    xf = (not x_fastest) if mutant == "offsets_flipped" else bool(x_fastest)
    lim = 1 << e
    for l in (2, 3, 4):
        c, lk = lcoords[l], lkeys[l]
        srt = np.argsort(lk, kind="stable")
        nbr = np.full((len(c), 27), -1, np.int32)
        for k in range(27):
            d = np.array(_offset(k, 3, xf), np.int64)
            t = c[:, 1:] + (d << l) - origin
            if mutant == "no_box_limit":
                ok = np.ones(len(c), bool)
                t = t & (lim - 1)
            else:
                ok = ((t >= 0) & (t < lim)).all(1)
                t = np.where(ok[:, None], t, 0)
            want = _zkey(c[:, 0] - b0, t, e) >> np.uint64(kshift(l))
            have = lk[srt]
            if mutant == "lookup_ignores_batch":
                m = np.uint64((1 << max(3 * e - 3 * l, 0)) - 1)
                want = want & m
                srt_k = np.argsort(lk & m, kind="stable")
                have, src = (lk & m)[srt_k], srt_k
            else:
                src = srt
            pos = np.minimum(np.searchsorted(have, want), len(have) - 1)
            nbr[:, k] = np.where(ok & (have[pos] == want), src[pos], -1)
        out["k3_%d" % l] = nbr
    # levels 1 and 0 from the parent level: the neighbour at offset d of a voxel with parity p is child (p + d) & 1 of the parent's
    # neighbour at (p + d) >> 1
    half = (lambda t: np.trunc(t / 2).astype(np.int64)) if mutant == "derive_div2" else (lambda t: t >> 1)
    for l in (1, 0):
        k3_up, nd = out["k3_%d" % (l + 1)], nbr_down[l]
        par, ck = out["parent_row%d" % l].astype(np.int64), out["child_k%d" % l].astype(np.int64)
        p3 = np.stack([ck & 1, (ck >> 1) & 1, (ck >> 2) & 1], 1)
        for name, ksize in (("k3_%d" % l, 3),) + ((("k5", 5),) if l == 0 and want_k5 else ()):
            nbr = np.full((len(par), ksize ** 3), -1, np.int32)
            for k in range(ksize ** 3):
                t = p3 + np.array(_offset(k, ksize, xf), np.int64)
                h = half(t)
                kp3 = (h[:, 0] + 1) + 3 * (h[:, 1] + 1) + 9 * (h[:, 2] + 1) if xf else (h[:, 2] + 1) + 3 * (h[:, 1] + 1) + 9 * (h[:, 0] + 1)
                q = k3_up[par, kp3]
                child = (t[:, 0] & 1) + 2 * (t[:, 1] & 1) + 4 * (t[:, 2] & 1)
                nbr[:, k] = np.where(q >= 0, nd[np.maximum(q, 0), child], -1)
            out[name] = nbr
    return out
