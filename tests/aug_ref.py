"""Host restatement of csrc/augment.hip, one function per entry point (pbn_aug_affine, _elastic, _sub_min, _crop, _compact,
_instances, _quantize): plain numpy float64, every expression in the reference's order, no BLAS call (a fused multiply-add
in a matrix product would change last bits).  The box blur, the grid interpolation and the relabel loop are
tests/merge_ref.py's (its crop loop and instance statistics are the cross-check in tests/test_aug_cases_cpu.py); this
file states what each ENTRY returns, intermediates included, so tests/test_aug_entry_gpu.py can compare the float64 outputs bit for bit.  `merge` composes the entries in the order of
pbnet_amd.loader.DeviceMerge._merge; tests/test_aug_cases_cpu.py holds it against merge_ref.train_merge / val_merge on the
golden batches.

An extent (`ext`) row is (min xyz, max xyz); for a segment without rows it is NaN here and unspecified on the device."""
import math

import numpy as np

from merge_ref import axes, blur, interp, relabel

ROWS_PER_THREAD = 8
ROWS_PER_WAVE = 64 * ROWS_PER_THREAD
CHUNK = 256 * ROWS_PER_THREAD
SCAN_TILE = 256
CROP_TRIES, CROP_LEVELS = 5, 17
CROP_TRIPLES = CROP_TRIES * CROP_LEVELS
NO_INST = -100
ST_DONE, ST_NEXT, ST_USED, ST_LAST_START, ST_LAST_K, ST_SUCCESS, ST_ERROR, ST_TRIES = range(8)
ST_UNSPECIFIED_ON_ERROR = (ST_USED, ST_LAST_START, ST_LAST_K)     # a scene that ran out of triples: see `crop`


def extent(x):
    return np.concatenate([x.min(0), x.max(0)]) if x.shape[0] else np.full(6, np.nan)


def segment_of_rows(off):
    """Row -> segment, by filling each range (empty segments own no row)."""
    off = np.asarray(off, np.int64)
    seg = np.zeros(int(off[-1]), np.int64)
    for u in range(off.size - 1):
        seg[off[u]:off[u + 1]] = u
    return seg


# ---- pbn_aug_affine -----------------------------------------------------------------------------------------------------------
def pre_subtract(x32):
    """trainMerge's `xyz - xyz.min(0)` on the float32 array: subtracted in float32, widened afterwards."""
    y = x32 - x32.min(0)
    assert y.dtype == np.float32
    return y.astype(np.float64)


def affine(xyz32, uoff, pre_min, mats, scale, has_scale):
    """-> out f64[n,3], ext f64[U,6].  The float32 minimum is subtracted in float32 before widening; the product is
    elementwise, left to right."""
    xyz32 = np.asarray(xyz32)
    assert xyz32.dtype == np.float32
    U = len(uoff) - 1
    out = np.zeros((xyz32.shape[0], 3))
    ext = np.full((U, 6), np.nan)
    for u in range(U):
        x = xyz32[uoff[u]:uoff[u + 1]]
        if not x.shape[0]:
            continue
        x = pre_subtract(x) if pre_min[u] else x.astype(np.float64)
        m = np.asarray(mats[u], np.float64).reshape(3, 3)
        y = np.stack([x[:, 0] * m[0, j] + x[:, 1] * m[1, j] + x[:, 2] * m[2, j] for j in range(3)], 1)
        y = y - y.min(0)
        if has_scale[u]:
            y = y * np.float64(scale[u])
        out[uoff[u]:uoff[u + 1]] = y
        ext[u] = extent(y)
    return out, ext


# ---- pbn_aug_elastic / pbn_aug_sub_min ----------------------------------------------------------------------------------------
def elastic_pass(xyz, uoff, desc, noise, gran, mag):
    """One pass.  desc: [(unit, (b0, b1, b2))], noise: per descriptor its 3 float32 grids.  -> xyz (rows of other units
    unchanged), ext f64[U,6] (NaN = a unit the pass does not touch: unspecified on the device)."""
    out = np.array(xyz, np.float64)
    ext = np.full((len(uoff) - 1, 6), np.nan)
    for (u, shape), grids in zip(desc, noise):
        x = out[uoff[u]:uoff[u + 1]]
        assert all(g.shape == tuple(shape) and g.dtype == np.float32 for g in grids)
        ax = axes(shape, gran)
        g = np.stack([interp(ax, blur(n), x) for n in grids], 1)
        y = x + g * mag
        out[uoff[u]:uoff[u + 1]] = y
        ext[u] = extent(y)
    return out, ext


def sub_min(xyz, uoff, flags, ext):
    out = np.array(xyz, np.float64)
    for u in range(len(uoff) - 1):
        if flags[u]:
            out[uoff[u]:uoff[u + 1]] = out[uoff[u]:uoff[u + 1]] - ext[u, :3]
    return out


# ---- pbn_aug_crop -------------------------------------------------------------------------------------------------------------
def crop_offset(ext, level, t):
    room = ext[3:] - ext[:3]
    return np.clip(level - room + 0.001, None, 0) * t


def crop_valid(x, o, level):
    xo = x + o
    return (xo.min(1) >= 0) * ((xo < level).sum(1) == 3)


def offset_extent(xo, valid):
    """Extent of the offset scene over ALL its rows: the reference takes `xyz.min(0)` before the mask selects rows."""
    return extent(xo)


def crop(xyz, soff, mode, triples, n_triples, levels, max_crop_p, min_crop_p):
    """-> dict(counts i32[5,B,17] with -1 where a try does not go, state i32[B,8], ext_pre, ext_post f64[B,6]).
    A level k of try t consumes triple (first triple of the try) + k.  When that triple does not exist the scene ends with
    ST_ERROR 2; what the device leaves in ST_UNSPECIFIED_ON_ERROR then depends on rows of `triples` nobody supplied.
    ST_ERROR 1 (17 levels without reaching max_crop_p) cannot happen with max_crop_p >= 0: levels[16][0] is 0, so level 16
    admits no point and its count 0 ends the try."""
    B = len(mode)
    counts = np.full((CROP_TRIES, B, CROP_LEVELS), -1, np.int32)
    state = np.zeros((B, 8), np.int32)
    ext_pre = np.full((B, 6), np.nan)
    ext_post = np.full((B, 6), np.nan)
    for s in range(B):
        x = xyz[soff[s]:soff[s + 1]]
        ext_pre[s] = ext_post[s] = extent(x)
        if mode[s] != 0:
            continue
        st = state[s]
        for t in range(CROP_TRIES):
            start, k = int(st[ST_NEXT]), 0
            while True:
                assert k < CROP_LEVELS, "a try did not stop within 17 shrink levels"
                if start + k >= n_triples[s]:
                    st[ST_ERROR] = 2
                    break
                o = crop_offset(ext_pre[s], levels[k], triples[s, start + k])
                valid = crop_valid(x, o, levels[k])
                c = int(valid.sum())
                counts[t, s, k] = c
                if c <= max_crop_p:
                    break
                k += 1
            if st[ST_ERROR]:
                break
            st[ST_LAST_START], st[ST_LAST_K], st[ST_USED], st[ST_TRIES] = start, k, start + k + 1, t + 1
            if c >= min_crop_p:
                st[ST_SUCCESS] = 1
                ext_post[s] = offset_extent(x + o, valid.astype(bool))
                break
            st[ST_NEXT] = start + k + 1
        st[ST_DONE] = 1
    return dict(counts=counts, state=state, ext_pre=ext_pre, ext_post=ext_post)


def crop_view(s, mode, triples, levels, state, ext_pre):
    """What the compaction derives from a scene's state: (keep all, offset or None, level of the mask, apply the offset)."""
    if mode[s] != 0:
        return True, None, None, False
    k = int(state[s, ST_LAST_K])
    q = int(state[s, ST_LAST_START]) + k
    return False, crop_offset(ext_pre[s], levels[k], triples[s, q]), levels[k], bool(state[s, ST_SUCCESS])


# ---- pbn_aug_compact ----------------------------------------------------------------------------------------------------------
def shift_labels(ins, shift_of_row):
    """The partner's `mins[np.where(mins != -100)] += ins_num_a`: -100 stays."""
    out = np.asarray(ins, np.int32).copy()
    move = out != NO_INST
    out[move] += np.asarray(shift_of_row, np.int32)[move]
    return out


def compact(xyz, rgb, nl, sem, ins, shift, ins_shift, uoff, soff, mode, triples, levels, state, ext_pre, ext_post):
    """-> dict(mask, xyz f64[K,3], feat f32[K,6], sem i64[K], label i32[K], scene_info i32[B,4], scan i32[chunks+1]).
    Kept rows in input order.  An empty scene has instance_num 0; a scene whose kept labels are all -100 has -99."""
    n, B = xyz.shape[0], len(mode)
    unit = segment_of_rows(uoff)
    assert unit.size == n and int(soff[-1]) == n
    mask = np.zeros(n, bool)
    shifted = shift_labels(ins, np.asarray(ins_shift, np.int32)[unit])
    feat_all = np.concatenate([(np.asarray(rgb, np.float32).astype(np.float64) + np.asarray(shift, np.float64)[unit])
                               .astype(np.float32), np.asarray(nl, np.float32)], 1) if n else np.zeros((0, 6), np.float32)
    parts, labels = [], []
    info = np.zeros((B, 4), np.int32)
    first = 0
    for s in range(B):
        a, b = int(soff[s]), int(soff[s + 1])
        x = xyz[a:b]
        keep_all, o, level, offset = crop_view(s, mode, triples, levels, state, ext_pre)
        m = np.ones(b - a, bool) if keep_all else crop_valid(x, o, level).astype(bool)
        if offset:
            x = x + o
        mask[a:b] = m
        if b > a:
            x = x - ext_post[s, :3]              # the minimum over ALL rows of the scene, taken before the mask selects
        parts.append(x[m])
        lab = shifted[a:b][m].copy()
        inst = 0
        if lab.size:
            lab = relabel(lab)
            inst = int(lab.max()) + 1
        labels.append(lab)
        info[s] = (lab.size, inst, first, 0)
        first += lab.size
    n_chunks = max(1, -(-n // CHUNK))
    per_chunk = np.array([mask[c * CHUNK:(c + 1) * CHUNK].sum() for c in range(n_chunks)], np.int64)
    scan = np.concatenate([[0], np.cumsum(per_chunk)]).astype(np.int32)
    return dict(mask=mask, xyz=np.concatenate(parts) if parts else np.zeros((0, 3)), feat=feat_all[mask],
                sem=np.asarray(sem, np.int64)[mask], label=np.concatenate(labels).astype(np.int32), scene_info=info,
                scan=scan)


# ---- pbn_aug_instances --------------------------------------------------------------------------------------------------------
def instance_tables(inst_num):
    """(inst_start i32[B+1], inst_off i64[B]) as the loader derives them: a scene of instance_num -99 owns no instance
    but lowers the running offset of the scenes after it."""
    inst_num = np.asarray(inst_num, np.int64)
    start = np.concatenate([[0], np.cumsum(np.maximum(inst_num, 0))]).astype(np.int32)
    off = np.concatenate([[0], np.cumsum(inst_num)[:-1]]).astype(np.int64)
    return start, off


def instances(xyz, label, ostart, inst_num):
    """-> dict(pointnum i32[I], stats f32[I,9] = (mean, min, max), inst_info f32[n,9], ins i64[n]).  The mean is the
    correctly rounded float32(fsum / n); the device sums in a fixed tree, so its mean may sit one float32 ulp away."""
    start, off = instance_tables(inst_num)
    n = int(ostart[-1])
    pointnum = np.zeros(int(start[-1]), np.int32)
    stats = np.zeros((int(start[-1]), 9), np.float32)
    info = np.full((n, 9), -100.0, np.float32)
    ins = np.full(n, NO_INST, np.int64)
    for s in range(len(inst_num)):
        a, b = int(ostart[s]), int(ostart[s + 1])
        lab = np.asarray(label[a:b], np.int64)
        x = xyz[a:b]
        for i in range(max(int(inst_num[s]), 0)):
            w = np.nonzero(lab == i)[0]
            assert w.size, "instance without points"
            p = x[w]
            g = int(start[s]) + i
            pointnum[g] = w.size
            stats[g, 0:3] = [np.float32(math.fsum(p[:, d]) / w.size) for d in range(3)]
            stats[g, 3:6] = p.min(0)
            stats[g, 6:9] = p.max(0)
            info[a + w] = stats[g]
        ins[a:b] = np.where(lab != NO_INST, lab + off[s], NO_INST)
    return dict(pointnum=pointnum, stats=stats, inst_info=info, ins=ins, inst_start=start, inst_off=off)


# ---- pbn_aug_quantize ---------------------------------------------------------------------------------------------------------
def voxel_index(x, voxel):
    return np.floor(x / np.float64(voxel)).astype(np.int32)


def quantize(xyz, ostart, voxel):
    seg = segment_of_rows(ostart)
    q = voxel_index(np.asarray(xyz, np.float64), voxel).reshape(-1, 3)
    return np.concatenate([seg[:, None].astype(np.int32), q], 1), np.asarray(xyz, np.float64).astype(np.float32)


# ---- the loader's order -------------------------------------------------------------------------------------------------------
def merge(scenes, units, per_scene, cfg, crop_draws=None):
    """DeviceMerge._merge on the host.  units: [(scene name, AugDraws, enumerate index, pre-min in float32)];
    crop_draws: per scene the crop triples (None: valMerge, every point kept).  -> the batch dict as numpy arrays."""
    from pbnet_amd.loader import ELASTIC, compose_matrix, crop_levels, elastic_shape
    U = len(units)
    B = U // per_scene
    sizes = [scenes[u[0]]["xyz"].shape[0] for u in units]
    uoff = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    soff = uoff[::per_scene].copy()
    cat = lambda key: np.concatenate([np.asarray(scenes[u[0]][key]) for u in units], 0)
    mats = np.stack([compose_matrix(a, i) for _, a, i, _ in units]).reshape(U, 9)
    xyz, ext = affine(cat("xyz"), uoff, [u[3] for u in units], mats,
                      [a.scale if a.scale is not None else 1.0 for _, a, _, _ in units],
                      [a.scale is not None for _, a, _, _ in units])
    el = [u for u in range(U) if units[u][1].elastic]
    if el:
        for p, (gran, mag) in enumerate(ELASTIC):
            desc = [(u, elastic_shape(np.maximum(np.abs(ext[u, :3]), np.abs(ext[u, 3:])), gran)) for u in el]
            xyz, ext = elastic_pass(xyz, uoff, desc, [units[u][1].noise[p] for u in el], gran, mag)
        xyz = sub_min(xyz, uoff, [u in el for u in range(U)], ext)
    shifts = np.stack([a.shift * 0.1 for _, a, _, _ in units])
    mode = np.zeros(B, np.int32)
    trip = np.zeros((B, CROP_TRIPLES, 3))
    n_trip = np.zeros(B, np.int32)
    for s in range(B):
        if crop_draws is None or soff[s + 1] - soff[s] <= cfg.max_crop_p:
            mode[s] = 1
        else:
            trip[s, :crop_draws[s].shape[0]] = crop_draws[s]
            n_trip[s] = crop_draws[s].shape[0]
    levels = crop_levels(cfg)
    c = crop(xyz, soff, mode, trip, n_trip, levels, cfg.max_crop_p, cfg.min_crop_p)
    assert not c["state"][:, ST_ERROR].any()
    ins_shift = np.zeros(U, np.int32)
    for u in range(U):
        if u % per_scene == 1:
            prev = np.asarray(scenes[units[u - 1][0]]["ins_label"])
            ins_shift[u] = int(prev.max()) + 1
    k = compact(xyz, cat("rgb"), cat("nl"), cat("sem_label"), cat("ins_label"), shifts, ins_shift, uoff, soff, mode, trip,
                levels, c["state"], c["ext_pre"], c["ext_post"])
    info = k["scene_info"]
    ostart = np.concatenate([[0], np.cumsum(info[:, 0])]).astype(np.int32)
    inst = instances(k["xyz"], k["label"], ostart, info[:, 1])
    c4, xyz32 = quantize(k["xyz"], ostart, cfg.voxel_size)
    _, first, inverse = np.unique(c4, axis=0, return_index=True, return_inverse=True)
    order = np.argsort(first, kind="stable")
    rank = np.empty_like(order)
    rank[order] = np.arange(order.size)
    index = first[order]
    return dict(xyz_voxel=c4[index], feat_voxel=k["feat"][index], xyz_original=xyz32, sem=k["sem"], ins=inst["ins"],
                inst_info=inst["inst_info"], instance_pointnum=inst["pointnum"],
                v2p_index=rank[inverse.reshape(-1)].astype(np.int64), crop_used=c["state"][:, ST_USED].copy())
