"""Float64 numpy restatement of the reference's trainMerge / valMerge (datasets/scannetv2/dataset_preprocess.py:82-385) that
consumes a `pbnet_amd.loader.MergeDraws` instead of np.random.  The elastic blur and interpolation are restated in closed
form (scipy.ndimage.convolve / RegularGridInterpolator semantics, checked against scipy in tests/test_merge_cpu.py), so this
file needs numpy only.  `margins` collects the smallest distance of any point to a voxel or crop boundary (the golden
generator asserts it stays above 1e-9, so the fixtures do not hang on float64 summation order)."""
import itertools

import numpy as np

from pbnet_amd.loader import CROP_LEVELS, CROP_TRIES, ELASTIC, compose_matrix, elastic_shape

W3 = np.float64(np.float32(1) / np.float32(3))


def blur(n):
    """The six scipy.ndimage.convolve passes of `elastic` (blur0, blur1, blur2, blur0, blur1, blur2) on a float32 grid."""
    n = np.asarray(n, np.float32)
    for axis in (0, 1, 2, 0, 1, 2):
        p = np.pad(n.astype(np.float64), [(1, 1) if a == axis else (0, 0) for a in range(3)])
        sl = [lambda o, a=a: slice(o, o + n.shape[a]) if a == axis else slice(None) for a in range(3)]
        t = [p[tuple(s(o) for s in sl)] for o in range(3)]
        n = (((0.0 + t[0] * W3) + t[1] * W3) + t[2] * W3).astype(np.float32)
    return n


def axes(shape, gran):
    return [np.linspace(-(b - 1) * gran, (b - 1) * gran, b) for b in shape]


def interp(ax, values, x):
    """RegularGridInterpolator(ax, values, bounds_error=0, fill_value=0)(x), method 'linear'."""
    idx, nd = [], []
    oob = np.zeros(x.shape[0], bool)
    for d, a in enumerate(ax):
        xd = x[:, d]
        i = np.searchsorted(a, xd, side="right") - 1
        i = np.clip(i, 0, a.size - 2)
        idx.append(i)
        nd.append((xd - a[i]) / (a[i + 1] - a[i]))
        oob |= (xd < a[0]) | (xd > a[-1])
    value = np.zeros(x.shape[0])
    for h in itertools.product(*[((i, 1 - y), (i + 1, y)) for i, y in zip(idx, nd)]):
        e, w = zip(*h)
        weight = np.ones(x.shape[0])
        for wd in w:
            weight = weight * wd
        value = value + values[e].astype(np.float64) * weight
    value[oob] = 0.0
    return value


def elastic(x, gran, mag, noise):
    shape = elastic_shape(np.abs(x).max(0), gran)
    assert all(g.shape == shape for g in noise), (shape, [g.shape for g in noise])
    ax = axes(shape, gran)
    g = np.stack([interp(ax, blur(n), x) for n in noise], 1)
    return x + g * mag


def augment(xyz, rgb, a, i):
    m = compose_matrix(a, i)
    xyz = np.matmul(xyz, m)
    xyz = xyz - xyz.min(0)
    if a.scale is not None:
        xyz = xyz * a.scale
    if a.elastic:
        for p, (gran, mag) in enumerate(ELASTIC):
            xyz = elastic(xyz, gran, mag, a.noise[p])
        xyz = xyz - xyz.min(0)
    rgb = rgb + a.shift * 0.1
    return xyz, rgb


def relabel(ins):
    """getCroppedInstLabel / getInstLabel (the reference's loop, verbatim)."""
    j = 0
    while j < ins.max():
        if len(np.where(ins == j)[0]) == 0:
            ins[ins == ins.max()] = j
        j += 1
    return ins


def instance_info(xyz, ins):
    info = np.ones((xyz.shape[0], 9), np.float32) * -100.0
    num = int(ins.max()) + 1
    pointnum = []
    for i in range(num):
        w = np.where(ins == i)
        p = xyz[w]
        info[w[0], 0:3] = p.mean(0)
        info[w[0], 3:6] = p.min(0)
        info[w[0], 6:9] = p.max(0)
        pointnum.append(w[0].size)
    return num, info, pointnum


def _margin_vox(xyz, voxel):
    """Distance to the nearest voxel boundary; exact zeros (the minimum point after `xyz - xyz.min(0)`) are exact."""
    x = xyz[xyz != 0]
    f = x / voxel
    return float((np.abs(f - np.round(f)) * voxel).min()) if x.size else np.inf


class Margins:
    def __init__(self):
        self.voxel = np.inf
        self.crop = np.inf

    def crop_candidate(self, x, off, fs):
        """x = xyz + off against 0 (exact where off is 0: the minimum point is 0 itself) and against full_scale."""
        if x.size:
            self.crop = min(self.crop, float(np.abs(x - fs).min()))
            for d in range(3):
                if off[d] != 0:
                    self.crop = min(self.crop, float(np.abs(x[:, d]).min()))


def crop_loop(xyz, draws, cfg, margins=None):
    """The max_tries loop around crop(): -> (xyz, mask, triples used, a try succeeded)."""
    n = xyz.shape[0]
    if n <= cfg.max_crop_p:
        return xyz, np.ones(n, bool), 0, n >= cfg.min_crop_p
    trip = draws.crop
    used = 0
    room = xyz.max(0) - xyz.min(0)
    valid = None
    for _ in range(CROP_TRIES):
        fs = np.array([512 * cfg.scale_size / 50.0] * 3)
        valid = np.ones(n, bool)
        it = 0
        while valid.sum() > cfg.max_crop_p:
            assert it < CROP_LEVELS, "a try did not stop within 17 shrink levels"
            off = np.clip(fs - room + 0.001, None, 0) * trip[used]
            used += 1
            xo = xyz + off
            if margins is not None:
                margins.crop_candidate(xo, off, fs)
            valid = (xo.min(1) >= 0) * ((xo < fs).sum(1) == 3)
            fs[:2] -= 32 * cfg.scale_size / 50.0
            it += 1
        if valid.sum() >= cfg.min_crop_p:
            return xo, valid, used, True
    return xyz, valid, used, False


def _collate(parts, voxel, margins):
    from pbnet_amd.synth import voxelize_numpy
    out = {k: [] for k in ("xyz_voxel", "feat_voxel", "xyz_original", "sem", "ins", "inst_info", "v2p_index")}
    pointnum = []
    tot_inst, tot_vox = 0, 0
    for b, (xyz, feats, sem, ins) in enumerate(parts):
        if margins is not None:
            margins.voxel = min(margins.voxel, _margin_vox(xyz, voxel))
        q, first, inv = voxelize_numpy(xyz, voxel)
        num, info, pn = instance_info(xyz, ins.astype(np.int32))
        ins = ins.copy()
        ins[np.where(ins != -100)] += tot_inst
        tot_inst += num
        out["xyz_voxel"].append(np.concatenate([np.full((len(q), 1), b, np.int32), q.astype(np.int32)], 1))
        out["feat_voxel"].append(feats[first])
        out["v2p_index"].append(inv + tot_vox)
        tot_vox += len(q)
        out["xyz_original"].append(xyz)
        out["sem"].append(sem)
        out["ins"].append(ins.astype(np.float32))
        out["inst_info"].append(info)
        pointnum.extend(pn)
    res = dict(xyz_voxel=np.concatenate(out["xyz_voxel"]).astype(np.int32),
               feat_voxel=np.concatenate(out["feat_voxel"]).astype(np.float32),
               xyz_original=np.concatenate(out["xyz_original"]).astype(np.float32),
               sem=np.concatenate(out["sem"]).astype(np.int64), ins=np.concatenate(out["ins"]).astype(np.int64),
               inst_info=np.concatenate(out["inst_info"]).astype(np.float32),
               instance_pointnum=np.asarray(pointnum, np.int32),
               v2p_index=np.concatenate(out["v2p_index"]).astype(np.int64))
    return res


def train_merge(scenes, train_list, ids, draws, cfg, mixup=True, margins=None):
    """scenes: name -> dict(xyz, rgb, sem_label, ins_label, nl) numpy.  Returns the batch dict as numpy arrays + 'fn' +
    'crop_used' (triples consumed per scene)."""
    parts, fn, used, ok = [], [], [], []
    for i, idx in enumerate(ids):
        s = draws.scenes[i]
        sc = scenes[train_list[idx]]
        fn.append(train_list[idx])
        xyz = sc["xyz"].copy()
        xyz = xyz - xyz.min(0)
        xyz, rgb = augment(xyz, sc["rgb"], s.primary, i)
        nl, sem, ins = sc["nl"], sc["sem_label"], sc["ins_label"].copy()
        if mixup:
            mix_id = np.floor(s.mix_u * len(train_list)).astype(np.int64)
            mx = scenes[train_list[mix_id]]
            mxyz, mrgb = augment(mx["xyz"].copy(), mx["rgb"], s.partner, i)
            mins = mx["ins_label"].copy()
            xyz = np.concatenate((xyz, mxyz), 0)
            rgb = np.concatenate((rgb, mrgb), 0)
            sem = np.concatenate((sem, mx["sem_label"]), 0)
            nl = np.concatenate((nl, mx["nl"]), 0)
            ins_num_a = ins.max() + 1
            mins[np.where(mins != -100)] += ins_num_a
            ins = np.concatenate((ins, mins), 0)
        xyz, valid, u, success = crop_loop(xyz, s, cfg, margins)
        used.append(u)
        ok.append(success)
        xyz = xyz - xyz.min(0)
        xyz, rgb, sem, nl = xyz[valid], rgb[valid], sem[valid], nl[valid]
        ins = relabel(ins[valid])
        parts.append((xyz, np.concatenate((rgb, nl), 1).astype(np.float32), sem, ins))
    res = _collate(parts, cfg.voxel_size, margins)
    res["fn"] = fn
    res["crop_used"] = np.asarray(used, np.int32)
    res["crop_success"] = np.asarray(ok, bool)
    return res


def val_merge(scenes, val_list, ids, draws, cfg, margins=None):
    ids = list(ids) + list(ids) + list(ids)
    parts, fn = [], []
    for i, idx in enumerate(ids):
        sc = scenes[val_list[idx]]
        fn.append(val_list[idx])
        xyz, rgb = augment(sc["xyz"].copy(), sc["rgb"], draws.copies[i], i)
        ins = relabel(sc["ins_label"].copy())
        parts.append((xyz, np.concatenate((rgb, sc["nl"]), 1).astype(np.float32), sc["sem_label"], ins))
    res = _collate(parts, cfg.voxel_size, margins)
    res["fn"] = fn
    res["sup"] = scenes[val_list[ids[-1]]]["sup"]
    return res


OUT_KEYS = ("xyz_voxel", "feat_voxel", "xyz_original", "sem", "ins", "inst_info", "instance_pointnum", "v2p_index")


def load_golden(path):
    """tests/golden/merge_*.npz -> (kind, scenes, names, ids, draws, cfg, expected outputs)."""
    from types import SimpleNamespace
    from pbnet_amd.loader import MergeDraws
    g = np.load(path)
    kind = str(g["kind"])
    names = [str(n) for n in g["names"]]
    scenes = {}
    for j, n in enumerate(names):
        scenes[n] = {k: g["scene%d_%s" % (j, k)] for k in ("xyz", "rgb", "sem_label", "ins_label", "nl", "sup")}
    ids = [int(i) for i in g["ids"]]
    draws = MergeDraws.replay(kind, g["draw_kind"], g["draw_shape"], g["draw_val"], len(ids))
    cfg = SimpleNamespace(voxel_size=float(g["voxel_size"]), scale_size=int(g["scale_size"]),
                          max_crop_p=int(g["max_crop_p"]), min_crop_p=int(g["min_crop_p"]))
    want = {k: g["out_" + k] for k in OUT_KEYS}
    if kind == "val":
        want["sup"] = g["out_sup"]
    else:
        want["crop_used"] = g["crop_used"]
    return kind, scenes, names, ids, draws, cfg, want


def assert_batch(got, want, where=""):
    """Integers and feat_voxel exact; xyz_original and inst_info within one float32 ulp."""
    for k in OUT_KEYS:
        a, b = np.asarray(got[k]), np.asarray(want[k])
        assert a.shape == b.shape, (where, k, a.shape, b.shape)
        assert a.dtype == b.dtype, (where, k, a.dtype, b.dtype)
        if k in ("xyz_original", "inst_info"):
            ulp = np.spacing(np.maximum(np.abs(a), np.abs(b)).astype(np.float32))
            bad = np.abs(a.astype(np.float64) - b.astype(np.float64)) > ulp
            assert not bad.any(), (where, k, int(bad.sum()), np.argwhere(bad)[:5].tolist())
        else:
            assert np.array_equal(a, b), (where, k, int((a != b).sum()))


def synth_scenes(seeds, pitch=0.0225, val=False):
    """Raw ScanNet-like scenes from pbnet_amd.synth.synth_room (configs[1] size at the default pitch): float32 xyz off the
    origin, instance labels with holes, a superpoint id per point."""
    from pbnet_amd.synth import synth_room
    out = {}
    for s in seeds:
        sc = synth_room(seed=s, pitch=pitch)
        rng = np.random.default_rng(1000 + s)
        ins = sc["ins"].copy()
        ins[ins >= 0] = ins[ins >= 0] * 2 + 1
        out["scene%04d_00" % s] = dict(xyz=(sc["xyz"] + rng.uniform(-3, 3, 3)).astype(np.float32), rgb=sc["rgb"],
                                       sem_label=sc["sem"], ins_label=ins, nl=sc["normal"],
                                       sup=(np.floor(sc["xyz"] / 0.25).astype(np.int64) @ np.array([1, 64, 4096])))
    return out


def to_numpy(batch):
    return {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in batch.items()}
