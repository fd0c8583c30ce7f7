"""Device-side batch construction: the reference's `trainMerge` / `valMerge`
(datasets/scannetv2/dataset_preprocess.py:178-305, :308-385) from the scene arrays up to the batch dict that `model_fn` /
`model_fn_eval` consume, on the MI355X.

    cache = SceneCache({"scene0000_00": dict(xyz=..., rgb=..., sem_label=..., ins_label=..., nl=...), ...}, "cuda",
                       train=[...], val=[...])
    merge = DeviceMerge(cache, cfg, seed=rank_seed)
    batch = merge.train_merge([3, 17, 5, 9])          # or DataLoader(range(n), collate_fn=merge, num_workers=0)

Everything random that one merge consumes is a `MergeDraws`: drawn from a seeded torch.Generator, or rebuilt from a
recorded numpy stream (golden replay against the reference).  The 3x3 augmentation matrix is composed on the host in numpy
float64 exactly as `dataAugment` composes it; the device receives those bits.  The hot path is `csrc/augment.hip`:
affine + extent, elastic distortion (box blur of the noise grids, trilinear sampling), the crop loop (candidates of one try
per launch, the stopping iteration picked on the device), compaction, instance relabelling and instance statistics; the
voxelisation reuses `pbn_coords_unique`.  Host read-backs per merge: one per elastic pass (grid shapes), one for the
per-scene point / instance counts, one for the voxel count.
"""
import ctypes
import math

import numpy as np
import torch

from . import _native as N
from .MinkowskiEngine.core import CoordinateManager

CROP_TRIES = 5
CROP_LEVELS = 17                       # full_scale[:2] reaches 0 at the 17th shrink: a try ends within 17 iterations
ELASTIC = ((6, 40.0), (20, 160.0))     # (gran, mag) of the two elastic passes (dataAugment)
NO_INST = -100

_KIND = {"rand": 0, "randn": 1, "randint": 2, "uniform": 3}


# ---------------------------------------------------------------------------------------------------------------- draws
class AugDraws:
    """The draws of one dataAugment call, in the reference's order.  A gate is the `np.random.rand()` of
    `if flag and np.random.rand() < prob`; None = not drawn (flag False).  The value behind a gate is None when the gate
    did not pass."""
    __slots__ = ("jitter_gate", "jitter", "flip_gate", "flip", "rot_gate", "theta_u", "scale_gate", "scale",
                 "elastic_gate", "noise", "shift")

    def __init__(self):
        for s in self.__slots__:
            setattr(self, s, None)
        self.noise = [None, None]        # per elastic pass: 3 float32 grids (randn(...).astype(float32))

    @property
    def elastic(self):
        return self.elastic_gate is not None and self.elastic_gate < 1.0


class SceneDraws:
    __slots__ = ("primary", "mix_u", "partner", "crop")

    def __init__(self):
        self.primary, self.mix_u, self.partner, self.crop = AugDraws(), None, None, np.zeros((0, 3))


class MergeDraws:
    """Every random number one merge consumes.  `scenes[i]` for trainMerge, `copies[i]` (an AugDraws with only `shift`)
    for valMerge's 3B copies.  Crop triples: at most CROP_TRIES * CROP_LEVELS per scene, none when the merged scene has
    no more than max_crop_p points."""

    def __init__(self, kind):
        assert kind in ("train", "val")
        self.kind = kind
        self.scenes = []
        self.copies = []
        self._gen = None

    # -- seeded generator ------------------------------------------------------------------------------------------
    @classmethod
    def draw_train(cls, gen, n_ids, n_train, merged_sizes, max_crop_p, mixup=True):
        """`merged_sizes(i, mix_id)` -> number of points of scene i merged with its partner (decides whether the crop
        loop runs).  Noise grids are drawn later, once their shapes are known (`noise_for`)."""
        d = cls("train")
        d._gen = gen

        def u():
            return float(torch.rand((), dtype=torch.float64, generator=gen))

        def aug():
            a = AugDraws()
            a.jitter_gate = u()
            a.jitter = torch.randn(3, 3, dtype=torch.float64, generator=gen).numpy()
            a.flip_gate = u()
            a.flip = int(torch.randint(0, 2, (), generator=gen))
            a.rot_gate = u()
            a.theta_u = u()
            a.scale_gate = u()
            a.scale = 0.95 + (1.05 - 0.95) * u()
            a.elastic_gate = u()
            a.shift = torch.randn(3, dtype=torch.float64, generator=gen).numpy()
            return a
        for i in range(n_ids):
            s = SceneDraws()
            s.primary = aug()
            if mixup:
                s.mix_u = u()
                s.partner = aug()
            mix_id = int(np.floor(s.mix_u * n_train)) if mixup else None
            if merged_sizes(i, mix_id) > max_crop_p:
                s.crop = torch.rand(CROP_TRIES * CROP_LEVELS, 3, dtype=torch.float64, generator=gen).numpy()
            d.scenes.append(s)
        return d

    @classmethod
    def draw_val(cls, gen, n_ids):
        d = cls("val")
        for _ in range(3 * n_ids):
            a = AugDraws()
            a.shift = torch.randn(3, dtype=torch.float64, generator=gen).numpy()
            d.copies.append(a)
        return d

    def noise_for(self, a, p, shape):
        """The 3 float32 noise grids of elastic pass p of AugDraws `a`, drawn now when this MergeDraws comes from a
        generator; a replayed one must have recorded exactly this shape."""
        shape = tuple(int(b) for b in shape)
        if a.noise[p] is None:
            assert self._gen is not None, "replayed draws lack elastic noise"
            a.noise[p] = [torch.randn(shape, dtype=torch.float64, generator=self._gen).numpy().astype(np.float32)
                          for _ in range(3)]
        for g in a.noise[p]:
            assert g.shape == shape, "recorded noise grid %s, the scene needs %s" % (g.shape, shape)
        return a.noise[p]

    # -- recorded numpy stream -------------------------------------------------------------------------------------
    @staticmethod
    def record_arrays(records):
        """[(kind, value)] as np.random returned them -> flat arrays for an .npz."""
        kinds = np.array([_KIND[k] for k, _ in records], np.int32)
        shapes = np.zeros((len(records), 3), np.int32)
        vals = []
        for r, (_, v) in enumerate(records):
            v = np.asarray(v, np.float64)
            shapes[r, :v.ndim] = v.shape
            shapes[r, v.ndim:] = -1
            vals.append(v.reshape(-1))
        return dict(draw_kind=kinds, draw_shape=shapes, draw_val=np.concatenate(vals) if vals else np.zeros(0))

    @classmethod
    def replay(cls, kind, draw_kind, draw_shape, draw_val, n_ids, mixup=True, prob=1.0):
        """Rebuild from a recorded stream (record_arrays' layout) by walking the reference's draw order."""
        recs, pos = [], 0
        for k, sh in zip(draw_kind, draw_shape):
            shape = tuple(int(x) for x in sh if x >= 0)
            n = int(np.prod(shape)) if shape else 1
            v = draw_val[pos:pos + n]
            pos += n
            recs.append((int(k), v.reshape(shape) if shape else float(v[0])))
        it = [0]

        def take(kind_, scalar=True):
            k, v = recs[it[0]]
            assert k == _KIND[kind_], "draw %d: expected %s, recorded kind %d" % (it[0], kind_, k)
            it[0] += 1
            return v

        def peek_crop():
            return it[0] < len(recs) and recs[it[0]][0] == 0 and np.ndim(recs[it[0]][1]) == 1

        def aug(elastic_ok=True):
            a = AugDraws()
            a.jitter_gate = take("rand")
            if a.jitter_gate < prob:
                a.jitter = np.asarray(take("randn"))
            a.flip_gate = take("rand")
            if a.flip_gate < prob:
                a.flip = int(take("randint"))
            a.rot_gate = take("rand")
            if a.rot_gate < prob:
                a.theta_u = take("rand")
            a.scale_gate = take("rand")
            if a.scale_gate < prob:
                a.scale = take("uniform")
            a.elastic_gate = take("rand")
            if a.elastic_gate < prob:
                a.noise = [[np.asarray(take("randn")).astype(np.float32) for _ in range(3)] for _p in range(2)]
            a.shift = np.asarray(take("randn"))
            return a
        d = cls(kind)
        if kind == "train":
            for _ in range(n_ids):
                s = SceneDraws()
                s.primary = aug()
                if mixup:
                    s.mix_u = take("rand")
                    s.partner = aug()
                crop = []
                while peek_crop():
                    crop.append(take("rand"))
                s.crop = np.asarray(crop, np.float64).reshape(-1, 3)
                d.scenes.append(s)
        else:
            for _ in range(3 * n_ids):
                a = AugDraws()
                a.shift = np.asarray(take("randn"))
                d.copies.append(a)
        assert it[0] == len(recs), "%d recorded draws left over" % (len(recs) - it[0])
        return d


def compose_matrix(a, i):
    """dataAugment's 3x3 matrix (dataset_preprocess.py:85-99), the same numpy float64 operations in the same order."""
    m = np.eye(3)
    if a.jitter is not None:
        m += a.jitter * 0.1
    if a.flip is not None:
        m[0][0] *= a.flip * 2 - 1
    if a.theta_u is not None:
        theta = a.theta_u * 2 * math.pi
    else:
        theta = 0.35 * math.pi + math.pi * i * (2 / 3)
    m = np.matmul(m, [[math.cos(theta), math.sin(theta), 0],
                      [-math.sin(theta), math.cos(theta), 0], [0, 0, 1]])
    return m


def elastic_shape(absmax, gran):
    """`np.abs(x).max(0).astype(np.int32) // gran + 3` from the per-axis |x| maximum."""
    return tuple(int(v) for v in (np.asarray(absmax, np.float64).astype(np.int32) // gran + 3))


def crop_levels(cfg):
    """full_scale after 0..16 shrinks, by the reference's repeated float64 subtraction: f64[17,3]."""
    fs = np.array([512 * cfg.scale_size / 50.0] * 3)
    out = np.zeros((CROP_LEVELS, 3))
    for k in range(CROP_LEVELS):
        out[k] = fs
        fs[:2] -= 32 * cfg.scale_size / 50.0
    return out


# ---------------------------------------------------------------------------------------------------------------- cache
class SceneCache:
    """The reference's cfg.cache (SharedArray store): per scene xyz f32[N,3], rgb f32[N,3], sem_label, ins_label (-100 =
    none), nl f32[N,3] and, for validation scenes, sup -- resident on `device`.  Addressed by name; `train` / `val` are the
    ordered name lists (train_file_list / val_file_list)."""
    KEYS = ("xyz", "rgb", "sem_label", "ins_label", "nl")

    def __init__(self, scenes, device="cuda", train=None, val=None):
        self.device = torch.device(device)
        self.scenes = {}
        self.host = {}                     # per scene: n, max raw instance label (sizes the relabel tables)
        for name, s in scenes.items():
            t = {}
            for k in self.KEYS:
                v = np.asarray(s[k])
                t[k] = torch.from_numpy(np.ascontiguousarray(v)).to(self.device)
            assert t["xyz"].dtype == torch.float32 and t["rgb"].dtype == torch.float32 and t["nl"].dtype == torch.float32
            if "sup" in s and s["sup"] is not None:
                t["sup"] = torch.from_numpy(np.ascontiguousarray(np.asarray(s["sup"]))).to(self.device)
            ins = np.asarray(s["ins_label"])
            self.host[name] = dict(n=int(ins.shape[0]), ins_max=int(ins.max()) if ins.size else NO_INST,
                                   sem_dtype=np.asarray(s["sem_label"]).dtype)
            self.scenes[name] = t
        self.train = list(train) if train is not None else sorted(self.scenes)
        self.val = list(val) if val is not None else sorted(self.scenes)

    def __getitem__(self, name):
        return self.scenes[name]


# ---------------------------------------------------------------------------------------------------------------- merge
def _i32(x, dev):
    return torch.as_tensor(np.ascontiguousarray(np.asarray(x, np.int32)), device=dev)


def _f64(x, dev):
    return torch.as_tensor(np.ascontiguousarray(np.asarray(x, np.float64)), device=dev)


class DeviceMerge:
    """trainMerge / valMerge on the device.  `cfg` supplies voxel_size, scale_size, max_crop_p, min_crop_p
    (pbnet_amd/config.py).  Usable as a DataLoader collate_fn with num_workers=0 (the train merge)."""

    def __init__(self, cache, cfg, seed=None, mixup=True):
        self.cache = cache
        self.cfg = cfg
        self.mixup = mixup
        self.dev = cache.device
        self.gen = torch.Generator()
        self.gen.manual_seed(int(seed) if seed is not None else int(torch.initial_seed()))
        self.readbacks = 0                 # host read-backs of the last merge

    def __call__(self, ids):
        return self.train_merge(ids)

    # -- public ----------------------------------------------------------------------------------------------------
    def train_merge(self, ids, draws=None):
        ids = [int(i) for i in ids]
        names = self.cache.train
        if draws is None:
            def merged(i, mix_id):
                n = self.cache.host[names[ids[i]]]["n"]
                return n + (self.cache.host[names[mix_id]]["n"] if mix_id is not None else 0)
            draws = MergeDraws.draw_train(self.gen, len(ids), len(names), merged, self.cfg.max_crop_p, self.mixup)
        assert draws.kind == "train" and len(draws.scenes) == len(ids)
        units = []                          # (scene name, AugDraws, enumerate index, pre-min in float32)
        for i, idx in enumerate(ids):
            s = draws.scenes[i]
            units.append((names[idx], s.primary, i, True))
            if self.mixup:
                mix_id = int(np.floor(s.mix_u * len(names)))
                units.append((names[mix_id], s.partner, i, False))
        per_scene = 2 if self.mixup else 1
        return self._merge(units, per_scene, draws, [names[i] for i in ids], crop=True, sup=None)

    def val_merge(self, ids, draws=None):
        ids = [int(i) for i in ids]
        ids3 = ids + ids + ids
        names = self.cache.val
        if draws is None:
            draws = MergeDraws.draw_val(self.gen, len(ids))
        assert draws.kind == "val" and len(draws.copies) == len(ids3)
        units = [(names[idx], draws.copies[i], i, False) for i, idx in enumerate(ids3)]
        sup = self.cache[names[ids3[-1]]].get("sup")
        return self._merge(units, 1, draws, [names[i] for i in ids3], crop=False, sup=sup)

    # -- the pipeline ----------------------------------------------------------------------------------------------
    def _merge(self, units, per_scene, draws, fn, crop, sup):
        lib, dev, cfg = N.lib(), self.dev, self.cfg
        stream = N.current_stream()
        hold = []                       # small uploads stay referenced until the merge has enqueued its last launch: a

        def i32(x):                     # block freed early would be handed to the next upload before the launch reads it
            hold.append(_i32(x, dev))
            return hold[-1]

        def f64(x):
            hold.append(_f64(x, dev))
            return hold[-1]
        self.readbacks = 0
        U = len(units)
        B = U // per_scene
        sizes = [self.cache.host[u[0]]["n"] for u in units]
        uoff = np.zeros(U + 1, np.int64)
        uoff[1:] = np.cumsum(sizes)
        n_all = int(uoff[-1])
        assert n_all < 2 ** 31 - 1
        soff = uoff[::per_scene].copy()                   # scene s = units [s*per_scene, (s+1)*per_scene): contiguous rows
        cat = lambda key: torch.cat([self.cache[u[0]][key] for u in units], 0)
        xyz32, rgb32, nl32 = cat("xyz").contiguous(), cat("rgb").contiguous(), cat("nl").contiguous()
        sem_all = cat("sem_label").to(torch.int64).contiguous()
        ins_raw = cat("ins_label").to(torch.int32).contiguous()
        uoff_d, soff_d = _i32(uoff, dev), _i32(soff, dev)
        max_u = int(max(sizes)) if sizes else 0
        max_s = int((soff[1:] - soff[:-1]).max())
        ws = torch.empty(lib.pbn_aug_workspace_bytes(max(U, B)), dtype=torch.uint8, device=dev)

        # affine + extent (float32 pre-min for the primary training scene), then scale
        mats = np.stack([compose_matrix(a, i) for _, a, i, _ in units]).reshape(U, 9)
        pre_min = [1 if pm else 0 for _, _, _, pm in units]
        scale = [a.scale if a.scale is not None else 1.0 for _, a, _, _ in units]
        has_scale = [1 if a.scale is not None else 0 for _, a, _, _ in units]
        xyz = torch.empty(n_all, 3, dtype=torch.float64, device=dev)
        ext = torch.empty(U, 6, dtype=torch.float64, device=dev)
        N.check(lib.pbn_aug_affine(N.ptr(xyz32), N.ptr(uoff_d), U, max_u, N.ptr(i32(pre_min)),
                                   N.ptr(f64(mats)), N.ptr(f64(scale)), N.ptr(i32(has_scale)), N.ptr(xyz),
                                   N.ptr(ext), N.ptr(ws), stream), "pbn_aug_affine")
        el = [u for u in range(U) if units[u][1].elastic]
        if el:
            for p, (gran, mag) in enumerate(ELASTIC):
                e = ext.cpu().numpy()                       # one read-back per pass: the grid shapes
                self.readbacks += 1
                self._elastic(lib, units, el, e, p, gran, mag, xyz, uoff_d, max_u, ext, ws, draws, i32, stream)
            N.check(lib.pbn_aug_sub_min(N.ptr(xyz), N.ptr(uoff_d), U, max_u, N.ptr(i32([1 if units[u][1].elastic else 0
                                                                                   for u in range(U)])), N.ptr(ext),
                                        stream), "pbn_aug_sub_min")

        # RGB shift (float64, cast at the feature concat)
        shifts = np.stack([a.shift * 0.1 for _, a, _, _ in units])
        # crop (train) or keep all (val) -> mask + offset + final min subtraction + compaction
        max_crop_p, min_crop_p = int(getattr(cfg, "max_crop_p", 300000)), int(getattr(cfg, "min_crop_p", 50000))
        mode = np.zeros(B, np.int32)                    # 0: crop loop, 1: keep all points un-offset
        trip = np.zeros((B, CROP_TRIES * CROP_LEVELS, 3))
        n_trip = np.zeros(B, np.int32)
        for s in range(B):
            n_s = int(soff[s + 1] - soff[s])
            if not crop or n_s <= max_crop_p:
                mode[s] = 1
            else:
                t = draws.scenes[s].crop
                assert t.shape[0] <= CROP_TRIES * CROP_LEVELS and t.shape[1] == 3
                trip[s, :t.shape[0]] = t
                n_trip[s] = t.shape[0]
        state = torch.zeros(B, 8, dtype=torch.int32, device=dev)      # see augment.hip k_crop_pick
        counts = torch.zeros(CROP_TRIES, B, CROP_LEVELS, dtype=torch.int32, device=dev)
        levels = _f64(crop_levels(cfg), dev)
        trip_d = _f64(trip, dev)
        mode_d = _i32(mode, dev)
        ext_pre = torch.empty(B, 6, dtype=torch.float64, device=dev)
        ext_post = torch.empty(B, 6, dtype=torch.float64, device=dev)
        N.check(lib.pbn_aug_crop(N.ptr(xyz), N.ptr(soff_d), B, max_s, N.ptr(mode_d), N.ptr(trip_d),
                                 N.ptr(i32(n_trip)), N.ptr(levels), max_crop_p, min_crop_p, N.ptr(counts), N.ptr(state),
                                 N.ptr(ext_pre), N.ptr(ext_post), N.ptr(ws), stream), "pbn_aug_crop")
        # compaction + labels: partner label shift by the primary's raw ins.max()+1 (train)
        ins_shift = np.zeros(U, np.int32)
        lab_cap = np.zeros(B, np.int64)
        for s in range(B):
            hi = 0
            for k in range(per_scene):
                u = s * per_scene + k
                h = self.cache.host[units[u][0]]
                if k == 1:
                    ins_shift[u] = self.cache.host[units[u - 1][0]]["ins_max"] + 1
                hi = max(hi, h["ins_max"] + int(ins_shift[u]))
            lab_cap[s] = max(hi, 0) + 1
        loff = np.zeros(B + 1, np.int64)
        loff[1:] = np.cumsum(lab_cap)
        n_chunks = lib.pbn_aug_chunks(n_all)
        xyz_o = torch.empty(max(n_all, 1), 3, dtype=torch.float64, device=dev)
        feat_o = torch.empty(max(n_all, 1), 6, dtype=torch.float32, device=dev)
        sem_o = torch.empty(max(n_all, 1), dtype=torch.int64, device=dev)
        lab_o = torch.empty(max(n_all, 1), dtype=torch.int32, device=dev)
        scan = torch.empty(n_chunks + 1, dtype=torch.int32, device=dev)
        sinfo = torch.empty(B, 4, dtype=torch.int32, device=dev)       # rows kept, instance_num, first row, 0
        n_labels = int(loff[-1])
        lmap = torch.empty(n_labels, dtype=torch.int32, device=dev)
        present = torch.empty(n_labels, dtype=torch.int32, device=dev)
        scene_i32 = torch.empty(2 * B, dtype=torch.int32, device=dev)
        N.check(lib.pbn_aug_compact(N.ptr(xyz), N.ptr(rgb32), N.ptr(nl32), N.ptr(sem_all), N.ptr(ins_raw),
                                    N.ptr(f64(shifts)), N.ptr(i32(ins_shift)), N.ptr(uoff_d), U,
                                    N.ptr(soff_d), B, N.ptr(mode_d), N.ptr(trip_d), N.ptr(levels), N.ptr(state),
                                    N.ptr(ext_pre), N.ptr(ext_post), N.ptr(i32(loff)), N.ptr(lmap), N.ptr(present),
                                    N.ptr(scene_i32), N.ptr(scan), N.ptr(xyz_o), N.ptr(feat_o), N.ptr(sem_o), N.ptr(lab_o),
                                    N.ptr(sinfo), n_all, n_labels, stream), "pbn_aug_compact")
        host = torch.cat([sinfo.view(-1), state.view(-1)]).cpu().numpy()             # per-scene counts + crop states
        self.readbacks += 1
        sinfo_h = host[:4 * B].reshape(B, 4)
        state_h = host[4 * B:].reshape(B, 8)
        if (state_h[:, 6] != 0).any():                  # state word 6: 1 = out of shrink levels, 2 = out of triples
            why = []
            if (state_h[:, 6] == 1).any():
                why.append("a try did not stop within %d shrink levels (scenes %s)"
                           % (CROP_LEVELS, np.nonzero(state_h[:, 6] == 1)[0].tolist()))
            if (state_h[:, 6] == 2).any():
                short = np.nonzero(state_h[:, 6] == 2)[0].tolist()
                why.append("the crop triples ran out (scenes %s, %s drawn)" % (short, [int(n_trip[s]) for s in short]))
            if not why:
                why.append("unknown error state %s" % state_h[:, 6].tolist())
            raise RuntimeError("crop: " + "; ".join(why))
        self.last_crop_used = state_h[:, 2].copy()
        n_out = int(sinfo_h[:, 0].sum())
        inst_num = sinfo_h[:, 1].astype(np.int64)
        n_inst = int(np.maximum(inst_num, 0).sum())
        inst_off = np.concatenate([[0], np.cumsum(inst_num)[:-1]]).astype(np.int64)
        ipos = np.concatenate([[0], np.cumsum(np.maximum(inst_num, 0))]).astype(np.int32)
        inst_info = torch.empty(max(n_out, 1), 9, dtype=torch.float32, device=dev)
        ins_o = torch.empty(max(n_out, 1), dtype=torch.int64, device=dev)
        pointnum = torch.empty(max(n_inst, 1), dtype=torch.int32, device=dev)
        stats = torch.empty(max(n_inst, 1), 9, dtype=torch.float32, device=dev)
        ostart = np.concatenate([[0], np.cumsum(sinfo_h[:, 0])]).astype(np.int32)
        N.check(lib.pbn_aug_instances(N.ptr(xyz_o), N.ptr(lab_o), N.ptr(i32(ostart)), B,
                                      N.ptr(i32(ipos)), N.ptr(i32(inst_off)), n_inst, n_out, N.ptr(pointnum),
                                      N.ptr(stats), N.ptr(inst_info), N.ptr(ins_o), stream), "pbn_aug_instances")
        # voxelisation of the float64 coordinates (batch index in the key, first occurrence survives)
        c4 = torch.empty(max(n_out, 1), 4, dtype=torch.int32, device=dev)
        xyz32_o = torch.empty(max(n_out, 1), 3, dtype=torch.float32, device=dev)
        N.check(lib.pbn_aug_quantize(N.ptr(xyz_o), N.ptr(i32(ostart)), B, n_out, ctypes.c_double(cfg.voxel_size),
                                     N.ptr(c4), N.ptr(xyz32_o), stream), "pbn_aug_quantize")
        c4, xyz32_o = c4[:n_out], xyz32_o[:n_out]
        cm = CoordinateManager(c4, prepare="unique")
        cm.num_rows(1)                                  # the voxel count: read back once
        self.readbacks += 1
        index, inverse = cm.unique_index, cm.inverse_mapping
        out = {"xyz_voxel": c4[index], "feat_voxel": feat_o[:n_out][index], "xyz_original": xyz32_o,
               "sem": sem_o[:n_out], "ins": ins_o[:n_out], "inst_info": inst_info[:n_out],
               "instance_pointnum": pointnum[:n_inst], "v2p_index": inverse.to(torch.int64), "fn": list(fn)}
        if sup is not None:
            out["sup"] = sup
        return out

    def _elastic(self, lib, units, el, e, p, gran, mag, xyz, uoff_d, max_u, ext, ws, draws, i32, stream):
        dev = self.dev
        shapes, grids = [], []
        for u in el:
            absmax = np.maximum(np.abs(e[u, 0:3]), np.abs(e[u, 3:6]))
            shape = elastic_shape(absmax, gran)
            g = draws.noise_for(units[u][1], p, shape)
            shapes.append(shape)
            grids.extend(x.reshape(-1) for x in g)
        desc = np.zeros((len(el), 5), np.int32)        # unit, b0, b1, b2, first float of its 3 grids
        off = 0
        for j, (u, sh) in enumerate(zip(el, shapes)):
            desc[j] = (u, sh[0], sh[1], sh[2], off)
            off += 3 * sh[0] * sh[1] * sh[2]
        noise = torch.from_numpy(np.concatenate(grids).astype(np.float32)).to(dev)
        tmp = torch.empty_like(noise)
        N.check(lib.pbn_aug_elastic(N.ptr(xyz), N.ptr(uoff_d), len(units), max_u, N.ptr(i32(desc)), len(el), off,
                                    N.ptr(noise), N.ptr(tmp), int(gran), ctypes.c_double(mag), N.ptr(ext), N.ptr(ws), stream),
                "pbn_aug_elastic")
