"""GPU tier: csrc/augment.hip entry point by entry point (pbn_aug_affine, _elastic, _sub_min, _crop, _compact, _instances,
_quantize) on the designed cases of tests/aug_cases.py against the host restatement tests/aug_ref.py (anchored by
tests/test_aug_cases_cpu.py).  Integers are compared exactly, float64 and float32 outputs bit for bit (zeros by value: the
ordered-key reduction may return -0.0 where numpy returns +0.0); only the instance mean, which the kernel sums in a fixed
tree, gets the one float32 ulp of merge_ref.assert_batch against float32(fsum / n).  Every output lies inside a larger
buffer filled with a byte pattern that must survive outside the documented extent."""
import ctypes
from collections import OrderedDict

import numpy as np
import pytest
import torch

import aug_cases as C
import aug_ref as R
from pbnet_amd import _native as N
from pbnet_amd.loader import ELASTIC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
VP = ctypes.c_void_p
PAT = 0x5A
F64, F32, I32, I64 = torch.float64, torch.float32, torch.int32, torch.int64


# ---- guarded buffers --------------------------------------------------------------------------------------------------------
def _is_pattern(t):
    return bool((t.contiguous().view(-1).view(torch.uint8) == PAT).all().item())


class Guarded(object):
    """n elements of `dtype` (at least one, so the address is never null) between two margins, everything filled with the
    byte pattern; kernels get the address of the body."""

    def __init__(self, n_elems, dtype, margin=64):
        self.n, self.m, self.es = int(n_elems), margin, torch.empty(0, dtype=dtype).element_size()
        self.buf = torch.full(((max(self.n, 1) + 2 * margin) * self.es,), PAT, dtype=torch.uint8, device=DEV).view(dtype)

    @property
    def ptr(self):
        return VP(self.buf.data_ptr() + self.m * self.es)

    @property
    def body(self):
        return self.buf[self.m:self.m + self.n]

    def fill(self, a):
        self.body.copy_(torch.from_numpy(np.ascontiguousarray(a)).reshape(-1))
        return self

    def host(self, k=None):
        return self.body[:self.n if k is None else int(k)].cpu().numpy()

    def untouched_from(self, k):
        """The buffer from body element k on, and the margin in front, still hold the pattern."""
        return _is_pattern(self.buf[:self.m]) and _is_pattern(self.buf[self.m + int(k):])


def _dev(a, dtype):
    """A device copy with at least one element behind it (an empty tensor has a null address)."""
    a = np.ascontiguousarray(np.asarray(a), dtype=dtype).reshape(-1)
    return torch.from_numpy(a if a.size else np.zeros(1, dtype)).to(DEV)


def _ws(n):
    return torch.empty(N.lib().pbn_aug_workspace_bytes(int(n)), dtype=torch.uint8, device=DEV)


def _call(fn, args, override):
    for k, v in (override or {}).items():
        assert k in args, k
        args[k] = v
    rc = fn(*[N.ptr(v) if isinstance(v, torch.Tensor) else (v.ptr if isinstance(v, Guarded) else v) for v in args.values()])
    torch.cuda.synchronize()
    return rc


def _bits_equal(got, want, what):
    got, want = np.asarray(got), np.asarray(want).reshape(np.asarray(got).shape)
    assert got.dtype == want.dtype, (what, got.dtype, want.dtype)
    iv = {4: np.int32, 8: np.int64}[got.dtype.itemsize]
    bad = (got.view(iv) != want.view(iv)) & ~((got == 0) & (want == 0))
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:5].tolist(), got[bad][:3], want[bad][:3])


def _ints_equal(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and np.array_equal(got, want), (what, int((got != want).sum()) if got.shape == want.shape
                                                                   else (got.shape, want.shape))


# =============================================================================================================================
# pbn_aug_affine
# =============================================================================================================================
def _run_affine(c, override=None):
    n, U = c["xyz"].shape[0], len(c["uoff"]) - 1
    out, ext = Guarded(3 * n, F64), Guarded(6 * U, F64)
    args = OrderedDict(xyz=_dev(c["xyz"], np.float32), uoff=_dev(c["uoff"], np.int32), n_units=U, max_rows=c["max_rows"],
                       pre_min=_dev(c["pre_min"], np.int32), mats=_dev(c["mats"], np.float64),
                       scale=_dev(c["scale"], np.float64), has_scale=_dev(c["has_scale"], np.int32), out=out, ext=ext,
                       ws=_ws(U), stream=N.current_stream())
    return _call(N.lib().pbn_aug_affine, args, override), out, ext


def test_affine():
    c = C.affine_case()
    rc, out, ext = _run_affine(c)
    assert rc == 0 and out.untouched_from(out.n) and ext.untouched_from(ext.n)
    want, want_ext = R.affine(c["xyz"], c["uoff"], c["pre_min"], c["mats"], c["scale"], c["has_scale"])
    _bits_equal(out.host().reshape(-1, 3), want, "affine out")
    _bits_equal(ext.host().reshape(-1, 6), want_ext, "affine ext")


# =============================================================================================================================
# pbn_aug_elastic, pbn_aug_sub_min
# =============================================================================================================================
def _run_elastic(c, p, xyz, override=None):
    gran, mag = ELASTIC[p]
    U = len(c["uoff"]) - 1
    desc, off = [], 0
    for u, sh in zip(c["units"], c["shapes"][p]):
        desc.append((u, sh[0], sh[1], sh[2], off))
        off += 3 * sh[0] * sh[1] * sh[2]
    noise = np.concatenate([g.reshape(-1) for grids in c["noise"][p] for g in grids]).astype(np.float32)
    assert noise.size == off
    ext = Guarded(6 * U, F64)
    args = OrderedDict(xyz=xyz, uoff=_dev(c["uoff"], np.int32), n_units=U, max_rows=c["max_rows"],
                       desc=_dev(np.array(desc), np.int32), n_el=len(desc), total=off, noise=_dev(noise, np.float32),
                       tmp=torch.empty(off, dtype=F32, device=DEV), gran=int(gran), mag=ctypes.c_double(mag), ext=ext,
                       ws=_ws(U), stream=N.current_stream())
    return _call(N.lib().pbn_aug_elastic, args, override), ext


def _run_sub_min(c, xyz, ext, override=None):
    args = OrderedDict(xyz=xyz, uoff=_dev(c["uoff"], np.int32), n_units=len(c["uoff"]) - 1, max_rows=c["max_rows"],
                       flags=_dev(c["flags"], np.int32), ext=ext, stream=N.current_stream())
    return _call(N.lib().pbn_aug_sub_min, args, override)


def test_elastic_and_sub_min():
    c = C.elastic_case()
    steps, last = C.elastic_ref(c)
    n = c["xyz"].shape[0]
    xyz = Guarded(3 * n, F64).fill(c["xyz"])
    rows = np.concatenate([np.arange(c["uoff"][u], c["uoff"][u + 1]) for u in c["units"]])
    others = np.setdiff1d(np.arange(n), rows)
    ext = None
    for p in range(len(ELASTIC)):
        rc, ext = _run_elastic(c, p, xyz)
        assert rc == 0 and xyz.untouched_from(xyz.n) and ext.untouched_from(ext.n)
        _bits_equal(xyz.host().reshape(-1, 3), steps[p][0], "elastic pass %d" % p)
        _bits_equal(ext.host().reshape(-1, 6)[c["units"]], steps[p][1][c["units"]], "elastic ext %d" % p)
    assert _run_sub_min(c, xyz, ext) == 0 and xyz.untouched_from(xyz.n)
    got = xyz.host().reshape(-1, 3)
    _bits_equal(got, last, "sub_min")
    assert np.array_equal(got[others].view(np.int64), c["xyz"][others].view(np.int64))     # not a bit of the others moved


# =============================================================================================================================
# pbn_aug_crop
# =============================================================================================================================
def _run_crop(c, override=None):
    B = len(c["mode"])
    counts, state = Guarded(R.CROP_TRIES * B * R.CROP_LEVELS, I32), Guarded(8 * B, I32)
    pre, post = Guarded(6 * B, F64), Guarded(6 * B, F64)
    args = OrderedDict(xyz=_dev(c["xyz"], np.float64), soff=_dev(c["soff"], np.int32), n_scenes=B, max_rows=c["max_rows"],
                       mode=_dev(c["mode"], np.int32), triples=_dev(c["triples"], np.float64),
                       n_triples=_dev(c["n_triples"], np.int32), levels=_dev(c["levels"], np.float64),
                       max_crop_p=int(c["max_crop_p"]), min_crop_p=int(c["min_crop_p"]), counts=counts, state=state,
                       ext_pre=pre, ext_post=post, ws=_ws(B), stream=N.current_stream())
    return _call(N.lib().pbn_aug_crop, args, override), counts, state, pre, post


@pytest.mark.parametrize("name", ["crop", "crop_short", "crop_boundary"])
def test_crop(name):
    c = getattr(C, name + "_case")()
    want = C.crop_ref(c)
    rc, counts, state, pre, post = _run_crop(c)
    assert rc == 0 and all(g.untouched_from(g.n) for g in (counts, state, pre, post))
    B = len(c["mode"])
    got_counts = counts.host().reshape(R.CROP_TRIES, B, R.CROP_LEVELS)
    visited = want["counts"] >= 0
    _ints_equal(got_counts[visited], want["counts"][visited], "counts")
    assert not got_counts[:, c["mode"] != 0].any()
    got_state = state.host().reshape(B, 8)
    failed = want["state"][:, R.ST_ERROR] != 0
    _ints_equal(got_state[~failed], want["state"][~failed], "state")
    words = [w for w in range(8) if w not in R.ST_UNSPECIFIED_ON_ERROR]
    _ints_equal(got_state[failed][:, words], want["state"][failed][:, words], "state of scenes out of triples")
    assert failed.any() == (name == "crop_short")
    full = np.diff(c["soff"]) > 0
    _bits_equal(pre.host().reshape(B, 6)[full], want["ext_pre"][full], "ext_pre")
    _bits_equal(post.host().reshape(B, 6)[full], want["ext_post"][full], "ext_post")


# =============================================================================================================================
# pbn_aug_compact
# =============================================================================================================================
def _run_compact(c, override=None):
    n, U, B = c["n_rows"], len(c["uoff"]) - 1, len(c["mode"])
    n_labels = int(c["label_off"][-1])
    n_chunks = N.lib().pbn_aug_chunks(n)
    assert n_chunks == max(1, -(-n // R.CHUNK))
    out = OrderedDict(scan=Guarded(n_chunks + 1, I32), xyz=Guarded(3 * n, F64), feat=Guarded(6 * n, F32), sem=Guarded(n, I64),
                      label=Guarded(n, I32), info=Guarded(4 * B, I32))
    args = OrderedDict(xyz=_dev(c["xyz"], np.float64), rgb=_dev(c["rgb"], np.float32), nl=_dev(c["nl"], np.float32),
                       sem=_dev(c["sem"], np.int64), ins=_dev(c["ins"], np.int32), shift=_dev(c["shift"], np.float64),
                       ins_shift=_dev(c["ins_shift"], np.int32), uoff=_dev(c["uoff"], np.int32), n_units=U,
                       soff=_dev(c["soff"], np.int32), n_scenes=B, mode=_dev(c["mode"], np.int32),
                       triples=_dev(c["triples"], np.float64), levels=_dev(c["levels"], np.float64),
                       state=_dev(c["state"], np.int32), ext_pre=_dev(c["ext_pre"], np.float64),
                       ext_post=_dev(c["ext_post"], np.float64), label_off=_dev(c["label_off"], np.int32),
                       label_map=torch.empty(n_labels, dtype=I32, device=DEV), present=torch.empty(n_labels, dtype=I32, device=DEV),
                       scene_i32=torch.empty(2 * B, dtype=I32, device=DEV), scan=out["scan"], xyz_out=out["xyz"],
                       feat_out=out["feat"], sem_out=out["sem"], label_out=out["label"], scene_info=out["info"], n_rows=n,
                       n_labels=n_labels, stream=N.current_stream())
    return _call(N.lib().pbn_aug_compact, args, override), out


@pytest.mark.parametrize("name", sorted(C.compact_cases()))
def test_compact(name):
    c = C.compact_cases()[name]()
    want = C.compact_ref(c)
    rc, out = _run_compact(c)
    assert rc == 0
    k = int(want["mask"].sum())
    assert out["xyz"].untouched_from(3 * k) and out["feat"].untouched_from(6 * k) and out["sem"].untouched_from(k)
    assert out["label"].untouched_from(k) and out["scan"].untouched_from(out["scan"].n) and out["info"].untouched_from(out["info"].n)
    _ints_equal(out["info"].host().reshape(-1, 4), want["scene_info"], "scene_info")
    _ints_equal(out["scan"].host(), want["scan"], "scan")
    _ints_equal(out["sem"].host(k), want["sem"], "sem")
    _ints_equal(out["label"].host(k), want["label"], "label")
    _bits_equal(out["xyz"].host(3 * k).reshape(-1, 3), want["xyz"], "xyz_out")
    _bits_equal(out["feat"].host(6 * k).reshape(-1, 6), want["feat"], "feat_out")
    if name in ("in_thread", "wave_chunk_edges", "two_units", "relabel", "rows2049"):      # bit-identical on a repeat
        rc2, again = _run_compact(c)
        assert rc2 == 0 and all(torch.equal(out[key].buf.view(torch.uint8), again[key].buf.view(torch.uint8)) for key in out)


def test_compact_no_rows():
    """n_rows == 0: one chunk, scan = (0, 0), scene_info = (0, 0, 0, 0), no row output touched."""
    c = C.compact_no_rows()
    assert c["n_rows"] == 0
    rc, out = _run_compact(c)
    assert rc == 0 and all(out[key].untouched_from(0) for key in ("xyz", "feat", "sem", "label"))
    assert out["scan"].host().tolist() == [0, 0] and out["info"].host().tolist() == [0, 0, 0, 0]
    assert out["scan"].untouched_from(2) and out["info"].untouched_from(4)


# =============================================================================================================================
# pbn_aug_instances
# =============================================================================================================================
def _run_instances(c, override=None):
    r = C.instances_ref(c)
    n, n_inst = c["n_rows"], int(r["inst_start"][-1])
    out = OrderedDict(pointnum=Guarded(n_inst, I32), stats=Guarded(9 * n_inst, F32), info=Guarded(9 * n, F32), ins=Guarded(n, I64))
    args = OrderedDict(xyz=_dev(c["xyz"], np.float64), label=_dev(c["label"], np.int32), ostart=_dev(c["ostart"], np.int32),
                       n_scenes=len(c["inst_num"]), inst_start=_dev(r["inst_start"], np.int32),
                       inst_off=_dev(r["inst_off"], np.int32), n_inst=n_inst, n_rows=n, pointnum=out["pointnum"],
                       stats=out["stats"], inst_info=out["info"], ins=out["ins"], stream=N.current_stream())
    return _call(N.lib().pbn_aug_instances, args, override), out, r


def _ulp_apart(got, want):
    return np.abs(got.astype(np.float64) - want.astype(np.float64)) > np.spacing(np.maximum(np.abs(got), np.abs(want)))


def test_instances():
    c = C.instances_case()
    rc, out, want = _run_instances(c)
    assert rc == 0 and all(g.untouched_from(g.n) for g in out.values())
    _ints_equal(out["pointnum"].host(), want["pointnum"], "pointnum")
    _ints_equal(out["ins"].host(), want["ins"], "ins")
    stats, info = out["stats"].host().reshape(-1, 9), out["info"].host().reshape(-1, 9)
    _bits_equal(stats[:, 3:], want["stats"][:, 3:], "stats min / max")
    _bits_equal(info[:, 3:], want["inst_info"][:, 3:], "inst_info min / max")
    assert not _ulp_apart(stats[:, :3], want["stats"][:, :3]).any() and not _ulp_apart(info[:, :3], want["inst_info"][:, :3]).any()
    print("instance means not bit-equal to float32(fsum / n): %d of %d"
          % (int((stats[:, :3].view(np.int32) != want["stats"][:, :3].view(np.int32)).sum()), stats[:, :3].size))
    # every labelled row carries its instance's statistics, the others -100
    for s in range(len(c["inst_num"])):
        a, b = c["ostart"][s], c["ostart"][s + 1]
        lab = c["label"][a:b]
        has = lab >= 0
        assert np.array_equal(info[a:b][has].view(np.int32), stats[want["inst_start"][s] + lab[has]].view(np.int32))
        assert (info[a:b][~has] == -100).all()
    rc2, again, _ = _run_instances(c)                                                        # bit-identical on a repeat
    assert rc2 == 0 and all(torch.equal(out[k].buf.view(torch.uint8), again[k].buf.view(torch.uint8)) for k in out)


def test_instances_none():
    """n_inst == 0: rows get -100, pointnum and stats stay untouched."""
    c = C.instances_none_case()
    rc, out, want = _run_instances(c)
    assert rc == 0 and out["pointnum"].untouched_from(0) and out["stats"].untouched_from(0)
    assert out["info"].untouched_from(out["info"].n) and out["ins"].untouched_from(out["ins"].n)
    assert (out["info"].host() == -100).all() and (out["ins"].host() == -100).all()
    _ints_equal(out["ins"].host(), want["ins"], "ins")


def test_instances_no_rows():
    rc, out, _ = _run_instances(C.instances_no_rows_case())
    assert rc == 0 and all(g.untouched_from(0) for g in out.values())


# =============================================================================================================================
# pbn_aug_quantize
# =============================================================================================================================
def _run_quantize(c, override=None):
    n = c["n_rows"]
    out = OrderedDict(coords=Guarded(4 * n, I32), xyz32=Guarded(3 * n, F32))
    args = OrderedDict(xyz=_dev(c["xyz"], np.float64), ostart=_dev(c["ostart"], np.int32), n_scenes=len(c["ostart"]) - 1,
                       n_rows=n, voxel=ctypes.c_double(c["voxel"]), coords=out["coords"], xyz32=out["xyz32"],
                       stream=N.current_stream())
    return _call(N.lib().pbn_aug_quantize, args, override), out


@pytest.mark.parametrize("voxel", [0.02, 0.01])
def test_quantize(voxel):
    c = C.quantize_case(voxel)
    rc, out = _run_quantize(c)
    assert rc == 0 and all(g.untouched_from(g.n) for g in out.values())
    want_c, want_x = R.quantize(c["xyz"], c["ostart"], c["voxel"])
    _ints_equal(out["coords"].host().reshape(-1, 4), want_c, "coords")
    got = out["xyz32"].host().reshape(-1, 3)
    assert np.array_equal(got.view(np.int32), want_x.view(np.int32))                           # -0.0 stays -0.0


def test_quantize_no_rows():
    rc, out = _run_quantize(dict(xyz=np.zeros((0, 3)), ostart=np.array([0, 0, 0], np.int32), voxel=0.02, n_rows=0))
    assert rc == 0 and all(g.untouched_from(0) for g in out.values())


# =============================================================================================================================
# argument errors: PBN_ERR_ARG, outputs untouched
# =============================================================================================================================
def _refused(rc, outs):
    assert rc == N.PBN_ERR_ARG
    assert all(g.untouched_from(0) for g in outs)


def test_argument_errors():
    a, e, cr = C.affine_case(), C.elastic_case(), C.crop_boundary_case()
    small = dict(a, xyz=a["xyz"][:8], uoff=np.array([0, 1, 8], np.int32), max_rows=7)
    for bad in (dict(n_units=0), dict(n_units=-1), dict(xyz=None), dict(mats=None), dict(ws=None)):
        rc, out, ext = _run_affine(small, bad)
        _refused(rc, (out, ext))
    xyz = Guarded(3 * e["xyz"].shape[0], F64)
    for bad in (dict(n_units=0), dict(gran=0), dict(gran=-6), dict(noise=None), dict(desc=None), dict(n_el=0)):
        rc, ext = _run_elastic(e, 0, xyz, bad)
        _refused(rc, (xyz, ext))
    ext = Guarded(6 * 5, F64)
    for bad in (dict(n_units=0), dict(flags=None), dict(ext=None)):
        _refused(_run_sub_min(e, xyz, ext, bad), (xyz, ext))
    for bad in (dict(n_scenes=0), dict(triples=None), dict(n_triples=None), dict(ws=None)):
        rc, *outs = _run_crop(cr, bad)
        _refused(rc, outs)
    k = C.compact_single(9)
    for bad in (dict(n_units=0), dict(n_scenes=0), dict(n_labels=0), dict(n_rows=-1), dict(rgb=None), dict(label_map=None)):
        rc, out = _run_compact(k, bad)
        _refused(rc, out.values())
    for bad in (dict(n_scenes=0), dict(n_inst=-1), dict(n_rows=-1), dict(label=None), dict(inst_off=None)):
        rc, out, _ = _run_instances(C.instances_case(), bad)
        _refused(rc, out.values())
    q = C.quantize_case(0.02)
    for bad in (dict(voxel=ctypes.c_double(0.0)), dict(voxel=ctypes.c_double(-0.02)), dict(voxel=ctypes.c_double(float("nan"))),
                dict(n_scenes=0), dict(xyz=None)):
        rc, out = _run_quantize(q, bad)
        _refused(rc, out.values())
