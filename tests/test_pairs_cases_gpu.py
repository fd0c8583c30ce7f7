"""GPU tier: csrc/pairs.hip through the C ABI on the designed maps of tests/pairs_cases.py against tests/pairs_ref.py.  Every output --
totals, the post-scan table, seg_begin (all K + 1 words), in_idx, out_idx, seg_offset -- sits inside an allocation filled with the
byte 0x5a on both sides and is compared WHOLE with the reference's words: what the reference leaves unwritten (the device form's
tails, everything from seg_begin[K] * seg on, an empty map's table) must still be the pattern.  Host form with two surplus segments,
device form, the multi launch over every job table; refusals leave every buffer untouched; every case runs twice with the same bytes.
No tolerance anywhere."""
import ctypes

import numpy as np
import pytest
import torch

import pairs_cases as PC
import pairs_mutants as PM
import pairs_ref as PR
from pbnet_amd import _native as N

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
PAT = 0x5A
SURPLUS = 2
I32, I64 = torch.int32, torch.int64
LISTS = ("totals", "table", "seg_begin", "in_idx", "out_idx", "seg_offset")


class Guarded(object):
    """n elements of `dtype` (at least one, so the address is never null) between two margins, everything filled with the byte
    pattern; kernels get the address of the body."""

    def __init__(self, n_elems, dtype, margin=64):
        self.n, self.m, self.es = int(n_elems), margin, torch.empty(0, dtype=dtype).element_size()
        self.buf = torch.full(((max(self.n, 1) + 2 * margin) * self.es,), PAT, dtype=torch.uint8, device=DEV).view(dtype)

    @property
    def ptr(self):
        return ctypes.c_void_p(self.buf.data_ptr() + self.m * self.es)

    @property
    def address(self):
        return self.buf.data_ptr() + self.m * self.es

    def host(self):
        return self.buf[self.m:self.m + self.n].cpu().numpy().astype(np.int64)

    def margins_intact(self):
        return bool((self.buf[:self.m].view(torch.uint8) == PAT).all()) and bool((self.buf[self.m + self.n:].view(torch.uint8) == PAT).all())

    def untouched(self):
        return bool((self.buf.view(torch.uint8) == PAT).all())


def _dev(a):
    """A device copy of an int32 map with at least one element behind it (an empty tensor has a null address)."""
    a = np.array(a, dtype=np.int32, order="C", copy=True).reshape(-1)         # the cases' arrays are read-only
    return torch.from_numpy(a if a.size else np.full(1, -1, np.int32)).to(DEV)


class Lists(object):
    """The buffers of one map's lists at the device form's worst case (or n_segments of the host form)."""

    def __init__(self, nbr, seg, n_segments=None):
        self.n, self.K = nbr.shape
        self.seg = seg
        self.nbr = _dev(nbr)
        cap = PR.worst_case_segments(self.n, self.K, seg) if n_segments is None else n_segments
        self.cap = cap
        blocks = N.lib().pbn_rulebook_pair_blocks(self.n)
        assert blocks == PC.blocks(self.n)
        self.table = Guarded(max(blocks, 1) * self.K, I32)
        self.totals, self.seg_begin = Guarded(self.K, I32), Guarded(self.K + 1, I32)
        self.in_idx, self.out_idx, self.seg_offset = Guarded(cap * seg, I32), Guarded(cap * seg, I32), Guarded(cap, I64)

    def all(self):
        return [getattr(self, k) for k in LISTS]

    def result(self):
        r = {k: getattr(self, k).host() for k in LISTS}
        r["table"] = r["table"].reshape(-1, self.K)
        r["oob"] = not all(g.margins_intact() for g in self.all())
        return r

    def counts(self):
        return N.lib().pbn_rulebook_pair_counts(N.ptr(self.nbr), self.n, self.K, self.table.ptr, self.totals.ptr, N.current_stream())

    def fill_dev(self, **over):
        a = dict(nbr=N.ptr(self.nbr), table=self.table.ptr, totals=self.totals.ptr, seg=self.seg, seg_begin=self.seg_begin.ptr,
                 in_idx=self.in_idx.ptr, out_idx=self.out_idx.ptr, seg_offset=self.seg_offset.ptr)
        a.update(over)
        return N.lib().pbn_rulebook_pair_fill_dev(a["nbr"], self.n, self.K, a["table"], a["totals"], a["seg"], a["seg_begin"], a["in_idx"],
                                                  a["out_idx"], a["seg_offset"], N.current_stream())

    def fill_host(self, first_segments, **over):
        self.seg_start = _dev(first_segments)
        a = dict(nbr=N.ptr(self.nbr), table=self.table.ptr, seg_start=N.ptr(self.seg_start), seg=self.seg, n_segments=self.cap,
                 in_idx=self.in_idx.ptr, out_idx=self.out_idx.ptr, seg_offset=self.seg_offset.ptr)
        a.update(over)
        return N.lib().pbn_rulebook_pair_fill(a["nbr"], self.n, self.K, a["table"], a["seg_start"], a["seg"], a["n_segments"], a["in_idx"],
                                              a["out_idx"], a["seg_offset"], N.current_stream())

    def job(self, q):
        q.nbr, q.n, q.n_offsets = self.nbr.data_ptr(), self.n, self.K
        q.table, q.totals, q.seg_begin = self.table.address, self.totals.address, self.seg_begin.address
        q.in_idx, q.out_idx, q.seg_offset = self.in_idx.address, self.out_idx.address, self.seg_offset.address


def _same_bytes(a, b):
    return all(torch.equal(x.buf.view(torch.uint8), y.buf.view(torch.uint8)) for x, y in zip(a.all(), b.all()))


def _explain(got, want):
    for k in PM.KEYS:
        if got[k].shape != want[k].shape or not np.array_equal(got[k], want[k]):
            bad = np.nonzero(got[k].reshape(-1) != want[k].reshape(-1))[0] if got[k].shape == want[k].shape else []
            return "%s differs (%d words, first at %s: got %s, want %s)" % (
                k, len(bad), bad[:1], got[k].reshape(-1)[bad[:1]], want[k].reshape(-1)[bad[:1]])
    return "a margin was written" if got["oob"] else "equal"


def _run_dev(nbr, seg):
    L = Lists(nbr, seg)
    assert L.counts() == N.PBN_OK and L.fill_dev() == N.PBN_OK
    torch.cuda.synchronize()
    return L


def _run_host(nbr, seg, seg_start, n_seg):
    L = Lists(nbr, seg, n_seg)
    assert L.counts() == N.PBN_OK
    assert L.fill_host(seg_start) == N.PBN_OK
    torch.cuda.synchronize()
    return L


def _run_multi(maps, seg):
    Ls = [Lists(m, seg) for m in maps]
    jobs = (N.PairJob * len(Ls))()
    for q, L in zip(jobs, Ls):
        L.job(q)
    assert N.lib().pbn_rulebook_pairs_multi(jobs, len(Ls), seg, N.current_stream()) == N.PBN_OK
    torch.cuda.synchronize()
    return Ls


@pytest.mark.parametrize("name", PC.SINGLE)
def test_device_form_equals_reference(name):
    c = PC.case(name)
    want = PM.reference_dev(c["nbr"], c["seg"])
    L = _run_dev(c["nbr"], c["seg"])
    got = L.result()
    assert PM.same(got, want), _explain(got, want)
    used = int(want["seg_begin"][-1])
    assert used <= L.cap, "worst-case sizing exceeded"
    print("\nDEV %-16s segments %5d of %5d (margin %d)" % (name, used, L.cap, L.cap - used))
    assert _same_bytes(L, _run_dev(c["nbr"], c["seg"])), "second run"


@pytest.mark.parametrize("name", PC.SINGLE)
def test_host_form_equals_reference(name):
    c = PC.case(name)
    want, seg_start, n_seg = PM.reference_host(c["nbr"], c["seg"], SURPLUS)
    L = _run_host(c["nbr"], c["seg"], seg_start, n_seg)
    got = L.result()
    assert PM.same(got, want), _explain(got, want)
    pad = got["in_idx"] < 0
    assert np.array_equal(pad, got["out_idx"] < 0) and (got["in_idx"][pad] == -1).all() and (got["out_idx"][pad] == -1).all()
    assert not got["seg_offset"][n_seg - SURPLUS:].any() and pad[(n_seg - SURPLUS) * c["seg"]:].all()         # the surplus segments
    assert _same_bytes(L, _run_host(c["nbr"], c["seg"], seg_start, n_seg)), "second run"


@pytest.mark.parametrize("name", [n for n in PC.MULTI if not PC.case(n)["grouped"]])
def test_multi_equals_single_equals_reference(name):
    c = PC.case(name)
    Ls = _run_multi(c["maps"], c["seg"])
    for j, (m, L) in enumerate(zip(c["maps"], Ls)):
        want, got = PM.reference_multi(m, c["seg"]), L.result()
        assert PM.same(got, want), "job %d: %s" % (j, _explain(got, want))
        one = _run_dev(m, c["seg"]).result()
        for k in PM.KEYS:
            if not (k == "table" and m.shape[0] == 0):                   # an empty map's one block: zeroed by the multi count only
                assert np.array_equal(one[k], got[k]), (j, k)
    again = _run_multi(c["maps"], c["seg"])
    assert all(_same_bytes(a, b) for a, b in zip(Ls, again)), "second run"


def _check_wrapper_lists(nbr_np, seg, hit):
    """What conv.rulebook_pairs_dev* returns (torch.empty buffers: only the written words are defined) against the reference."""
    ref = PR.pair_lists(nbr_np, seg)
    in_idx, out_idx, seg_begin, counts = [t.cpu().numpy().astype(np.int64) for t in hit]
    assert np.array_equal(counts, ref["totals"]) and np.array_equal(seg_begin, ref["seg_begin"])
    assert len(in_idx) == len(out_idx) == PR.worst_case_segments(nbr_np.shape[0], nbr_np.shape[1], seg) * seg >= int(ref["seg_begin"][-1]) * seg
    for k, p in enumerate(ref["pairs"]):
        lo = int(ref["seg_begin"][k]) * seg
        assert np.array_equal(in_idx[lo:lo + len(p)], p[:, 0]) and np.array_equal(out_idx[lo:lo + len(p)], p[:, 1]), k


def test_seventeen_maps_and_a_cached_one():
    """conv.rulebook_pairs_dev_multi: 17 maps go out as 16 + 1; a map whose lists exist is skipped and keeps its tensors."""
    from pbnet_amd.MinkowskiEngine import conv as C
    c = PC.case("M_17_groups")
    maps = [torch.from_numpy(np.array(m)).to(DEV) for m in c["maps"]]
    assert len(maps) == 17 and all(m.numel() for m in maps)
    hits = C.rulebook_pairs_dev_multi(maps, c["seg"])
    for m, hit in zip(c["maps"], hits):
        _check_wrapper_lists(m, c["seg"], hit)
    fresh = [torch.from_numpy(np.array(m)).to(DEV) for m in c["maps"][:5]]
    cached = C.rulebook_pairs_dev(fresh[2], c["seg"])
    _check_wrapper_lists(c["maps"][2], c["seg"], cached)
    hits = C.rulebook_pairs_dev_multi(fresh, c["seg"])
    assert all(a is b for a, b in zip(hits[2], cached)), "the cached lists were rebuilt"
    for m, hit in zip(c["maps"][:5], hits):
        _check_wrapper_lists(m, c["seg"], hit)
    again = C.rulebook_pairs_dev_multi(fresh, c["seg"] * 2)                 # another segment: the cache does not answer
    for m, hit in zip(c["maps"][:5], again):
        _check_wrapper_lists(m, c["seg"] * 2, hit)


def test_production_segment_on_real_maps():
    """The k = 3 map of a small voxelised room and its down / up maps at conv.WGRAD_PAIR_SEGMENT, all three forms."""
    import pbnet_amd.MinkowskiEngine as ME
    from pbnet_amd import synth
    from pbnet_amd.MinkowskiEngine import conv as C
    sc = synth.synth_room(seed=61, pitch=0.0225, room=(0.5, 0.4, 0.3), n_boxes=1)
    q, _, _ = synth.voxelize_numpy(sc["xyz"], 0.02)
    coords = np.concatenate([np.zeros((len(q), 1), np.int32), q], 1).astype(np.int32)
    cm = ME.CoordinateManager(torch.from_numpy(coords).to(DEV))
    maps = [cm.kernel_map(1, 3), cm.down_map(1), cm.up_map(2)]
    seg = C.WGRAD_PAIR_SEGMENT
    host = [m.cpu().numpy() for m in maps]
    assert [m.shape[1] for m in host] == [27, 8, 8] and all(0 < m.shape[0] <= 16385 for m in host) and seg == 4096
    Ls = _run_multi(host, seg)
    for m, L in zip(host, Ls):
        print("\nREAL %5d x %2d pairs %d" % (m.shape + (int((m >= 0).sum()),)))
        want, got = PM.reference_multi(m, seg), L.result()
        assert PM.same(got, want), _explain(got, want)
        one = _run_dev(m, seg).result()
        assert PM.same(one, PM.reference_dev(m, seg))
        want_h, seg_start, n_seg = PM.reference_host(m, seg, SURPLUS)
        got_h = _run_host(m, seg, seg_start, n_seg).result()
        assert PM.same(got_h, want_h), _explain(got_h, want_h)
    for m, t in zip(host, maps):
        _check_wrapper_lists(m, seg, C.rulebook_pairs_dev(t))


# ---- refusals: the documented code, and not a byte written -------------------------------------------------------------------------
def test_513_offsets_counts_succeed_fills_refuse():
    c = PC.case("K_k513")
    nbr, seg = c["nbr"], c["seg"]
    want = PM.reference_dev(nbr, seg)
    L = Lists(nbr, seg)
    assert L.counts() == N.PBN_OK
    assert L.fill_dev() == N.PBN_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    got = L.result()
    assert PM.same(got, want), _explain(got, want)                         # totals and table are the reference's, the rest is pattern
    assert all(g.untouched() for g in (L.seg_begin, L.in_idx, L.out_idx, L.seg_offset))
    want_h, seg_start, n_seg = PM.reference_host(nbr, seg, SURPLUS)
    H = Lists(nbr, seg, n_seg)
    assert H.counts() == N.PBN_OK and H.fill_host(seg_start) == N.PBN_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert PM.same(H.result(), want_h) and all(g.untouched() for g in (H.in_idx, H.out_idx, H.seg_offset))
    M = [Lists(PC.case("K_k3")["nbr"], seg), Lists(nbr, seg)]             # a legal job in front of it: nothing is launched for it either
    jobs = (N.PairJob * 2)()
    for q, l in zip(jobs, M):
        l.job(q)
    assert N.lib().pbn_rulebook_pairs_multi(jobs, 2, seg, N.current_stream()) == N.PBN_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert all(g.untouched() for l in M for g in l.all())


def test_argument_refusals_leave_every_buffer_untouched():
    lib = N.lib()
    c = PC.case("K_k3")
    nbr, seg = c["nbr"], c["seg"]
    ref = PR.pair_lists(nbr, seg)
    n_seg = int(ref["seg_begin"][-1])

    def counted(n_segments=None):
        L = Lists(nbr, seg, n_segments)
        assert L.counts() == N.PBN_OK
        torch.cuda.synchronize()
        return L, [g.buf.clone() for g in L.all()]

    def unchanged(L, before):
        torch.cuda.synchronize()
        return all(torch.equal(g.buf, b) for g, b in zip(L.all(), before))

    L, before = counted()
    assert L.fill_dev(seg=0) == N.PBN_ERR_ARG and unchanged(L, before)
    for k in ("nbr", "table", "totals", "seg_begin", "in_idx", "out_idx", "seg_offset"):
        assert L.fill_dev(**{k: None}) == N.PBN_ERR_ARG and unchanged(L, before), k
    H, before = counted(n_seg)
    assert H.fill_host(ref["seg_begin"][:-1], seg=0) == N.PBN_ERR_ARG and unchanged(H, before)
    assert H.fill_host(ref["seg_begin"][:-1], n_segments=-1) == N.PBN_ERR_ARG and unchanged(H, before)
    for k in ("nbr", "table", "seg_start", "in_idx", "out_idx", "seg_offset"):
        assert H.fill_host(ref["seg_begin"][:-1], **{k: None}) == N.PBN_ERR_ARG and unchanged(H, before), k
    # the counts: a NULL among their buffers
    Z = Lists(nbr, seg)
    st = N.current_stream()
    assert lib.pbn_rulebook_pair_counts(None, Z.n, Z.K, Z.table.ptr, Z.totals.ptr, st) == N.PBN_ERR_ARG
    assert lib.pbn_rulebook_pair_counts(N.ptr(Z.nbr), Z.n, Z.K, None, Z.totals.ptr, st) == N.PBN_ERR_ARG
    assert lib.pbn_rulebook_pair_counts(N.ptr(Z.nbr), Z.n, Z.K, Z.table.ptr, None, st) == N.PBN_ERR_ARG
    assert lib.pbn_rulebook_pair_counts(N.ptr(Z.nbr), Z.n, 0, Z.table.ptr, Z.totals.ptr, st) == N.PBN_ERR_ARG
    torch.cuda.synchronize()
    assert all(g.untouched() for g in Z.all())
    # the job table: no job, one job too many, segment 0, a NULL among one job's buffers
    many = [Lists(PC.case("K_k1")["nbr"], seg) for _ in range(17)]
    jobs = (N.PairJob * 17)()
    for q, l in zip(jobs, many):
        l.job(q)
    assert lib.pbn_rulebook_pairs_multi(jobs, 0, seg, st) == N.PBN_ERR_ARG
    assert lib.pbn_rulebook_pairs_multi(jobs, 17, seg, st) == N.PBN_ERR_ARG
    assert lib.pbn_rulebook_pairs_multi(jobs, 16, 0, st) == N.PBN_ERR_ARG
    assert lib.pbn_rulebook_pairs_multi(None, 1, seg, st) == N.PBN_ERR_ARG
    for field in ("nbr", "table", "totals", "seg_begin", "in_idx", "out_idx", "seg_offset"):
        keep = getattr(jobs[15], field)
        setattr(jobs[15], field, None)
        assert lib.pbn_rulebook_pairs_multi(jobs, 16, seg, st) == N.PBN_ERR_ARG, field
        setattr(jobs[15], field, keep)
    torch.cuda.synchronize()
    assert all(g.untouched() for l in many for g in l.all())
    assert lib.pbn_rulebook_pairs_multi(jobs, 16, seg, st) == N.PBN_OK      # the same table, whole: accepted
    torch.cuda.synchronize()
    want = PM.reference_multi(PC.case("K_k1")["nbr"], seg)
    assert all(PM.same(l.result(), want) for l in many[:16]) and all(g.untouched() for g in many[16].all())
