"""GPU tier: the device-side control flow of the inference forward, entry point by entry point, against tests/plan_ref.py
(plain host references, anchored by tests/test_plan_ref_cpu.py):
  csrc/plan.hip     pbn_class_gate, pbn_local_plan, pbn_proposal_offsets, pbn_batch_starts
  csrc/front.hip    pbn_local_scene_rows, pbn_gather_pad_rows, pbn_mask_count, pbn_proposal_rows
  csrc/heads.hip    pbn_mlp_rows (each with a device count against its size-exact call, NULL count, on the first
                    min(n, cap) rows)
No model, no scene generator: every input is built here from a fixed seed, at the sizes where the kernels change path (a
second chunk of a scan, more clusters than lanes, counts at and beyond a capacity).  Every comparison is exact: integers
with array_equal, floats bit for bit.  Every output lies inside a larger buffer filled with a byte pattern that must
survive outside the documented extent.  Each case asserts on the reference side that it reaches the path it is named for."""
import ctypes

import numpy as np
import pytest
import torch

import plan_ref as R
from pbnet_amd import _native as N
from pbnet_amd import stage_ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
VP = ctypes.c_void_p
_DT = {torch.float32: 0, torch.bfloat16: 1, torch.float16: 2}
PAT = 0x5A


# ---- guarded buffers --------------------------------------------------------------------------------------------------------
def _pattern(n_elems, dtype):
    es = torch.empty(0, dtype=dtype).element_size()
    return torch.full((int(n_elems) * es,), PAT, dtype=torch.uint8, device=DEV).view(dtype)


def _is_pattern(t):
    return bool((t.contiguous().view(-1).view(torch.uint8) == PAT).all().item())


class Guarded(object):
    """n elements of `dtype` between two margins, everything filled with the byte pattern; kernels get the address of the
    body.  64 elements of margin keep the 16-byte alignment some kernels ask of their outputs."""

    def __init__(self, n_elems, dtype, margin=64):
        self.n, self.m, self.es = int(n_elems), margin, torch.empty(0, dtype=dtype).element_size()
        self.buf = _pattern(self.n + 2 * margin, dtype)

    @property
    def ptr(self):
        return VP(self.buf.data_ptr() + self.m * self.es)

    @property
    def body(self):
        return self.buf[self.m:self.m + self.n]

    def margins_intact(self):
        return _is_pattern(self.buf[:self.m]) and _is_pattern(self.buf[self.m + self.n:])

    def untouched_from(self, k):
        """The body from element k on still holds the pattern (and so do the margins)."""
        return self.margins_intact() and _is_pattern(self.body[int(k):])


def _dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a), dtype=dtype)).to(DEV)


def _counts(**kw):
    c = torch.zeros(R.CNT_WORDS, dtype=torch.int32)
    for k, v in kw.items():
        c[getattr(R, "CNT_" + k)] = v
    return c.to(DEV)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


# =============================================================================================================================
# pbn_class_gate
# =============================================================================================================================
def _run_gate(table, thr05, nb, m_cap, n_points, overflow_before=0):
    n_cls = table.shape[0]
    cb, sl = Guarded(n_cls, torch.int32), Guarded((n_cls - 2) * nb, torch.int32)
    counts = _counts(OVERFLOW=overflow_before)
    table_d, thr_d = _dev(table, np.int32), _dev(thr05, np.float32)
    rc = N.lib().pbn_class_gate(N.ptr(table_d), N.ptr(thr_d), n_cls, nb, int(m_cap), int(n_points), cb.ptr, sl.ptr,
                                N.ptr(counts), N.current_stream())
    assert rc == 0
    torch.cuda.synchronize()
    assert cb.margins_intact() and sl.margins_intact()
    return cb.body.cpu().numpy(), sl.body.cpu().numpy(), counts.cpu().numpy()


def _check_gate(table, thr05, nb, m_cap, n_points, overflow_before=0):
    want = R.class_gate(table, thr05, nb, m_cap, n_points)
    cb, sl, counts = _run_gate(table, thr05, nb, m_cap, n_points, overflow_before)
    assert np.array_equal(cb, want["class_base"])
    assert np.array_equal(sl, want["seg_len"])
    exp = np.zeros(R.CNT_WORDS, dtype=np.int32)
    exp[R.CNT_POINTS], exp[R.CNT_OVERFLOW] = want["points"], want["flags"] | overflow_before
    assert np.array_equal(counts, exp)
    return want


def _gate_table(rng, n_cls, nb):
    """Random populations around random gates; class `ce` stands exactly AT its gate, classes 0 and 1 are huge."""
    thr = np.concatenate([[-1.0, -1.0], rng.uniform(30, 300, n_cls - 2)]).astype(np.float32)
    table = rng.integers(0, 400 // nb + 2, (n_cls, nb))
    table[0], table[1] = 100000, 70000
    ce = 2 + (n_cls - 2) // 2
    thr[ce] = np.float32(8 * nb + 3)                              # an integer: a population can equal it
    table[ce] = 8
    table[ce, nb - 1] += 3
    return table, thr, ce


@pytest.mark.parametrize("nb", [1, 3, 8])
@pytest.mark.parametrize("n_cls", [3, 20, 64])
def test_class_gate(n_cls, nb):
    rng = np.random.default_rng(100 * n_cls + nb)
    table, thr, ce = _gate_table(rng, n_cls, nb)
    n_points = int(table.sum())
    big = 2 ** 30
    want = _check_gate(table, thr, nb, big, n_points)
    assert want["flags"] == 0 and want["class_base"][ce] >= 0     # a population equal to the gate is kept
    assert want["class_base"][0] == want["class_base"][1] == -1   # never grouped, however large
    if n_cls > 3:
        assert (want["class_base"][2:] >= 0).any() and (want["class_base"][2:] < 0).any()
    m = want["points"]
    # one point fewer: below the gate, dropped
    t2 = table.copy()
    t2[ce, 0] -= 1
    w2 = _check_gate(t2, thr, nb, big, n_points - 1)
    assert w2["flags"] == 0 and w2["class_base"][ce] == -1 and w2["points"] == m - int(table[ce].sum())
    # the capacity: m == m_cap is fine, one slot fewer is not
    assert _check_gate(table, thr, nb, m, n_points)["flags"] == 0
    w3 = _check_gate(table, thr, nb, m - 1, n_points)
    assert w3["flags"] == R.OVF_POINTS and w3["points"] == 0 and (w3["class_base"] == -1).all() and not w3["seg_len"].any()
    # a table that does not account for every point (a batch index outside [0, nb))
    for wrong in (n_points + 1, n_points - 1):
        w4 = _check_gate(table, thr, nb, big, wrong)
        assert w4["flags"] == R.OVF_BATCH and w4["points"] == 0 and (w4["class_base"] == -1).all() and not w4["seg_len"].any()
    # both at once, on top of a flag raised earlier in the forward
    w5 = _check_gate(table, thr, nb, m - 1, n_points + 1, overflow_before=R.OVF_LEVEL)
    assert w5["flags"] == R.OVF_BATCH | R.OVF_POINTS


def test_class_gate_compares_in_float32():
    """(float)count < thr: a population of 2^24 + 1 converts to 2^24 and is NOT below a gate of 2^24."""
    nb, n_cls = 2, 4
    table = np.asarray([[0, 0], [0, 0], [2 ** 24, 1], [2 ** 24 - 1, 0]])
    thr = np.asarray([-1, -1, 2.0 ** 24, 2.0 ** 24], dtype=np.float32)
    want = _check_gate(table, thr, nb, 2 ** 30, int(table.sum()))
    assert list(want["class_base"]) == [-1, -1, 0, -1]


# =============================================================================================================================
# pbn_local_plan
# =============================================================================================================================
def _plan_inputs(rng, cluster_num, n_cls, nb, big_frac=0.35, kmax=None, thr=None):
    cluster_num = np.asarray(cluster_num, dtype=np.int64)
    assert len(cluster_num) == (n_cls - 2) * nb
    C = int(cluster_num.sum())
    thr02 = np.concatenate([[-1, -1], rng.integers(20, 60, n_cls - 2)]).astype(np.float32) if thr is None else thr
    if kmax is None:
        kmax = np.concatenate([[0, 0], rng.choice([1, 3, 6, 9], n_cls - 2)])
    sizes = rng.integers(1, 20, C)
    sizes[rng.random(C) < big_frac] += 60                         # above every gate
    member_start = np.concatenate([[0], np.cumsum(sizes)])
    centers = rng.normal(0, 2, (C, 3)).astype(np.float32)
    return dict(cluster_num=cluster_num, nb=nb, member_start=member_start, centers=centers, thr02=thr02,
                kmax=np.asarray(kmax, dtype=np.int32))


def _run_plan(inp, c_cap, e_cap, r_cap, n_clusters=None, overflow_before=0):
    lib = N.lib()
    C = int(inp["cluster_num"].sum())
    n_clusters = C if n_clusters is None else n_clusters
    wsb = int(lib.pbn_local_plan_workspace_bytes(int(c_cap)))
    out = dict(ent_row_start=Guarded(e_cap + 1, torch.int32), ent_member_start=Guarded(e_cap, torch.int32),
               ent_scene=Guarded(e_cap, torch.int32), ent_weight=Guarded(e_cap, torch.float32),
               workspace=Guarded(wsb, torch.uint8, margin=256))
    counts = _counts(OVERFLOW=overflow_before)
    keep = [_dev(inp["cluster_num"], np.int32), _dev(inp["member_start"], np.int32), _dev(inp["centers"].reshape(-1), np.float32),
            _dev([n_clusters], np.int32), _dev(inp["thr02"], np.float32), _dev(inp["kmax"], np.int32)]
    rc = lib.pbn_local_plan(N.ptr(keep[0]), len(inp["cluster_num"]), inp["nb"], N.ptr(keep[1]), N.ptr(keep[2]), N.ptr(keep[3]),
                            N.ptr(keep[4]), N.ptr(keep[5]), int(c_cap), int(e_cap), int(r_cap), out["ent_row_start"].ptr,
                            out["ent_member_start"].ptr, out["ent_scene"].ptr, out["ent_weight"].ptr, N.ptr(counts),
                            out["workspace"].ptr, wsb, N.current_stream())
    assert rc == 0
    torch.cuda.synchronize()
    return out, counts.cpu().numpy()


def _check_plan(inp, c_cap=None, e_cap=None, r_cap=2 ** 31 - 1, n_clusters=None, overflow_before=0):
    C = int(inp["cluster_num"].sum())
    c_cap = C if c_cap is None else c_cap
    e_cap = 7 * max(c_cap, 1) if e_cap is None else e_cap
    want = R.local_plan(inp["cluster_num"], inp["nb"], inp["member_start"], inp["centers"], inp["thr02"], inp["kmax"], c_cap,
                        e_cap, r_cap, n_clusters=n_clusters)
    got, counts = _run_plan(inp, c_cap, e_cap, r_cap, n_clusters, overflow_before)
    exp = np.zeros(R.CNT_WORDS, dtype=np.int32)
    for k, v in want["counts"].items():
        exp[getattr(R, "CNT_" + k)] = v
    exp[R.CNT_OVERFLOW] = want["flags"] | overflow_before
    assert np.array_equal(counts, exp), (counts[:8], exp[:8])
    for name in ("ent_row_start", "ent_member_start", "ent_scene"):
        k = len(want[name])
        assert np.array_equal(got[name].body[:k].cpu().numpy(), want[name]), name
        assert got[name].untouched_from(k), name
    k = len(want["ent_weight"])
    assert np.array_equal(_bits(got["ent_weight"].body[:k].cpu().numpy()), _bits(want["ent_weight"]))
    assert got["ent_weight"].untouched_from(k)
    assert got["workspace"].margins_intact()
    return want


def test_local_plan_segment_lookup_beyond_64_segments():
    """nb = 8, 18 grouped classes: 144 (class, batch) segments; clusters in segments 63, 64 and 143 only."""
    rng = np.random.default_rng(11)
    n_cls, nb = 20, 8
    cluster_num = np.zeros((n_cls - 2) * nb, dtype=np.int64)
    cluster_num[63], cluster_num[64], cluster_num[143] = 5, 7, 4
    inp = _plan_inputs(rng, cluster_num, n_cls, nb, big_frac=1.0, kmax=[0, 0] + [6] * 18)
    assert len(cluster_num) > 64 and cluster_num[:63].sum() == 0 and cluster_num[65:143].sum() == 0
    want = _check_plan(inp)
    assert want["flags"] == 0
    assert [len(s[0]) for s in want["scenes"]] == [5] * 5 + [7] * 7 + [4] * 4
    # every neighbour lies in the scene's own segment
    for c, (ids, _) in enumerate(want["scenes"]):
        lo, hi = (0, 5) if c < 5 else (5, 12) if c < 12 else (12, 16)
        assert all(lo <= i < hi for i in ids)


def test_local_plan_every_segment_populated_nb8():
    rng = np.random.default_rng(12)
    n_cls, nb = 20, 8
    cluster_num = rng.integers(0, 9, (n_cls - 2) * nb)
    cluster_num[[0, 63, 64, 127, 128, 143]] = [3, 2, 6, 1, 4, 5]
    inp = _plan_inputs(rng, cluster_num, n_cls, nb, big_frac=0.6)
    assert len(cluster_num) > 128 and int(cluster_num.sum()) > 256
    want = _check_plan(inp)
    assert want["flags"] == 0 and want["counts"]["ENTRIES"] > 256


@pytest.mark.parametrize("C", [1, 255, 256, 257, 3001])
def test_local_plan_pack_chunks(C):
    """k_plan_pack scans scenes and entries in chunks of 256 with carries."""
    rng = np.random.default_rng(C)
    n_cls, nb = 20, 3
    n_seg = (n_cls - 2) * nb
    cluster_num = np.bincount(rng.integers(0, n_seg, C), minlength=n_seg) if C > 1 else np.eye(1, n_seg, 17, dtype=np.int64)[0]
    inp = _plan_inputs(rng, cluster_num, n_cls, nb, big_frac=0.5)
    want = _check_plan(inp)
    assert want["counts"]["CLUSTERS"] == C == want["counts"]["SCENES"]
    if C == 1:
        assert want["counts"]["ENTRIES"] == 1 and want["flags"] == 0
    else:
        assert want["counts"]["ENTRIES"] > 256
    if C == 3001:
        assert C > 256 * 11 and want["counts"]["ENTRIES"] > 256 * 20 and max(cluster_num) > 64
        assert want["flags"] == R.OVF_CDIST
    elif C > 1:
        assert max(cluster_num) <= 25 and want["flags"] == 0


@pytest.mark.parametrize("cb,flag", [(25, 0), (26, R.OVF_CDIST), (70, R.OVF_CDIST), (200, R.OVF_CDIST)])
def test_local_plan_large_segments(cb, flag):
    """More clusters than lanes in one segment (the distance walk strides 64); above 25 the plan is written AND flagged."""
    rng = np.random.default_rng(cb)
    n_cls, nb = 6, 3
    cluster_num = [3, 0, 4, 0, cb, 2, 0, 0, 5, 1, 0, 6]
    inp = _plan_inputs(rng, cluster_num, n_cls, nb, big_frac=0.5, kmax=[0, 0, 6, 6, 6, 6])
    first = 7
    inp["member_start"] = np.concatenate([[0], np.cumsum(np.where(np.arange(sum(cluster_num)) % 2 == 0, 80, 5))])
    want = _check_plan(inp)
    assert max(cluster_num) == cb and want["flags"] == flag
    assert len(want["scenes"][first + cb - 1][0]) == 7 or len(want["scenes"][first + cb - 2][0]) == 7
    if cb > 64:
        # a neighbour found beyond the first 64 clusters of the segment, and one scene whose own index is beyond them
        assert any(i >= first + 64 for ids, _ in want["scenes"][first:first + 64] for i in ids[1:])
        assert any(len(ids) == 7 for ids, _ in want["scenes"][first + 64:first + cb])


def test_local_plan_large_segment_not_flagged_without_a_large_cluster():
    rng = np.random.default_rng(5)
    inp = _plan_inputs(rng, [40, 3, 0], 3, 3, big_frac=0.0, kmax=[0, 0, 6])
    want = _check_plan(inp)
    assert want["flags"] == 0 and all(len(s[0]) == 1 for s in want["scenes"])


def test_local_plan_segment_beyond_lds():
    """2049 clusters in one segment: its large cluster keeps a single entry and raises PBN_OVF_SEGMENT."""
    rng = np.random.default_rng(6)
    n_cls, nb = 4, 2
    cluster_num = [3, 2049, 0, 30]
    inp = _plan_inputs(rng, cluster_num, n_cls, nb, big_frac=0.0, kmax=[0, 0, 6, 6])
    sizes = np.diff(inp["member_start"])
    sizes[[1, 3 + 1000, 3 + 2049 + 4]] = 90                        # one large cluster per populated segment
    inp["member_start"] = np.concatenate([[0], np.cumsum(sizes)])
    want = _check_plan(inp)
    assert max(cluster_num) > R.SEG_CLUSTERS and want["flags"] == R.OVF_SEGMENT | R.OVF_CDIST
    assert want["scenes"][3 + 1000][0] == [3 + 1000]
    assert len(want["scenes"][1][0]) == 3 and len(want["scenes"][3 + 2049 + 4][0]) == 7
    # exactly 2048 clusters are ranked
    cluster_num = [3, 2048, 0, 30]
    inp = _plan_inputs(rng, cluster_num, n_cls, nb, big_frac=0.0, kmax=[0, 0, 6, 6])
    sizes = np.diff(inp["member_start"])
    sizes[[3 + 5, 3 + 2047]] = 90
    inp["member_start"] = np.concatenate([[0], np.cumsum(sizes)])
    want = _check_plan(inp)
    assert want["flags"] == R.OVF_CDIST and len(want["scenes"][3 + 2047][0]) == 7


def test_local_plan_para_k():
    """para_k = min(C_b - 1, kmax[cls], 6): single-cluster segments, kmax in {0, 1, 6, 9}, segments smaller than kmax."""
    rng = np.random.default_rng(7)
    n_cls, nb = 6, 2
    kmax = [0, 0, 0, 1, 6, 9]
    cluster_num = [12, 1, 12, 1, 12, 3, 12, 1]
    inp = _plan_inputs(rng, cluster_num, n_cls, nb, big_frac=1.0, kmax=kmax)
    want = _check_plan(inp)
    lens = [len(s[0]) for s in want["scenes"]]
    assert lens == [1] * 12 + [1] + [2] * 12 + [1] + [7] * 12 + [3] * 3 + [7] * 12 + [1]
    assert want["flags"] == 0
    w2 = want["scenes"][13][1]
    assert [float(v) for v in w2] == [1.0, 0.5]
    w7 = want["scenes"][30][1]
    assert _bits(w7).tolist() == _bits([1.0] + [0.5 * (7 - i) / 7 for i in range(6)]).tolist()


def test_local_plan_size_gate_is_strict():
    """A cluster of exactly thr02 points is not large; one point more is.  Gates that are no integers as well."""
    rng = np.random.default_rng(8)
    n_cls, nb = 5, 1
    thr = np.asarray([-1, -1, 50.0, 460.6, 2.0 ** 24], dtype=np.float32)
    inp = _plan_inputs(rng, [4, 4, 3], n_cls, nb, big_frac=0.0, kmax=[0, 0, 6, 6, 6], thr=thr)
    sizes = np.asarray([50, 51, 49, 5, 460, 461, 5, 5, 2 ** 24, 2 ** 24 + 2, 5])
    inp["member_start"] = np.concatenate([[0], np.cumsum(sizes)])
    assert int(inp["member_start"][-1]) < 2 ** 31
    want = _check_plan(inp)
    assert [len(s[0]) for s in want["scenes"]] == [1, 4, 1, 1, 1, 4, 1, 1, 1, 3, 1]


_TIE_CENTERS = np.asarray([[1, 0, 0], [0, 1, 0], [0, 2, 0], [0, 0, 0], [-2, 0, 0], [0, 0, -1], [3, 3, 3]], dtype=np.float32)


@pytest.mark.parametrize("k", [1, 2, 4, 6])
def test_local_plan_ties_take_the_lower_id(k):
    """From cluster 3: clusters 0, 1, 5 at d^2 = 1 and 2, 4 at d^2 = 4."""
    rng = np.random.default_rng(k)
    inp = _plan_inputs(rng, [7], 3, 1, big_frac=1.0, kmax=[0, 0, k])
    inp["centers"] = _TIE_CENTERS.copy()
    want = _check_plan(inp)
    assert want["scenes"][3][0] == [3, 0, 1, 5, 2, 4, 6][:k + 1]


@pytest.mark.parametrize("shape", [(2, 3, 4), (5, 5, 8), (3, 3, 30)])
def test_local_plan_ties_on_a_lattice(shape):
    """Every point of a lattice of multiples of 1/4, in shuffled order: each query has whole shells of equidistant clusters, among
    them clusters that different lanes (and, beyond 64, different strides of one lane) hold."""
    rng = np.random.default_rng(sum(shape))
    cb = int(np.prod(shape))
    pts = np.stack(np.meshgrid(*[np.arange(s) for s in shape], indexing="ij"), -1).reshape(-1, 3).astype(np.float32) / 4
    n_cls, nb = 4, 2
    inp = _plan_inputs(rng, [cb, 0, 3, cb], n_cls, nb, big_frac=1.0, kmax=[0, 0, 6, 6])
    inp["centers"] = np.concatenate([pts[rng.permutation(cb)], rng.normal(0, 1, (3, 3)).astype(np.float32),
                                     pts[rng.permutation(cb)] * np.float32(4)])
    want = _check_plan(inp)
    # the case is about ties: the 6th and the 7th nearest of some query are at the same distance, so is a pair inside the plan
    ties_in, ties_at_cut = 0, 0
    for c in range(cb):
        d = sorted(float(R.dist2_f32(inp["centers"][c], inp["centers"][o])) for o in range(cb) if o != c)
        ties_in += d[0] == d[1]
        ties_at_cut += d[5] == d[6]
    assert ties_in > 0 and ties_at_cut > 0
    assert want["flags"] == (R.OVF_CDIST if cb > 25 else 0)


def test_local_plan_more_clusters_than_capacity():
    rng = np.random.default_rng(21)
    n_cls, nb = 20, 3
    cluster_num = rng.integers(3, 14, (n_cls - 2) * nb)
    inp = _plan_inputs(rng, cluster_num, n_cls, nb, big_frac=0.5)
    C = int(cluster_num.sum())
    full = _check_plan(inp)
    assert C > 300
    for c_cap in (C - 1, 300, 256, 1):
        want = _check_plan(inp, c_cap=c_cap, e_cap=7 * C)
        assert want["flags"] == R.OVF_CLUSTERS and want["counts"]["SCENES"] == want["counts"]["CLUSTERS"] == c_cap
        assert want["scenes"] == full["scenes"][:c_cap]
    # a scene below the capacity keeps neighbours beyond it
    assert any(i >= 256 for ids, _ in full["scenes"][:256] for i in ids)
    # a capacity above the count changes nothing
    assert _check_plan(inp, c_cap=C + 100, e_cap=7 * C)["flags"] == 0


def test_local_plan_entry_and_row_capacities():
    rng = np.random.default_rng(22)
    n_cls, nb = 20, 3
    cluster_num = rng.integers(3, 14, (n_cls - 2) * nb)
    inp = _plan_inputs(rng, cluster_num, n_cls, nb, big_frac=0.5)
    C = int(cluster_num.sum())
    full = _check_plan(inp)
    n_ent, rows = full["counts"]["ENTRIES"], full["counts"]["ROWS"]
    assert n_ent > 512 and full["flags"] == 0
    # entries: exactly the capacity is fine; one fewer drops the plan (and writes ent_row_start[0] = 0, nothing else)
    assert _check_plan(inp, e_cap=n_ent)["flags"] == 0
    for e_cap in (n_ent - 1, 256, 1):
        want = _check_plan(inp, e_cap=e_cap, overflow_before=R.OVF_LEVEL)
        assert want["flags"] == R.OVF_ENTRIES and len(want["ent_row_start"]) == 1 and want["ent_row_start"][0] == 0
        assert want["counts"] == {"ENTRIES": 0, "ROWS": 0, "SCENES": 0, "CLUSTERS": C}
    # rows: the same; the entry arrays are written all the same
    assert _check_plan(inp, e_cap=n_ent, r_cap=rows)["flags"] == 0
    for r_cap in (rows - 1, 1):
        want = _check_plan(inp, e_cap=n_ent, r_cap=r_cap)
        assert want["flags"] == R.OVF_ROWS and len(want["ent_row_start"]) == n_ent + 1
        assert want["counts"] == {"ENTRIES": 0, "ROWS": 0, "SCENES": 0, "CLUSTERS": C}
    # clusters and entries at once
    want = _check_plan(inp, c_cap=C - 5, e_cap=64)
    assert want["flags"] == R.OVF_CLUSTERS | R.OVF_ENTRIES and want["counts"]["CLUSTERS"] == C - 5


# =============================================================================================================================
# pbn_proposal_offsets
# =============================================================================================================================
def _run_offsets(per_scene, n_scenes_dev, s_cap):
    po, al, de = Guarded(s_cap + 1, torch.int64), Guarded(s_cap, torch.int64), Guarded(s_cap, torch.int32)
    counts = _counts(SCENES=n_scenes_dev, ROWS=12345, OVERFLOW=R.OVF_LEVEL)
    per = _dev(per_scene, np.int32)
    assert per.numel() >= min(n_scenes_dev, s_cap)
    rc = N.lib().pbn_proposal_offsets(N.ptr(per), int(s_cap), po.ptr, al.ptr, de.ptr, N.ptr(counts), N.current_stream())
    assert rc == 0
    return po, al, de, counts


def _check_offsets(per_scene, n_scenes_dev, s_cap, got=None):
    off, alive, dense, n_prop, n_rows = R.proposal_offsets(per_scene, n_scenes_dev, s_cap)
    po, al, de, counts = got if got is not None else _run_offsets(per_scene, n_scenes_dev, s_cap)
    torch.cuda.synchronize()
    assert np.array_equal(po.body[:n_prop + 1].cpu().numpy(), off) and po.untouched_from(n_prop + 1)
    assert np.array_equal(al.body[:n_prop].cpu().numpy(), alive) and al.untouched_from(n_prop)
    assert np.array_equal(de.body[:len(dense)].cpu().numpy(), dense) and de.untouched_from(len(dense))
    exp = np.zeros(R.CNT_WORDS, dtype=np.int32)
    exp[R.CNT_SCENES], exp[R.CNT_ROWS], exp[R.CNT_OVERFLOW] = n_scenes_dev, 12345, R.OVF_LEVEL
    exp[R.CNT_PROPOSALS], exp[R.CNT_PROPOSAL_ROWS] = n_prop, n_rows
    assert np.array_equal(counts.cpu().numpy(), exp)
    return n_prop, n_rows


def _per_scene(rng, S, mode):
    per = rng.integers(1, 700, S)
    if mode == "dead":
        per[:] = 0
    elif mode == "alternate":
        per[(S % 2)::2] = 0
    elif mode == "random":
        per[rng.random(S) < 0.4] = 0
    return per


@pytest.mark.parametrize("mode", ["dead", "alive", "alternate", "random"])
@pytest.mark.parametrize("S", [1, 256, 257, 1000])
def test_proposal_offsets(S, mode):
    rng = np.random.default_rng(S)
    per = _per_scene(rng, S, mode)
    for s_cap in (S, S + 300):
        n_prop, n_rows = _check_offsets(per, S, s_cap)
        assert n_rows == int(per.sum()) and n_prop == int((per > 0).sum())
        assert n_prop == {"dead": 0, "alive": S}.get(mode, n_prop)
    if S == 1000:
        assert S > 3 * 256 and (mode == "dead" or n_rows > 2 ** 16)


def test_proposal_offsets_scene_count_beyond_capacity():
    rng = np.random.default_rng(31)
    per = _per_scene(rng, 600, "random")
    for n_scenes_dev, s_cap in ((605, 600), (600, 300), (2 ** 30, 257), (0, 600)):
        n_prop, _ = _check_offsets(per, n_scenes_dev, s_cap)
        assert n_prop == int((per[:min(n_scenes_dev, s_cap)] > 0).sum())


def test_proposal_offsets_back_to_back():
    """Many launches in a row, every one checked: both scans of every chunk go through the same shared words, so a chunk that
    starts before the previous one was read out shows as a wrong carry in one of them."""
    rng = np.random.default_rng(32)
    S = 1000
    runs = []
    for i in range(40):
        per = _per_scene(rng, S, "random" if i % 2 else "alive")
        runs.append((per, _run_offsets(per, S, S)))
    assert S > 3 * 256
    for per, got in runs:
        _check_offsets(per, S, S, got=got)


# =============================================================================================================================
# pbn_batch_starts
# =============================================================================================================================
def _check_batch_starts(batch, n_dev, n_cap, n_seg, rng):
    """batch: the (sorted) batch index of the first min(n_dev, n_cap) rows; the rows beyond them, up to n_cap, hold indices
    that would break the order if they were read."""
    n = n_cap if n_dev is None else min(n_dev, n_cap)
    coords = rng.integers(-500, 500, (max(n_cap, 1), 4))
    coords[:n, 0] = batch[:n]
    coords[n:, 0] = rng.integers(-3, 2, max(n_cap, 1) - n)
    out = Guarded(n_seg + 1, torch.int32)
    cd = _dev(coords, np.int32)
    nd = None if n_dev is None else _dev([n_dev], np.int32)
    rc = N.lib().pbn_batch_starts(N.ptr(cd), N.ptr(nd), int(n_cap), int(n_seg), out.ptr, N.current_stream())
    assert rc == 0
    torch.cuda.synchronize()
    want = R.batch_starts(coords[:, 0], n_cap if n_dev is None else n_dev, n_seg, n_cap)
    assert np.array_equal(out.body.cpu().numpy(), want) and out.margins_intact()
    return want


@pytest.mark.parametrize("n_seg", [0, 1, 9, 300])
def test_batch_starts(n_seg):
    rng = np.random.default_rng(40 + n_seg)
    # batch indices missing at the front (0), in the middle (every 5th) and at the end (the last three)
    present = [b for b in range(1, max(n_seg - 3, 2)) if b % 5 != 3]
    n_cap = 900
    batch = np.sort(rng.choice(present, n_cap))
    want = _check_batch_starts(batch, None, n_cap, n_seg, rng)                      # n_dev NULL: all n_cap rows
    assert want[0] == 0 and want[-1] == (n_cap if n_seg >= max(present) + 1 else want[-1])
    if n_seg >= 9:
        assert want[1] == 0 and want[3] == want[4] and want[n_seg] == want[n_seg - 1] == want[n_seg - 2] == n_cap
        assert len(set(want.tolist())) > 4
    for n_dev in (0, 1, n_cap - 1, n_cap, n_cap + 5, 2 ** 30):
        want = _check_batch_starts(batch, n_dev, n_cap, n_seg, rng)
        assert want.max() <= min(n_dev, n_cap)
        if n_dev == 0:
            assert not want.any()


def test_batch_starts_single_batch_and_many_rows():
    rng = np.random.default_rng(49)
    _check_batch_starts(np.zeros(5000, dtype=np.int64), 4000, 5000, 3, rng)
    _check_batch_starts(np.full(5000, 2), 5000, 5000, 3, rng)
    _check_batch_starts(np.sort(rng.integers(0, 40, 70000)), 65537, 70000, 40, rng)


# =============================================================================================================================
# the `_dev` forms of the stage kernels
# =============================================================================================================================
def _ns(cap):
    """Device-side counts around a capacity."""
    return [0, 1, cap - 1, cap, cap + 5]


def _local_scene_case(rng, dtype):
    n_points, m, n_clusters, c = 5000, 3000, 37, 32
    sizes = rng.integers(1, 120, n_clusters)
    sizes[5] = 700
    member_start = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    member_idx = rng.integers(0, m, int(member_start[-1])).astype(np.int32)
    ins_ind = rng.permutation(n_points)[:m].astype(np.int64)
    xyz = rng.uniform(-3, 6, (n_points, 3)).astype(np.float32)
    point_feat = torch.from_numpy(rng.normal(0, 1, (n_points, c)).astype(np.float32)).to(dtype)
    sem_prob = torch.from_numpy(rng.uniform(0.1, 1, (n_points, 1)).astype(np.float32)).to(dtype)
    ent_cluster, ent_weight, ent_scene = [], [], []
    for s in range(23):
        for j in range(int(rng.integers(1, 5))):
            ent_cluster.append(int(rng.integers(0, n_clusters)))
            ent_weight.append(1.0 if j == 0 else float(R.entry_weight(4, j)))
            ent_scene.append(s)
    ec = np.asarray(ent_cluster)
    row_start = np.concatenate([[0], np.cumsum(sizes[ec])]).astype(np.int32)
    return dict(member_idx=member_idx, ins_ind=ins_ind, xyz=xyz, point_feat=point_feat, sem_prob=sem_prob,
                row_start=row_start, ent_member=member_start[:-1][ec], ent_scene=np.asarray(ent_scene, dtype=np.int32),
                ent_weight=np.asarray(ent_weight, dtype=np.float32), E=len(ec), Rw=int(row_start[-1]), c=c)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_local_scene_rows_dev(dtype):
    rng = np.random.default_rng(51)
    k = _local_scene_case(rng, dtype)
    E, Rw, c = k["E"], k["Rw"], k["c"]
    assert 2000 < Rw < 20000
    voxel = 0.02
    d = dict(rs=_dev(k["row_start"], np.int32), em=_dev(k["ent_member"], np.int32), es=_dev(k["ent_scene"], np.int32),
             ew=_dev(k["ent_weight"], np.float32), mi=_dev(k["member_idx"], np.int32), ii=_dev(k["ins_ind"], np.int64),
             xyz=_dev(k["xyz"], np.float32), pf=k["point_feat"].to(DEV), sp=k["sem_prob"].to(DEV))
    # the size-exact sibling on all rows
    packed = torch.cat([d["rs"], d["em"], d["es"], d["ew"].view(torch.int32)])
    e_idx, e_scene, e_coords, e_feat = stage_ops.local_scene_rows(packed, E, Rw, d["mi"], d["ii"], d["xyz"], voxel, d["pf"],
                                                                  d["sp"], None)
    if dtype == torch.float32:
        w_idx, w_scene, w_coords, w_feat = R.local_scene_rows(
            k["row_start"], k["ent_member"], k["ent_scene"], k["ent_weight"], E, Rw, k["member_idx"], k["ins_ind"], k["xyz"],
            stage_ops.reciprocal_f32(voxel), k["point_feat"].numpy(), k["sem_prob"].numpy()[:, 0])
        assert np.array_equal(e_idx.cpu().numpy(), w_idx) and np.array_equal(e_scene.cpu().numpy(), w_scene)
        assert np.array_equal(e_coords.cpu().numpy(), w_coords)
        assert np.array_equal(_bits(e_feat.cpu().numpy()), _bits(w_feat))
    ld = c + 2
    for n_rows in _ns(Rw):
        for n_ent in ((E, E + 5) if n_rows >= Rw else (E,)):
            pi, rsn, co, fe = (Guarded(Rw, torch.int64), Guarded(Rw, torch.int64), Guarded(Rw * 4, torch.int32),
                               Guarded(Rw * ld, dtype))
            cnt = _counts(ENTRIES=n_ent, ROWS=n_rows)
            rc = N.lib().pbn_local_scene_rows(
                N.ptr(d["rs"]), N.ptr(d["em"]), N.ptr(d["es"]), N.ptr(d["ew"]), E, Rw, VP(cnt.data_ptr() + 4 * R.CNT_ENTRIES),
                VP(cnt.data_ptr() + 4 * R.CNT_ROWS), N.ptr(d["mi"]), N.ptr(d["ii"]), N.ptr(d["xyz"]),
                stage_ops.reciprocal_f32(voxel), VP(d["pf"].data_ptr()), d["pf"].stride(0), c, VP(d["sp"].data_ptr()), 1, None,
                _DT[dtype], pi.ptr, rsn.ptr, co.ptr, fe.ptr, ld, N.current_stream())
            assert rc == 0
            torch.cuda.synchronize()
            kk = R.dev_rows(n_rows, Rw)
            assert torch.equal(pi.body[:kk], e_idx[:kk]) and pi.untouched_from(kk)
            assert torch.equal(rsn.body[:kk], e_scene[:kk]) and rsn.untouched_from(kk)
            assert torch.equal(co.body[:4 * kk].view(kk, 4), e_coords[:kk]) and co.untouched_from(4 * kk)
            assert torch.equal(fe.body[:ld * kk].view(torch.uint8), e_feat[:kk].contiguous().view(-1).view(torch.uint8))
            assert fe.untouched_from(ld * kk)


@pytest.mark.parametrize("two_level", [False, True])
def test_gather_pad_rows_dev(two_level):
    rng = np.random.default_rng(52)
    n_in, width, width_out, cap = 3000, 34, 40, 2500
    x = torch.from_numpy(rng.normal(0, 1, (n_in, width)).astype(np.float32)).to(torch.bfloat16).to(DEV)
    idx2 = _dev(rng.permutation(n_in), np.int64) if two_level else None
    idx = _dev(rng.integers(0, n_in, cap), np.int64)
    es = 2
    # the size-exact call (NULL count) with one index level: the second is resolved on the host side of the call
    flat = idx2[idx] if two_level else idx
    exact = torch.empty(cap, width_out, dtype=torch.bfloat16, device=DEV)
    rc = N.lib().pbn_gather_pad_rows(VP(x.data_ptr()), width * es, width * es, N.ptr(flat), None, cap, None,
                                     VP(exact.data_ptr()), width_out * es, N.current_stream())
    assert rc == 0
    want = R.gather_pad_rows(x.cpu().view(torch.int16).numpy(), idx.cpu().numpy(), None if idx2 is None else idx2.cpu().numpy(),
                             cap, width_out)
    assert np.array_equal(exact.cpu().view(torch.int16).numpy(), want)
    for n in _ns(cap) + [None]:
        out = Guarded(cap * width_out, torch.bfloat16)
        nd = None if n is None else _dev([n], np.int32)
        rc = N.lib().pbn_gather_pad_rows(VP(x.data_ptr()), width * es, width * es, N.ptr(idx), N.ptr(idx2), cap, N.ptr(nd),
                                         out.ptr, width_out * es, N.current_stream())
        assert rc == 0
        torch.cuda.synchronize()
        kk = R.dev_rows(n, cap)
        assert torch.equal(out.body[:kk * width_out].view(torch.int16), exact[:kk].view(-1).view(torch.int16))
        assert out.untouched_from(kk * width_out)


def _head(rng, hidden, n_out):
    f = lambda *s: _dev(rng.normal(0, 0.4, s), np.float32)
    return dict(w1=f(hidden, 32), scale=_dev(rng.uniform(0.5, 1.5, hidden), np.float32), shift=f(hidden),
                slope=_dev(np.full(hidden, 0.2), np.float32), w2=f(n_out, hidden), b2=f(n_out), hidden=hidden, n_out=n_out)


def _mlp_exact(h, x, idx_a, idx_b, n, sigmoid, dtype):
    out = torch.empty(max(n, 1), h["n_out"], dtype=dtype, device=DEV)
    rc = N.lib().pbn_mlp_rows(VP(x.data_ptr()), x.stride(0), -1, 32, N.ptr(idx_a), N.ptr(idx_b), int(n), None, N.ptr(h["w1"]),
                              N.ptr(h["scale"]), N.ptr(h["shift"]), N.ptr(h["slope"]), h["hidden"], N.ptr(h["w2"]), N.ptr(h["b2"]),
                              h["n_out"], int(sigmoid), VP(out.data_ptr()), h["n_out"], _DT[dtype], N.current_stream())
    assert rc == 0
    return out[:n]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("n_out,sigmoid,hidden", [(1, True, 16), (20, False, 16), (32, False, 32)])
def test_mlp_rows_dev(dtype, n_out, sigmoid, hidden):
    rng = np.random.default_rng(53 + n_out)
    in_rows, n_mid, cap = 3000, 2500, 4000
    h = _head(rng, hidden, n_out)
    x = torch.from_numpy(rng.normal(0, 1, (in_rows, 32)).astype(np.float32)).to(dtype).to(DEV)
    ia = rng.integers(0, n_mid, cap)
    ib = rng.permutation(in_rows)[:n_mid]
    ia[[0, 17, cap - 1]] = -1                                      # no row at all
    ib[[ia[3], ia[1000]]] = in_rows                                # a row just beyond the slab
    ib[ia[2000]] = in_rows + 12345
    zero_rows = np.nonzero((ia < 0) | (ib[np.maximum(ia, 0)] >= in_rows))[0]
    assert len(zero_rows) >= 6 and set([0, 3, 17, 1000, 2000, cap - 1]) <= set(zero_rows.tolist())
    idx_a = _dev(ia, np.int64)
    idx_b = _dev(ib, np.int64)
    # the sibling does not bound its rows: give it a slab whose row `in_rows` IS a row of zeros
    x_ext = torch.cat([x, torch.zeros(1, 32, dtype=dtype, device=DEV)])
    ib_ext = _dev(np.minimum(ib, in_rows), np.int64)
    exact = _mlp_exact(h, x_ext, idx_a, ib_ext, cap, sigmoid, dtype)
    # ... and such a row gives what the head makes of zeros
    of_zero = _mlp_exact(h, torch.zeros(1, 32, dtype=dtype, device=DEV), None, None, 1, sigmoid, dtype)
    assert all(torch.equal(exact[int(r)], of_zero[0]) for r in zero_rows)
    es = torch.empty(0, dtype=dtype).element_size()
    for n in _ns(cap) + [None]:
        out = Guarded(cap * n_out, dtype)
        nd = None if n is None else _dev([n], np.int32)
        rc = N.lib().pbn_mlp_rows(VP(x.data_ptr()), x.stride(0), in_rows, 32, N.ptr(idx_a), N.ptr(idx_b), cap, N.ptr(nd),
                                  N.ptr(h["w1"]), N.ptr(h["scale"]), N.ptr(h["shift"]), N.ptr(h["slope"]), hidden,
                                  N.ptr(h["w2"]), N.ptr(h["b2"]), n_out, int(sigmoid), out.ptr, n_out, _DT[dtype],
                                  N.current_stream())
        assert rc == 0
        torch.cuda.synchronize()
        kk = R.dev_rows(n, cap)
        # bit for bit the size-exact kernel on the same rows
        want = _mlp_exact(h, x_ext, idx_a, ib_ext, kk, sigmoid, dtype)
        assert torch.equal(want.reshape(-1).view(torch.uint8), exact[:kk].reshape(-1).view(torch.uint8))
        assert torch.equal(out.body[:kk * n_out].view(torch.uint8), want.reshape(-1).view(torch.uint8)), (n, es)
        assert out.untouched_from(kk * n_out)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_mask_count_offsets_proposal_rows_dev_chain(dtype):
    """pbn_mask_count -> pbn_proposal_offsets -> pbn_proposal_rows with device counts as the planned forward chains them: one counts block,
    the row count read from counts[ROWS], the scene count from counts[SCENES]."""
    rng = np.random.default_rng(54)
    lib = N.lib()
    n_scenes, s_cap, n_points, c = 41, 48, 9000, 32
    lens = rng.integers(0, 300, n_scenes)
    lens[3], lens[17] = 0, 2500
    row_scene_np = np.repeat(np.arange(n_scenes), lens).astype(np.int64)
    cap = len(row_scene_np)
    assert 3000 < cap < 20000
    score_np = rng.uniform(0, 1, cap).astype(np.float32)
    score_np[row_scene_np == 9] = 0.1                              # a scene that dies entirely
    score_np[100], score_np[101] = 0.45, np.nextafter(np.float32(0.45), np.float32(1))   # at the threshold: not kept; above: kept
    assert not (score_np[100] > np.float32(0.45)) and score_np[101] > np.float32(0.45)
    score = torch.from_numpy(score_np).to(dtype).to(DEV).view(-1, 1)
    score_host = score.float().cpu().numpy()[:, 0] if dtype != torch.float32 else score_np
    row_scene = _dev(row_scene_np, np.int64)
    point_idx_np = rng.integers(0, n_points, cap)
    point_idx = _dev(point_idx_np, np.int64)
    xyz_np = rng.uniform(-2, 6, (n_points, 3)).astype(np.float32)
    xyz = _dev(xyz_np, np.float32)
    feat = torch.from_numpy(rng.normal(0, 1, (n_points, c)).astype(np.float32)).to(dtype).to(DEV)
    thd, scale, voxel = 0.45, 1.0, 0.02
    n_blocks = int(lib.pbn_select_blocks(cap))
    for n in _ns(cap):
        kk = R.dev_rows(n, cap)
        counts = _counts(ROWS=n, SCENES=n_scenes, ENTRIES=77)
        cptr = counts.data_ptr()
        per, blk = Guarded(s_cap, torch.int32), Guarded(n_blocks, torch.int32)
        rc = lib.pbn_mask_count(VP(score.data_ptr()), 1, thd, N.ptr(row_scene), cap, VP(cptr + 4 * R.CNT_ROWS), s_cap,
                                _DT[dtype], per.ptr, blk.ptr, N.current_stream())
        assert rc == 0
        po, al, de = Guarded(s_cap + 1, torch.int64), Guarded(s_cap, torch.int64), Guarded(s_cap, torch.int32)
        rc = lib.pbn_proposal_offsets(per.ptr, s_cap, po.ptr, al.ptr, de.ptr, VP(cptr), N.current_stream())
        assert rc == 0
        pidx, pms, pco, pfe = (Guarded(cap * 2, torch.int64), Guarded(cap, dtype), Guarded(cap * 4, torch.int32),
                               Guarded(cap * c, dtype))
        rc = lib.pbn_proposal_rows(VP(score.data_ptr()), 1, thd, N.ptr(row_scene), N.ptr(point_idx), cap,
                                   VP(cptr + 4 * R.CNT_ROWS), de.ptr, blk.ptr, N.ptr(xyz), float(np.float32(scale)),
                                   stage_ops.reciprocal_f32(voxel), VP(feat.data_ptr()), feat.stride(0), c, _DT[dtype],
                                   pidx.ptr, pms.ptr, pco.ptr, pfe.ptr, N.current_stream())
        assert rc == 0
        torch.cuda.synchronize()
        # ---- the size-exact siblings on the first kk rows ----
        w_per, w_blk = R.mask_count(score_host, thd, row_scene_np, kk, s_cap, cap)
        if kk:
            e_per, e_blk = stage_ops.mask_count(score[:kk], thd, row_scene[:kk], n_scenes)
            assert np.array_equal(e_per.cpu().numpy(), w_per[:n_scenes])
        assert not w_per[n_scenes:].any()
        assert np.array_equal(per.body.cpu().numpy(), w_per) and per.margins_intact()
        assert np.array_equal(blk.body.cpu().numpy(), w_blk) and blk.margins_intact()
        if kk:
            assert np.array_equal(e_blk.cpu().numpy(), w_blk[:len(e_blk)]) and not w_blk[len(e_blk):].any()
        off, alive, dense, n_prop, n_rows = R.proposal_offsets(w_per, n_scenes, s_cap)
        assert np.array_equal(po.body[:n_prop + 1].cpu().numpy(), off) and po.untouched_from(n_prop + 1)
        assert np.array_equal(al.body[:n_prop].cpu().numpy(), alive) and al.untouched_from(n_prop)
        assert np.array_equal(de.body[:n_scenes].cpu().numpy(), dense) and de.untouched_from(n_scenes)
        exp = np.zeros(R.CNT_WORDS, dtype=np.int32)
        exp[R.CNT_ROWS], exp[R.CNT_SCENES], exp[R.CNT_ENTRIES] = n, n_scenes, 77
        exp[R.CNT_PROPOSALS], exp[R.CNT_PROPOSAL_ROWS] = n_prop, n_rows
        assert np.array_equal(counts.cpu().numpy(), exp)
        if kk > 200:
            assert n_prop < n_scenes and n_rows > 0 and n_rows == int((score_host[:kk] > np.float32(thd)).sum())
        if kk == 0:
            assert n_prop == 0 and n_rows == 0
            assert pidx.untouched_from(0) and pms.untouched_from(0) and pco.untouched_from(0) and pfe.untouched_from(0)
            continue
        e_idx, e_ms, e_co, e_fe = stage_ops.proposal_rows(score[:kk], thd, row_scene[:kk], point_idx[:kk], _dev(dense, np.int32),
                                                          e_blk, n_rows, xyz, scale, voxel, feat)
        assert torch.equal(pidx.body[:2 * n_rows].view(n_rows, 2), e_idx) and pidx.untouched_from(2 * n_rows)
        assert torch.equal(pms.body[:n_rows].view(torch.uint8), e_ms.view(torch.uint8)) and pms.untouched_from(n_rows)
        assert torch.equal(pco.body[:4 * n_rows].view(n_rows, 4), e_co) and pco.untouched_from(4 * n_rows)
        assert torch.equal(pfe.body[:c * n_rows].view(torch.uint8), e_fe.reshape(-1).view(torch.uint8))
        assert pfe.untouched_from(c * n_rows)
        if dtype == torch.float32:
            w_idx, w_ms, w_co, w_fe = R.proposal_rows(score_np, thd, row_scene_np, point_idx_np, kk, dense, xyz_np,
                                                      np.float32(scale), stage_ops.reciprocal_f32(voxel), feat.cpu().numpy())
            assert np.array_equal(e_idx.cpu().numpy(), w_idx) and np.array_equal(_bits(e_ms.cpu().numpy()), _bits(w_ms))
            assert np.array_equal(e_co.cpu().numpy(), w_co) and np.array_equal(_bits(e_fe.cpu().numpy()), _bits(w_fe))
