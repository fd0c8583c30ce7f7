"""Designed inputs for the seven entry points of csrc/augment.hip.  Every case is a dict of numpy inputs built from a fixed
seed plus `reaches`, a predicate evaluated on the REFERENCE side (tests/aug_ref.py) that asserts the case hits the path it
is named for; tests/test_aug_cases_cpu.py runs every predicate, tests/test_aug_entry_gpu.py runs the kernels on the same
inputs.  Shapes are the smallest at which each path exists: 8 rows per thread, 512 per wave, 2048 per chunk, 256 chunks per
scan tile, row sweeps of at most 256 blocks x 256 threads."""
import functools
from types import SimpleNamespace

import numpy as np

import aug_ref as R
from pbnet_amd.loader import ELASTIC, crop_levels

LEVELS = crop_levels(SimpleNamespace(scale_size=50))            # 512, 480, ..., 0 on x and y; 512 on z
assert LEVELS[16, 0] == 0.0 and LEVELS[1, 0] == 480.0
SWEEP = 256 * 256                                               # rows one grid-stride sweep of a unit covers


def _rot(rng):
    th = rng.uniform(0, 2 * np.pi)
    m = np.eye(3) + rng.standard_normal((3, 3)) * 0.1           # jitter
    m[0][0] *= -1 if rng.integers(0, 2) else 1
    return np.matmul(m, [[np.cos(th), np.sin(th), 0], [-np.sin(th), np.cos(th), 0], [0, 0, 1]])


# ---- affine ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def affine_case():
    rng = np.random.default_rng(101)
    sizes = [1, 7, 4 * SWEEP + 1025, 300, 1025, 4096]
    pre_min = [1, 0, 1, 0, 1, 0]
    has_scale = [1, 0, 0, 1, 1, 0]
    uoff = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    xyz = np.concatenate([(rng.uniform(0, 8, (n, 3)) + rng.uniform(-3, 3, 3)).astype(np.float32) for n in sizes])
    case = dict(xyz=xyz, uoff=uoff, pre_min=np.array(pre_min, np.int32), has_scale=np.array(has_scale, np.int32),
                mats=np.stack([_rot(rng) for _ in sizes]).reshape(-1, 9), scale=rng.uniform(0.95, 1.05, len(sizes)),
                max_rows=max(sizes))

    def reaches(c=case):
        n = np.diff(c["uoff"])
        assert n.max() > 4 * SWEEP and n.min() == 1 and (n < 1024).sum() >= 3       # a fifth sweep; whole blocks empty
        assert {(int(p), int(h)) for p, h in zip(c["pre_min"], c["has_scale"])} == {(0, 0), (0, 1), (1, 0), (1, 1)}
        differ = 0
        for u in np.nonzero(c["pre_min"])[0]:
            x = c["xyz"][c["uoff"][u]:c["uoff"][u + 1]]
            differ += int((R.pre_subtract(x) != x.astype(np.float64) - x.min(0).astype(np.float64)).sum())
        assert differ > 1000, differ                             # the float32 subtraction rounds: its place matters
        return True
    case["reaches"] = reaches
    return case


# ---- elastic + sub_min ------------------------------------------------------------------------------------------------------
def _node_points(shape, gran, rng):
    """Per axis d: a point on the last axis value, one nextafter beyond it, one on the first value; plus interior nodes."""
    ax = R.axes(shape, gran)
    inner = lambda d: rng.uniform(ax[d][0] * 0.6, ax[d][-1] * 0.6)
    pts = [[a[1] for a in ax], [a[-2] for a in ax]]              # interior nodes in all three axes
    for d in range(3):
        for v in (ax[d][-1], np.nextafter(ax[d][-1], np.inf), ax[d][0], np.nextafter(ax[d][0], -np.inf)):
            p = [inner(0), inner(1), inner(2)]
            p[d] = v
            pts.append(p)
    return np.array(pts, np.float64)


def node_kinds(x, shape, gran):
    """Counts of rows (interior node, on a last axis value and in bounds, just beyond a last value, on a first value)."""
    ax = R.axes(shape, gran)
    lo, hi = np.array([a[0] for a in ax]), np.array([a[-1] for a in ax])
    inb = ((x >= lo) & (x <= hi)).all(1)
    node = np.stack([np.isin(x[:, d], ax[d][1:-1]) for d in range(3)], 1).all(1)
    return (int(node.sum()), int(((x == hi).any(1) & inb).sum()), int((x == np.nextafter(hi, np.inf)).any(1).sum()),
            int(((x == lo).any(1) & inb).sum()))


@functools.lru_cache(None)
def elastic_case():
    """5 units, units 1 and 3 elastic.  Unit 1 carries the designed points for pass 0 (gran 6).  Unit 3's pass-0 noise is
    zero, so its rows reach pass 1 (gran 20) unchanged and carry the designed points for that grid."""
    rng = np.random.default_rng(202)
    sizes = [50, 400, 1, 700, 129]
    shapes = [[(4, 5, 3), (3, 3, 4)], [(3, 3, 3), (3, 4, 3)]]   # [pass][descriptor]
    uoff = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    xyz = rng.uniform(-22, 22, (int(uoff[-1]), 3))
    p1 = _node_points(shapes[0][0], ELASTIC[0][0], rng)
    xyz[uoff[1]:uoff[1] + len(p1)] = p1
    xyz[uoff[3]:uoff[4]] = rng.uniform(-66, 66, (sizes[3], 3))
    p3 = _node_points(shapes[1][1], ELASTIC[1][0], rng)
    xyz[uoff[3]:uoff[3] + len(p3)] = p3
    noise = [[[rng.standard_normal(sh).astype(np.float32) for _ in range(3)] for sh in shapes[p]] for p in range(2)]
    noise[0][1] = [np.zeros(shapes[0][1], np.float32) for _ in range(3)]
    case = dict(xyz=xyz, uoff=uoff, units=[1, 3], shapes=shapes, noise=noise, max_rows=max(sizes),
                flags=np.array([0, 1, 0, 1, 0], np.int32))

    def reaches(c=case):
        mid, _ = R.elastic_pass(c["xyz"], c["uoff"], list(zip(c["units"], c["shapes"][0])), c["noise"][0], *ELASTIC[0])
        a, b = c["uoff"][3], c["uoff"][4]
        assert np.array_equal(mid[a:b], c["xyz"][a:b])          # zero noise: unit 3 arrives at pass 1 unchanged
        k0 = node_kinds(c["xyz"][c["uoff"][1]:c["uoff"][2]], c["shapes"][0][0], ELASTIC[0][0])
        k1 = node_kinds(mid[a:b], c["shapes"][1][1], ELASTIC[1][0])
        assert min(k0) >= 1 and min(k1) >= 1, (k0, k1)
        assert c["shapes"][0][0] != c["shapes"][0][1] and c["shapes"][1][0] != c["shapes"][1][1]
        assert (mid[c["uoff"][1]:c["uoff"][2]] != c["xyz"][c["uoff"][1]:c["uoff"][2]]).any()
        return True
    case["reaches"] = reaches
    return case


def elastic_ref(c):
    """Both passes and the closing sub_min: [(xyz, ext) after pass 0, after pass 1], final xyz."""
    steps, xyz = [], c["xyz"]
    for p, (gran, mag) in enumerate(ELASTIC):
        xyz, ext = R.elastic_pass(xyz, c["uoff"], list(zip(c["units"], c["shapes"][p])), c["noise"][p], gran, mag)
        steps.append((xyz, ext))
    return steps, R.sub_min(xyz, c["uoff"], c["flags"], steps[-1][1])


# ---- crop -------------------------------------------------------------------------------------------------------------------
def _box(rng, n, hi):
    return rng.uniform(0, 1, (n, 3)) * np.asarray(hi, np.float64)


def _cluster_scene(rng):
    """150 points in x 1500..1600, 151 spread over x 0..1400, ends at 0 and 2000: a level-0 window (512 wide, at
    1487.999 * t) holds 100..200 points only where it covers the cluster."""
    x = np.concatenate([rng.uniform(1500, 1600, 150), rng.uniform(0, 1400, 151), [0.0, 2000.0]])
    p = _box(rng, x.size, (1, 300, 100))
    p[:, 0] = x
    return p[rng.permutation(x.size)]


def _crop_pack(scenes, mode, trips, n_trip, max_p, min_p):
    soff = np.concatenate([[0], np.cumsum([s.shape[0] for s in scenes])]).astype(np.int32)
    triples = np.zeros((len(scenes), R.CROP_TRIPLES, 3))
    for s, t in enumerate(trips):
        if t is not None:
            triples[s, :len(t)] = t
    return dict(xyz=np.concatenate(scenes), soff=soff, mode=np.array(mode, np.int32), triples=triples,
                n_triples=np.array(n_trip, np.int32), levels=LEVELS, max_crop_p=max_p, min_crop_p=min_p,
                max_rows=int(np.diff(soff).max()))


def crop_ref(c):
    return R.crop(c["xyz"], c["soff"], c["mode"], c["triples"], c["n_triples"], c["levels"], c["max_crop_p"],
                  c["min_crop_p"])


@functools.lru_cache(None)
def crop_case():
    """mode 1 | try 0, level 0 | try 0 after shrinking | empty, mode 1 | tries 0-3 fail, try 4 succeeds | all five fail."""
    rng = np.random.default_rng(303)
    full = lambda: rng.uniform(0, 1, (R.CROP_TRIPLES, 3))
    t_late, t_never = full(), full()
    t_late[:5, 0] = (0.1, 0.2, 0.3, 0.05, 0.8)
    t_never[:5, 0] = (0.1, 0.2, 0.3, 0.05, 0.15)
    scenes = [_box(rng, 150, (400, 400, 100)), _box(rng, 300, (1000, 500, 100)), _box(rng, 600, (600, 600, 100)),
              np.zeros((0, 3)), _cluster_scene(rng), _cluster_scene(rng)]
    t_first = full()
    t_first[0, 0] = 0.5
    case = _crop_pack(scenes, [1, 0, 0, 1, 0, 0], [None, t_first, full(), None, t_late, t_never], [0, 85, 85, 0, 85, 85],
                      200, 100)

    def reaches(c=case):
        st = crop_ref(c)["state"]
        assert (np.diff(c["soff"])[c["mode"] == 0] > c["max_crop_p"]).all()
        assert not st[0].any() and not st[3].any() and c["soff"][3] == c["soff"][4]
        assert st[1].tolist() == [1, 0, 1, 0, 0, 1, 0, 1]                         # try 0 without shrinking
        assert st[2, R.ST_TRIES] == 1 and st[2, R.ST_SUCCESS] == 1 and st[2, R.ST_LAST_K] >= 3
        assert st[4].tolist() == [1, 4, 5, 4, 0, 1, 0, 5]                         # done two launches after scenes 1, 2
        assert st[5].tolist() == [1, 5, 5, 4, 0, 0, 0, 5]                         # the last mask, un-offset
        return True
    case["reaches"] = reaches
    return case


@functools.lru_cache(None)
def crop_short_case():
    """Too few triples: scene 0 needs a fourth try, scene 1 a fourth shrink level, with 3 triples each; scene 2 is fine."""
    rng = np.random.default_rng(304)
    t_never = rng.uniform(0, 1, (3, 3))
    t_never[:3, 0] = (0.1, 0.2, 0.3)
    scenes = [_cluster_scene(rng), _box(rng, 600, (600, 600, 100)), _box(rng, 300, (1000, 500, 100))]
    t_ok = rng.uniform(0, 1, (R.CROP_TRIPLES, 3))
    t_ok[0, 0] = 0.5
    case = _crop_pack(scenes, [0, 0, 0], [t_never, rng.uniform(0, 1, (3, 3)), t_ok], [3, 3, 85], 200, 100)

    def reaches(c=case):
        r = crop_ref(c)
        st = r["state"]
        assert st[0, R.ST_ERROR] == 2 and st[0, R.ST_TRIES] == 3 and st[0, R.ST_NEXT] == 3 and st[0, R.ST_DONE] == 1
        assert st[1, R.ST_ERROR] == 2 and st[1, R.ST_TRIES] == 0 and (r["counts"][0, 1, :3] > c["max_crop_p"]).all()
        assert st[2].tolist() == [1, 0, 1, 0, 0, 1, 0, 1]
        return True
    case["reaches"] = reaches
    return case


@functools.lru_cache(None)
def crop_boundary_case():
    """Triples whose x component is exactly 0.0 (o == -0.0 on x; y and z rooms are below every level, o == 0 there too),
    rows with x exactly 0.0 (kept), exactly at level 0 and level 1 (dropped), one nextafter below each (kept).
    x = 0, 2.5, ..., 997.5 puts 205 rows below 512 and 192 below 480; level 0 holds 207 > 200, level 1 holds 193."""
    rng = np.random.default_rng(305)
    x = np.concatenate([np.arange(400) * 2.5, [512.0, np.nextafter(512.0, 0), np.nextafter(480.0, 0)]])
    p = _box(rng, x.size, (1, 100, 100))
    p[:, 0] = x
    p[5:9, 1] = 0.0
    p[9:12, 2] = 0.0
    p = p[rng.permutation(x.size)]
    t = rng.uniform(0, 1, (R.CROP_TRIPLES, 3))
    t[:, 0] = 0.0
    case = _crop_pack([p, _box(rng, 300, (1000, 500, 100))], [0, 0], [t, rng.uniform(0, 1, (R.CROP_TRIPLES, 3))],
                      [85, 85], 200, 100)

    def reaches(c=case):
        r = crop_ref(c)
        assert r["state"][0].tolist() == [1, 0, 2, 0, 1, 1, 0, 1] and r["counts"][0, 0, :2].tolist() == [207, 193]
        x0 = c["xyz"][:c["soff"][1]]
        for k in (0, 1):
            o = R.crop_offset(r["ext_pre"][0], LEVELS[k], c["triples"][0, k])
            assert (o == 0).all()
            v = R.crop_valid(x0, o, LEVELS[k]).astype(bool)
            lv = LEVELS[k, 0]
            on0, onl, below = (x0 == 0).any(1), x0[:, 0] == lv, x0[:, 0] == np.nextafter(lv, 0)
            assert on0.sum() >= 8 and v[on0 & (x0[:, 0] < lv)].all()               # x + o == 0 is kept
            assert onl.sum() == 1 and not v[onl].any()                             # x + o == level is dropped
            assert below.sum() == 1 and v[below].all()
        return True
    case["reaches"] = reaches
    return case


# ---- compaction -------------------------------------------------------------------------------------------------------------
def _crop_rows(rng, n):
    """Rows of a cropping scene: x spread over 1000 (a 512 window keeps about half), both ends present."""
    p = _box(rng, n, (1000, 300, 100))
    p[0, 0], p[-1, 0] = 0.0, 1000.0
    return p


def _labels(rng, n, values, none_every=0):
    lab = np.asarray(values, np.int32)[rng.integers(0, len(values), n)] if len(values) else np.full(n, -100, np.int32)
    lab[:min(n, len(values))] = np.asarray(values, np.int32)[:n]                    # every value present where n allows
    if none_every:
        lab[len(values)::none_every] = -100
    return lab


def _compact_pack(seed, unit_rows, unit_labels, per_scene, mode, max_p, min_p, trips=None):
    """unit_rows: per unit its xyz rows; unit_labels: per unit its raw labels.  The crop state is the crop reference's."""
    rng = np.random.default_rng(seed)
    U = len(unit_rows)
    B = U // per_scene
    uoff = np.concatenate([[0], np.cumsum([x.shape[0] for x in unit_rows])]).astype(np.int32)
    soff = uoff[::per_scene].copy()
    n = int(uoff[-1])
    xyz = np.concatenate(unit_rows) if n else np.zeros((0, 3))
    ins = np.concatenate(unit_labels).astype(np.int32) if n else np.zeros(0, np.int32)
    ins_shift = np.zeros(U, np.int32)
    label_cap = np.zeros(B, np.int64)
    for s in range(B):
        hi = 0
        for k in range(per_scene):
            u = s * per_scene + k
            raw_max = int(unit_labels[u].max()) if unit_labels[u].size else -100
            if k == 1:
                prev = unit_labels[u - 1]
                ins_shift[u] = (int(prev.max()) if prev.size else -100) + 1
            hi = max(hi, raw_max + int(ins_shift[u]))
        label_cap[s] = max(hi, 0) + 1
    triples = rng.uniform(0, 1, (B, R.CROP_TRIPLES, 3))
    for s, t in (trips or {}).items():
        triples[s, :len(t)] = t
    mode = np.array(mode, np.int32)
    n_trip = np.where(mode == 0, R.CROP_TRIPLES, 0).astype(np.int32)
    assert (np.diff(soff)[mode == 0] > max_p).all()
    cr = R.crop(xyz, soff, mode, triples, n_trip, LEVELS, max_p, min_p)
    assert not cr["state"][:, R.ST_ERROR].any()
    return dict(xyz=xyz, rgb=rng.uniform(0, 1, (n, 3)).astype(np.float32), nl=rng.standard_normal((n, 3)).astype(np.float32),
                sem=rng.integers(0, 20, n).astype(np.int64), ins=ins, shift=rng.standard_normal((U, 3)) * 0.1,
                ins_shift=ins_shift, uoff=uoff, soff=soff, mode=mode, triples=triples, levels=LEVELS, state=cr["state"],
                ext_pre=cr["ext_pre"], ext_post=cr["ext_post"],
                label_off=np.concatenate([[0], np.cumsum(label_cap)]).astype(np.int32), n_rows=n)


def compact_ref(c):
    return R.compact(c["xyz"], c["rgb"], c["nl"], c["sem"], c["ins"], c["shift"], c["ins_shift"], c["uoff"], c["soff"],
                     c["mode"], c["triples"], c["levels"], c["state"], c["ext_pre"], c["ext_post"])


def _with(case, reaches):
    case["reaches"] = lambda c=case: bool(reaches(c, compact_ref(c)) or True)
    return case


def relabel_moves(lab):
    """How often the relabel loop moves the maximum label."""
    lab, moves, j = np.array(lab), 0, 0
    while lab.size and j < lab.max():
        if not (lab == j).any():
            lab[lab == lab.max()] = j
            moves += 1
        j += 1
    return moves


SINGLE_ROWS = (1, 7, 8, 9, 511, 512, 513, 2047, 2048, 2049)


@functools.lru_cache(None)
def compact_single(n):
    """One scene of n rows; it crops (about half kept) from 7 rows on."""
    rng = np.random.default_rng(400 + n)
    crops = n >= 7
    c = _compact_pack(400 + n, [_crop_rows(rng, n) if crops else _box(rng, n, (9, 9, 9))],
                      [_labels(rng, n, [0, 2, 3, 7], none_every=5)], 1, [0 if crops else 1], n // 2, 1)

    def reaches(c, r):
        assert c["n_rows"] == n and r["scan"].size == max(1, -(-n // R.CHUNK)) + 1
        if crops:
            assert 0 < r["mask"].sum() < n
    return _with(c, reaches)


def _scenes_case(seed, sizes, crop_scenes, max_p, label_sets=None):
    rng = np.random.default_rng(seed)
    rows = [_crop_rows(rng, n) if s in crop_scenes else _box(rng, n, (9, 9, 9)) for s, n in enumerate(sizes)]
    labs = [_labels(rng, n, (label_sets or {}).get(s, [0, 1, 4]), none_every=7) for s, n in enumerate(sizes)]
    return _compact_pack(seed, rows, labs, 1, [0 if s in crop_scenes else 1 for s in range(len(sizes))], max_p, 1)


@functools.lru_cache(None)
def compact_in_thread():
    """Scene boundaries at rows 3, 5 and 8: thread 0's eight rows span three scenes, thread 1 starts a fourth (its wave
    is not uniform).  The boundary at row 708 falls inside the rows of lane 24 of wave 1."""
    c = _scenes_case(421, [3, 2, 3, 700, 50], {3}, 300)

    def reaches(c, r):
        assert c["soff"].tolist() == [0, 3, 5, 8, 708, 758] and 0 < r["scene_info"][3, 0] < 700
        assert (708 // R.ROWS_PER_THREAD) % 64 == 24 and 708 % R.ROWS_PER_THREAD != 0
    return _with(c, reaches)


@functools.lru_cache(None)
def compact_wave_chunk_edges():
    """Scene boundaries at row 515 (inside wave 1, past its first row, inside a thread's eight rows), 2048 (a chunk edge)
    and 2051.  Row 515 belongs to lane 0 of its wave: that lane flushes scene 0 itself and leads the wave with scene 1."""
    c = _scenes_case(422, [515, 1533, 3, 500], {1, 3}, 300)

    def reaches(c, r):
        assert c["soff"].tolist() == [0, 515, 2048, 2051, 2551]
        assert 515 // R.ROWS_PER_WAVE == 1 and 515 % R.ROWS_PER_WAVE != 0 and 515 % R.ROWS_PER_THREAD != 0
        assert 0 < r["scene_info"][1, 0] < 1533 and 0 < r["scene_info"][3, 0] < 500
    return _with(c, reaches)


@functools.lru_cache(None)
def compact_empty_between():
    c = _scenes_case(423, [100, 0, 400], {2}, 150)

    def reaches(c, r):
        assert r["scene_info"][1].tolist() == [0, 0, 100, 0] and 0 < r["scene_info"][2, 0] < 400
    return _with(c, reaches)


@functools.lru_cache(None)
def compact_two_units():
    """Primary + partner per scene; the partner's labels move up by the primary's maximum + 1.  Scene 1's primary has no
    instance (shift -99: negative labels that are not -100), scene 2's partner is empty."""
    rng = np.random.default_rng(424)
    sizes = [300, 200, 40, 60, 90, 0]
    rows = [_crop_rows(rng, n) if u < 2 else _box(rng, n, (9, 9, 9)) for u, n in enumerate(sizes)]
    labs = [_labels(rng, 300, [0, 2, 5], 6), _labels(rng, 200, [0, 1, 3], 6), np.full(40, -100, np.int32),
            _labels(rng, 60, [0, 2], 4), _labels(rng, 90, [1, 2], 0), np.zeros(0, np.int32)]
    c = _compact_pack(424, rows, labs, 2, [0, 1, 1], 300, 1)

    def reaches(c, r):
        assert c["ins_shift"].tolist() == [0, 6, 0, -99, 0, 3]
        assert 0 < r["scene_info"][0, 0] < 500
        s1 = r["label"][r["scene_info"][1, 2]:r["scene_info"][2, 2]]
        assert ((s1 < 0) & (s1 != -100)).any() and r["scene_info"][1, 1] == -96
    return _with(c, reaches)


@functools.lru_cache(None)
def compact_chunk_all_or_none():
    """One cropping scene of three chunks: the window (x in 122..634 at level 0) drops every row of chunk 1 and keeps
    every row of chunk 2."""
    rng = np.random.default_rng(425)
    p = _crop_rows(rng, 3 * R.CHUNK)
    p[R.CHUNK:2 * R.CHUNK, 0] = rng.uniform(800, 1000, R.CHUNK)
    p[2 * R.CHUNK:, 0] = rng.uniform(250, 480, R.CHUNK)
    p[-1, 0] = 470.0
    p[R.CHUNK, 0] = 1000.0
    t = rng.uniform(0, 1, (1, 3))
    t[0, 0] = 0.25
    c = _compact_pack(425, [p], [_labels(rng, 3 * R.CHUNK, [0, 1, 2, 3, 9], 11)], 1, [0], 4000, 100, trips={0: t})

    def reaches(c, r):
        assert c["state"][0].tolist() == [1, 0, 1, 0, 0, 1, 0, 1]
        d = np.diff(r["scan"])
        assert 0 < d[0] < R.CHUNK and d[1] == 0 and d[2] == R.CHUNK
    return _with(c, reaches)


@functools.lru_cache(None)
def compact_second_tile():
    """256 * 2048 + 1 rows kept alternately (x = 100 | 900, window 0..512): 257 chunks, the scan's second tile."""
    rng = np.random.default_rng(426)
    n = R.SCAN_TILE * R.CHUNK + 1
    p = _box(rng, n, (1, 300, 100))
    p[:, 0] = np.where(np.arange(n) % 2 == 0, 100.0, 900.0)
    t = rng.uniform(0, 1, (1, 3))
    t[0, 0] = 0.0
    c = _compact_pack(426, [p], [_labels(rng, n, [0, 1, 5], 9)], 1, [0], 300000, 50000, trips={0: t})

    def reaches(c, r):
        assert r["scan"].size == R.SCAN_TILE + 2 and c["state"][0, R.ST_SUCCESS] == 1
        assert np.array_equal(r["mask"], np.arange(n) % 2 == 0)
    return _with(c, reaches)


RELABEL_SETS = {0: [0, 3, 5], 1: [1], 2: [0], 3: [], 4: list(range(2, 41)), 5: [0, 1, 2, 3, 6, 9]}


@functools.lru_cache(None)
def compact_relabel():
    """The relabel tables {0,3,5} | {1} | {0} | all -100 | {2..40} with -100 mixed in | a cropping scene whose window drops
    every row of label 0 and of the maximum label 9."""
    c = _scenes_case(427, [60, 10, 10, 30, 200, 500], {5}, 400, RELABEL_SETS)
    a = int(c["soff"][5])
    lab = c["ins"][a:]
    c["xyz"][a:][(lab == 0) | (lab == 9), 0] = np.random.default_rng(428).uniform(900, 1000, int(((lab == 0) | (lab == 9)).sum()))
    c["xyz"][a:][~((lab == 0) | (lab == 9)), 0] = np.random.default_rng(429).uniform(0, 400, int((~((lab == 0) | (lab == 9))).sum()))
    c["xyz"][a, 0] = 1000.0
    c["triples"][5, :, 0] = 0.0                                                    # window x in 0..512 at level 0
    cr = R.crop(c["xyz"], c["soff"], c["mode"], c["triples"], np.where(c["mode"] == 0, 85, 0), LEVELS, 400, 1)
    c.update(state=cr["state"], ext_pre=cr["ext_pre"], ext_post=cr["ext_post"])

    def reaches(c, r):
        info = r["scene_info"]
        assert info[:, 1].tolist() == [3, 1, 1, -99, 39, 4]
        kept = c["ins"][int(c["soff"][5]):][r["mask"][int(c["soff"][5]):]]
        assert set(kept.tolist()) == {1, 2, 3, 6, -100}                            # 0 and the maximum 9 are gone
        assert relabel_moves([0, 3, 5]) == 2 and relabel_moves(list(range(2, 41))) == 2 and relabel_moves(kept) == 1
    return _with(c, reaches)


def compact_no_rows():
    return _compact_pack(430, [np.zeros((0, 3))], [np.zeros(0, np.int32)], 1, [1], 10, 1)


def compact_cases():
    cases = {"rows%d" % n: (lambda n=n: compact_single(n)) for n in SINGLE_ROWS}
    cases.update(in_thread=compact_in_thread, wave_chunk_edges=compact_wave_chunk_edges,
                 empty_between=compact_empty_between, two_units=compact_two_units,
                 chunk_all_or_none=compact_chunk_all_or_none, second_tile=compact_second_tile, relabel=compact_relabel)
    return cases


# ---- instances --------------------------------------------------------------------------------------------------------------
def _inst_pack(xyz, label, sizes, inst_num):
    ostart = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    return dict(xyz=xyz, label=label.astype(np.int32), ostart=ostart, inst_num=np.array(inst_num, np.int32),
                n_rows=int(ostart[-1]))


def instances_ref(c):
    return R.instances(c["xyz"], c["label"], c["ostart"], c["inst_num"])


@functools.lru_cache(None)
def instances_case():
    """Scene 0: instances of 1, 255, 256, 257 and 3000 rows interleaved, plus unlabelled rows; scene 1: nothing but -100
    (instance_num -99, the running offset goes down); scene 2: three ordinary instances."""
    rng = np.random.default_rng(501)
    l0 = np.concatenate([np.full(k, i) for i, k in enumerate((1, 255, 256, 257, 3000))] + [np.full(77, -100)])
    l2 = np.concatenate([np.full(k, i) for i, k in enumerate((40, 9, 300))] + [np.full(13, -100)])
    labs = [l0[rng.permutation(l0.size)], np.full(40, -100), l2[rng.permutation(l2.size)]]
    sizes = [x.size for x in labs]
    c = _inst_pack(rng.uniform(0, 9, (sum(sizes), 3)), np.concatenate(labs), sizes, [5, -99, 3])

    def reaches(c=c):
        r = instances_ref(c)
        assert r["pointnum"].tolist() == [1, 255, 256, 257, 3000, 40, 9, 300]
        assert r["inst_start"].tolist() == [0, 5, 5, 8] and r["inst_off"].tolist() == [0, 5, -94]
        last = r["ins"][c["ostart"][2]:]
        assert set(last.tolist()) == {-94, -93, -92, -100}
        return True
    c["reaches"] = reaches
    return c


@functools.lru_cache(None)
def instances_none_case():
    rng = np.random.default_rng(502)
    c = _inst_pack(rng.uniform(0, 9, (300, 3)), np.full(300, -100), [120, 180], [-99, -99])
    c["reaches"] = lambda c=c: instances_ref(c)["pointnum"].size == 0 and c["n_rows"] == 300
    return c


@functools.lru_cache(None)
def instances_no_rows_case():
    c = _inst_pack(np.zeros((0, 3)), np.zeros(0), [0], [0])
    c["reaches"] = lambda c=c: c["n_rows"] == 0 and instances_ref(c)["pointnum"].size == 0
    return c


# ---- quantize ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def quantize_case(voxel):
    """k * voxel for k = 0..50 (float64 products) with both neighbours, +-0.0 and small negatives; scene 1 is empty."""
    k = np.arange(51, dtype=np.float64) * np.float64(voxel)
    v = np.concatenate([k, np.nextafter(k, np.inf), np.nextafter(k, -np.inf), [0.0, -0.0, -1e-300, -1e-9, -voxel / 2,
                        -voxel, np.nextafter(-voxel, 0), np.nextafter(-voxel, -1)]])
    rng = np.random.default_rng(601)
    v = np.concatenate([v, rng.uniform(-0.1, 1.1, (-v.size) % 3 + 30)])
    xyz = v[rng.permutation(v.size)].reshape(-1, 3)
    n = xyz.shape[0]
    c = dict(xyz=xyz, ostart=np.array([0, 20, 20, n], np.int32), voxel=float(voxel), n_rows=n)

    def reaches(c=c):
        c4, _ = R.quantize(c["xyz"], c["ostart"], c["voxel"])
        assert set(c4[:, 0].tolist()) == {0, 2}                                    # the batch index skips the empty scene
        assert (c4[:, 1:] == -1).any() and (c4[:, 1:] == -2).any() and (c4[:, 1:] == 50).any()
        assert (np.signbit(c["xyz"]) & (c["xyz"] == 0)).any()
        q = c["xyz"] / c["voxel"]
        assert (q == np.round(q)).sum() > 30                                       # quotients exactly on a boundary
        return True
    c["reaches"] = reaches
    return c


def all_cases():
    """name -> thunk, every case of this file."""
    cases = dict(affine=affine_case, elastic=elastic_case, crop=crop_case, crop_short=crop_short_case,
                 crop_boundary=crop_boundary_case, instances=instances_case, instances_none=instances_none_case,
                 instances_no_rows=instances_no_rows_case)
    cases.update({"compact_" + k: v for k, v in compact_cases().items()})
    cases.update({"quantize_%g" % v: (lambda v=v: quantize_case(v)) for v in (0.02, 0.01)})
    return cases
