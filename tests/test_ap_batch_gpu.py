"""GPU tier: pbn_ap_assoc_batch (csrc/apassoc_batch.hip) through the C ABI on seeded synthetic inputs, no network.  For every case
the log words AND the state block are compared with == against the numpy restatement tests/ap_batch_ref.py; buffers sit between
guard words.  Also: two runs give the same bytes, the per-scene path (AssociationLog.append on dense(j)) gives the same words, and
every argument error returns its code and leaves the state untouched."""
import ctypes

import numpy as np
import pytest
import torch

import ap_batch_ref as B
import ap_record_ref as R
from pbnet_amd import _native as N
from pbnet_amd import evaluate as E
from pbnet_amd import postprocess as P

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
GUARD, PAD = 0x5a5a5a5a, 64
CODES = [0] + [c * 1000 + k + 1 for k, c in enumerate([3, 4, 5, 7, 39, 1, 2, 8, 9, 10, 11, 12])]


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t if dtype is None else t.to(dtype)


def bed(n_words, fill=0):
    """int32 buffer of n_words between guard words: (whole bed, its inside view)."""
    t = torch.full((n_words + 2 * PAD,), GUARD, dtype=torch.int32, device=DEV)
    t[PAD:PAD + n_words] = fill
    return t, t[PAD:PAD + n_words]


def guards_intact(t):
    h = t.cpu().numpy()
    return bool((h[:PAD] == GUARD).all() and (h[-PAD:] == GUARD).all())


def make_batch(seed, sizes, n_prop, keeps, n_ids, special=None):
    """Seeded merged forward: per scene labels in [0, n_keep) with about a fifth -100 and ids from a pool of n_ids codes, laid out
    in runs (even seeds) or scattered.  special[j]: 'empty' (all -100, n_keep 0), 'one' (one instance owns every point), 'beyond'
    (some labels >= n_keep and one negative other than -100), 'one_id' (n_gt = 1)."""
    rng = np.random.default_rng(seed)
    special = special or {}
    labels, ids, keep = [], [], list(keeps)
    for j, n in enumerate(sizes):
        kind = special.get(j)
        k = keep[j]
        lab = rng.integers(0, max(k, 1), n).astype(np.int32) if k else np.full(n, -100, np.int32)
        lab[rng.random(n) < 0.2] = -100
        pool = np.array(CODES[:n_ids] if n_ids <= len(CODES) else list(range(0, 7 * n_ids, 7)), np.int64)
        gid = pool[rng.integers(0, pool.shape[0], n)] if (seed + j) % 2 else pool[(np.arange(n) * pool.shape[0]) // max(n, 1)]
        if kind == "empty":
            lab[:], keep[j] = -100, 0
        elif kind == "one":
            lab[:], keep[j] = 0, 1
        elif kind == "beyond":
            lab[::3] = k + 2
            lab[1::7] = -5
        elif kind == "one_id":
            gid[:] = 3001
        labels.append(lab)
        ids.append(gid)
    b = len(sizes)
    starts = np.concatenate([[0], np.cumsum(sizes)]).astype(int).tolist()
    return dict(point_starts=starts, point_instance=np.concatenate(labels) if b else np.zeros(0, np.int32), n_keep=keep,
                post_status=[0] * b, scores=rng.random((b, n_prop)).astype(np.float32),
                semantic_id=rng.integers(1, 40, (b, n_prop)).astype(np.int64), ids=np.concatenate(ids), tags=[100 + 3 * j for j in range(b)])


def table_of(starts, copies=1):
    t = N.TtaTable()
    t.n_scenes, t.copies = len(starts) - 1, copies
    for j, v in enumerate(starts):
        t.point_start[j], t.sp_start[j] = int(v), 0
    return t


def tags_of(tags):
    st = N.SceneTags()
    for j, v in enumerate(tags):
        st.tag[j] = int(v)
    return st


def run(c, u_cap=64, id_cap=65536, n_inst_cap=16, log_words=1 << 16, ids_dtype=torch.int64, copies=1, sem=None, ins=None,
        state=None, mutate=None):
    """One call of the entry on case `c`; returns (rc, state int32[8], log int32[log_words]) and checks the guard words."""
    lib = N.lib()
    b, n_total, n_prop = len(c["n_keep"]), c["point_starts"][-1], c["scores"].shape[1]
    nbytes = int(lib.pbn_ap_assoc_batch_workspace_bytes(n_total, b, u_cap, id_cap, 0 if sem is None else n_inst_cap))
    assert nbytes > 0
    ws_bed, ws = bed(nbytes // 4)
    log_bed, log = bed(log_words)
    st_bed, st = bed(8)
    if state is not None:
        st.copy_(dev(np.asarray(state, np.int32)))
    pi = dev(c["point_instance"].astype(np.int32))
    scal = dev(np.array(list(c["n_keep"]) + list(c["post_status"]), np.int32))
    scores, sid = dev(c["scores"]), dev(c["semantic_id"])
    ids_t = None if sem is not None else dev(c["ids"], ids_dtype)
    sem_t, ins_t = (None, None) if sem is None else (dev(sem, ids_dtype), dev(ins, ids_dtype))
    label_table = dev(B.SEMANTIC_LABEL_IDX.astype(np.int32))
    i64 = int(ids_dtype == torch.int64)
    args = dict(units=table_of(c["point_starts"], copies), pi=N.ptr(pi), scal=N.ptr(scal), scores=N.ptr(scores), sid=N.ptr(sid),
                n_prop=n_prop, ids=N.ptr(ids_t), sem=N.ptr(sem_t), ins=N.ptr(ins_t), lt=N.ptr(label_table), n_labels=20, u_cap=u_cap,
                id_cap=id_cap, n_inst_cap=n_inst_cap, tags=tags_of(c["tags"]), state=N.ptr(st), log=N.ptr(log), log_words=log_words,
                ws=N.ptr(ws), ws_bytes=nbytes)
    if mutate:
        mutate(args)
    a = args
    rc = lib.pbn_ap_assoc_batch(a["units"], a["pi"], a["scal"], a["scores"], a["sid"], a["n_prop"], a["ids"], i64, a["sem"], i64,
                                a["ins"], i64, a["lt"], a["n_labels"], a["u_cap"], a["id_cap"], a["n_inst_cap"], a["tags"], a["state"],
                                a["log"], a["log_words"], a["ws"], a["ws_bytes"], N.current_stream())
    torch.cuda.synchronize()
    assert guards_intact(ws_bed) and guards_intact(log_bed) and guards_intact(st_bed)
    return rc, st.cpu().numpy(), log.cpu().numpy()


def want(c, u_cap=64, id_cap=65536, n_inst_cap=16, log_words=1 << 16, sem=None, ins=None, state=None):
    return B.assoc_batch(c["point_starts"], c["point_instance"], c["n_keep"], c["post_status"], c["scores"], c["semantic_id"], c["tags"],
                         u_cap, id_cap, log_words, ids=None if sem is not None else c["ids"], sem=sem, ins=ins, n_inst_cap=n_inst_cap,
                         state=state)


def check(c, **kw):
    rc, state, log = run(c, **kw)
    kw.pop("ids_dtype", None), kw.pop("copies", None)
    ref_state, ref_log = want(c, **kw)
    assert rc == 0
    assert state.tolist() == ref_state.tolist()
    assert np.array_equal(log, ref_log)
    return state, log


SHAPES = {1: ([4100], [9], {}),
          3: ([65, 0, 257], [5, 4, 7], {}),
          8: ([0, 1, 63, 64, 65, 257, 4100, 64], [2, 3, 4, 1, 5, 6, 9, 2],
              {1: "empty", 3: "one", 4: "beyond", 5: "one_id"})}


@pytest.mark.parametrize("dtype", [torch.int32, torch.int64], ids=["i32", "i64"])
@pytest.mark.parametrize("b", [1, 3, 8])
def test_equals_the_restatement(b, dtype):
    sizes, keeps, special = SHAPES[b]
    c = make_batch(10 + b, sizes, 40, keeps, 9, special)
    c["post_status"][-1] = 1                                   # the post-processing's word is ORed in
    state, log = check(c, ids_dtype=dtype)
    assert state[2] == b and state[3] == 0
    _, state2, log2 = run(c, ids_dtype=dtype)                  # two runs: the same bytes
    assert state2.tobytes() == state.tobytes() and log2.tobytes() == log.tobytes()


def test_boundaries_inside_a_wave_and_continuing_an_epoch():
    c = make_batch(21, [63, 1, 65, 0, 64, 257], 16, [3, 1, 4, 2, 2, 5], 5, {1: "one"})
    first, _ = want(c)
    check(c, state=[7, 9, 2, 0, 3, 0, 0, 0])                   # a log that already holds records: appended behind word 7
    assert first[0] > 0


def test_id_range_and_id_count_bits():
    c = make_batch(31, [257, 65, 4100], 12, [4, 3, 6], 9)
    c["ids"][3], c["ids"][260] = 65536, -1                     # scene 0: an id >= id_cap; scene 1: a negative id
    state, log = check(c)
    recs = list(E._walk_association_log(log[:state[0]], []))
    assert [bool(r[2]) for r in recs] == [True, True, False] and "id_cap" in recs[0][2][0]
    state, log = check(c, u_cap=4)                             # nine ids per scene, four slots: bit 8 everywhere
    assert all(int(log[o + 5]) & B.ID_COUNT and int(log[o + 3]) == 4 for o in record_offsets(log, state))


def record_offsets(log, state):
    out, pos = [], 0
    while pos < state[0]:
        out.append(pos)
        pos += int(log[pos + 6])
    return out


@pytest.mark.parametrize("dtype", [torch.int32, torch.int64], ids=["i32", "i64"])
def test_sem_ins_form_and_its_bits(dtype):
    sizes = [65, 257, 4100, 0, 63]
    c = make_batch(41, sizes, 12, [3, 4, 6, 1, 2], 5)
    rng = np.random.default_rng(41)
    n = c["point_starts"][-1]
    ins = rng.integers(-1, 9, n).astype(np.int64)
    ins[ins == 4] = -100
    sem = rng.integers(0, 20, n).astype(np.int64)
    sem[rng.random(n) < 0.2] = -100
    state, log = check(c, sem=sem, ins=ins, ids_dtype=dtype)   # clean: instance numbers repeat across scenes, firsts are per scene
    assert not any(int(log[o + 5]) for o in record_offsets(log, state))
    ins[70] = 16                                               # scene 1: an instance >= n_inst_cap
    first_of_2 = c["point_starts"][2] + int(np.nonzero(ins[c["point_starts"][2]:c["point_starts"][3]] == 2)[0][0])
    sem[first_of_2] = 20                                       # scene 2: the lowest point of instance 2 carries a bad label
    state, log = check(c, sem=sem, ins=ins, ids_dtype=dtype)
    bits = [int(log[o + 5]) for o in record_offsets(log, state)]
    assert bits == [0, B.INSTANCE_CAP, B.SEMANTIC_RANGE, 0, 0]


def test_above_the_lds_bound_takes_the_global_path():
    bound = N.lib().pbn_ap_assoc_batch_lds_counters()
    n_keep, n_ids = 40, 1100
    assert n_keep * n_ids > bound > 6 * 9                      # scene 0 above the bound, scene 1 below it
    c = make_batch(51, [4100, 257, 4100], 48, [n_keep, 6, n_keep], n_ids)
    c["ids"][4100:4357] = np.array(CODES[:9])[np.arange(257) % 9]
    state, log = check(c, u_cap=2048, log_words=1 << 17)
    offs = record_offsets(log, state)
    assert int(log[offs[0] + 3]) > bound // n_keep and int(log[offs[1] + 3]) == 9


def test_log_too_small_for_the_second_record():
    c = make_batch(61, [257, 4100, 65], 12, [4, 6, 3], 9)
    full_state, full_log = want(c)
    offs = record_offsets(full_log, full_state)
    words = offs[2] - 1                                        # the second of three records does not fit; the third alone would
    state, log = check(c, log_words=words)
    assert state.tolist()[:5] == [offs[1], int(full_state[0]), 1, 1, -1]
    assert np.array_equal(log[:offs[1]], full_log[:offs[1]]) and not log[offs[1]:].any()


def test_n_prop_zero_gives_header_only_records():
    c = make_batch(71, [65, 0, 257], 0, [0, 0, 0], 5)
    state, log = check(c)
    assert state.tolist()[:4] == [3 * R.HEADER, 3 * R.HEADER, 3, 0]


def test_copies_three_table_with_folded_numbering():
    c = make_batch(81, [257, 65], 12, [4, 3], 9)
    s1, l1 = check(c, copies=3)                                # the table is over folded points: the copies change nothing here
    _, s2, l2 = run(c, copies=1)
    assert s1.tobytes() == s2.tobytes() and l1.tobytes() == l2.tobytes()


def test_equals_the_per_scene_path():
    """AssociationLog.append on RefinedBatch.dense(j), scene by scene, into a fresh log, against append_batch on the same
    RefinedBatch: the same words.  Also: append_batch does not synchronise once its buffers fit."""
    sizes, keeps = [65, 257, 0, 4100], [3, 5, 2, 9]
    c = make_batch(91, sizes, 20, keeps, 9, {2: "empty"})
    ws = P.PostBatchWorkspace(20, sum(sizes), 4, 0, DEV)
    ws.point_instance[:sum(sizes)].copy_(dev(c["point_instance"]))
    ws.scores[:4 * 20].copy_(dev(c["scores"]).view(-1))
    ws.semantic_id[:4 * 20].copy_(dev(c["semantic_id"]).view(-1))
    ws.scalars[:8].copy_(dev(np.array(c["n_keep"] + [0] * 4, np.int32)))
    rb = P.RefinedBatch(ws, 20, c["point_starts"], [0] * 5)
    gts = [dev(c["ids"][c["point_starts"][j]:c["point_starts"][j + 1]]) for j in range(4)]
    names = ["s%d" % j for j in range(4)]
    one = E.AssociationLog(20, 4100, u_cap=64, log_words=1 << 14, device=DEV)
    scalars = rb.scalars.tolist()
    for j in range(4):
        k = c["n_keep"][j]
        one.append(names[j], rb.dense(j, scalars), rb.scores[j, :k], rb.semantic_id[j, :k], None, None, gts[j])
    batch = E.AssociationLog(1, 1, u_cap=64, log_words=1 << 14, device=DEV)
    batch.append_batch(names, rb, gts)
    assert batch.state.tolist() == one.state.tolist() and batch.names == names
    assert np.array_equal(batch.log.cpu().numpy(), one.log.cpu().numpy())
    ref_state, ref_log = want(dict(c, tags=[0, 1, 2, 3]), log_words=1 << 14)
    assert np.array_equal(batch.log.cpu().numpy(), ref_log) and batch.state.cpu().numpy().tolist() == ref_state.tolist()
    # the second call fits: no allocation, no synchronisation; merged ids= instead of per-scene vectors
    merged = dev(c["ids"])
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    torch.cuda.set_sync_debug_mode("error")
    try:
        batch.append_batch(["t%d" % j for j in range(4)], rb, ids=merged)
        batch.append_batch(["u%d" % j for j in range(4)], rb, gts)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.cuda.memory_allocated() == before
    matches, dropped = batch.collect()
    assert dropped == ["s2", "t2", "u2"] and len(matches) == 9
    for j in (0, 1, 3):
        pred = dict(conf=c["scores"][j, :keeps[j]], label_id=c["semantic_id"][j, :keeps[j]], mask=rb.dense(j, scalars))
        host = E.assign_instances_for_scan("u%d" % j, pred, c["ids"][c["point_starts"][j]:c["point_starts"][j + 1]], device=DEV)
        for field in E.SceneMatches.__slots__:
            x, y = getattr(matches["u%d" % j], field), getattr(host, field)
            assert (x == y) if isinstance(x, str) else np.array_equal(np.asarray(x), np.asarray(y)), field


def test_argument_errors_leave_the_state_untouched():
    c = make_batch(95, [65, 257], 12, [3, 4], 5)
    sentinel = [11, 22, 3, 0, 5, 0, 0, 0]
    null = ctypes.c_void_p(None)

    def bad_table(a):
        a["units"].point_start[1] = 400                        # not ascending

    def bad_first(a):
        a["units"].point_start[0] = 1

    def too_many(a):
        a["units"].copies = 5                                  # 2 x 5 > PBN_MAX_SCENES

    def no_scenes(a):
        a["units"].n_scenes = 0

    cases = [(bad_table, -1), (bad_first, -1), (too_many, -1), (no_scenes, -1),
             (lambda a: a.update(state=null), -1), (lambda a: a.update(log=null), -1), (lambda a: a.update(pi=null), -1),
             (lambda a: a.update(scal=null), -1), (lambda a: a.update(ids=null), -1), (lambda a: a.update(ws=null), -1),
             (lambda a: a.update(u_cap=0), -1), (lambda a: a.update(n_prop=-1), -1),
             (lambda a: a.update(n_prop=N.lib().pbn_post_max_proposals() + 1), -5), (lambda a: a.update(id_cap=(1 << 20) + 1), -5),
             (lambda a: a.update(ws_bytes=a["ws_bytes"] - 256), -2)]
    for mutate, code in cases:
        rc, state, log = run(c, state=sentinel, mutate=mutate)
        assert rc == code, (mutate, rc)
        assert state.tolist() == sentinel and not log.any()
    assert N.lib().pbn_ap_assoc_batch_workspace_bytes(100, 9, 64, 65536, 0) == 0
    assert N.lib().pbn_ap_assoc_batch_workspace_bytes(100, 2, 64, (1 << 20) + 1, 0) == 0
