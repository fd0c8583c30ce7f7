"""Seeded synthetic merged batches for the batched post-processing (csrc/post_batch.hip, postprocess.refine_batch_device), and
their per-scene yardstick: tests/post_ref.py run on each scene's own rows with point_num = 3 * n_j (the fold is then the
identity).  numpy only.  The shapes are small on purpose -- these are the sizes at which the kernels can go wrong (bitset word
edges inside and at the ends of scenes, a scene of one point, eight scenes, interleaved proposals), not the workload's.

A case is a dict: sizes, point_starts, pred_sem i64[N], pidx i64[M, 2] (merged proposal, merged point), off [P + 1], clt f32[P],
sups (per scene: i64[n_j] scene-local ids or None), n_sp (per scene bound or None = default), thresholds, error_scene (with
error_at, the scene-local point whose id was raised to the bound, and error_was, its id before)."""
import functools

import numpy as np

import post_ref as R

SIZES = (70, 33, 257, 1, 64, 100, 31, 96)
SCORE_T, NPOINT_T, NMS_T = 0.3, 4, 0.3


def _superpoints(rng, n):
    """Runs of 4..14 neighbouring points share an id; ids 0..k-1 in order."""
    ids, k = np.empty(n, np.int64), 0
    at = 0
    while at < n:
        run = int(rng.integers(4, 15))
        ids[at:at + run] = k
        at, k = at + run, k + 1
    return ids, k


def _proposal(rng, n, members):
    """3..30 points out of a window of neighbouring points (so that proposals overlap and superpoints are shared)."""
    m = min(n, int(rng.integers(members[0], members[1] + 1)))
    span = min(n, m + m // 3)
    start = int(rng.integers(0, n - span + 1))
    return np.sort(start + rng.permutation(span)[:m]).astype(np.int64)


def make_case(name, seed, sizes, n_props, no_superpoints=(), default_bound=(), score_range=(0.05, 1.0), ties=(), members=(3, 30),
              off_dtype=np.int64, error_scene=None):
    """n_props[j] proposals for scene j, interleaved by scene in the merged order (each scene's own order kept).
    ties: (scene a, local proposal i, scene b, local proposal k) -- proposal k of scene b gets the score AND (inside one scene) the
    point set of proposal i shifted by one point, so the pair overlaps and only the tie rule orders it.
    error_scene: one id of that scene is raised to the scene's bound."""
    rng = np.random.default_rng(seed)
    starts = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    per_scene, scores = [], []
    for j, n in enumerate(sizes):
        per_scene.append([_proposal(rng, n, members) for _ in range(n_props[j])])
        scores.append(rng.uniform(score_range[0], score_range[1], n_props[j]).astype(np.float32))
    for a, i, b, k in ties:
        scores[b][k] = scores[a][i] = np.float32(max(float(scores[a][i]), 0.5))
        if a == b:
            if per_scene[a][i].shape[0] < 8:                                       # well above the size threshold
                per_scene[a][i] = _proposal(rng, sizes[a], (8, 20))
            pts = per_scene[a][i]
            per_scene[b][k] = np.unique(np.clip(np.concatenate([pts[1:], pts[-1:] + 1]), 0, sizes[a] - 1))
    tags = rng.permutation(np.repeat(np.arange(len(sizes)), n_props))          # scene of every merged proposal
    taken = [0] * len(sizes)
    rows, clt = [], []
    for p, j in enumerate(tags):
        pts = per_scene[j][taken[j]] + starts[j]
        rows.append(np.stack([np.full(pts.shape[0], p, np.int64), pts], 1))
        clt.append(scores[j][taken[j]])
        taken[j] += 1
    pidx = np.concatenate(rows) if rows else np.zeros((0, 2), np.int64)
    off = np.concatenate([[0], np.cumsum([r.shape[0] for r in rows])]).astype(off_dtype)
    sups, n_sp = [], []
    for j, n in enumerate(sizes):
        ids, k = _superpoints(rng, n)
        sups.append(None if j in no_superpoints else ids)
        n_sp.append(None if (j in no_superpoints or j in default_bound) else k)
    error_at = error_was = None
    if error_scene is not None:
        error_at = int(per_scene[error_scene][0][0])                              # a point some proposal of the scene holds
        error_was = int(sups[error_scene][error_at])
        sups[error_scene][error_at] = n_sp[error_scene]
    return dict(name=name, sizes=tuple(sizes), point_starts=[int(s) for s in starts], pidx=pidx, off=off,
                pred_sem=rng.integers(0, 20, int(starts[-1])).astype(np.int64), clt=np.asarray(clt, np.float32), sups=sups,
                n_sp=n_sp, score_t=SCORE_T, npoint_t=NPOINT_T, nms_t=NMS_T, error_scene=error_scene, error_at=error_at,
                error_was=error_was)


@functools.lru_cache(maxsize=None)
def cases():
    s = SIZES
    out = [
        # B = 8: scene 3 is one point (its proposal fails the size threshold), scene 4 has no proposals, scene 5 no superpoints,
        # scene 6 only scores below the threshold (see below); equal scores inside scene 0 and across scenes 0 and 2
        make_case("b8", 11, s, (14, 6, 28, 1, 0, 16, 5, 12), no_superpoints=(5,), default_bound=(1,),
                  ties=((0, 2, 0, 7), (0, 2, 2, 3))),
        make_case("b1", 12, (257,), (30,), ties=((0, 1, 0, 9),)),
        make_case("b2", 13, (70, 33), (12, 7), default_bound=(0, 1), off_dtype=np.int32),
        make_case("b3", 14, (33, 257, 1), (6, 26, 2), no_superpoints=(0,)),
        # fixed grids stride more than once: >= 120 survivors in scene 0 (14 400 live pairs on a grid of 8192), 3 in scene 1
        make_case("stride", 15, (257, 31), (140, 3), score_range=(0.31, 1.0), members=(5, 30)),
        make_case("p0", 16, (70, 33), (0, 0)),
        # the middle scene holds an id AT its bound: row sp_start[2] of the flat table is the next scene's first row
        make_case("sp_error", 17, (70, 33, 257), (10, 6, 20), error_scene=1),
    ]
    low = out[0]                                                        # scene 6 of b8: every score below the threshold
    first = low["pidx"][low["off"][:-1].astype(np.int64), 1]
    low["clt"][(first >= low["point_starts"][6]) & (first < low["point_starts"][7])] = np.float32(0.1)
    return tuple(out)


def case(name):
    return next(c for c in cases() if c["name"] == name)


def without_error(c):
    """The error case with the raised id put back: the same batch, every id in range."""
    sups = list(c["sups"])
    sups[c["error_scene"]] = c["sups"][c["error_scene"]].copy()
    sups[c["error_scene"]][c["error_at"]] = c["error_was"]
    return dict(c, name=c["name"] + "_clean", sups=sups, error_scene=None, error_at=None, error_was=None)


def scene_inputs(c, j):
    """Scene j's own rows in the form post_ref.refine (and refine_instances_device) take: proposals numbered from 0 in their
    merged order, points local to the scene, point_num = 3 * n_j; a scene without superpoints gets arange(n_j)."""
    lo, hi = c["point_starts"][j], c["point_starts"][j + 1]
    off = c["off"].astype(np.int64)
    first = c["pidx"][off[:-1], 1] if off.shape[0] > 1 else np.zeros(0, np.int64)
    mine = np.nonzero((first >= lo) & (first < hi))[0]
    rows = [np.stack([np.full(off[p + 1] - off[p], q, np.int64), c["pidx"][off[p]:off[p + 1], 1] - lo], 1) for q, p in enumerate(mine)]
    n = hi - lo
    sp = c["sups"][j]
    return dict(pred_sem=c["pred_sem"][lo:hi], pidx=np.concatenate(rows) if rows else np.zeros((0, 2), np.int64),
                off=np.concatenate([[0], np.cumsum([r.shape[0] for r in rows])]).astype(np.int64), clt=c["clt"][mine],
                point_num=3 * n, sp=np.arange(n, dtype=np.int64) if sp is None else sp,
                n_sp=n if (sp is None or c["n_sp"][j] is None) else c["n_sp"][j], merged_proposals=mine)


@functools.lru_cache(maxsize=None)
def reference(name):
    """post_ref.refine per scene of the case, computed once and shared (do not modify)."""
    c = case(name)
    out = []
    for j in range(len(c["sizes"])):
        i = scene_inputs(c, j)
        r = R.refine(i["pred_sem"], i["pidx"], i["off"], i["clt"], i["point_num"], i["sp"], c["score_t"], c["npoint_t"], c["nms_t"],
                     n_superpoints=i["n_sp"])
        r["npoints"] = r["counts2"][r["keep"]].astype(np.int32)
        out.append(r)
    return out


def greedy_nms_other_tie_rule(ious, scores, threshold):
    """post_ref.greedy_nms with the OPPOSITE tie rule (among equal scores the higher survivor index first)."""
    s = np.asarray(scores)
    order = np.lexsort((-np.arange(s.shape[0]), -s.astype(np.float64)))
    suppressed = np.zeros(s.shape[0], bool)
    pick = []
    for it in order:
        if suppressed[it]:
            continue
        pick.append(it)
        suppressed |= ious[it] > np.float32(threshold)
    return np.array(pick, np.int32)
