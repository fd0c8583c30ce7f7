"""Seeded synthetic merged TTA batches for the folding batched post-processing (pbn_post_batch_tta,
postprocess.refine_tta_merged_device), and their per-scene yardstick: tests/post_ref.py run on the scene's own slice with
point_num = 3 * n_j, so that its fold is `% n_j`.  numpy only; small shapes on purpose (tests/post_batch_cases.py says why).

Numbering.  A case has B scenes of n_j (folded) points and `copies` copies of each: scene j owns the merged, unfolded points
copies * point_starts[j] .. copies * point_starts[j + 1], copy after copy; point q of copy c is copies * point_starts[j] + c * n_j + q.

A case is a dict: sizes, copies, point_starts (folded), pred_sem i64[copies * N] (drawn per copy, so a class read at a folded index
is wrong), pidx i64[M, 2] (merged proposal, merged unfolded point), off [P + 1], clt f32[P], sups (per scene: i64[n_j] scene-local
ids or None), n_sp, thresholds, error_scene / error_at / error_was, and what the generator planted (`planted`: per kind a list of
merged proposal numbers) so that the CPU tier can find it again."""
import functools

import numpy as np

import post_batch_cases as B
import post_ref as R

SCORE_T, NPOINT_T, NMS_T = B.SCORE_T, B.NPOINT_T, B.NMS_T


def make_case(name, seed, sizes, n_props, copies=3, no_superpoints=(), default_bound=(), score_range=(0.05, 1.0), ties=(),
              fold_pairs=(), cross_copy=(), foreign=(), low_scenes=(), members=(3, 30), off_dtype=np.int64, error_scene=None):
    """n_props[j] proposals for scene j, each drawn inside ONE copy of the scene (as the forward makes them), interleaved by scene
    in the merged order.
    ties: (scene, i, k) -- proposal k gets the score, the copy and the point set of proposal i shifted by one point: only the tie
    rule orders the pair.
    fold_pairs: (scene, i, k) -- proposal k gets the point set of i shifted by one point but lies in the NEXT copy, both scores
    above the threshold and distinct: the pair overlaps only after the fold.
    cross_copy: (scene, i) -- every second member of proposal i (not the first) moves to the next copy.
    foreign: (scene, i, other) -- proposal i gets one more member, a point of scene `other`.
    low_scenes: every score of the scene below the score threshold.  error_scene: one id of that scene is raised to its bound."""
    rng = np.random.default_rng(seed)
    starts = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    per_scene, copy_of, scores = [], [], []
    for j, n in enumerate(sizes):
        per_scene.append([B._proposal(rng, n, members) for _ in range(n_props[j])])
        copy_of.append([int(c) for c in rng.integers(0, copies, n_props[j])])
        scores.append(rng.uniform(score_range[0], score_range[1], n_props[j]).astype(np.float32))

    def shifted(j, i):
        if per_scene[j][i].shape[0] < 8:                                           # well above the size threshold
            per_scene[j][i] = B._proposal(rng, sizes[j], (8, 20))
        pts = per_scene[j][i]
        return np.unique(np.clip(np.concatenate([pts[1:], pts[-1:] + 1]), 0, sizes[j] - 1))

    for j, i, k in ties:
        scores[j][k] = scores[j][i] = np.float32(max(float(scores[j][i]), 0.5))
        per_scene[j][k], copy_of[j][k] = shifted(j, i), copy_of[j][i]
    for j, i, k in fold_pairs:
        scores[j][i], scores[j][k] = np.float32(0.9), np.float32(0.8)
        per_scene[j][k], copy_of[j][k] = shifted(j, i), (copy_of[j][i] + 1) % copies
    for j in low_scenes:
        scores[j][:] = np.float32(0.1)
    # folded local points -> merged unfolded points
    merged = [[copies * starts[j] + copy_of[j][i] * sizes[j] + per_scene[j][i] for i in range(n_props[j])] for j in range(len(sizes))]
    for j, i in cross_copy:
        step = sizes[j] if copy_of[j][i] + 1 < copies else -(copies - 1) * sizes[j]
        merged[j][i] = merged[j][i].copy()
        merged[j][i][1::2] += step
    for j, i, other in foreign:
        merged[j][i] = np.concatenate([merged[j][i], [copies * starts[other] + int(rng.integers(0, copies * sizes[other]))]])
    tags = rng.permutation(np.repeat(np.arange(len(sizes)), n_props))              # scene of every merged proposal
    taken = [0] * len(sizes)
    rows, clt, number = [], [], {}
    for p, j in enumerate(tags):
        pts = merged[j][taken[j]]
        rows.append(np.stack([np.full(pts.shape[0], p, np.int64), pts], 1))
        clt.append(scores[j][taken[j]])
        number[(int(j), taken[j])] = p
        taken[j] += 1
    pidx = np.concatenate(rows) if rows else np.zeros((0, 2), np.int64)
    off = np.concatenate([[0], np.cumsum([r.shape[0] for r in rows])]).astype(off_dtype)
    sups, n_sp = [], []
    for j, n in enumerate(sizes):
        ids, k = B._superpoints(rng, n)
        sups.append(None if j in no_superpoints else ids)
        n_sp.append(None if (j in no_superpoints or j in default_bound) else k)
    error_at = error_was = None
    if error_scene is not None:
        error_at = int(per_scene[error_scene][0][0])                              # a point some proposal of the scene holds
        error_was = int(sups[error_scene][error_at])
        sups[error_scene][error_at] = n_sp[error_scene]
    planted = dict(ties=[(number[(j, i)], number[(j, k)]) for j, i, k in ties],
                   fold_pairs=[(number[(j, i)], number[(j, k)]) for j, i, k in fold_pairs],
                   cross_copy=[number[(j, i)] for j, i in cross_copy], foreign=[number[(j, i)] for j, i, _ in foreign])
    return dict(name=name, sizes=tuple(sizes), copies=copies, point_starts=[int(s) for s in starts], pidx=pidx, off=off,
                pred_sem=rng.integers(0, 20, copies * int(starts[-1])).astype(np.int64), clt=np.asarray(clt, np.float32), sups=sups,
                n_sp=n_sp, score_t=SCORE_T, npoint_t=NPOINT_T, nms_t=NMS_T, error_scene=error_scene, error_at=error_at,
                error_was=error_was, planted=planted)


@functools.lru_cache(maxsize=None)
def cases():
    return (
        # two scenes of different size (the pitch is scene 0's), 70 and 33 points: neither a multiple of 32; everything planted
        make_case("t2", 21, (70, 33), (18, 9), default_bound=(1,), ties=((0, 2, 7),), fold_pairs=((0, 3, 11), (1, 1, 4)),
                  cross_copy=((0, 5), (1, 2)), foreign=((0, 6, 1), (1, 3, 0))),
        # B = 1: the single-scene device form's own unit
        make_case("t1", 22, (257,), (30,), ties=((0, 1, 9),), fold_pairs=((0, 4, 12),), cross_copy=((0, 6),)),
        # scene 0 loses every proposal to the score threshold; scene 1 brings no superpoints
        make_case("low", 23, (33, 100), (7, 16), no_superpoints=(1,), low_scenes=(0,), fold_pairs=((1, 0, 5),), off_dtype=np.int32),
        # more than 256 proposals: the block scans of the per-scene kernels take two trips, the IoU grid strides
        make_case("many", 24, (257, 31), (270, 5), score_range=(0.31, 1.0), members=(5, 30), fold_pairs=((0, 10, 200),)),
        make_case("p0", 25, (70, 33), (0, 0)),
        # scene 1 holds an id AT its bound
        make_case("sp_error", 26, (70, 33), (12, 8), error_scene=1, fold_pairs=((0, 2, 6),)),
        # another number of copies: four scenes of two copies (eight batch elements)
        make_case("c2x4", 27, (70, 33, 64, 31), (10, 6, 9, 5), copies=2, no_superpoints=(2,), fold_pairs=((0, 1, 4),),
                  cross_copy=((1, 0),), foreign=((2, 3, 3),)),
    )


def case(name):
    return next(c for c in cases() if c["name"] == name)


def without_error(c):
    return B.without_error(c)


def scene_of_proposals(c):
    """Scene of every merged proposal: the scene of its first member in merged numbering (-1: none)."""
    off = c["off"].astype(np.int64)
    first = c["pidx"][off[:-1], 1] if off.shape[0] > 1 else np.zeros(0, np.int64)
    return np.searchsorted(c["copies"] * np.asarray(c["point_starts"]), first, side="right") - 1


def scene_inputs(c, j):
    """Scene j's own slice in the form post_ref.refine (and refine_instances_device) take: its proposals numbered from 0 in their
    merged order, their members INSIDE the scene's slice with points local to the slice (unfolded: 0 .. copies * n_j), the slice's
    copies * n_j labels, point_num = 3 * n_j (the yardsticks fold with % (point_num // 3)); a scene without superpoints gets
    arange(n_j)."""
    k = c["copies"]
    lo, hi = k * c["point_starts"][j], k * c["point_starts"][j + 1]
    off = c["off"].astype(np.int64)
    mine = np.nonzero(scene_of_proposals(c) == j)[0]
    rows = []
    for q, p in enumerate(mine):
        pts = c["pidx"][off[p]:off[p + 1], 1]
        pts = pts[(pts >= lo) & (pts < hi)] - lo
        rows.append(np.stack([np.full(pts.shape[0], q, np.int64), pts], 1))
    n = c["sizes"][j]
    sp = c["sups"][j]
    return dict(pred_sem=c["pred_sem"][lo:hi], pidx=np.concatenate(rows) if rows else np.zeros((0, 2), np.int64),
                off=np.concatenate([[0], np.cumsum([r.shape[0] for r in rows])]).astype(np.int64), clt=c["clt"][mine],
                point_num=3 * n, sp=np.arange(n, dtype=np.int64) if sp is None else sp,
                n_sp=n if (sp is None or c["n_sp"][j] is None) else c["n_sp"][j], merged_proposals=mine)


def _refine(c, i, point_num, sp, n_sp):
    r = R.refine(i["pred_sem"], i["pidx"], i["off"], i["clt"], point_num, sp, c["score_t"], c["npoint_t"], c["nms_t"], n_superpoints=n_sp)
    r["npoints"] = r["counts2"][r["keep"]].astype(np.int32)
    return r


@functools.lru_cache(maxsize=None)
def reference(name):
    """post_ref.refine per scene of the case, computed once and shared (do not modify)."""
    c = case(name)
    out = []
    for j in range(len(c["sizes"])):
        i = scene_inputs(c, j)
        out.append(_refine(c, i, i["point_num"], i["sp"], i["n_sp"]))
    return out


@functools.lru_cache(maxsize=None)
def reference_without_fold(name):
    """What an implementation that forgets the fold computes: post_ref.refine per scene over the copies * n_j unfolded points
    (point_num = 3 * copies * n_j makes its fold the identity; every copy of a point keeps the point's superpoint)."""
    c = case(name)
    out = []
    for j in range(len(c["sizes"])):
        i = scene_inputs(c, j)
        k, n = c["copies"], c["sizes"][j]
        out.append(_refine(c, i, 3 * k * n, np.tile(i["sp"], k), i["n_sp"]))
    return out
