"""The device stages that work on points and not on a mesh: what pbnet_amd.mesh.decode_points chains together.

knn_graph, point_normals, knn_edges, radius_count, radius_outlier_mask, radius_raw_index (csrc/cloud.hip), orient_normals
(csrc/orient.hip), fit_plane, upright (csrc/upright.hip), thin_points, outlier_mask, raw_index (csrc/thin.hip), carry_labels
and vote_labels (csrc/vote.hip); pbnet_amd/mesh.py's docstring says in a line what each is, and each states its contract.
Every function checks in one order: values, dtypes and shapes on the host, then the tensors' device, then the library.
There is no CPU path: a missing library or a CPU tensor raises."""
import ctypes

import numpy as np
import torch

from . import _native as N

# The status bits the stages of the scan chain share (csrc/scan_dev.h, SCAN_*): a coordinate is NaN or infinite; an axis spans
# 2^21 cells or more of thin_points' pitch; the device sort gave up; a link chain of orient_normals did not end.
CLOUD_NONFINITE, CLOUD_EXTENT, CLOUD_SORT_SPIN, CLOUD_WALK_CAP = 1, 2, 8, 16
CLOUD_MAX_K = 32                                             # csrc/scan_dev.h: SCAN_MAX_K = pbn_cloud_max_k(), known without the library
VOTE_SEM_RANGE, VOTE_INS_RANGE, VOTE_ROW_RANGE = 1, 2, 4     # pbn_cloud_vote_labels' own status bits, next to CLOUD_SORT_SPIN
VOTE_MAX_CLASSES, VOTE_MAX_INS = 1023, (1 << 21) - 1         # n_classes in 1..1023; instance ids in 0..2^21 - 2

CLOUD_STAGES = ("box", "keys + sort", "cell table", "search")
ORIENT_STAGES = ("edge codes", "rounds", "tail")
THIN_STAGES = ("box + keys", "low-word sort", "high-word keys + sort", "run heads + scan", "cells")
RADIUS_STAGES = ("box", "keys + sort", "cell table", "count")
UPRIGHT_STAGES = ("hypotheses", "score", "select + refit", "apply")
VOTE_STAGES = ("fill + keys", "key sort", "row pairs + row sort", "run heads + scan + starts", "pick", "compaction")
RADIUS_MAX_CAP, UPRIGHT_MAX_HYP = (1 << 31) - 1, 4096        # the second is csrc/upright.hip's UPR_MAX_HYP = pbn_cloud_upright_max_hyp()
UPRIGHT_KEYS = ("threshold", "hypotheses", "seed", "up_hint", "max_tilt", "below_frac")


# ------------------------------------------------------------------------------------------ argument checks, stated once
def _got(t):
    return "%s %s" % (t.dtype, tuple(t.shape)) if torch.is_tensor(t) else type(t).__name__


def _f32(name, t, cols=3):
    """`t` is a float32 [n, cols] tensor (cols None = [n, k], any width): n."""
    if not torch.is_tensor(t) or t.dtype != torch.float32 or t.dim() != 2 or (cols is not None and t.shape[1] != cols):
        raise TypeError("%s must be a float32 [n, %s] tensor, got %s" % (name, cols or "k", _got(t)))
    return int(t.shape[0])


def _i32(name, t, *shape):
    """`t` is an int32 tensor of `shape`: an int is an axis' required size, a string only its name in the message."""
    if not torch.is_tensor(t) or t.dtype != torch.int32 or t.dim() != len(shape) or \
            any(isinstance(s, int) and t.shape[a] != s for a, s in enumerate(shape)):
        raise TypeError("%s must be an int32 [%s] tensor, got %s" % (name, ", ".join(map(str, shape)), _got(t)))


def _bool(name, t, m="m"):
    """`t` is a bool [m] tensor (m an int = the required length): its length."""
    if not torch.is_tensor(t) or t.dtype != torch.bool or t.dim() != 1 or (isinstance(m, int) and t.shape[0] != m):
        raise TypeError("%s must be a bool [%s] tensor, got %s" % (name, m, _got(t)))
    return int(t.shape[0])


def _int_in(what, name, v, lo, hi, shown):
    """An int (not a bool) in lo..hi, which the message shows as `shown`."""
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= int(v) <= hi:
        raise ValueError("%s: %s must be an int in %s, got %r" % (what, name, shown, v))
    return int(v)


def _real(what, name, v, kind="a number"):
    if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)):
        raise TypeError("%s: %s must be %s, got %r" % (what, name, kind, v))
    return v


def _positive_f32(what, name, v):
    """A radius or threshold as the float32 the device computes with: positive and finite after the rounding."""
    with np.errstate(over="ignore"):
        f = np.float32(v)
    if not (np.isfinite(f) and f > 0):
        raise ValueError("%s: %s must be positive and finite as a float32, got %r" % (what, name, v))
    return float(f)


def _k(what, k):
    if not 1 <= k <= CLOUD_MAX_K:
        raise ValueError("%s: k must lie in 1..%d, got %d" % (what, CLOUD_MAX_K, k))
    return k


def _cell(what, cell):
    """The grid's cell size as the library takes it: 0 = choose."""
    h = 0.0 if cell is None else float(cell)
    if cell is not None and not h > 0.0:
        raise ValueError("%s: cell must be positive, got %r" % (what, cell))
    return h


# The status word, per stage: the bits that speak of the input, as (bit, message), and what any other bit means there.
_NONFINITE = (CLOUD_NONFINITE, "a coordinate is NaN or infinite")
_SORT = "the device sort gave up (status %(status)d)"
_STATUS = {
    **dict.fromkeys(("knn_graph", "radius_count", "radius_raw_index"), ((_NONFINITE,), _SORT)),
    **dict.fromkeys(("fit_plane", "upright"), ((_NONFINITE,), "status %(status)d")),
    "thin_points": ((_NONFINITE, (CLOUD_EXTENT, "the cloud spans 2^21 cells or more of pitch %(pitch)r on an axis")), _SORT),
    "orient_normals": ((), "a link chain did not end (status %(status)d)"),
    "frames_to_points": ((), "the write pass met more valid pixels than the count pass: the frames changed between the two "
                             "(status %(status)d)"),
    "vote_labels": (((VOTE_SEM_RANGE, "a semantic label is %(n_classes)d or more"),
                     (VOTE_INS_RANGE, "an instance label is %(max_ins)d or more"),
                     (VOTE_ROW_RANGE, "a row lies outside [-1, %(m)d)")), _SORT),
}


def _scan_status(what, status, **details):
    """Raise what a stage's status word says: ValueError for the first input bit set, RuntimeError for anything else."""
    if status:
        details.update(status=status, max_ins=VOTE_MAX_INS)
        inputs, other = _STATUS[what]
        for bit, text in inputs:
            if status & bit:
                raise ValueError("%s: %s" % (what, text % details))
        raise RuntimeError("%s: %s" % (what, other % details))


def _device(*tensors):
    """After the host's checks: every tensor lives on the device (None passes); they come back contiguous."""
    N.require_cuda(*tensors)
    return [t if t is None else t.contiguous() for t in tensors]


def _scan_workspace(nbytes, dev, what, kind="point cloud"):
    """The workspace of a stage of the scan chain; 0 bytes is the library's refusal of the size."""
    if nbytes == 0:
        raise ValueError("%s too large for the library: %s" % (kind, what))
    return torch.empty(nbytes, dtype=torch.uint8, device=dev)


def _staged_call(entry, args, stages, times):
    """pbn_<entry>, or with `times` (a dict) pbn_<entry>_timed, which synchronises and adds its time per stage in ms."""
    if times is None:
        N.check(getattr(N.lib(), "pbn_" + entry)(*args), "pbn_" + entry)
        return
    t = (ctypes.c_float * len(stages))()
    N.check(getattr(N.lib(), "pbn_%s_timed" % entry)(*args, t), "pbn_%s_timed" % entry)
    times.update({name: float(t[i]) for i, name in enumerate(stages)})


# ---------------------------------------------------------------------------------------------------- point clouds
def knn_graph(xyz, k=16, cell=None, times=None):
    """The exact k nearest neighbours of every point (csrc/cloud.hip): idx int32 [N, k] and d2 float32 [N, k] on the
    device, in the caller's point order.  d2 = ((dx*dx + dy*dy) + dz*dz) in float32; a row holds the k points j != i with
    the smallest (bits of d2, j), ascending; when N - 1 < k it ends in idx = -1, d2 = +inf.  `cell` (the grid's cell size;
    None lets the library choose) changes the speed, never the result.  A non-finite coordinate raises ValueError."""
    n, k, h = _f32("xyz", xyz), _k("knn_graph", int(k)), _cell("knn_graph", cell)
    xyz = _device(xyz)[0]
    dev = xyz.device
    ws = _scan_workspace(N.lib().pbn_cloud_workspace_bytes(n, k), dev, "%d points" % n)
    idx = torch.empty(n, k, dtype=torch.int32, device=dev)
    d2 = torch.empty(n, k, dtype=torch.float32, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    args = (N.ptr(xyz), n, k, h, N.ptr(idx), N.ptr(d2), N.ptr(status), N.ptr(ws), ws.numel(), N.current_stream())
    _staged_call("cloud_knn", args, CLOUD_STAGES, times)
    _scan_status("knn_graph", int(status.item()))
    return idx, d2


def point_normals(xyz, idx, viewpoint=None, views=None, view_of=None):
    """PCA normals over each point and its neighbours `idx` (int32 [N, k], -1 = none): float32 [N, 3] on the device, the
    float64 eigenvector of the smallest covariance eigenvalue, turned towards `viewpoint` (three numbers or a tensor; None
    = the float64 mean of xyz).  Fewer than three points in a neighbourhood give the zero vector.

    With `views` (f32 [V, 3]) and `view_of` (int32 [N]), both or neither and not together with `viewpoint`, every normal is
    turned towards its own point's viewpoint views[view_of[i]] -- the sensor position that saw the point -- by the same
    test; a view_of outside [0, V) leaves the eigenvector's sign as it is."""
    n = _f32("xyz", xyz)
    _i32("idx", idx, n, "k")
    if (views is None) != (view_of is None):
        raise ValueError("point_normals: give both views and view_of, or neither")
    if views is not None:
        if viewpoint is not None:
            raise ValueError("point_normals: viewpoint and views are two ways to turn the normals, give one")
        n_views = _f32("views", views)
        _i32("view_of", view_of, n)
        xyz, idx, views, view_of = _device(xyz, idx, views, view_of)
        nl = torch.empty(n, 3, dtype=torch.float32, device=xyz.device)
        N.check(N.lib().pbn_cloud_normals_views(N.ptr(xyz), n, N.ptr(idx), int(idx.shape[1]), N.ptr(views), n_views,
                                                N.ptr(view_of), N.ptr(nl), N.current_stream()), "pbn_cloud_normals_views")
        return nl
    xyz, idx = _device(xyz, idx)
    k = int(idx.shape[1])
    if viewpoint is None:
        vp = xyz.double().mean(0).float() if n else torch.zeros(3, dtype=torch.float32, device=xyz.device)
    elif torch.is_tensor(viewpoint):
        vp = viewpoint.to(device=xyz.device, dtype=torch.float32).reshape(3)
    else:
        vp = torch.tensor([float(v) for v in viewpoint], dtype=torch.float32).reshape(3).to(xyz.device)
    vp = vp.contiguous()
    nl = torch.empty(n, 3, dtype=torch.float32, device=xyz.device)
    N.check(N.lib().pbn_cloud_normals(N.ptr(xyz), n, N.ptr(idx), k, N.ptr(vp), N.ptr(nl), N.current_stream()),
            "pbn_cloud_normals")
    return nl


def knn_edges(idx):
    """The kNN graph as segment_point's edges: int64 [E, 2] rows (i, idx[i, r]), i-major and rank-minor, -1 entries
    dropped."""
    n, k = int(idx.shape[0]), int(idx.shape[1])
    src = torch.arange(n, dtype=torch.int64, device=idx.device).repeat_interleave(k)
    dst = idx.reshape(-1).to(torch.int64)
    keep = dst >= 0
    return torch.stack([src[keep], dst[keep]], dim=1)


def orient_normals(nl, idx, times=None):
    """Consistent signs for a cloud's normals (csrc/orient.hip; Hoppe et al. 1992, PCL / Open3D's
    orient_normals_consistent_tangent_plane).  `nl` f32 [N, 3] (point_normals), `idx` int32 [N, k] (knn_graph, -1 or
    anything outside [0, N) = no neighbour).  Slot e = i * k + r is an edge (i, idx[i, r]) of weight 1 - |n_i . n_j| in
    float32 and key (order bits of the weight, e); the signs are propagated along the minimum spanning forest under that
    key -- unique, because the keys are distinct -- with s_a ^ s_b = (n_a . n_b < 0) on its edges.  Per tree the assignment
    that keeps more input signs wins, and on a tie the one that keeps the tree's lowest-index point.  A point whose normal
    is zero or not finite is null: no edges, never flipped, a tree of its own.

    Returns a dict on the device: nl f32 [N, 3] (rows negated exactly where flipped), flipped bool [N], tree int32 [N]
    (the lowest point index of the point's tree), stats int32 [4] (trees among the non-null points, flipped points, null
    points, 0) and rounds (int: the Boruvka rounds that merged something).  One read-back (status and rounds); integer
    atomics only, so two runs give the same bytes.  `times` (a dict) takes the stage times of the measurement entry, which
    synchronises."""
    n = _f32("nl", nl)
    _i32("idx", idx, n, "k")
    k = _k("orient_normals", int(idx.shape[1]))
    if n * k > (1 << 31) - 1:
        raise ValueError("orient_normals: %d points x %d neighbours exceed 2^31 - 1 edge slots" % (n, k))
    nl, idx = _device(nl, idx)
    dev = nl.device
    ws = _scan_workspace(N.lib().pbn_cloud_orient_workspace_bytes(n, k), dev, "%d points, k = %d" % (n, k))
    out = torch.empty(n, 3, dtype=torch.float32, device=dev)
    flipped = torch.empty(n, dtype=torch.bool, device=dev)
    tree = torch.empty(n, dtype=torch.int32, device=dev)
    stats = torch.empty(4, dtype=torch.int32, device=dev)
    status = torch.zeros(2, dtype=torch.int32, device=dev)
    args = (N.ptr(nl), n, N.ptr(idx), k, N.ptr(out), N.ptr(flipped), N.ptr(tree), N.ptr(stats), N.ptr(status), N.ptr(ws),
            ws.numel(), N.current_stream())
    _staged_call("cloud_orient", args, ORIENT_STAGES, times)
    st, rounds = (int(v) for v in status.tolist())           # the one read-back
    _scan_status("orient_normals", st)
    return {"nl": out, "flipped": flipped, "tree": tree, "stats": stats, "rounds": rounds}


# ------------------------------------------------------------------------------------------------------- raw scans
def thin_points(xyz, colours=None, pitch=0.02, times=None):
    """One point per occupied cell of a grid of `pitch` (csrc/thin.hip).  The grid starts at the per-axis float32 minimum;
    cell = floor((double(p) - double(origin)) / pitch); rows come in ascending order of cz << 42 | cy << 21 | cx.  Returns a
    dict on the device: xyz f32 [M, 3] (the float32 rounding of the float64 mean of a cell's members, summed in ascending
    point index), rgb f32 [M, 3] likewise when `colours` (f32 [N, 3]) are given, count int32 [M] (members), first int32 [M]
    (the lowest member index) and inverse int32 [N] (the row of every input point).  One read-back (status and M); a
    non-finite coordinate or an extent of 2^21 cells or more on an axis raises ValueError."""
    pitch = float(pitch)
    if not (pitch > 0.0 and np.isfinite(pitch)):
        raise ValueError("thin_points: pitch must be positive and finite, got %r" % (pitch,))
    n = _f32("xyz", xyz)
    if colours is not None:
        _f32("colours", colours)
        if colours.shape[0] != n:
            raise ValueError("thin_points: %d colours for %d points" % (colours.shape[0], n))
    xyz, rgb = _device(xyz, colours)
    dev = xyz.device
    ws = _scan_workspace(N.lib().pbn_thin_workspace_bytes(n), dev, "%d points" % n)
    out_xyz = torch.empty(n, 3, dtype=torch.float32, device=dev)
    out_rgb = torch.empty(n, 3, dtype=torch.float32, device=dev) if rgb is not None else None
    count, first, inverse = (torch.empty(n, dtype=torch.int32, device=dev) for _ in range(3))
    result = torch.empty(2, dtype=torch.int32, device=dev)
    args = (N.ptr(xyz), N.ptr(rgb), n, pitch, N.ptr(out_xyz), N.ptr(out_rgb), N.ptr(count), N.ptr(first), N.ptr(inverse),
            N.ptr(result), N.ptr(ws), ws.numel(), N.current_stream())
    _staged_call("thin_points", args, THIN_STAGES, times)
    st, m = (int(v) for v in result.tolist())                # the one read-back
    _scan_status("thin_points", st, pitch=pitch)
    out = {"xyz": out_xyz[:m], "count": count[:m], "first": first[:m], "inverse": inverse}
    if rgb is not None:
        out["rgb"] = out_rgb[:m]
    return out


def outlier_mask(d2, ratio=2.0):
    """Statistical outlier removal on knn_graph's d2 (f32 [N, k]): m_i = the float64 mean of sqrt(d2[i, r]) over the finite
    entries, mu and sigma (population) over the rows that have one, keep_i = m_i <= mu + ratio * sigma.  Returns keep (bool
    [N]) and stats (float64 [3]: mu, sigma, n_valid), both on the device; every sum has a fixed shape (csrc/thin.hip), so
    two runs give the same bytes.  A row without a finite entry is not kept."""
    ratio = float(ratio)
    if not (ratio >= 0.0 and np.isfinite(ratio)):
        raise ValueError("outlier_mask: ratio must be finite and >= 0, got %r" % (ratio,))
    n, k = _f32("d2", d2, None), _k("outlier_mask", int(d2.shape[1]))
    d2, dev, lib = _device(d2)[0], d2.device, N.lib()
    ws = _scan_workspace(lib.pbn_cloud_outlier_workspace_bytes(n), dev, "%d points" % n)
    keep = torch.empty(n, dtype=torch.bool, device=dev)
    stats = torch.empty(3, dtype=torch.float64, device=dev)
    N.check(lib.pbn_cloud_outlier_mask(N.ptr(d2), n, k, ratio, N.ptr(keep), N.ptr(stats), N.ptr(ws), ws.numel(),
                                       N.current_stream()), "pbn_cloud_outlier_mask")
    return keep, stats


def raw_index(inverse, keep, idx):
    """For every raw point the row, among the kept points, that speaks for it: int32 [N_raw] on the device.  With
    t = inverse[i]: t's row among the kept points (the exclusive scan of keep) when keep[t]; else the row of the first kept
    neighbour in rank order in idx[t, :]; else -1.  `inverse` int32 [N_raw] (thin_points), `keep` bool [M] (outlier_mask),
    `idx` int32 [M, k] (knn_graph over the same M points)."""
    _i32("inverse", inverse, "n")
    m = _bool("keep", keep)
    _i32("idx", idx, m, "k")
    n_raw, k = int(inverse.shape[0]), _k("raw_index", int(idx.shape[1]))
    (inverse, keep, idx), lib = _device(inverse, keep, idx), N.lib()
    ws = _scan_workspace(lib.pbn_cloud_raw_index_workspace_bytes(m), inverse.device, "%d points" % m)
    out = torch.empty(n_raw, dtype=torch.int32, device=inverse.device)
    N.check(lib.pbn_cloud_raw_index(N.ptr(inverse), n_raw, N.ptr(keep), N.ptr(idx), m, k, N.ptr(out), N.ptr(ws), ws.numel(),
                                    N.current_stream()), "pbn_cloud_raw_index")
    return out


def radius_count(xyz, radius, cap=None, cell=None, times=None):
    """The number of other points within `radius` of every point (csrc/cloud.hip): count int32 [N] on the device, in the
    caller's point order.  rf = float32(radius), r2 = rf * rf in float32; j counts for i when j != i and knn_graph's
    d2(i, j) <= r2, so coincident points count at 0.  count = min(neighbours, cap): `cap` is an int in 1..2^31 - 1 (None =
    2^31 - 1) at which a query stops looking.  `cell` (the grid's cell size; None = a hair above the radius) changes the
    speed, never the result.  One read-back (the status); a non-finite coordinate raises ValueError.  `times` (a dict)
    takes the stage times of the measurement entry, which synchronises."""
    rf, h = _positive_f32("radius_count", "radius", radius), _cell("radius_count", cell)
    cap = _int_in("radius_count", "cap", RADIUS_MAX_CAP if cap is None else cap, 1, RADIUS_MAX_CAP, "1..2^31 - 1")
    _f32("xyz", xyz)
    xyz, n, dev = _device(xyz)[0], int(xyz.shape[0]), xyz.device
    ws = _scan_workspace(N.lib().pbn_cloud_radius_workspace_bytes(n), dev, "%d points" % n)
    count = torch.empty(n, dtype=torch.int32, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    args = (N.ptr(xyz), n, rf, cap, h, N.ptr(count), N.ptr(status), N.ptr(ws), ws.numel(), N.current_stream())
    _staged_call("cloud_radius_count", args, RADIUS_STAGES, times)
    _scan_status("radius_count", int(status.item()))         # the one read-back
    return count


def radius_outlier_mask(xyz, radius, min_pts, cell=None):
    """Radius outlier removal (PCL's RadiusOutlierRemoval, Open3D's remove_radius_outlier): keep bool [N] on the device,
    keep[i] = at least `min_pts` (>= 1) other points lie within `radius` of point i.  It is
    radius_count(xyz, radius, cap=min_pts) >= min_pts: the count stops at min_pts, and the comparison is a torch
    expression on the device."""
    min_pts = _int_in("radius_outlier_mask", "min_pts", min_pts, 1, RADIUS_MAX_CAP, "1..2^31 - 1")
    return radius_count(xyz, radius, cap=min_pts, cell=cell) >= min_pts


def radius_raw_index(inverse, keep, xyz, radius, cell=None):
    """raw_index without a kNN graph: int32 [N_raw] on the device.  With t = inverse[i]: t's row among the kept points (the
    exclusive scan of keep) when keep[t]; else the row of the KEPT point j with the smallest (bits of d2(t, j), j) among
    those with d2(t, j) <= r2 (radius_count's d2 and r2) -- a dropped point is never an answer, however near; else -1.
    `inverse` int32 [N_raw] (thin_points), `keep` bool [M] (radius_outlier_mask), `xyz` f32 [M, 3] (the same M points).
    One read-back (the status)."""
    rf, h = _positive_f32("radius_raw_index", "radius", radius), _cell("radius_raw_index", cell)
    m = _f32("xyz", xyz)
    _i32("inverse", inverse, "n")
    _bool("keep", keep, m)
    inverse, keep, xyz = _device(inverse, keep, xyz)
    n_raw, dev = int(inverse.shape[0]), inverse.device
    ws = _scan_workspace(N.lib().pbn_cloud_radius_raw_index_workspace_bytes(m, n_raw), dev,
                         "%d points, %d raw points" % (m, n_raw))
    out = torch.empty(n_raw, dtype=torch.int32, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    N.check(N.lib().pbn_cloud_radius_raw_index(N.ptr(xyz), m, N.ptr(keep), rf, h, N.ptr(inverse), n_raw, N.ptr(out),
                                               N.ptr(status), N.ptr(ws), ws.numel(), N.current_stream()),
            "pbn_cloud_radius_raw_index")
    _scan_status("radius_raw_index", int(status.item()))     # the one read-back
    return out


# ------------------------------------------------------------------------------------------ floor plane, upright frame
def _upright_args(what, xyz, threshold, hypotheses, seed, up_hint, max_tilt, below_frac):
    """fit_plane's checks, values and dtypes before the device or the library: (float32 threshold, H, seed, the float64
    unit hint as a ctypes double[3] or None, cos(max_tilt), max_below)."""
    tf = _positive_f32(what, "threshold", _real(what, "threshold", threshold))
    n_hyp = _int_in(what, "hypotheses", hypotheses, 1, UPRIGHT_MAX_HYP, "1..%d" % UPRIGHT_MAX_HYP)
    seed = _int_in(what, "seed", seed, 0, (1 << 64) - 1, "0..2^64 - 1")
    hint = None
    if up_hint is not None:
        try:
            h = np.asarray(up_hint.detach().cpu().numpy() if torch.is_tensor(up_hint) else up_hint, dtype=np.float64).reshape(-1)
        except (TypeError, ValueError):
            raise TypeError("%s: up_hint must be three numbers, got %r" % (what, up_hint)) from None
        if h.shape != (3,) or not np.all(np.isfinite(h)):
            raise ValueError("%s: up_hint must be three finite numbers, got %r" % (what, up_hint))
        length = np.sqrt((h[0] * h[0] + h[1] * h[1]) + h[2] * h[2])
        if not (length > 0 and np.isfinite(length)):
            raise ValueError("%s: up_hint must have a non-zero length, got %r" % (what, up_hint))
        hint = (ctypes.c_double * 3)(*(float(v) for v in h / length))
    if not 0.0 < float(_real(what, "max_tilt", max_tilt, "a number of degrees")) <= 90.0:
        raise ValueError("%s: max_tilt must lie in (0, 90] degrees, got %r" % (what, max_tilt))
    if below_frac is not None and not 0.0 <= float(_real(what, "below_frac", below_frac, "a number or None")) <= 1.0:
        raise ValueError("%s: below_frac must lie in [0, 1] or be None, got %r" % (what, below_frac))
    n = _f32("xyz", xyz)
    max_below = -1 if below_frac is None else int(float(below_frac) * n)
    return tf, n_hyp, seed, hint, float(np.cos(np.deg2rad(np.float64(max_tilt)))), max_below


def _upright(what, rotate, xyz, threshold, hypotheses, seed, up_hint, max_tilt, below_frac, times, chunk=None):
    tf, n_hyp, seed, hint, cos_tilt, max_below = _upright_args(what, xyz, threshold, hypotheses, seed, up_hint, max_tilt,
                                                               below_frac)
    xyz, n, dev = _device(xyz)[0], int(xyz.shape[0]), xyz.device
    ws = _scan_workspace(N.lib().pbn_cloud_upright_workspace_bytes(n, n_hyp), dev, "%d points" % n)
    out = torch.empty(n, 3, dtype=torch.float32, device=dev) if rotate else None
    floor = torch.empty(n, dtype=torch.bool, device=dev)
    height = torch.empty(n, dtype=torch.float32, device=dev)
    f64 = torch.empty(4 + 9 + 10, dtype=torch.float64, device=dev)       # plane, R, moments
    plane, R, moments = f64[:4], f64[4:13], f64[13:]
    plane0 = torch.empty(4, dtype=torch.float32, device=dev)
    res = torch.zeros(9, dtype=torch.int32, device=dev)                  # info[8], status
    head = (N.ptr(xyz), n, tf, n_hyp, seed, hint, cos_tilt, max_below)
    tail = (N.ptr(out), N.ptr(floor), N.ptr(height), N.ptr(plane), N.ptr(plane0), N.ptr(R), N.ptr(moments), N.ptr(res),
            N.ptr(res[8:]), N.ptr(ws), ws.numel(), N.current_stream())
    if chunk is None:
        _staged_call("cloud_upright", head + tail, UPRIGHT_STAGES, times)
    else:                                                    # the score kernel's launch geometry, for the tests
        N.check(N.lib().pbn_cloud_upright_chunked(*head, int(chunk), *tail), "pbn_cloud_upright_chunked")
    host = res.tolist()                                      # the one read-back
    _scan_status(what, host[8])
    r = {"plane": plane, "plane0": plane0, "floor": floor, "height": height, "moments": moments, "info": res[:8],
         "found": bool(host[0]), "hypothesis": host[1], "inliers": host[2]}
    if rotate:
        r.update(R=R.reshape(3, 3), xyz=out)
    return r


def fit_plane(xyz, threshold, hypotheses=1024, seed=0, up_hint=None, max_tilt=30.0, below_frac=0.01, times=None):
    """The floor plane of a scan (csrc/upright.hip; PCL / Open3D's segment_plane): `hypotheses` planes through three
    points each, drawn from a splitmix64 stream of `seed`, every one scored against every point in float32 -- inliers within
    `threshold`, points above, points below -- and the winner refitted by least squares over its inliers in float64.
    include/pbnet_hip.h ("Floor plane and upright frame") states every operation; tests/upright_ref.py restates it in numpy.

    `up_hint` (three numbers, any length; None = unknown) is roughly where up is in the scan's frame: a hypothesis is turned
    to agree with it and dropped when it leans more than `max_tilt` degrees away.  Without a hint a plane is turned so
    that more points lie above it than below.  `below_frac` is the floor rule: a plane with more than
    int(below_frac * N) points below it is dropped -- nothing lies under a floor -- which rejects the ceiling under a hint
    and table tops always; None turns it off, which is plain segment_plane: the largest plane, whatever it is.

    Returns a dict on the device: plane f64 [4] (unit normal and offset after the refit), plane0 f32 [4] (the winning
    hypothesis), floor bool [N] and height f32 [N] (|height| <= threshold, the signed distance from the refit plane),
    moments f64 [10] (inliers, centroid, six centred second-moment sums), info int32 [8] (found, winner, its in / above /
    below, refit inliers, hypotheses alive at the end, 0), and the Python values found, hypothesis and inliers.  Without a
    live hypothesis found is False and everything else is zero.  One read-back; integer atomics only, so two runs give the
    same bytes.  A non-finite coordinate raises ValueError.  `times` (a dict) takes the stage times of the measurement
    entry, which synchronises."""
    return _upright("fit_plane", False, xyz, threshold, hypotheses, seed, up_hint, max_tilt, below_frac, times)


def upright(xyz, threshold, hypotheses=1024, seed=0, up_hint=None, max_tilt=30.0, below_frac=0.01, times=None):
    """fit_plane, and the scan turned upright by the minimal rotation that takes the plane's normal to +z: the same dict
    plus R f64 [3, 3] and xyz f32 [N, 3] = float32(R) . p, on the device.  R is a pure rotation with no shift, so camera
    poses can take it as well; the floor ends at z = -plane[3].  Without a plane (found False) R is the identity and xyz
    the input's bytes."""
    return _upright("upright", True, xyz, threshold, hypotheses, seed, up_hint, max_tilt, below_frac, times)


# ------------------------------------------------------------------------------------------------- annotated scans
def carry_labels(labels, raw_index, fill=-1):
    """The gather that goes with raw_index: out[i] = labels[raw_index[i]], `fill` where raw_index[i] is -1.  `labels` is
    any integer tensor whose first axis is the kept points; the result has raw_index's length on that axis."""
    if labels.dtype.is_floating_point or labels.dtype == torch.bool:
        raise TypeError("carry_labels: labels must be an integer tensor, got %s" % labels.dtype)
    ri = raw_index.to(device=labels.device, dtype=torch.int64)
    none = ri < 0
    out = labels.index_select(0, ri.clamp(min=0)) if labels.shape[0] else \
        labels.new_zeros((ri.shape[0],) + tuple(labels.shape[1:]))
    out[none] = fill
    return out


def vote_labels(rows, sem, ins=None, m=None, n_classes=20, compact=True, times=None):
    """An annotated raw scan's labels voted down to the kept points (csrc/vote.hip): per kept row the most frequent
    (semantic, instance) pair among the raw points routed to it.  `rows` int32 [N_raw] (decode_points' raw_index or
    thin_points' inverse: a row in [0, m) or -1 = votes nowhere), `sem` int32 [N_raw], `ins` int32 [N_raw] or None (every
    point then carries instance 0).  Any negative label is "unannotated": a label like any other, ordered LAST (the
    reference's align_superpoint_label); ties go to the lowest (sem, ins) pair.  Returns a dict on the device: sem_label
    and ins_label int64 [m] (-100 = unannotated, or a row without members), votes int32 [m] (the winner's count), members
    int32 [m] and old_id int64 [I'].  With `compact` the instance ids that won a row are renumbered 0..I'-1 in ascending
    order and old_id[new] = old; without it ins_label keeps the raw ids and old_id is empty.  One read-back (status and
    I'); `m` None takes rows.max() + 1, which costs a read-back of its own.  sem >= n_classes, ins >= 2^21 - 1 or a row
    outside [-1, m) raises ValueError.  `times` (a dict) takes the stage times of the measurement entry, which synchronises."""
    for name, t in (("rows", rows), ("sem", sem), ("ins", ins)):
        if t is not None:
            _i32(name, t, "n")
    n_raw, n_classes = int(rows.shape[0]), int(n_classes)
    if sem.shape[0] != n_raw or (ins is not None and ins.shape[0] != n_raw):
        raise ValueError("vote_labels: %d rows, %d sem, %s ins" % (n_raw, sem.shape[0], None if ins is None else ins.shape[0]))
    if not 1 <= n_classes <= VOTE_MAX_CLASSES:
        raise ValueError("vote_labels: n_classes must lie in 1..%d, got %d" % (VOTE_MAX_CLASSES, n_classes))
    if m is not None and int(m) < 0:
        raise ValueError("vote_labels: m must not be negative, got %d" % m)
    rows, sem, ins = _device(rows, sem, ins)
    m = int(m) if m is not None else (int(rows.max().item()) + 1 if n_raw else 0)
    dev = rows.device
    ws = _scan_workspace(N.lib().pbn_cloud_vote_workspace_bytes(n_raw, m), dev, "%d raw points, %d rows" % (n_raw, m))
    out_sem, out_ins = (torch.empty(m, dtype=torch.int64, device=dev) for _ in range(2))
    votes, members = (torch.empty(m, dtype=torch.int32, device=dev) for _ in range(2))
    old_id = torch.empty(max(1, min(m, VOTE_MAX_INS + 1)), dtype=torch.int64, device=dev) if compact else None
    result = torch.empty(2, dtype=torch.int32, device=dev)
    args = (N.ptr(rows), N.ptr(sem), N.ptr(ins), n_raw, m, n_classes, N.ptr(out_sem), N.ptr(out_ins), N.ptr(votes),
            N.ptr(members), N.ptr(result), N.ptr(old_id), N.ptr(ws), ws.numel(), N.current_stream())
    _staged_call("cloud_vote_labels", args, VOTE_STAGES, times)
    st, n_ins = (int(v) for v in result.tolist())            # the one read-back
    _scan_status("vote_labels", st, n_classes=n_classes, m=m)
    return {"sem_label": out_sem, "ins_label": out_ins, "votes": votes, "members": members,
            "old_id": old_id[:n_ins] if compact else torch.empty(0, dtype=torch.int64, device=dev)}
