"""Mesh decode on the MI355X: the first stage of the reference's pipeline (datasets/scannetv2/decode_scannet.py f_test,
README "Dataset Preparation" step 3) -- a scan's `_vh_clean_2.ply` mesh to the per-scene arrays xyz, rgb, nl, face, sup.

vertex_normals   decode_scannet.py:76-96 (face_normal + vertex_normal), bit for bit in float32
segment_mesh     lib/segmentator segment_mesh + main.py's torch.unique relabel (Felzenszwalb graph segmentation)
segment_point    lib/segmentator segment_point (caller-given normals and E x 2 edges)
read_ply         a minimal reader of ScanNet's binary_little_endian meshes (plyfile is not a dependency)
decode_mesh      f_test without the file writes: mean-centred xyz, rgb / 127.5 - 1, nl, face (int32), sup
save_decoded     the reference's `<scene>_{xyz,rgb,nl,face,sup}.npy` (+ labels when given) through scene_io

Scans without a mesh (csrc/cloud.hip): segment_point's normals and edges from the points alone.
knn_graph        the exact k nearest neighbours over a uniform grid, bit for bit a float32 brute force
point_normals    float64 PCA normals over each point and its neighbours, turned towards a viewpoint
knn_edges        the graph as segment_point's E x 2 edges
orient_normals   point_normals' signs made consistent over the graph (csrc/orient.hip), bit for bit tests/orient_ref.py
read_ply_points  the vertex-only counterpart of read_ply
decode_points    decode_mesh without faces: xyz, rgb, nl, sup
fit_plane        the floor plane of a scan (csrc/upright.hip): RANSAC scored on the device and a float64 refit, bit for bit
                 tests/upright_ref.py
upright          fit_plane and the scan rotated so that the plane's normal is +z

Raw sensor scans (csrc/thin.hip): to the network's pitch and back.
thin_points      one float64 centroid per occupied cell of a grid, bit for bit tests/thin_ref.py
outlier_mask     statistical outlier removal over knn_graph's d2, sums of a fixed shape
raw_index        for every raw point its row among the kept points (itself, or its first kept neighbour)
radius_count     how many other points lie within a radius of each point (csrc/cloud.hip), bit for bit tests/radius_ref.py
radius_outlier_mask, radius_raw_index   the radius filter on top of it and its raw_index: no kNN graph
carry_labels     per-point results of the kept points gathered back to the raw ones
vote_labels      the other direction (csrc/vote.hip): an annotated raw scan's (semantic, instance) pairs voted down to the
                 kept points, surviving instance ids renumbered densely; bit for bit tests/vote_ref.py

The normals, edge weights, sort and relabel run in csrc/mesh.hip; the Felzenszwalb sweep (segment_graph and the
small-segment join) is sequential by definition and runs in the library's host C++ over one read-back.  There is no CPU
path: a missing library or a CPU tensor raises.

Edge order.  The reference sorts the edges with std::sort, which is unstable: tied weights come out in an unspecified
order, which can change which segments the small-segment join merges (never the partition of the first phase) and which
vertex ends up as a segment's root.  Here the order is total: (weight, edge index), NaN weights last.

Degenerate faces (a zero cross product, e.g. a face naming one vertex twice) give the segmentator NaN face normals; every
edge of their vertices then has a NaN weight, and the reference's std::sort is undefined on such input.  The library's
defined outcome: NaN weights sort after every number, never pass the first phase's threshold test, and can still join in
the small-segment phase; ids stay finite.  Parity with the reference is not claimed there.  For the normals of
decode_scannet.py a degenerate face contributes a zero vector (its length is 0 + 1e-8), as in numpy.
"""
import ctypes

import numpy as np
import torch

from . import _native as N
from . import scene_io

MESH_NORMALS, MESH_SEGMENT, MESH_SEGMENT_POINT = 0, 1, 2
STAGES = ("incidence", "normals", "weights", "sort", "read-back", "host sweep", "relabel")
# The status bits that every stage of the scan chain shares (csrc/scan_dev.h: SCAN_NONFINITE, SCAN_EXTENT, SCAN_SORT_SPIN):
# a coordinate is NaN or infinite; an axis spans 2^21 cells or more of thin_points' pitch; the device sort gave up.
CLOUD_NONFINITE, CLOUD_EXTENT, CLOUD_SORT_SPIN = 1, 2, 8


def _check_xyz(name, t):
    N.require_cuda(t)
    if t.dtype != torch.float32 or t.dim() != 2 or t.shape[1] != 3:
        raise TypeError("%s must be a float32 [n, 3] tensor, got %s %s" % (name, t.dtype, tuple(t.shape)))
    return t.contiguous()


def _check_index(name, t, width):
    N.require_cuda(t)
    if t.dtype not in (torch.int32, torch.int64) or t.dim() != 2 or t.shape[1] != width:
        raise TypeError("%s must be an int32 or int64 [n, %d] tensor, got %s %s" % (name, width, t.dtype, tuple(t.shape)))
    return t.contiguous(), int(t.dtype == torch.int64)


def _workspace(mode, n_vertices, n_elems, dev):
    nbytes = N.lib().pbn_mesh_workspace_bytes(mode, n_vertices, n_elems)
    if nbytes == 0:
        raise ValueError("mesh too large for the library: %d vertices, %d elements" % (n_vertices, n_elems))
    return torch.empty(nbytes, dtype=torch.uint8, device=dev)


def _scan_workspace(nbytes, dev, what):
    """The workspace of a stage of the scan chain; 0 bytes is the library's refusal of the size."""
    if nbytes == 0:
        raise ValueError("point cloud too large for the library: %s" % what)
    return torch.empty(nbytes, dtype=torch.uint8, device=dev)


def _staged_call(entry, args, stages, times):
    """pbn_<entry>, or with `times` (a dict) pbn_<entry>_timed, which synchronises and adds its time per stage in ms."""
    if times is None:
        N.check(getattr(N.lib(), "pbn_" + entry)(*args), "pbn_" + entry)
        return
    t = (ctypes.c_float * len(stages))()
    N.check(getattr(N.lib(), "pbn_%s_timed" % entry)(*args, t), "pbn_%s_timed" % entry)
    times.update({name: float(t[i]) for i, name in enumerate(stages)})


def _raise(rc, what):
    if rc == N.PBN_ERR_RANGE:
        raise ValueError("%s: an index lies outside [0, number of vertices)" % what)
    N.check(rc, what)


def vertex_normals(xyz, faces):
    """decode_scannet.py vertex_normal(xyz, faces): float32 [V, 3] on the device, bit for bit."""
    xyz = _check_xyz("xyz", xyz)
    faces, i64 = _check_index("faces", faces, 3)
    v, f = int(xyz.shape[0]), int(faces.shape[0])
    nl = torch.empty(v, 3, dtype=torch.float32, device=xyz.device)
    status = torch.zeros(1, dtype=torch.int32, device=xyz.device)
    ws = _workspace(MESH_NORMALS, v, f, xyz.device)
    lib = N.lib()
    N.check(lib.pbn_mesh_vertex_normals(N.ptr(xyz), v, N.ptr(faces), i64, f, N.ptr(nl), N.ptr(status), N.ptr(ws),
                                        ws.numel(), N.current_stream()), "pbn_mesh_vertex_normals")
    if int(status.item()) != 0:
        raise ValueError("vertex_normals: a face index lies outside [0, %d)" % v)
    return nl


def _segment_mesh(vertices, faces, kThresh, segMinVerts, nl=None, times=None):
    vertices = _check_xyz("vertices", vertices)
    faces, i64 = _check_index("faces", faces, 3)
    v, f = int(vertices.shape[0]), int(faces.shape[0])
    sup = torch.empty(v, dtype=torch.int64, device=vertices.device)
    ws = _workspace(MESH_SEGMENT, v, f, vertices.device)
    t = (ctypes.c_float * len(STAGES))() if times is not None else None
    rc = N.lib().pbn_mesh_segment(N.ptr(vertices), v, N.ptr(faces), i64, f, float(kThresh), int(segMinVerts), N.ptr(sup),
                                  N.ptr(nl), N.ptr(ws), ws.numel(), t, N.current_stream())
    _raise(rc, "segment_mesh")
    if times is not None:
        times.update({name: float(t[i]) for i, name in enumerate(STAGES)})
    return sup


def segment_mesh(vertices, faces, kThresh=0.01, segMinVerts=20):
    """lib/segmentator segment_mesh: superpoint id per vertex, int64 [V] on the device, ids 0..S-1 in ascending order of
    the segments' root vertices (the reference wrapper's torch.unique(..., return_inverse=True)[1]).  Synchronises."""
    return _segment_mesh(vertices, faces, kThresh, segMinVerts)


def segment_point(vertices, normals, edges, kThresh=0.01, segMinVerts=20):
    """lib/segmentator segment_point: the same segmentation over caller-given normals and edges [E, 2]."""
    vertices = _check_xyz("vertices", vertices)
    normals = _check_xyz("normals", normals)
    edges, i64 = _check_index("edges", edges, 2)
    v, e = int(vertices.shape[0]), int(edges.shape[0])
    if normals.shape[0] != v:
        raise ValueError("segment_point: %d normals for %d vertices" % (normals.shape[0], v))
    sup = torch.empty(v, dtype=torch.int64, device=vertices.device)
    ws = _workspace(MESH_SEGMENT_POINT, v, e, vertices.device)
    rc = N.lib().pbn_mesh_segment_point(N.ptr(vertices), N.ptr(normals), v, N.ptr(edges), i64, e, float(kThresh),
                                        int(segMinVerts), N.ptr(sup), N.ptr(ws), ws.numel(), N.current_stream())
    _raise(rc, "segment_point")
    return sup


# ---------------------------------------------------------------------------------------------------- point clouds
CLOUD_STAGES = ("box", "keys + sort", "cell table", "search")


def knn_graph(xyz, k=16, cell=None, times=None):
    """The exact k nearest neighbours of every point (csrc/cloud.hip): idx int32 [N, k] and d2 float32 [N, k] on the
    device, in the caller's point order.  d2 = ((dx*dx + dy*dy) + dz*dz) in float32; a row holds the k points j != i with
    the smallest (bits of d2, j), ascending; when N - 1 < k it ends in idx = -1, d2 = +inf.  `cell` (the grid's cell size;
    None lets the library choose) changes the speed, never the result.  A non-finite coordinate raises ValueError."""
    xyz = _check_xyz("xyz", xyz)
    n, k = int(xyz.shape[0]), int(k)
    lib = N.lib()
    if not 1 <= k <= lib.pbn_cloud_max_k():
        raise ValueError("knn_graph: k must lie in 1..%d, got %d" % (lib.pbn_cloud_max_k(), k))
    dev = xyz.device
    ws = _scan_workspace(lib.pbn_cloud_workspace_bytes(n, k), dev, "%d points" % n)
    idx = torch.empty(n, k, dtype=torch.int32, device=dev)
    d2 = torch.empty(n, k, dtype=torch.float32, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    h = 0.0 if cell is None else float(cell)
    if cell is not None and not h > 0.0:
        raise ValueError("knn_graph: cell must be positive, got %r" % (cell,))
    args = (N.ptr(xyz), n, k, h, N.ptr(idx), N.ptr(d2), N.ptr(status), N.ptr(ws), ws.numel(), N.current_stream())
    _staged_call("cloud_knn", args, CLOUD_STAGES, times)
    st = int(status.item())
    if st & CLOUD_NONFINITE:
        raise ValueError("knn_graph: a coordinate is NaN or infinite")
    if st:                                                   # CLOUD_SORT_SPIN
        raise RuntimeError("knn_graph: the device sort gave up (status %d)" % st)
    return idx, d2


def point_normals(xyz, idx, viewpoint=None):
    """PCA normals over each point and its neighbours `idx` (int32 [N, k], -1 = none): float32 [N, 3] on the device, the
    float64 eigenvector of the smallest covariance eigenvalue, turned towards `viewpoint` (three numbers or a tensor; None
    = the float64 mean of xyz).  Fewer than three points in a neighbourhood give the zero vector."""
    xyz = _check_xyz("xyz", xyz)
    N.require_cuda(idx)
    n = int(xyz.shape[0])
    if idx.dtype != torch.int32 or idx.dim() != 2 or idx.shape[0] != n:
        raise TypeError("idx must be an int32 [%d, k] tensor, got %s %s" % (n, idx.dtype, tuple(idx.shape)))
    idx = idx.contiguous()
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


ORIENT_STAGES = ("edge codes", "rounds", "tail")
CLOUD_WALK_CAP = 16                                          # csrc/scan_dev.h: SCAN_WALK_CAP
CLOUD_MAX_K = 32                                             # csrc/scan_dev.h: SCAN_MAX_K = pbn_cloud_max_k(), known without the library


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
    if not torch.is_tensor(nl) or nl.dtype != torch.float32 or nl.dim() != 2 or nl.shape[1] != 3:
        raise TypeError("nl must be a float32 [n, 3] tensor, got %s" % (
            "%s %s" % (nl.dtype, tuple(nl.shape)) if torch.is_tensor(nl) else type(nl).__name__))
    n = int(nl.shape[0])
    if not torch.is_tensor(idx) or idx.dtype != torch.int32 or idx.dim() != 2 or idx.shape[0] != n:
        raise TypeError("idx must be an int32 [%d, k] tensor, got %s" % (
            n, "%s %s" % (idx.dtype, tuple(idx.shape)) if torch.is_tensor(idx) else type(idx).__name__))
    k = int(idx.shape[1])
    if not 1 <= k <= CLOUD_MAX_K:
        raise ValueError("orient_normals: k must lie in 1..%d, got %d" % (CLOUD_MAX_K, k))
    if n * k > (1 << 31) - 1:
        raise ValueError("orient_normals: %d points x %d neighbours exceed 2^31 - 1 edge slots" % (n, k))
    N.require_cuda(nl, idx)
    nl, idx = nl.contiguous(), idx.contiguous()
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
    if st:                                                   # CLOUD_WALK_CAP
        raise RuntimeError("orient_normals: a link chain did not end (status %d)" % st)
    return {"nl": out, "flipped": flipped, "tree": tree, "stats": stats, "rounds": rounds}


# ------------------------------------------------------------------------------------------------------- raw scans
THIN_STAGES = ("box + keys", "low-word sort", "high-word keys + sort", "run heads + scan", "cells")


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
    xyz = _check_xyz("xyz", xyz)
    rgb = None if colours is None else _check_xyz("colours", colours)
    n = int(xyz.shape[0])
    if rgb is not None and rgb.shape[0] != n:
        raise ValueError("thin_points: %d colours for %d points" % (rgb.shape[0], n))
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
    if st & CLOUD_NONFINITE:
        raise ValueError("thin_points: a coordinate is NaN or infinite")
    if st & CLOUD_EXTENT:
        raise ValueError("thin_points: the cloud spans 2^21 cells or more of pitch %r on an axis" % (pitch,))
    if st:                                                   # CLOUD_SORT_SPIN
        raise RuntimeError("thin_points: the device sort gave up (status %d)" % st)
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
    N.require_cuda(d2)
    if d2.dtype != torch.float32 or d2.dim() != 2:
        raise TypeError("d2 must be a float32 [n, k] tensor, got %s %s" % (d2.dtype, tuple(d2.shape)))
    d2 = d2.contiguous()
    n, k = int(d2.shape[0]), int(d2.shape[1])
    lib = N.lib()
    if not 1 <= k <= lib.pbn_cloud_max_k():
        raise ValueError("outlier_mask: k must lie in 1..%d, got %d" % (lib.pbn_cloud_max_k(), k))
    dev = d2.device
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
    N.require_cuda(inverse, keep, idx)
    if inverse.dtype != torch.int32 or inverse.dim() != 1:
        raise TypeError("inverse must be an int32 [n] tensor, got %s %s" % (inverse.dtype, tuple(inverse.shape)))
    m = int(keep.shape[0])
    if keep.dtype != torch.bool or keep.dim() != 1:
        raise TypeError("keep must be a bool [m] tensor, got %s %s" % (keep.dtype, tuple(keep.shape)))
    if idx.dtype != torch.int32 or idx.dim() != 2 or idx.shape[0] != m:
        raise TypeError("idx must be an int32 [%d, k] tensor, got %s %s" % (m, idx.dtype, tuple(idx.shape)))
    inverse, keep, idx = inverse.contiguous(), keep.contiguous(), idx.contiguous()
    n_raw, k = int(inverse.shape[0]), int(idx.shape[1])
    lib = N.lib()
    if not 1 <= k <= lib.pbn_cloud_max_k():
        raise ValueError("raw_index: k must lie in 1..%d, got %d" % (lib.pbn_cloud_max_k(), k))
    ws = _scan_workspace(lib.pbn_cloud_raw_index_workspace_bytes(m), inverse.device, "%d points" % m)
    out = torch.empty(n_raw, dtype=torch.int32, device=inverse.device)
    N.check(lib.pbn_cloud_raw_index(N.ptr(inverse), n_raw, N.ptr(keep), N.ptr(idx), m, k, N.ptr(out), N.ptr(ws), ws.numel(),
                                    N.current_stream()), "pbn_cloud_raw_index")
    return out


RADIUS_STAGES = ("box", "keys + sort", "cell table", "count")
RADIUS_MAX_CAP = (1 << 31) - 1


def _radius_args(what, xyz, radius, cell):
    """The checks the fixed-radius functions share, values and dtypes before the device: (xyz, float32 radius, cell)."""
    with np.errstate(over="ignore"):
        rf = np.float32(radius)
    if not (np.isfinite(rf) and rf > 0):
        raise ValueError("%s: radius must be positive and finite as a float32, got %r" % (what, radius))
    h = 0.0 if cell is None else float(cell)
    if cell is not None and not h > 0.0:
        raise ValueError("%s: cell must be positive, got %r" % (what, cell))
    if not torch.is_tensor(xyz) or xyz.dtype != torch.float32 or xyz.dim() != 2 or xyz.shape[1] != 3:
        raise TypeError("xyz must be a float32 [n, 3] tensor, got %s" % (
            "%s %s" % (xyz.dtype, tuple(xyz.shape)) if torch.is_tensor(xyz) else type(xyz).__name__))
    return float(rf), h


def _scan_status(what, status):
    st = int(status.item())                                  # the one read-back
    if st & CLOUD_NONFINITE:
        raise ValueError("%s: a coordinate is NaN or infinite" % what)
    if st:                                                   # CLOUD_SORT_SPIN
        raise RuntimeError("%s: the device sort gave up (status %d)" % (what, st))


def radius_count(xyz, radius, cap=None, cell=None, times=None):
    """The number of other points within `radius` of every point (csrc/cloud.hip): count int32 [N] on the device, in the
    caller's point order.  rf = float32(radius), r2 = rf * rf in float32; j counts for i when j != i and knn_graph's
    d2(i, j) <= r2, so coincident points count at 0.  count = min(neighbours, cap): `cap` is an int in 1..2^31 - 1 (None =
    2^31 - 1) at which a query stops looking.  `cell` (the grid's cell size; None = a hair above the radius) changes the
    speed, never the result.  One read-back (the status); a non-finite coordinate raises ValueError.  `times` (a dict)
    takes the stage times of the measurement entry, which synchronises."""
    rf, h = _radius_args("radius_count", xyz, radius, cell)
    cap = RADIUS_MAX_CAP if cap is None else cap
    if isinstance(cap, bool) or not isinstance(cap, (int, np.integer)) or not 1 <= int(cap) <= RADIUS_MAX_CAP:
        raise ValueError("radius_count: cap must be an int in 1..2^31 - 1, got %r" % (cap,))
    xyz = _check_xyz("xyz", xyz)
    n, dev = int(xyz.shape[0]), xyz.device
    ws = _scan_workspace(N.lib().pbn_cloud_radius_workspace_bytes(n), dev, "%d points" % n)
    count = torch.empty(n, dtype=torch.int32, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    args = (N.ptr(xyz), n, rf, int(cap), h, N.ptr(count), N.ptr(status), N.ptr(ws), ws.numel(), N.current_stream())
    _staged_call("cloud_radius_count", args, RADIUS_STAGES, times)
    _scan_status("radius_count", status)
    return count


def radius_outlier_mask(xyz, radius, min_pts, cell=None):
    """Radius outlier removal (PCL's RadiusOutlierRemoval, Open3D's remove_radius_outlier): keep bool [N] on the device,
    keep[i] = at least `min_pts` (>= 1) other points lie within `radius` of point i.  It is
    radius_count(xyz, radius, cap=min_pts) >= min_pts: the count stops at min_pts, and the comparison is a torch
    expression on the device."""
    if isinstance(min_pts, bool) or not isinstance(min_pts, (int, np.integer)) or not 1 <= int(min_pts) <= RADIUS_MAX_CAP:
        raise ValueError("radius_outlier_mask: min_pts must be an int in 1..2^31 - 1, got %r" % (min_pts,))
    return radius_count(xyz, radius, cap=int(min_pts), cell=cell) >= int(min_pts)


def radius_raw_index(inverse, keep, xyz, radius, cell=None):
    """raw_index without a kNN graph: int32 [N_raw] on the device.  With t = inverse[i]: t's row among the kept points (the
    exclusive scan of keep) when keep[t]; else the row of the KEPT point j with the smallest (bits of d2(t, j), j) among
    those with d2(t, j) <= r2 (radius_count's d2 and r2) -- a dropped point is never an answer, however near; else -1.
    `inverse` int32 [N_raw] (thin_points), `keep` bool [M] (radius_outlier_mask), `xyz` f32 [M, 3] (the same M points).
    One read-back (the status)."""
    rf, h = _radius_args("radius_raw_index", xyz, radius, cell)
    if not torch.is_tensor(inverse) or inverse.dtype != torch.int32 or inverse.dim() != 1:
        raise TypeError("inverse must be an int32 [n] tensor, got %s %s" % (inverse.dtype, tuple(inverse.shape)))
    m = int(xyz.shape[0])
    if not torch.is_tensor(keep) or keep.dtype != torch.bool or keep.dim() != 1 or keep.shape[0] != m:
        raise TypeError("keep must be a bool [%d] tensor, got %s %s" % (m, keep.dtype, tuple(keep.shape)))
    N.require_cuda(inverse, keep, xyz)
    inverse, keep, xyz = inverse.contiguous(), keep.contiguous(), xyz.contiguous()
    n_raw, dev = int(inverse.shape[0]), inverse.device
    ws = _scan_workspace(N.lib().pbn_cloud_radius_raw_index_workspace_bytes(m, n_raw), dev,
                         "%d points, %d raw points" % (m, n_raw))
    out = torch.empty(n_raw, dtype=torch.int32, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    N.check(N.lib().pbn_cloud_radius_raw_index(N.ptr(xyz), m, N.ptr(keep), rf, h, N.ptr(inverse), n_raw, N.ptr(out),
                                               N.ptr(status), N.ptr(ws), ws.numel(), N.current_stream()),
            "pbn_cloud_radius_raw_index")
    _scan_status("radius_raw_index", status)
    return out


# ------------------------------------------------------------------------------------------ floor plane, upright frame
UPRIGHT_STAGES = ("hypotheses", "score", "select + refit", "apply")
UPRIGHT_MAX_HYP = 4096                                       # csrc/upright.hip: UPR_MAX_HYP = pbn_cloud_upright_max_hyp()
UPRIGHT_KEYS = ("threshold", "hypotheses", "seed", "up_hint", "max_tilt", "below_frac")


def _upright_args(what, xyz, threshold, hypotheses, seed, up_hint, max_tilt, below_frac):
    """fit_plane's checks, values and dtypes before the device or the library: (float32 threshold, H, seed, the float64
    unit hint as a ctypes double[3] or None, cos(max_tilt), max_below)."""
    if isinstance(threshold, bool) or not isinstance(threshold, (int, float, np.integer, np.floating)):
        raise TypeError("%s: threshold must be a number, got %r" % (what, threshold))
    with np.errstate(over="ignore"):
        tf = np.float32(threshold)
    if not (np.isfinite(tf) and tf > 0):
        raise ValueError("%s: threshold must be positive and finite as a float32, got %r" % (what, threshold))
    if isinstance(hypotheses, bool) or not isinstance(hypotheses, (int, np.integer)) or not 1 <= int(hypotheses) <= UPRIGHT_MAX_HYP:
        raise ValueError("%s: hypotheses must be an int in 1..%d, got %r" % (what, UPRIGHT_MAX_HYP, hypotheses))
    if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)) or not 0 <= int(seed) < (1 << 64):
        raise ValueError("%s: seed must be an int in 0..2^64 - 1, got %r" % (what, seed))
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
    if isinstance(max_tilt, bool) or not isinstance(max_tilt, (int, float, np.integer, np.floating)):
        raise TypeError("%s: max_tilt must be a number of degrees, got %r" % (what, max_tilt))
    if not 0.0 < float(max_tilt) <= 90.0:
        raise ValueError("%s: max_tilt must lie in (0, 90] degrees, got %r" % (what, max_tilt))
    if below_frac is not None:
        if isinstance(below_frac, bool) or not isinstance(below_frac, (int, float, np.integer, np.floating)):
            raise TypeError("%s: below_frac must be a number or None, got %r" % (what, below_frac))
        if not 0.0 <= float(below_frac) <= 1.0:
            raise ValueError("%s: below_frac must lie in [0, 1] or be None, got %r" % (what, below_frac))
    if not torch.is_tensor(xyz) or xyz.dtype != torch.float32 or xyz.dim() != 2 or xyz.shape[1] != 3:
        raise TypeError("xyz must be a float32 [n, 3] tensor, got %s" % (
            "%s %s" % (xyz.dtype, tuple(xyz.shape)) if torch.is_tensor(xyz) else type(xyz).__name__))
    max_below = -1 if below_frac is None else int(float(below_frac) * int(xyz.shape[0]))
    return float(tf), int(hypotheses), int(seed), hint, float(np.cos(np.deg2rad(np.float64(max_tilt)))), max_below


def _upright(what, rotate, xyz, threshold, hypotheses, seed, up_hint, max_tilt, below_frac, times, chunk=None):
    tf, n_hyp, seed, hint, cos_tilt, max_below = _upright_args(what, xyz, threshold, hypotheses, seed, up_hint, max_tilt,
                                                               below_frac)
    xyz = _check_xyz("xyz", xyz)
    n, dev = int(xyz.shape[0]), xyz.device
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
    if host[8] & CLOUD_NONFINITE:
        raise ValueError("%s: a coordinate is NaN or infinite" % what)
    if host[8]:
        raise RuntimeError("%s: status %d" % (what, host[8]))
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


def _upright_option(upright, pitch):
    """decode_points' `upright` as fit_plane's keyword arguments, or None; checked before anything is uploaded."""
    if upright is None or upright is False:
        return None
    if upright is True:
        upright = {}
    if not isinstance(upright, dict):
        raise TypeError("decode_points: upright must be None, True or a dict of fit_plane's arguments, got %r" % (upright,))
    unknown = sorted(set(upright) - set(UPRIGHT_KEYS))
    if unknown:
        raise TypeError("decode_points: upright has no argument %s (it takes %s)" % (", ".join(map(repr, unknown)),
                                                                                    ", ".join(UPRIGHT_KEYS)))
    kw = dict(threshold=pitch if pitch is not None else 0.02, hypotheses=1024, seed=0, up_hint=None, max_tilt=30.0,
              below_frac=0.01)
    kw.update(upright)
    _upright_args("decode_points: upright", torch.empty(0, 3), **kw)
    return kw


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


# ------------------------------------------------------------------------------------------------- annotated scans
VOTE_SEM_RANGE, VOTE_INS_RANGE, VOTE_ROW_RANGE = 1, 2, 4     # pbn_cloud_vote_labels' own status bits, next to CLOUD_SORT_SPIN
VOTE_MAX_CLASSES, VOTE_MAX_INS = 1023, (1 << 21) - 1         # n_classes in 1..1023; instance ids in 0..2^21 - 2
VOTE_STAGES = ("fill + keys", "key sort", "row pairs + row sort", "run heads + scan + starts", "pick", "compaction")


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
        if t is not None and (t.dtype != torch.int32 or t.dim() != 1):
            raise TypeError("%s must be an int32 [n] tensor, got %s %s" % (name, t.dtype, tuple(t.shape)))
    n_raw, n_classes = int(rows.shape[0]), int(n_classes)
    if sem.shape[0] != n_raw or (ins is not None and ins.shape[0] != n_raw):
        raise ValueError("vote_labels: %d rows, %d sem, %s ins" % (n_raw, sem.shape[0], None if ins is None else ins.shape[0]))
    if not 1 <= n_classes <= VOTE_MAX_CLASSES:
        raise ValueError("vote_labels: n_classes must lie in 1..%d, got %d" % (VOTE_MAX_CLASSES, n_classes))
    if m is not None and int(m) < 0:
        raise ValueError("vote_labels: m must not be negative, got %d" % m)
    N.require_cuda(rows, sem, ins)
    m = int(m) if m is not None else (int(rows.max().item()) + 1 if n_raw else 0)
    rows, sem, ins = rows.contiguous(), sem.contiguous(), None if ins is None else ins.contiguous()
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
    if st & VOTE_SEM_RANGE:
        raise ValueError("vote_labels: a semantic label is %d or more" % n_classes)
    if st & VOTE_INS_RANGE:
        raise ValueError("vote_labels: an instance label is %d or more" % VOTE_MAX_INS)
    if st & VOTE_ROW_RANGE:
        raise ValueError("vote_labels: a row lies outside [-1, %d)" % m)
    if st:                                                   # CLOUD_SORT_SPIN
        raise RuntimeError("vote_labels: the device sort gave up (status %d)" % st)
    return {"sem_label": out_sem, "ins_label": out_ins, "votes": votes, "members": members,
            "old_id": old_id[:n_ins] if compact else torch.empty(0, dtype=torch.int64, device=dev)}


def _raw_labels(name, labels, n):
    """decode_points' label argument as a host int32 [n] array: integer arrays or tensors, or the float64 arrays the
    reference's `.npy` files hold (integral values only)."""
    a = labels.detach().cpu().numpy() if torch.is_tensor(labels) else np.asarray(labels)
    if a.ndim != 1 or a.shape[0] != n:
        raise ValueError("decode_points: %s must have shape [%d], got %s" % (name, n, tuple(a.shape)))
    if a.dtype.kind == "f":
        if not np.all(np.isfinite(a)) or not np.array_equal(a, np.rint(a)):
            raise ValueError("decode_points: %s holds a value that is not an integer" % name)
    elif a.dtype.kind not in "iu":
        raise TypeError("decode_points: %s must be an integer or float array, got %s" % (name, a.dtype))
    if a.size and (a.min() < -(2 ** 31) or a.max() > 2 ** 31 - 1):
        raise ValueError("decode_points: %s holds a value outside int32" % name)
    return np.ascontiguousarray(a.astype(np.int32))


# ------------------------------------------------------------------------------------------------------------ PLY
_PLY_SCALARS = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "i2", "int16": "i2", "ushort": "u2",
                "uint16": "u2", "int": "i4", "int32": "i4", "uint": "u4", "uint32": "u4", "float": "f4", "float32": "f4",
                "double": "f8", "float64": "f8"}


def _read_ply_header(fh, path):
    """The header of an open PLY file: (fmt, elements, body) -- the words after `format`, a list of (name, count,
    properties) with every property as the tuple of its words, and the bytes after end_header."""
    if fh.readline().strip() != b"ply":
        raise ValueError("%s: not a PLY file" % path)
    elements, fmt = [], None
    while True:
        line = fh.readline()
        if not line:
            raise ValueError("%s: no end_header" % path)
        words = line.decode("ascii", "replace").split()
        if not words or words[0] in ("comment", "obj_info"):
            continue
        if words[0] == "end_header":
            break
        if words[0] == "format":
            fmt = words[1:]
        elif words[0] == "element" and len(words) == 3:
            elements.append((words[1], int(words[2]), []))
        elif words[0] == "property":
            if not elements:
                raise ValueError("%s: property before any element" % path)
            elements[-1][2].append(tuple(words[1:]))
        else:
            raise ValueError("%s: unsupported header line %r" % (path, line))
    if fmt != ["binary_little_endian", "1.0"]:
        raise ValueError("%s: only binary_little_endian 1.0 is supported, got %s" % (path, fmt))
    return fmt, elements, fh.read()


def _vertex_dtype(path, vprops):
    """The record of a vertex under the accepted property rules."""
    names = [p[-1] for p in vprops]
    types = [p[0] for p in vprops]
    if names not in (["x", "y", "z", "red", "green", "blue"], ["x", "y", "z", "red", "green", "blue", "alpha"]) or \
            any(_PLY_SCALARS.get(t) != "f4" for t in types[:3]) or any(_PLY_SCALARS.get(t) != "u1" for t in types[3:]):
        raise ValueError("%s: vertex properties must be float x y z + uchar red green blue [alpha], got %s" % (path, vprops))
    return np.dtype([(n, "<f4" if i < 3 else "u1") for i, n in enumerate(names)])


def _vertex_arrays(body, vdt, nv):
    """xyz float32 [V, 3] and colours uint8 [V, 3] of the nv vertex records at the start of `body`."""
    vert = np.frombuffer(body, vdt, nv, 0)
    xyz = np.stack([vert["x"], vert["y"], vert["z"]], axis=1).astype(np.float32)
    rgb = np.stack([vert["red"], vert["green"], vert["blue"]], axis=1).astype(np.uint8)
    return xyz, rgb


def read_ply(path):
    """ScanNet's `_vh_clean_2.ply`: returns (xyz float32 [V, 3], colours uint8 [V, 3], faces int64 [F, 3]).

    Accepted: format binary_little_endian 1.0; element vertex with exactly `float x, y, z` then `uchar red, green, blue`
    and an optional `uchar alpha`; element face with exactly `list uchar int vertex_indices` (or `uint`), triangles only.
    Anything else raises ValueError."""
    with open(path, "rb") as fh:
        _, elements, body = _read_ply_header(fh, path)
    if [e[0] for e in elements] != ["vertex", "face"]:
        raise ValueError("%s: expected elements [vertex, face], got %s" % (path, [e[0] for e in elements]))
    (_, nv, vprops), (_, nf, fprops) = elements
    vdt = _vertex_dtype(path, vprops)
    if len(fprops) != 1 or fprops[0][0] != "list" or fprops[0][-1] != "vertex_indices" or \
            _PLY_SCALARS.get(fprops[0][1]) != "u1" or _PLY_SCALARS.get(fprops[0][2]) not in ("i4", "u4"):
        raise ValueError("%s: face must be `list uchar int|uint vertex_indices`, got %s" % (path, fprops))
    fdt = np.dtype([("n", "u1"), ("i", "<" + _PLY_SCALARS[fprops[0][2]], (3,))])
    need = nv * vdt.itemsize + nf * fdt.itemsize
    if len(body) < need:
        raise ValueError("%s: truncated body (%d bytes, need %d for triangles)" % (path, len(body), need))
    face = np.frombuffer(body, fdt, nf, nv * vdt.itemsize)
    if nf and not np.all(face["n"] == 3):
        raise ValueError("%s: only triangle faces are supported" % path)
    return _vertex_arrays(body, vdt, nv) + (face["i"].astype(np.int64).reshape(-1, 3),)


def read_ply_points(path):
    """A point cloud's PLY: returns (xyz float32 [V, 3], colours uint8 [V, 3]).

    Accepted: format binary_little_endian 1.0 with the vertex element ONLY, under read_ply's property rules (`float x, y,
    z`, `uchar red, green, blue`, an optional `uchar alpha`).  Anything else raises ValueError; a file with faces is a mesh
    and belongs to read_ply."""
    with open(path, "rb") as fh:
        _, elements, body = _read_ply_header(fh, path)
    if [e[0] for e in elements] != ["vertex"]:
        raise ValueError("%s: expected the vertex element only, got %s" % (path, [e[0] for e in elements]))
    _, nv, vprops = elements[0]
    vdt = _vertex_dtype(path, vprops)
    if nv < 0 or len(body) < nv * vdt.itemsize:
        raise ValueError("%s: truncated body (%d bytes, need %d)" % (path, len(body), nv * vdt.itemsize))
    return _vertex_arrays(body, vdt, nv)


def write_ply(path, xyz, colours, faces, index_type="int", alpha=True):
    """The counterpart of read_ply (binary_little_endian, the layout ScanNet ships)."""
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    colours = np.asarray(colours, np.uint8).reshape(-1, 3)
    faces = np.asarray(faces).reshape(-1, 3)
    it = {"int": "<i4", "uint": "<u4"}[index_type]
    names = ["x", "y", "z", "red", "green", "blue"] + (["alpha"] if alpha else [])
    vdt = np.dtype([(n, "<f4" if i < 3 else "u1") for i, n in enumerate(names)])
    v = np.zeros(xyz.shape[0], vdt)
    for i, n in enumerate("xyz"):
        v[n] = xyz[:, i]
    for i, n in enumerate(["red", "green", "blue"]):
        v[n] = colours[:, i]
    if alpha:
        v["alpha"] = 255
    f = np.zeros(faces.shape[0], np.dtype([("n", "u1"), ("i", it, (3,))]))
    f["n"] = 3
    f["i"] = faces
    head = ["ply", "format binary_little_endian 1.0", "element vertex %d" % xyz.shape[0]]
    head += ["property float %s" % n for n in "xyz"] + ["property uchar %s" % n for n in names[3:]]
    head += ["element face %d" % faces.shape[0], "property list uchar %s vertex_indices" % index_type, "end_header"]
    with open(path, "wb") as fh:
        fh.write(("\n".join(head) + "\n").encode("ascii"))
        fh.write(v.tobytes())
        fh.write(f.tobytes())


# --------------------------------------------------------------------------------------------------------- decode
def centre_and_scale(xyz, colours):
    """decode_scannet.py:62-70 on host arrays, in its own layout and expressions: (xyz - mean, rgb / 127.5 - 1)."""
    xyz = np.asarray(xyz)
    vertices = np.zeros(shape=[xyz.shape[0], 6], dtype=np.float32)
    vertices[:, 0:3] = xyz
    vertices[:, 3:6] = np.asarray(colours)
    return vertices[:, :3] - vertices[:, :3].mean(0), vertices[:, 3:] / 127.5 - 1


def decode_mesh(src, device="cuda", kThresh=0.01, segMinVerts=20):
    """decode_scannet.py f_test for one mesh: `src` is a `.ply` path or (xyz [V,3], colours [V,3] 0..255, faces [F,3]).
    Returns xyz (mean-centred), rgb, nl (f32 [V,3]), face (int32 [F,3]) and sup (int64 [V]), all on `device`."""
    if isinstance(src, (str, bytes)) or hasattr(src, "__fspath__"):
        xyz, colours, faces = read_ply(src)
    else:
        xyz, colours, faces = (t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t) for t in src)
    faces = np.asarray(faces).reshape(-1, 3)
    xyz_c, rgb = centre_and_scale(xyz, colours)
    n = xyz_c.shape[0]
    if faces.size and (faces.min() < 0 or faces.max() >= n):
        raise ValueError("decode_mesh: a face index lies outside [0, %d)" % n)
    dev = torch.device(device)
    xyz_d = torch.from_numpy(np.ascontiguousarray(xyz_c, np.float32)).to(dev)
    face_d = torch.from_numpy(np.ascontiguousarray(faces.astype(np.int32))).to(dev)
    nl = torch.empty(n, 3, dtype=torch.float32, device=dev)
    sup = _segment_mesh(xyz_d, face_d, kThresh, segMinVerts, nl=nl)
    return {"xyz": xyz_d, "rgb": torch.from_numpy(np.ascontiguousarray(rgb, np.float32)).to(dev), "nl": nl,
            "face": face_d, "sup": sup}


def _kept_points(xyz, colours, dev, k, pitch, outlier_ratio, outlier_radius=None, outlier_min_pts=None, upright_kw=None):
    """decode_points' front for a raw scan: upload, thin_points (pitch), then knn_graph -> outlier_mask -> raw_index
    (outlier_ratio) or radius_outlier_mask -> radius_raw_index (outlier_radius, outlier_min_pts: no graph over the
    unfiltered points), and the compaction.  Returns the kept points' (xyz, colours) as host float32 arrays --
    centre_and_scale is a host numpy expression, so the kept M x 6 floats make one extra round trip -- and raw_index /
    count on the device, then upright's result or None.  With `upright_kw` (fit_plane's keyword arguments) the kept points
    are turned upright while they are still on the device: the returned xyz is in the upright frame, and the result's
    "kept_xyz" holds the kept points in the sensor's frame."""
    xyz_d = torch.from_numpy(np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)).to(dev)
    col_d = torch.from_numpy(np.ascontiguousarray(colours, np.float32).reshape(-1, 3)).to(dev)
    n_raw = int(xyz_d.shape[0])
    if pitch is not None:
        th = thin_points(xyz_d, col_d, pitch)
        xyz_d, col_d, count, inverse = th["xyz"], th["rgb"], th["count"], th["inverse"]
    else:
        count = torch.ones(n_raw, dtype=torch.int32, device=dev)
        inverse = torch.arange(n_raw, dtype=torch.int32, device=dev)
    if outlier_ratio is not None:
        idx, d2 = knn_graph(xyz_d, k=k)
        keep, _ = outlier_mask(d2, outlier_ratio)
        inverse = raw_index(inverse, keep, idx)
        xyz_d, col_d, count = xyz_d[keep], col_d[keep], count[keep]
    elif outlier_radius is not None:
        keep = radius_outlier_mask(xyz_d, outlier_radius, outlier_min_pts)
        inverse = radius_raw_index(inverse, keep, xyz_d, outlier_radius)
        xyz_d, col_d, count = xyz_d[keep], col_d[keep], count[keep]
    up = None
    if upright_kw is not None:
        up = upright(xyz_d, **upright_kw)
        if not up["found"]:
            raise ValueError("decode_points: no floor plane found among %d points (%d hypotheses, %d alive at the end); "
                             "check threshold, up_hint and below_frac" % (int(xyz_d.shape[0]), upright_kw["hypotheses"],
                                                                          int(up["info"][6])))
        up["kept_xyz"], xyz_d = xyz_d, up["xyz"]
    return xyz_d.cpu().numpy(), col_d.cpu().numpy(), inverse, count, up


def decode_points(src, device="cuda", k=16, kThresh=0.01, segMinVerts=20, viewpoint=None, return_graph=False, pitch=None,
                  outlier_ratio=None, return_kept=False, sem_label=None, ins_label=None, n_classes=20, outlier_radius=None,
                  outlier_min_pts=None, orient=None, upright=None):
    """decode_mesh for a scan without faces: `src` is a vertex-only `.ply` path or (xyz [V,3], colours [V,3] 0..255).
    centre_and_scale -> knn_graph -> point_normals -> knn_edges -> segment_point.  Returns xyz (mean-centred), rgb, nl and
    sup on `device` -- what SceneCache and save_decoded take (no `face`) -- plus idx and d2 when return_graph is set.
    `viewpoint` is given in the final frame (upright when `upright` is set, and centred); None is the cloud's mean.

    `orient="graph"` makes the normals' signs consistent over the kNN graph before the segmentation (orient_normals between
    point_normals and segment_point): towards one viewpoint, a surface seen edge-on gets its signs from noise, and
    segment_point cuts between two neighbours of opposite sign.  The result gains flipped (bool) and tree (int32).  None
    leaves the normals as point_normals gives them; any other value raises ValueError.

    A raw sensor scan (uneven density, flying pixels) is brought to the network's pitch first: with `pitch` the points are
    thinned to one centroid per cell (thin_points), with `outlier_ratio` the points whose mean neighbour distance exceeds
    mu + ratio * sigma are dropped (knn_graph over k neighbours, outlier_mask); the chain above then runs on the kept
    points exactly as if they had been given as `src`.  The result gains raw_index (int32 [V]: for every raw point its row
    among the kept points, -1 = none; see raw_index and carry_labels) and count (int32: raw points behind each kept one),
    and with return_kept also kept_xyz / kept_rgb, the kept points before centring and scaling.

    `outlier_radius` and `outlier_min_pts` (both or neither, and not together with `outlier_ratio`) are the other standard
    filter, for flying pixels: a point is kept when at least outlier_min_pts other points lie within outlier_radius
    (radius_outlier_mask), and a dropped point is spoken for by its nearest KEPT point within that radius
    (radius_raw_index).  No kNN graph is built over the unfiltered points; everything behind the front is the same.

    `upright` turns a scan that arrives in its sensor's frame (y down and z forward, or anything else) so that its floor is
    level and z is up, the one "up" the network's weights know: True, or a dict of fit_plane's keyword arguments
    (threshold defaults to `pitch` when given, else 0.02).  It takes effect on the kept points -- after thin_points and the
    outlier filter, directly after the upload without them -- and before the centring; everything behind it sees the
    upright cloud.  The result gains R (f64 [3, 3]), plane (f64 [4]), floor (bool [M]) and height (f32 [M]) of the kept
    points; kept_xyz (return_kept) stays in the sensor's frame, and R maps it.  Without a hint the largest one-sided plane
    wins, which in a room with a long wall may be that wall: a caller whose sensor knows roughly where up is should pass
    up_hint.  No plane at all raises ValueError("decode_points: no floor plane found ...").  None is the decode of
    before, byte for byte.

    An annotated scan: `sem_label` and `ins_label` (both or neither; one per raw point; integer arrays or tensors, or the
    float64 arrays the reference's `.npy` files hold; negative = unannotated) are voted down to the kept points over the
    final raw_index (vote_labels, `n_classes`): a raw point whose cell was dropped as an outlier votes for the kept
    neighbour that speaks for it, a point with -1 for nobody.  The result gains sem_label, ins_label (int64, -100 =
    unannotated, instance ids renumbered 0..I'-1), votes, members and ins_old_id (vote_labels' old_id).  Without pitch
    and outlier_ratio the labels pass through with the renumbering only (sem_label, ins_label, ins_old_id)."""
    if isinstance(src, (str, bytes)) or hasattr(src, "__fspath__"):
        xyz, colours = read_ply_points(src)
    else:
        xyz, colours = (t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t) for t in src)
    if orient is not None and orient != "graph":
        raise ValueError("decode_points: orient must be None or \"graph\", got %r" % (orient,))
    if (sem_label is None) != (ins_label is None):
        raise ValueError("decode_points: give both sem_label and ins_label, or neither")
    if (outlier_radius is None) != (outlier_min_pts is None):
        raise ValueError("decode_points: give both outlier_radius and outlier_min_pts, or neither")
    if outlier_radius is not None and outlier_ratio is not None:
        raise ValueError("decode_points: outlier_radius / outlier_min_pts and outlier_ratio are two filters, give one")
    upright_kw = _upright_option(upright, pitch)
    dev = torch.device(device)
    labels = None
    if sem_label is not None:
        n_raw = int(np.asarray(xyz).reshape(-1, 3).shape[0])
        labels = [_raw_labels(name, v, n_raw) for name, v in (("sem_label", sem_label), ("ins_label", ins_label))]
        labels = [torch.from_numpy(a).to(dev) for a in labels]
    raw, up = None, None
    if pitch is not None or outlier_ratio is not None or outlier_radius is not None:
        xyz, colours, *raw, up = _kept_points(xyz, colours, dev, k, pitch, outlier_ratio, outlier_radius, outlier_min_pts,
                                              upright_kw)
    elif return_kept:
        raise ValueError("decode_points: return_kept needs pitch, outlier_ratio or outlier_radius")
    elif upright_kw is not None:
        xyz, colours, _, _, up = _kept_points(xyz, colours, dev, k, None, None, upright_kw=upright_kw)
    xyz_c, rgb = centre_and_scale(xyz, colours)
    xyz_d = torch.from_numpy(np.ascontiguousarray(xyz_c, np.float32)).to(dev)
    idx, d2 = knn_graph(xyz_d, k=k)
    nl = point_normals(xyz_d, idx, viewpoint)
    oriented = orient_normals(nl, idx) if orient is not None else None
    if oriented is not None:
        nl = oriented["nl"]
    sup = segment_point(xyz_d, nl, knn_edges(idx), kThresh, segMinVerts)
    out = {"xyz": xyz_d, "rgb": torch.from_numpy(np.ascontiguousarray(rgb, np.float32)).to(dev), "nl": nl, "sup": sup}
    if oriented is not None:
        out.update(flipped=oriented["flipped"], tree=oriented["tree"])
    if up is not None:
        out.update(R=up["R"], plane=up["plane"], floor=up["floor"], height=up["height"])
    if return_graph:
        out.update(idx=idx, d2=d2)
    if raw is not None:
        out.update(raw_index=raw[0], count=raw[1])
        if return_kept:
            out.update(kept_xyz=up["kept_xyz"] if up is not None else torch.from_numpy(xyz).to(dev),
                       kept_rgb=torch.from_numpy(colours).to(dev))
    if labels is not None:
        m = int(xyz_d.shape[0])
        rows = raw[0] if raw is not None else torch.arange(m, dtype=torch.int32, device=dev)
        v = vote_labels(rows, labels[0], labels[1], m=m, n_classes=n_classes)
        out.update(sem_label=v["sem_label"], ins_label=v["ins_label"], ins_old_id=v["old_id"])
        if raw is not None:
            out.update(votes=v["votes"], members=v["members"])
    return out


SCENE_BOOKKEEPING = ("votes", "members", "ins_old_id", "raw_index", "count", "flipped", "tree",
                     "R", "plane", "floor", "height")        # of a decode, not of a scene on disk


def save_decoded(npy_dir, scene, decoded, sem_label=None, ins_label=None):
    """Write a decode_mesh result under the reference's names (`<scene>_xyz.npy` ...).  Without labels (a test-split scene
    or a user's own room) only xyz, rgb, nl, face and sup are written, as decode_scannet.py f_test does.  A decode_points
    result that carries its own sem_label / ins_label (an annotated scan) is written with them when none are passed; the
    bookkeeping arrays of a raw scan (votes, members, ins_old_id, raw_index, count, flipped, tree, R, plane, floor, height)
    are never scene files."""
    arrays = {k: (v.cpu().numpy() if torch.is_tensor(v) else np.asarray(v)) for k, v in decoded.items()
              if k not in SCENE_BOOKKEEPING}
    if (sem_label is None) != (ins_label is None):
        raise ValueError("save_decoded: give both sem_label and ins_label, or neither")
    if sem_label is not None:
        scene_io.save_scene(npy_dir, scene, sem_label=sem_label, ins_label=ins_label, **arrays)
    else:
        scene_io.save_arrays(npy_dir, scene, **arrays)          # the dict's own labels included; a scan has no face file
