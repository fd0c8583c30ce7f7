"""Mesh decode on the MI355X: the first stage of the reference's pipeline (datasets/scannetv2/decode_scannet.py f_test,
README "Dataset Preparation" step 3) -- a scan's `_vh_clean_2.ply` mesh to the per-scene arrays xyz, rgb, nl, face, sup.

vertex_normals   decode_scannet.py:76-96 (face_normal + vertex_normal), bit for bit in float32
segment_mesh     lib/segmentator segment_mesh + main.py's torch.unique relabel (Felzenszwalb graph segmentation)
segment_point    lib/segmentator segment_point (caller-given normals and E x 2 edges)
decode_mesh      f_test without the file writes: mean-centred xyz, rgb / 127.5 - 1, nl, face (int32), sup
decode_points    decode_mesh without faces: xyz, rgb, nl, sup
decode_frames    decode_points for posed depth frames: frames_to_points, then the same chain, normals towards each sensor
save_decoded     the reference's `<scene>_{xyz,rgb,nl,face,sup}.npy` (+ labels when given) through scene_io

The rest lives in two other modules and is reachable here as before.
read_ply, read_ply_points, write_ply   ply.py, numpy only: ScanNet's binary_little_endian meshes and vertex-only scans
cloud.py, scans without a mesh (csrc/cloud.hip): segment_point's normals and edges from the points alone.
knn_graph        the exact k nearest neighbours over a uniform grid, bit for bit a float32 brute force
point_normals    float64 PCA normals over each point and its neighbours, turned towards a viewpoint, or each towards its
                 own point's sensor position (views, view_of)
knn_edges        the graph as segment_point's E x 2 edges
orient_normals   point_normals' signs made consistent over the graph (csrc/orient.hip), bit for bit tests/orient_ref.py
fit_plane        the floor plane of a scan (csrc/upright.hip): RANSAC on the device, float64 refit, bit for bit tests/upright_ref.py
upright          fit_plane and the scan rotated so that the plane's normal is +z
frames.py, posed depth frames (csrc/frames.hip): what a depth camera hands over, before it is a cloud.
frames_to_points depth images, poses and intrinsics back-projected into one compacted raw cloud in pixel order, every point
                 with its pixel (hence its frame) and every frame with its sensor centre; bit for bit tests/frames_ref.py
cloud.py, raw sensor scans (csrc/thin.hip): to the network's pitch and back.
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
import types

import numpy as np
import torch

from . import _native as N
from . import frames as _frames
from . import scene_io
from .cloud import (CLOUD_EXTENT, CLOUD_MAX_K, CLOUD_NONFINITE, CLOUD_SORT_SPIN, CLOUD_STAGES, CLOUD_WALK_CAP, ORIENT_STAGES,  # noqa: F401
                    RADIUS_MAX_CAP, RADIUS_STAGES, THIN_STAGES, UPRIGHT_KEYS, UPRIGHT_MAX_HYP, UPRIGHT_STAGES, VOTE_INS_RANGE,
                    VOTE_MAX_CLASSES, VOTE_MAX_INS, VOTE_ROW_RANGE, VOTE_SEM_RANGE, VOTE_STAGES, _device, _f32, _got, _scan_workspace, _upright,
                    _upright_args, carry_labels, fit_plane, knn_edges, knn_graph, orient_normals, outlier_mask, point_normals,
                    radius_count, radius_outlier_mask, radius_raw_index, raw_index, thin_points, upright, vote_labels)
from .frames import FRAMES_STAGES, frames_to_points  # noqa: F401
from .ply import _PLY_SCALARS, _read_ply_header, _vertex_arrays, _vertex_dtype, read_ply, read_ply_points, write_ply  # noqa: F401

MESH_NORMALS, MESH_SEGMENT, MESH_SEGMENT_POINT = 0, 1, 2
STAGES = ("incidence", "normals", "weights", "sort", "read-back", "host sweep", "relabel")


def _index(name, t, width):
    """`t` is an int32 or int64 [n, width] tensor: 1 when it is int64."""
    if not torch.is_tensor(t) or t.dtype not in (torch.int32, torch.int64) or t.dim() != 2 or t.shape[1] != width:
        raise TypeError("%s must be an int32 or int64 [n, %d] tensor, got %s" % (name, width, _got(t)))
    return int(t.dtype == torch.int64)


def _workspace(mode, n_vertices, n_elems, dev):
    return _scan_workspace(N.lib().pbn_mesh_workspace_bytes(mode, n_vertices, n_elems), dev,
                           "%d vertices, %d elements" % (n_vertices, n_elems), "mesh")


def _raise(rc, what):
    if rc == N.PBN_ERR_RANGE:
        raise ValueError("%s: an index lies outside [0, number of vertices)" % what)
    N.check(rc, what)


def vertex_normals(xyz, faces):
    """decode_scannet.py vertex_normal(xyz, faces): float32 [V, 3] on the device, bit for bit."""
    _f32("xyz", xyz)
    i64 = _index("faces", faces, 3)
    xyz, faces = _device(xyz, faces)
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
    _f32("vertices", vertices)
    i64 = _index("faces", faces, 3)
    vertices, faces = _device(vertices, faces)
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
    _f32("vertices", vertices)
    _f32("normals", normals)
    i64 = _index("edges", edges, 2)
    v, e = int(vertices.shape[0]), int(edges.shape[0])
    if normals.shape[0] != v:
        raise ValueError("segment_point: %d normals for %d vertices" % (normals.shape[0], v))
    vertices, normals, edges = _device(vertices, normals, edges)
    sup = torch.empty(v, dtype=torch.int64, device=vertices.device)
    ws = _workspace(MESH_SEGMENT_POINT, v, e, vertices.device)
    rc = N.lib().pbn_mesh_segment_point(N.ptr(vertices), N.ptr(normals), v, N.ptr(edges), i64, e, float(kThresh),
                                        int(segMinVerts), N.ptr(sup), N.ptr(ws), ws.numel(), N.current_stream())
    _raise(rc, "segment_point")
    return sup


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


def _kept_points(xyz, colours, dev, k, pitch, outlier_ratio, outlier_radius, outlier_min_pts, upright_kw, want_first=False):
    """decode_points' front for a raw scan: upload (host arrays; device tensors are taken as they are), thin_points (pitch), then knn_graph -> outlier_mask -> raw_index
    (outlier_ratio) or radius_outlier_mask -> radius_raw_index (outlier_radius, outlier_min_pts: no graph over the
    unfiltered points), and the compaction.  The kept points come back as host arrays -- centre_and_scale is a host numpy
    expression, so the kept M x 6 floats make one extra round trip -- with raw_index and count on the device (None when the
    points were neither thinned nor filtered) and `up`, upright's result or None.  With `upright_kw` (fit_plane's keyword arguments) the
    kept points are turned upright while they are still on the device: the returned xyz is in the upright frame, and the
    result's "kept_xyz" holds the kept points in the sensor's frame.  `first` (with want_first) is the lowest raw member of
    every kept row -- thin_points' first, compacted by the filter's keep -- or None when nothing was thinned or filtered."""
    xyz_d, col_d = (t if torch.is_tensor(t) and t.is_cuda else
                    torch.from_numpy(np.ascontiguousarray(t, np.float32).reshape(-1, 3)).to(dev) for t in (xyz, colours))
    n_raw = int(xyz_d.shape[0])
    inverse = count = first = None
    if pitch is not None:
        th = thin_points(xyz_d, col_d, pitch)
        xyz_d, col_d, count, inverse, first = th["xyz"], th["rgb"], th["count"], th["inverse"], th["first"]
    elif outlier_ratio is not None or outlier_radius is not None:
        count = torch.ones(n_raw, dtype=torch.int32, device=dev)
        inverse = torch.arange(n_raw, dtype=torch.int32, device=dev)
        first = inverse
    keep = None
    if outlier_ratio is not None:
        idx, d2 = knn_graph(xyz_d, k=k)
        keep, _ = outlier_mask(d2, outlier_ratio)
        inverse = raw_index(inverse, keep, idx)
    elif outlier_radius is not None:
        keep = radius_outlier_mask(xyz_d, outlier_radius, outlier_min_pts)
        inverse = radius_raw_index(inverse, keep, xyz_d, outlier_radius)
    if keep is not None:
        xyz_d, col_d, count = xyz_d[keep], col_d[keep], count[keep]
        first = first[keep] if want_first else None
    up = None
    if upright_kw is not None:
        up = upright(xyz_d, **upright_kw)
        if not up["found"]:
            raise ValueError("decode_points: no floor plane found among %d points (%d hypotheses, %d alive at the end); "
                             "check threshold, up_hint and below_frac" % (int(xyz_d.shape[0]), upright_kw["hypotheses"],
                                                                          int(up["info"][6])))
        up["kept_xyz"], xyz_d = xyz_d, up["xyz"]
    return types.SimpleNamespace(xyz=xyz_d.cpu().numpy(), colours=col_d.cpu().numpy(), raw_index=inverse, count=count, up=up,
                                 first=first)


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
    opts = _decode_options("decode_points", k, kThresh, segMinVerts, viewpoint, return_graph, pitch, outlier_ratio, return_kept,
                           sem_label, ins_label, n_classes, outlier_radius, outlier_min_pts, orient, upright)
    dev = torch.device(device)
    labels = None
    if sem_label is not None:
        n_raw = int(np.asarray(xyz).reshape(-1, 3).shape[0])
        labels = [_raw_labels(name, v, n_raw) for name, v in (("sem_label", sem_label), ("ins_label", ins_label))]
        labels = [torch.from_numpy(a).to(dev) for a in labels]
    return _decode_cloud(xyz, colours, dev, labels, opts)


def _decode_options(what, k, kThresh, segMinVerts, viewpoint, return_graph, pitch, outlier_ratio, return_kept, sem_label, ins_label,
                    n_classes, outlier_radius, outlier_min_pts, orient, upright):
    """decode_points' options, checked before anything is uploaded: what _decode_cloud reads."""
    if orient is not None and orient != "graph":
        raise ValueError("%s: orient must be None or \"graph\", got %r" % (what, orient))
    if (sem_label is None) != (ins_label is None):
        raise ValueError("%s: give both sem_label and ins_label, or neither" % what)
    if (outlier_radius is None) != (outlier_min_pts is None):
        raise ValueError("%s: give both outlier_radius and outlier_min_pts, or neither" % what)
    if outlier_radius is not None and outlier_ratio is not None:
        raise ValueError("%s: outlier_radius / outlier_min_pts and outlier_ratio are two filters, give one" % what)
    upright_kw = _upright_option(upright, pitch)
    front = pitch is not None or outlier_ratio is not None or outlier_radius is not None
    if return_kept and not front:
        raise ValueError("%s: return_kept needs pitch, outlier_ratio or outlier_radius" % what)
    return types.SimpleNamespace(k=k, kThresh=kThresh, segMinVerts=segMinVerts, viewpoint=viewpoint, return_graph=return_graph,
                                 pitch=pitch, outlier_ratio=outlier_ratio, return_kept=return_kept, n_classes=n_classes,
                                 outlier_radius=outlier_radius, outlier_min_pts=outlier_min_pts, orient=orient,
                                 upright_kw=upright_kw, front=front)


def _centred_mean(xyz):
    """The float32 mean centre_and_scale subtracts, by its own expression on its own layout."""
    vertices = np.zeros(shape=[xyz.shape[0], 6], dtype=np.float32)
    vertices[:, 0:3] = xyz
    return vertices[:, :3].mean(0)


def _sensor_views(kept, sensor, n_kept, dev):
    """decode_frames(normals="sensor"): views f32 [F, 3], the sensor centres in the final frame, and view_of int32 [M], the
    frame of every kept row's lowest raw member.  On the host in float64: R . c when the scan was turned upright, minus the
    float32 mean centre_and_scale subtracted, rounded once."""
    c = sensor.centres.astype(np.float64)
    if kept.up is not None:
        R = kept.up["R"].cpu().numpy()
        c = np.stack([(R[r, 0] * c[:, 0] + R[r, 1] * c[:, 1]) + R[r, 2] * c[:, 2] for r in range(3)], axis=1)
    with np.errstate(invalid="ignore"):
        views = (c - _centred_mean(kept.xyz).astype(np.float64)[None, :]).astype(np.float32)
    first = getattr(kept, "first", None)
    frame = sensor.frame if first is None else sensor.frame[first.long()]
    assert int(frame.shape[0]) == n_kept
    return torch.from_numpy(np.ascontiguousarray(views)).to(dev), frame.contiguous()


def _fused_normals(nl, up):
    """decode_frames(fuse=, normals="tsdf"): the fused surface's normals in the final frame -- as they are, or with `upright`
    R . n in float64, (R[r,0]*n0 + R[r,1]*n1) + R[r,2]*n2, rounded once."""
    if up is None:
        return nl.contiguous()
    R, n = up["R"].to(nl.device, torch.float64), nl.double()
    return torch.stack([(R[r, 0] * n[:, 0] + R[r, 1] * n[:, 1]) + R[r, 2] * n[:, 2] for r in range(3)], dim=1).float().contiguous()


def _decode_cloud(xyz, colours, dev, labels, o, sensor=None, fused=None):
    """What decode_points does with a raw cloud -- host arrays, or the device tensors they would be uploaded to -- and its
    checked options `o` (_decode_options); `labels` are the raw points' int32 labels on the device or None.  `sensor`
    (decode_frames: frame int32 [N] on the device, centres f32 [F, 3] on the host; `turn` says whether the normals look at
    them) adds `frame`, the frame of every kept row.  `fused` (decode_frames with fuse: nl f32 [N, 3] and weight int32 [N] of
    the fused surface on the device; `turn` says whether nl replaces point_normals' output) adds `fuse_weight`."""
    kept = types.SimpleNamespace(xyz=xyz, colours=colours, up=None)     # the decode of before: nothing goes through the front
    if o.front or o.upright_kw is not None:
        kept = _kept_points(xyz, colours, dev, o.k, o.pitch, o.outlier_ratio, o.outlier_radius, o.outlier_min_pts, o.upright_kw,
                            want_first=sensor is not None or fused is not None)
    elif torch.is_tensor(xyz):
        kept = types.SimpleNamespace(xyz=xyz.cpu().numpy(), colours=colours.cpu().numpy(), up=None)
    xyz_c, rgb = centre_and_scale(kept.xyz, kept.colours)
    xyz_d = torch.from_numpy(np.ascontiguousarray(xyz_c, np.float32)).to(dev)
    idx, d2 = knn_graph(xyz_d, k=o.k)
    frame = None
    if sensor is not None:
        views, frame = _sensor_views(kept, sensor, int(xyz_d.shape[0]), dev)
    fuse_weight = None
    if fused is not None:                                     # a kept row speaks with its lowest raw member, as `frame` does
        first = getattr(kept, "first", None)
        rows = slice(None) if first is None else first.long()
        fuse_weight = fused.weight[rows].contiguous()
        assert int(fuse_weight.shape[0]) == int(xyz_d.shape[0])
    if fused is not None and fused.turn:
        nl = _fused_normals(fused.nl[rows], kept.up)
    elif sensor is not None and sensor.turn:
        nl = point_normals(xyz_d, idx, views=views, view_of=frame)
    else:
        nl = point_normals(xyz_d, idx, o.viewpoint)
    oriented = orient_normals(nl, idx) if o.orient is not None else None
    if oriented is not None:
        nl = oriented["nl"]
    sup = segment_point(xyz_d, nl, knn_edges(idx), o.kThresh, o.segMinVerts)
    out = {"xyz": xyz_d, "rgb": torch.from_numpy(np.ascontiguousarray(rgb, np.float32)).to(dev), "nl": nl, "sup": sup}
    if oriented is not None:
        out.update(flipped=oriented["flipped"], tree=oriented["tree"])
    up = kept.up
    if up is not None:
        out.update(R=up["R"], plane=up["plane"], floor=up["floor"], height=up["height"])
    if o.return_graph:
        out.update(idx=idx, d2=d2)
    if o.front:
        out.update(raw_index=kept.raw_index, count=kept.count)
    if o.return_kept:
        out.update(kept_xyz=up["kept_xyz"] if up is not None else torch.from_numpy(kept.xyz).to(dev),
                   kept_rgb=torch.from_numpy(kept.colours).to(dev))
    if labels is not None:
        m = int(xyz_d.shape[0])
        rows = kept.raw_index if o.front else torch.arange(m, dtype=torch.int32, device=dev)
        v = vote_labels(rows, labels[0], labels[1], m=m, n_classes=o.n_classes)
        out.update(sem_label=v["sem_label"], ins_label=v["ins_label"], ins_old_id=v["old_id"])
        if o.front:
            out.update(votes=v["votes"], members=v["members"])
    if frame is not None:
        out.update(frame=frame)
    if fuse_weight is not None:
        out.update(fuse_weight=fuse_weight)
    return out


_NORMALS_DEFAULT = "default"                                 # decode_frames: "sensor", or "tsdf" with fuse
FUSE_KEYS = ("voxel", "trunc", "min_weight")


def _fuse_option(fuse):
    """decode_frames' `fuse` as fuse_frames' keyword arguments, or None; checked before anything is uploaded."""
    if fuse is None or fuse is False:
        return None
    if fuse is True:
        fuse = {}
    if not isinstance(fuse, dict):
        raise TypeError("decode_frames: fuse must be None, True or a dict of voxel, trunc and min_weight, got %r" % (fuse,))
    unknown = sorted(set(fuse) - set(FUSE_KEYS))
    if unknown:
        raise TypeError("decode_frames: fuse has no argument %s (it takes %s)" % (", ".join(map(repr, unknown)), ", ".join(FUSE_KEYS)))
    kw = dict(voxel=0.02, trunc=None, min_weight=1)
    kw.update(fuse)
    _frames._fuse_args("decode_frames: fuse", kw["voxel"], kw["trunc"], kw["min_weight"])
    return kw


def _label_image(name, labels, shape):
    """decode_frames' label image, checked on the host: an integer tensor [F, H, W], wherever it lives."""
    t = labels if torch.is_tensor(labels) else torch.from_numpy(np.ascontiguousarray(labels))
    if t.dtype.is_floating_point or t.dtype == torch.bool or t.is_complex():
        raise TypeError("decode_frames: %s must be an integer image, got %s" % (name, t.dtype))
    if tuple(t.shape) != tuple(shape):
        raise ValueError("decode_frames: %s must have shape %s, got %s" % (name, list(shape), list(t.shape)))
    return t


def decode_frames(depth, poses, intrinsics, colour=None, device="cuda", depth_scale=1000.0, depth_min=0.0, depth_max=float("inf"),
                  stride=1, edge=None, normals=_NORMALS_DEFAULT, sem_label=None, ins_label=None, k=16, kThresh=0.01, segMinVerts=20,
                  viewpoint=None, return_graph=False, pitch=None, outlier_ratio=None, return_kept=False, n_classes=20,
                  outlier_radius=None, outlier_min_pts=None, orient=None, upright=None, fuse=None):
    """decode_points for what a depth camera hands over: frames_to_points (pbnet_amd/frames.py: `depth` [F, H, W] uint16 or
    float32, `colour` uint8 [F, H, W, 3] or None -- arrays or tensors, brought to `device` --, host `poses` [F, 4, 4] and
    `intrinsics`, and depth_scale, depth_min, depth_max, stride, edge), then decode_points' chain on the raw cloud with
    decode_points' options.  Without `colour` every point is black (0, 0, 0).  With `pitch` the N raw points never visit
    the host: the kept M points make the one round trip through centre_and_scale that decode_points documents.

    `normals="sensor"` turns every normal towards the sensor position that saw its point instead of one viewpoint for the
    whole cloud: a kept row's frame is that of its lowest raw member (thin_points' first, compacted by the outlier filter's
    keep; the point itself without a front), and the F sensor centres (frames_to_points' centres) are brought into the
    final frame on the host in float64 -- R . c when `upright` is set, minus the float32 mean centre_and_scale subtracted,
    rounded once -- and handed to point_normals(views=, view_of=).  It excludes `viewpoint`.  `orient="graph"` may still
    follow.  `normals=None` is decode_points on frames_to_points' cloud, byte for byte.

    `sem_label` and `ins_label` (both or neither) are integer images [F, H, W]: the raw points' labels are gathered through
    `pixel` and voted down as decode_points does.

    The result is decode_points' plus pixel (int32 [N], of the raw points: raw_index speaks of the same rows), frame (int32
    [M], of the kept points), centres (f32 [F, 3], in the frames' world), frame_start (int32 [F + 1], rows of the raw
    cloud) and skipped (bool [F]).

    `fuse` (True, or a dict of voxel, trunc and min_weight) puts volumetric fusion between the frames and the chain:
    fuse_frames' surface points (xyz, rgb; black without `colour`) are the raw cloud, and pitch, the outlier filters,
    upright and orient work on it as before.  `normals` is then "tsdf" (the default with fuse: a kept row takes the fused
    normal of its lowest raw member -- thin_points' first, compacted by the filter's keep --, turned by R when `upright` is
    set, in float64, rounded once; it replaces point_normals' output) or None (PCA normals, the chain as it is); "sensor"
    raises ValueError, because a fused point has no single frame.  Label images and a stride other than 1 raise ValueError
    with fuse: label fusion per voxel is not built.  The result gains fuse_weight (int32 [M], of the kept rows' lowest
    members) and n_blocks, and has no pixel, frame or frame_start.  fuse=None is the decode of before, byte for byte."""
    fuse_kw = _fuse_option(fuse)
    if fuse_kw is not None:
        return _decode_fused(depth, poses, intrinsics, colour, device, depth_scale, depth_min, depth_max, stride, edge, normals,
                             sem_label, ins_label, fuse_kw,
                             dict(k=k, kThresh=kThresh, segMinVerts=segMinVerts, viewpoint=viewpoint, return_graph=return_graph,
                                  pitch=pitch, outlier_ratio=outlier_ratio, return_kept=return_kept, n_classes=n_classes,
                                  outlier_radius=outlier_radius, outlier_min_pts=outlier_min_pts, orient=orient, upright=upright))
    if normals == _NORMALS_DEFAULT:
        normals = "sensor"
    if normals is not None and normals != "sensor":
        raise ValueError("decode_frames: normals must be None or \"sensor\", got %r" % (normals,))
    if normals == "sensor" and viewpoint is not None:
        raise ValueError("decode_frames: normals=\"sensor\" and viewpoint are two ways to turn the normals, give one")
    opts = _decode_options("decode_frames", k, kThresh, segMinVerts, viewpoint, return_graph, pitch, outlier_ratio, return_kept,
                           sem_label, ins_label, n_classes, outlier_radius, outlier_min_pts, orient, upright)
    dev = torch.device(device)
    depth, colour = (t if t is None or torch.is_tensor(t) else torch.from_numpy(np.ascontiguousarray(t)) for t in (depth, colour))
    shape, pose, _, _ = _frames._frames_args("decode_frames", depth, poses, intrinsics, colour, depth_scale, depth_min, depth_max,
                                             stride, edge)
    labels = None
    if sem_label is not None:
        labels = [_label_image(name, v, shape) for name, v in (("sem_label", sem_label), ("ins_label", ins_label))]
    cloud = _frames.frames_to_points(depth.to(dev), pose.reshape(-1, 4, 4), intrinsics, None if colour is None else colour.to(dev),
                                     depth_scale, depth_min, depth_max, stride, edge)
    pixel = cloud["pixel"]
    if labels is not None:
        labels = [t.to(dev).reshape(-1)[pixel.long()].to(torch.int32) for t in labels]
    n = int(pixel.shape[0])
    rgb = cloud["rgb"] if colour is not None else torch.zeros(n, 3, dtype=torch.float32, device=dev)
    sensor = types.SimpleNamespace(frame=torch.div(pixel, max(shape[1] * shape[2], 1), rounding_mode="floor").to(torch.int32),
                                   centres=_frames.host_centres(pose)[0], turn=normals == "sensor")
    out = _decode_cloud(cloud["xyz"], rgb, dev, labels, opts, sensor)
    out.update(pixel=pixel, centres=cloud["centres"], frame_start=cloud["frame_start"], skipped=cloud["skipped"])
    return out


def _decode_fused(depth, poses, intrinsics, colour, device, depth_scale, depth_min, depth_max, stride, edge, normals, sem_label,
                  ins_label, fuse_kw, chain):
    """decode_frames with `fuse`: every exclusion on the host first, then fuse_frames, then decode_points' chain."""
    if normals == _NORMALS_DEFAULT:
        normals = "tsdf"
    if normals == "sensor":
        raise ValueError("decode_frames: normals=\"sensor\" needs one frame per point, which a fused point does not have; "
                         "give \"tsdf\" or None with fuse")
    if normals is not None and normals != "tsdf":
        raise ValueError("decode_frames: normals must be None or \"tsdf\" with fuse, got %r" % (normals,))
    if sem_label is not None or ins_label is not None:
        raise ValueError("decode_frames: sem_label / ins_label cannot be given with fuse: labels are not fused per voxel")
    if isinstance(stride, bool) or stride != 1:
        raise ValueError("decode_frames: stride must be 1 with fuse (every depth sample is integrated), got %r" % (stride,))
    opts = _decode_options("decode_frames", chain["k"], chain["kThresh"], chain["segMinVerts"], chain["viewpoint"],
                           chain["return_graph"], chain["pitch"], chain["outlier_ratio"], chain["return_kept"], None, None,
                           chain["n_classes"], chain["outlier_radius"], chain["outlier_min_pts"], chain["orient"], chain["upright"])
    dev = torch.device(device)
    depth, colour = (t if t is None or torch.is_tensor(t) else torch.from_numpy(np.ascontiguousarray(t)) for t in (depth, colour))
    _, pose, _, _ = _frames._frames_args("decode_frames", depth, poses, intrinsics, colour, depth_scale, depth_min, depth_max, 1, edge)
    surface = _frames.fuse_frames(depth.to(dev), pose.reshape(-1, 4, 4), intrinsics, None if colour is None else colour.to(dev),
                                  depth_scale=depth_scale, depth_min=depth_min, depth_max=depth_max, edge=edge, **fuse_kw)
    n = int(surface["xyz"].shape[0])
    rgb = surface["rgb"] if colour is not None else torch.zeros(n, 3, dtype=torch.float32, device=dev)
    fused = types.SimpleNamespace(nl=surface["nl"], weight=surface["weight"], turn=normals == "tsdf")
    out = _decode_cloud(surface["xyz"], rgb, dev, None, opts, fused=fused)
    out.update(n_blocks=surface["n_blocks"], centres=surface["centres"], skipped=surface["skipped"])
    return out


SCENE_BOOKKEEPING = ("votes", "members", "ins_old_id", "raw_index", "count", "flipped", "tree",
                     "R", "plane", "floor", "height", "pixel", "frame", "centres", "frame_start", "skipped",
                     "fuse_weight", "n_blocks")   # of a decode, not of a scene on disk


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
