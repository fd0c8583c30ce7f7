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
read_ply_points  the vertex-only counterpart of read_ply
decode_points    decode_mesh without faces: xyz, rgb, nl, sup

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
CLOUD_NONFINITE, CLOUD_SORT_SPIN = 1, 8          # status bits of pbn_cloud_knn


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
    nbytes = lib.pbn_cloud_workspace_bytes(n, k)
    if nbytes == 0:
        raise ValueError("point cloud too large for the library: %d points" % n)
    dev = xyz.device
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    idx = torch.empty(n, k, dtype=torch.int32, device=dev)
    d2 = torch.empty(n, k, dtype=torch.float32, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    h = 0.0 if cell is None else float(cell)
    if cell is not None and not h > 0.0:
        raise ValueError("knn_graph: cell must be positive, got %r" % (cell,))
    args = (N.ptr(xyz), n, k, h, N.ptr(idx), N.ptr(d2), N.ptr(status), N.ptr(ws), ws.numel(), N.current_stream())
    if times is None:
        N.check(lib.pbn_cloud_knn(*args), "pbn_cloud_knn")
    else:
        t = (ctypes.c_float * len(CLOUD_STAGES))()
        N.check(lib.pbn_cloud_knn_timed(*args, t), "pbn_cloud_knn_timed")
        times.update({name: float(t[i]) for i, name in enumerate(CLOUD_STAGES)})
    st = int(status.item())
    if st & CLOUD_NONFINITE:
        raise ValueError("knn_graph: a coordinate is NaN or infinite")
    if st:
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


# ------------------------------------------------------------------------------------------------------------ PLY
_PLY_SCALARS = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "i2", "int16": "i2", "ushort": "u2",
                "uint16": "u2", "int": "i4", "int32": "i4", "uint": "u4", "uint32": "u4", "float": "f4", "float32": "f4",
                "double": "f8", "float64": "f8"}


def read_ply(path):
    """ScanNet's `_vh_clean_2.ply`: returns (xyz float32 [V, 3], colours uint8 [V, 3], faces int64 [F, 3]).

    Accepted: format binary_little_endian 1.0; element vertex with exactly `float x, y, z` then `uchar red, green, blue`
    and an optional `uchar alpha`; element face with exactly `list uchar int vertex_indices` (or `uint`), triangles only.
    Anything else raises ValueError."""
    with open(path, "rb") as fh:
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
            elif words[0] == "element":
                elements.append((words[1], int(words[2]), []))
            elif words[0] == "property":
                if not elements:
                    raise ValueError("%s: property before any element" % path)
                elements[-1][2].append(tuple(words[1:]))
            else:
                raise ValueError("%s: unsupported header line %r" % (path, line))
        body = fh.read()
    if fmt != ["binary_little_endian", "1.0"]:
        raise ValueError("%s: only binary_little_endian 1.0 is supported, got %s" % (path, fmt))
    if [e[0] for e in elements] != ["vertex", "face"]:
        raise ValueError("%s: expected elements [vertex, face], got %s" % (path, [e[0] for e in elements]))
    (_, nv, vprops), (_, nf, fprops) = elements
    names = [p[-1] for p in vprops]
    types = [p[0] for p in vprops]
    if names not in (["x", "y", "z", "red", "green", "blue"], ["x", "y", "z", "red", "green", "blue", "alpha"]) or \
            any(_PLY_SCALARS.get(t) != "f4" for t in types[:3]) or any(_PLY_SCALARS.get(t) != "u1" for t in types[3:]):
        raise ValueError("%s: vertex properties must be float x y z + uchar red green blue [alpha], got %s" % (path, vprops))
    if len(fprops) != 1 or fprops[0][0] != "list" or fprops[0][-1] != "vertex_indices" or \
            _PLY_SCALARS.get(fprops[0][1]) != "u1" or _PLY_SCALARS.get(fprops[0][2]) not in ("i4", "u4"):
        raise ValueError("%s: face must be `list uchar int|uint vertex_indices`, got %s" % (path, fprops))
    vdt = np.dtype([(n, "<f4" if i < 3 else "u1") for i, n in enumerate(names)])
    fdt = np.dtype([("n", "u1"), ("i", "<" + _PLY_SCALARS[fprops[0][2]], (3,))])
    need = nv * vdt.itemsize + nf * fdt.itemsize
    if len(body) < need:
        raise ValueError("%s: truncated body (%d bytes, need %d for triangles)" % (path, len(body), need))
    vert = np.frombuffer(body, vdt, nv, 0)
    face = np.frombuffer(body, fdt, nf, nv * vdt.itemsize)
    if nf and not np.all(face["n"] == 3):
        raise ValueError("%s: only triangle faces are supported" % path)
    xyz = np.stack([vert["x"], vert["y"], vert["z"]], axis=1).astype(np.float32)
    rgb = np.stack([vert["red"], vert["green"], vert["blue"]], axis=1).astype(np.uint8)
    return xyz, rgb, face["i"].astype(np.int64).reshape(-1, 3)


def read_ply_points(path):
    """A point cloud's PLY: returns (xyz float32 [V, 3], colours uint8 [V, 3]).

    Accepted: format binary_little_endian 1.0 with the vertex element ONLY, under read_ply's property rules (`float x, y,
    z`, `uchar red, green, blue`, an optional `uchar alpha`).  Anything else raises ValueError; a file with faces is a mesh
    and belongs to read_ply."""
    with open(path, "rb") as fh:
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
            elif words[0] == "property" and elements:
                elements[-1][2].append(tuple(words[1:]))
            else:
                raise ValueError("%s: unsupported header line %r" % (path, line))
        body = fh.read()
    if fmt != ["binary_little_endian", "1.0"]:
        raise ValueError("%s: only binary_little_endian 1.0 is supported, got %s" % (path, fmt))
    if [e[0] for e in elements] != ["vertex"]:
        raise ValueError("%s: expected the vertex element only, got %s" % (path, [e[0] for e in elements]))
    _, nv, vprops = elements[0]
    names = [p[-1] for p in vprops]
    types = [p[0] for p in vprops]
    if names not in (["x", "y", "z", "red", "green", "blue"], ["x", "y", "z", "red", "green", "blue", "alpha"]) or \
            any(_PLY_SCALARS.get(t) != "f4" for t in types[:3]) or any(_PLY_SCALARS.get(t) != "u1" for t in types[3:]):
        raise ValueError("%s: vertex properties must be float x y z + uchar red green blue [alpha], got %s" % (path, vprops))
    vdt = np.dtype([(n, "<f4" if i < 3 else "u1") for i, n in enumerate(names)])
    if nv < 0 or len(body) < nv * vdt.itemsize:
        raise ValueError("%s: truncated body (%d bytes, need %d)" % (path, len(body), nv * vdt.itemsize))
    vert = np.frombuffer(body, vdt, nv, 0)
    xyz = np.stack([vert["x"], vert["y"], vert["z"]], axis=1).astype(np.float32)
    rgb = np.stack([vert["red"], vert["green"], vert["blue"]], axis=1).astype(np.uint8)
    return xyz, rgb


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


def decode_points(src, device="cuda", k=16, kThresh=0.01, segMinVerts=20, viewpoint=None, return_graph=False):
    """decode_mesh for a scan without faces: `src` is a vertex-only `.ply` path or (xyz [V,3], colours [V,3] 0..255).
    centre_and_scale -> knn_graph -> point_normals -> knn_edges -> segment_point.  Returns xyz (mean-centred), rgb, nl and
    sup on `device` -- what SceneCache and save_decoded take (no `face`) -- plus idx and d2 when return_graph is set.
    `viewpoint` is given in the centred frame; None is the cloud's mean."""
    if isinstance(src, (str, bytes)) or hasattr(src, "__fspath__"):
        xyz, colours = read_ply_points(src)
    else:
        xyz, colours = (t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t) for t in src)
    xyz_c, rgb = centre_and_scale(xyz, colours)
    dev = torch.device(device)
    xyz_d = torch.from_numpy(np.ascontiguousarray(xyz_c, np.float32)).to(dev)
    idx, d2 = knn_graph(xyz_d, k=k)
    nl = point_normals(xyz_d, idx, viewpoint)
    sup = segment_point(xyz_d, nl, knn_edges(idx), kThresh, segMinVerts)
    out = {"xyz": xyz_d, "rgb": torch.from_numpy(np.ascontiguousarray(rgb, np.float32)).to(dev), "nl": nl, "sup": sup}
    if return_graph:
        out.update(idx=idx, d2=d2)
    return out


def save_decoded(npy_dir, scene, decoded, sem_label=None, ins_label=None):
    """Write a decode_mesh result under the reference's names (`<scene>_xyz.npy` ...).  Without labels (a test-split scene
    or a user's own room) only xyz, rgb, nl, face and sup are written, as decode_scannet.py f_test does."""
    arrays = {k: (v.cpu().numpy() if torch.is_tensor(v) else np.asarray(v)) for k, v in decoded.items()}
    if (sem_label is None) != (ins_label is None):
        raise ValueError("save_decoded: give both sem_label and ins_label, or neither")
    if sem_label is not None:
        scene_io.save_scene(npy_dir, scene, sem_label=sem_label, ins_label=ins_label, **arrays)
    else:
        scene_io.save_arrays(npy_dir, scene, **arrays)
