#!/usr/bin/env python3
"""Golden vectors for the mesh decode (pbnet_amd.mesh), produced on a CPU build machine by the reference's own code:

  * lib/segmentator/csrc/segmentator.cpp, compiled unmodified with torch.utils.cpp_extension into a scratch directory
    (-O3 -DNDEBUG, no -march: its CMake Release build), called as lib/segmentator/main.py does (segment + torch.unique);
  * face_normal / vertex_normal, taken out of datasets/scannetv2/decode_scannet.py with `ast` and exec'd (importing the
    module would start its multiprocessing Pool over the dataset).

    python tests/golden/make_mesh_golden.py [/path/to/reference [fixture ...]]      # writes tests/golden/mesh_*.npz

mesh_designed.npz is of another kind: the designed S and W cases of tests/mesh_cases.py whose sup does not depend on the order of
tied weights (ascending and descending agree, no NaN weight), each with its own k_thresh and seg_min_verts, through the same
compiled segmentator.  Inputs and sup only, under "<case>.<array>" keys, with the case names under "names".

Nothing compiled and no reference text is written to the repository: only the .npz data.

Tie condition.  std::sort is unstable, so the reference's small-segment join can depend on how tied weights are ordered.
A case is written only if its recorded sup partition equals the one tests/mesh_ref.py produces with ties in ascending AND
in descending edge-index order; otherwise the seed is perturbed.  `ids_exact` records whether the ids themselves agree
under both orders."""
import ast
import os
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import mesh_ref  # noqa: E402

REF = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
ONLY = sys.argv[2:]                      # fixture names to write; none = all
K_THRESH, MIN_VERTS = 0.01, 20


def load_reference():
    from torch.utils.cpp_extension import load
    build = tempfile.mkdtemp(prefix="segmentator_build_")
    seg = load(name="segmentator_ref", sources=[os.path.join(REF, "lib", "segmentator", "csrc", "segmentator.cpp")],
               extra_cflags=["-O3", "-DNDEBUG"], build_directory=build, verbose=False)
    src = open(os.path.join(REF, "datasets", "scannetv2", "decode_scannet.py")).read()
    tree = ast.parse(src)
    funcs = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in ("face_normal", "vertex_normal")]
    assert len(funcs) == 2
    ns = {"np": np}
    exec(compile(ast.Module(body=funcs, type_ignores=[]), "decode_scannet.py", "exec"), ns)
    return seg, ns["vertex_normal"]


def ref_segment_mesh(seg, xyz, faces, k_thresh=K_THRESH, min_verts=MIN_VERTS):
    index = seg.segment_mesh(torch.from_numpy(xyz.astype(np.float32)), torch.from_numpy(faces.astype(np.int64)),
                             k_thresh, min_verts)
    return torch.unique(index, return_inverse=True)[1].numpy().astype(np.int64)


def ref_segment_point(seg, xyz, normals, edges, k_thresh=K_THRESH, min_verts=MIN_VERTS):
    index = seg.segment_point(torch.from_numpy(xyz.astype(np.float32)), torch.from_numpy(normals.astype(np.float32)),
                              torch.from_numpy(edges.astype(np.int64)), k_thresh, min_verts)
    return torch.unique(index, return_inverse=True)[1].numpy().astype(np.int64)


# ------------------------------------------------------------------------------------------------------------ meshes
def grid(nu, nv, origin, du, dv):
    """(nu x nv) vertices origin + i du + j dv, two triangles per cell."""
    i, j = np.meshgrid(np.arange(nu), np.arange(nv), indexing="ij")
    v = np.asarray(origin, np.float64) + i[..., None] * np.asarray(du) + j[..., None] * np.asarray(dv)
    idx = np.arange(nu * nv).reshape(nu, nv)
    a, b, c, d = idx[:-1, :-1], idx[1:, :-1], idx[1:, 1:], idx[:-1, 1:]
    f = np.concatenate([np.stack([a, b, c], -1).reshape(-1, 3), np.stack([a, c, d], -1).reshape(-1, 3)])
    return v.reshape(-1, 3), f


def sphere(centre, r, nu, nv):
    th = np.linspace(0.15, np.pi - 0.15, nv)
    ph = np.linspace(0, 2 * np.pi, nu, endpoint=False)
    t, p = np.meshgrid(th, ph, indexing="ij")
    v = np.stack([np.sin(t) * np.cos(p), np.sin(t) * np.sin(p), np.cos(t)], -1) * r + np.asarray(centre)
    idx = np.arange(nv * nu).reshape(nv, nu)
    a, b = idx[:-1], np.roll(idx, -1, axis=1)[:-1]
    c, d = np.roll(idx, -1, axis=1)[1:], idx[1:]
    f = np.concatenate([np.stack([a, b, c], -1).reshape(-1, 3), np.stack([a, c, d], -1).reshape(-1, 3)])
    return v.reshape(-1, 3), f


def merge(parts):
    vs, fs, n = [], [], 0
    for v, f in parts:
        vs.append(v)
        fs.append(f + n)
        n += v.shape[0]
    return np.concatenate(vs), np.concatenate(fs)


def box(lo, hi, n):
    lo, hi = np.asarray(lo, float), np.asarray(hi, float)
    e = hi - lo
    X, Y, Z = np.array([e[0], 0, 0]), np.array([0, e[1], 0]), np.array([0, 0, e[2]])
    s = 1.0 / (n - 1)
    return merge([grid(n, n, lo + Z, X * s, Y * s), grid(n, n, lo, X * s, Z * s), grid(n, n, lo + Y, Z * s, X * s),
                  grid(n, n, lo, Z * s, Y * s), grid(n, n, lo + X, Y * s, Z * s)])


def room(seed):
    rng = np.random.default_rng(seed)
    parts = [grid(40, 40, [0, 0, 0], [0.1, 0, 0], [0, 0.1, 0]),
             grid(40, 14, [0, 0, 0], [0.1, 0, 0], [0, 0, 0.2]), grid(40, 14, [0, 3.9, 0], [0, 0, 0.2], [0.1, 0, 0]),
             grid(40, 14, [0, 0, 0], [0, 0, 0.2], [0, 0.1, 0]), grid(40, 14, [3.9, 0, 0], [0, 0.1, 0], [0, 0, 0.2])]
    for k in range(3):
        lo = np.array([0.5 + 1.1 * k, 0.6 + 0.7 * k, 0.0])
        parts.append(box(lo, lo + [0.6 + 0.1 * k, 0.5, 0.4 + 0.2 * k], 8))
    parts.append(sphere([2.6, 2.8, 0.9], 0.45, 26, 16))
    v, f = merge(parts)
    v = v + rng.normal(0, 0.004, v.shape)
    return v.astype(np.float32), f.astype(np.int32)


def flat(seed):
    v, f = grid(48, 48, [1.0, -2.0, 0.75], [0.05, 0, 0], [0, 0.05, 0])
    rng = np.random.default_rng(seed)
    return v.astype(np.float32), rng.permutation(f).astype(np.int32)      # face order shuffled: the same ties, other order


def oddities(seed):
    """Coincident-coordinate vertices (a seam whose column exists twice, each copy used by one side), unreferenced
    vertices, and one face that names a vertex twice, in the middle of a gently curved sheet."""
    rng = np.random.default_rng(seed)
    a_v, a_f = grid(20, 24, [0, 0, 0], [0.05, 0, 0], [0, 0.05, 0])
    b_v, b_f = grid(20, 24, [0.95, 0, 0], [0.05, 0, 0], [0, 0.05, 0])   # first column coincides with a's last
    v, f = merge([(a_v, a_f), (b_v, b_f)])
    v[:, 2] = 0.3 * np.sin(v[:, 0] * 2.0) + 0.02 * rng.normal(size=v.shape[0])
    v[480:504] = v[456:480]                                                # the seam copies stay coincident
    f = np.concatenate([f, [[252, 252, 253]]])                             # vertex (10, 12) of the first sheet, twice
    extra = rng.uniform(-1, 1, (7, 3))
    v = np.concatenate([v[:300], extra, v[300:]])                          # unreferenced vertices in the middle
    f = np.where(f >= 300, f + 7, f)
    return v.astype(np.float32), f.astype(np.int32)


def knn_case(seed):
    rng = np.random.default_rng(seed)
    n = 1800
    pts, nrm = [], []
    for k in range(4):                                                     # four noisy planes
        m = n // 4
        u = rng.uniform(0, 1, (m, 2))
        axis = np.eye(3)[k % 3]
        other = [a for a in range(3) if a != k % 3]
        p = np.zeros((m, 3))
        p[:, other[0]], p[:, other[1]] = u[:, 0], u[:, 1]
        p[:, k % 3] = 0.4 * k + rng.normal(0, 0.003, m)
        q = axis + rng.normal(0, 0.03, (m, 3))
        pts.append(p)
        nrm.append(q / np.linalg.norm(q, axis=1, keepdims=True))
    p, q = np.concatenate(pts), np.concatenate(nrm)
    p[5] = p[6]                                                            # coincident points: dd = 0 on their edge
    d = ((p[:, None, :] - p[None, :, :]) ** 2).sum(-1)
    np.fill_diagonal(d, np.inf)
    d[5, 6] = d[6, 5] = -1.0
    nn = np.argsort(d, axis=1, kind="stable")[:, :6]
    edges = np.stack([np.repeat(np.arange(p.shape[0]), 6), nn.reshape(-1)], 1)
    return p.astype(np.float32), q.astype(np.float32), edges.astype(np.int64)


def centred(v, rng):
    """decode_scannet.py:62-70 for synthetic colours: xyz - mean in its (N, 6) float32 layout, rgb / 127.5 - 1."""
    colours = rng.integers(0, 256, (v.shape[0], 3)).astype(np.uint8)
    vertices = np.zeros(shape=[v.shape[0], 6], dtype=np.float32)
    vertices[:, 0:3] = v
    vertices[:, 3:6] = colours
    return colours, vertices[:, :3] - vertices[:, :3].mean(0), vertices[:, 3:] / 127.5 - 1


def designed(seg):
    """The tie-free S and W cases of tests/mesh_cases.py through the compiled segmentator: inputs and its sup."""
    import mesh_cases
    names = [n for n in mesh_cases.SMALL if n[0] in "SW" and mesh_cases.tie_free(n)]
    arrays = {"names": np.array(names)}
    for n in names:
        c = mesh_cases.case(n)
        k, m = float(np.float32(c["k_thresh"])), int(c["seg_min_verts"])
        if c["mode"] == "mesh":
            sup = ref_segment_mesh(seg, c["xyz"], c["faces"], k, m)
            arrays.update({n + ".xyz": c["xyz"], n + ".faces": c["faces"]})
        else:
            sup = ref_segment_point(seg, c["xyz"], c["normals"], c["edges"], k, m)
            arrays.update({n + ".xyz": c["xyz"], n + ".normals": c["normals"], n + ".edges": c["edges"]})
        arrays.update({n + ".sup": sup, n + ".k_thresh": np.float32(k), n + ".seg_min_verts": np.int32(m)})
        print("mesh_designed %-22s V=%d segments=%d %s" % (n, c["xyz"].shape[0], sup.max() + 1, "== mesh_ref" if np.array_equal(
            sup, mesh_cases.sup_of(c)) else "DIFFERS from mesh_ref: %s" % sup.tolist()))
    path = os.path.join(HERE, "mesh_designed.npz")
    np.savez_compressed(path, **arrays)
    print("mesh_designed: %d cases %d bytes" % (len(names), os.path.getsize(path)))


def main():
    seg, vertex_normal = load_reference()
    if not ONLY or "mesh_designed" in ONLY:
        designed(seg)
    cases = {"mesh_room": room, "mesh_flat": flat, "mesh_oddities": oddities}
    for name, make in cases.items():
        if ONLY and name not in ONLY:
            continue
        for attempt in range(50):
            seed = 1000 * len(name) + attempt
            v, f = make(seed)
            colours, xyz, rgb = centred(v, np.random.default_rng(seed + 7))
            sup = ref_segment_mesh(seg, xyz, f)
            asc = mesh_ref.segment_mesh(xyz, f, K_THRESH, MIN_VERTS, ties="asc")
            desc = mesh_ref.segment_mesh(xyz, f, K_THRESH, MIN_VERTS, ties="desc")
            if mesh_ref.same_partition(sup, asc) and mesh_ref.same_partition(sup, desc):
                break
            print("%s seed %d: partition depends on tie order, next seed" % (name, seed))
        else:
            raise SystemExit("%s: no seed meets the tie condition" % name)
        nl = vertex_normal(xyz, f).astype(np.float32)
        ids_exact = bool(np.array_equal(sup, asc) and np.array_equal(sup, desc))
        path = os.path.join(HERE, name + ".npz")
        np.savez_compressed(path, vertices=v, colours=colours, faces=f, xyz=xyz, rgb=rgb, nl=nl, sup=sup,
                            ids_exact=np.array(ids_exact), seed=np.array(seed), k_thresh=np.float32(K_THRESH),
                            seg_min_verts=np.int32(MIN_VERTS))
        print("%s: V=%d F=%d segments=%d ids_exact=%s seed=%d %d bytes" % (name, xyz.shape[0], f.shape[0], sup.max() + 1,
                                                                         ids_exact, seed, os.path.getsize(path)))
    if ONLY and "mesh_point" not in ONLY:
        return
    for attempt in range(50):
        seed = 4242 + attempt
        p, q, e = knn_case(seed)
        sup = ref_segment_point(seg, p, q, e)
        asc = mesh_ref.segment_point(p, q, e, K_THRESH, MIN_VERTS, ties="asc")
        desc = mesh_ref.segment_point(p, q, e, K_THRESH, MIN_VERTS, ties="desc")
        if mesh_ref.same_partition(sup, asc) and mesh_ref.same_partition(sup, desc):
            break
        print("mesh_point seed %d: partition depends on tie order, next seed" % seed)
    else:
        raise SystemExit("mesh_point: no seed meets the tie condition")
    ids_exact = bool(np.array_equal(sup, asc) and np.array_equal(sup, desc))
    path = os.path.join(HERE, "mesh_point.npz")
    np.savez_compressed(path, points=p, normals=q, edges=e, sup=sup, ids_exact=np.array(ids_exact), seed=np.array(seed),
                        k_thresh=np.float32(K_THRESH), seg_min_verts=np.int32(MIN_VERTS))
    print("mesh_point: V=%d E=%d segments=%d ids_exact=%s seed=%d %d bytes" % (p.shape[0], e.shape[0], sup.max() + 1,
                                                                             ids_exact, seed, os.path.getsize(path)))


if __name__ == "__main__":
    main()
