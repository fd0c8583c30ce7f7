"""A minimal reader and writer of ScanNet's binary_little_endian PLY files (plyfile is not a dependency): numpy only."""
import numpy as np

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
