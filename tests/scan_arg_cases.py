"""Single-fault calls of every public function of pbnet_amd.mesh, pbnet_amd.cloud and pbnet_amd.ply, on CPU tensors and
numpy arrays: each case is (function, args, kwargs, the one thing that is wrong).  "device" means every value is fine and
only the tensors' device is not.  tests/golden/scan_arg_messages.json holds what each call raised before the modules were
split (tests/golden/make_scan_arg_messages.py records it); tests/test_scan_args_cpu.py replays the list.

STATUS_CALLS drives the shared status word: per stage a valid call and the keyword details its messages show, and
STATUS_BITS the single bits tried for each."""
import atexit
import os
import shutil
import tempfile

import numpy as np
import torch

NAN, INF = float("nan"), float("inf")
X = torch.zeros(4, 3)                                        # float32 [4, 3] on the CPU
X8 = torch.zeros(8, 3)
IDX = torch.zeros(4, 2, dtype=torch.int32)
D2 = torch.zeros(4, 3)
INV = torch.zeros(6, dtype=torch.int32)
KEEP = torch.ones(4, dtype=torch.bool)
FACES = torch.zeros(2, 3, dtype=torch.int64)
EDGES = torch.zeros(2, 2, dtype=torch.int64)
NPX = np.zeros((4, 3), np.float32)
SCAN = (np.zeros((4, 3), np.float32), np.zeros((4, 3), np.uint8))
SCAN8 = (np.zeros((8, 3), np.float32), np.zeros((8, 3), np.float32))
MESH = (np.zeros((4, 3), np.float32), np.zeros((4, 3), np.uint8), np.array([[0, 1, 4]]))


def i32(*v):
    return torch.tensor(v, dtype=torch.int32)


TMP = tempfile.mkdtemp(prefix="scan_arg_cases_")             # shown as <tmp> in a message
atexit.register(shutil.rmtree, TMP, ignore_errors=True)


def _ply(name, lines, body=b""):
    path = os.path.join(TMP, name)
    with open(path, "wb") as fh:
        fh.write(("\n".join(lines) + "\n").encode("ascii") + body)
    return path


_VERTEX = ["property float x", "property float y", "property float z", "property uchar red", "property uchar green",
           "property uchar blue"]
_HEAD = ["ply", "format binary_little_endian 1.0"]
_FACE = ["element face 1", "property list uchar int vertex_indices"]
PLY_NOT = _ply("not.ply", ["plx"])
PLY_ASCII = _ply("ascii.ply", ["ply", "format ascii 1.0", "element vertex 0"] + _VERTEX + ["end_header"])
PLY_NO_END = _ply("no_end.ply", _HEAD + ["element vertex 0"] + _VERTEX)
PLY_PROPERTY_FIRST = _ply("property_first.ply", _HEAD + ["property float x", "end_header"])
PLY_LINE = _ply("line.ply", _HEAD + ["elephant vertex 0", "end_header"])
PLY_POINTS = _ply("points.ply", _HEAD + ["element vertex 1"] + _VERTEX + ["end_header"], bytes(15))
PLY_MESH = _ply("mesh.ply", _HEAD + ["element vertex 1"] + _VERTEX + _FACE + ["end_header"], bytes(15) + b"\x03" + bytes(12))
PLY_DOUBLE = _ply("double.ply", _HEAD + ["element vertex 0", "property double x"] + _VERTEX[1:] + _FACE + ["end_header"])
PLY_FACE_TYPE = _ply("face_type.ply", _HEAD + ["element vertex 0"] + _VERTEX +
                     ["element face 0", "property list uchar short vertex_indices", "end_header"])
PLY_SHORT = _ply("short.ply", _HEAD + ["element vertex 1"] + _VERTEX + _FACE + ["end_header"], bytes(15))
PLY_QUAD = _ply("quad.ply", _HEAD + ["element vertex 1"] + _VERTEX + _FACE + ["end_header"], bytes(15) + b"\x04" + bytes(12))
PLY_POINTS_SHORT = _ply("points_short.ply", _HEAD + ["element vertex 2"] + _VERTEX + ["end_header"], bytes(15))

UP = dict(threshold=0.02)                                    # fit_plane's one required argument, valid


def _up(**kw):
    return dict(UP, **kw)


# tests/test_upright_ref_cpu.py's BAD, by the argument that is wrong
_UPRIGHT_BAD = [
    ("threshold", 0.0), ("threshold", -1.0), ("threshold", NAN), ("threshold", INF), ("threshold", 1e39),
    ("threshold", "0.02"), ("threshold", True),
    ("hypotheses", 0), ("hypotheses", 4097), ("hypotheses", 16.0), ("hypotheses", True),
    ("seed", -1), ("seed", 1 << 64), ("seed", 1.0),
    ("up_hint", (0, 0)), ("up_hint", (0, 0, 0)), ("up_hint", (0, NAN, 1)), ("up_hint", (0, INF, 1)), ("up_hint", "up"),
    ("max_tilt", 0.0), ("max_tilt", 90.5), ("max_tilt", NAN), ("max_tilt", None), ("max_tilt", False),
    ("below_frac", -0.1), ("below_frac", 1.5), ("below_frac", NAN), ("below_frac", "1%"), ("below_frac", True),
]
_XYZ_BAD = [X.double(), torch.zeros(4, 2), torch.zeros(12)]  # wrong dtype, wrong width, wrong rank
_XYZ_BAD_NEW = _XYZ_BAD + [NPX]                              # the functions that already name a non-tensor's type

CASES = []


def case(fn, args, kwargs, wrong):
    CASES.append((fn, tuple(args), dict(kwargs), wrong))


# ---- mesh.py ---------------------------------------------------------------------------------------------------------------
for bad in _XYZ_BAD:
    case("vertex_normals", (bad, FACES), {}, "xyz")
    case("segment_mesh", (bad, FACES), {}, "vertices")
    case("segment_point", (bad, X, EDGES), {}, "vertices")
    case("segment_point", (X, bad, EDGES), {}, "normals")
for bad in (FACES.float(), torch.zeros(2, 2, dtype=torch.int64), torch.zeros(6, dtype=torch.int64)):
    case("vertex_normals", (X, bad), {}, "faces")
    case("segment_mesh", (X, bad), {}, "faces")
for bad in (EDGES.float(), torch.zeros(2, 3, dtype=torch.int64), torch.zeros(4, dtype=torch.int32)):
    case("segment_point", (X, X, bad), {}, "edges")
case("segment_point", (X, X8, EDGES), {}, "normals")         # one normal per vertex
case("vertex_normals", (X, FACES), {}, "device")
case("segment_mesh", (X, FACES), {}, "device")
case("segment_point", (X, X, EDGES), {}, "device")
case("centre_and_scale", (np.zeros((4, 3)), np.zeros((5, 3))), {}, "colours")
case("decode_mesh", (MESH,), {"device": "cpu"}, "faces")
case("decode_mesh", (MESH[:2] + (np.array([[0, 1, 2]]),),), {"device": "cpu"}, "device")
case("decode_mesh", (PLY_POINTS,), {"device": "cpu"}, "src")
case("save_decoded", (TMP, "s", {"xyz": NPX}), {"sem_label": np.zeros(4)}, "ins_label")
case("save_decoded", (TMP, "s", {"xyz": NPX}), {"ins_label": np.zeros(4)}, "sem_label")

case("decode_points", (SCAN,), {"device": "cpu"}, "device")
case("decode_points", (SCAN8,), {"device": "cpu", "upright": True}, "device")
case("decode_points", (SCAN,), {"device": "cpu", "pitch": 0.05}, "device")
case("decode_points", (PLY_MESH,), {"device": "cpu"}, "src")
case("decode_points", (SCAN,), {"orient": "viewpoint"}, "orient")
case("decode_points", (SCAN,), {"return_kept": True}, "return_kept")
case("decode_points", (SCAN,), {"outlier_radius": 0.05}, "outlier_min_pts")
case("decode_points", (SCAN,), {"outlier_min_pts": 4}, "outlier_radius")
case("decode_points", (SCAN,), {"outlier_radius": 0.05, "outlier_min_pts": 4, "outlier_ratio": 2.0}, "outlier_ratio")
case("decode_points", (SCAN,), {"sem_label": np.zeros(4)}, "ins_label")
case("decode_points", (SCAN,), {"ins_label": np.zeros(4)}, "sem_label")
case("decode_points", (SCAN,), {"device": "cpu", "sem_label": np.array([0.0, 1.5, 2.0, 3.0]), "ins_label": np.zeros(4)}, "sem_label")
case("decode_points", (SCAN,), {"device": "cpu", "sem_label": np.zeros(4), "ins_label": np.array([0.0, NAN, 2.0, 3.0])}, "ins_label")
case("decode_points", (SCAN,), {"device": "cpu", "sem_label": np.zeros(5), "ins_label": np.zeros(5)}, "sem_label")
case("decode_points", (SCAN,), {"device": "cpu", "sem_label": np.zeros(4, bool), "ins_label": np.zeros(4)}, "sem_label")
case("decode_points", (SCAN,), {"device": "cpu", "sem_label": np.zeros(4), "ins_label": np.full(4, 2.0 ** 31)}, "ins_label")
for bad in ("floor", 1.0, ["up_hint"], {"rounds": 3}):
    case("decode_points", (SCAN8,), {"device": "cpu", "upright": bad}, "upright")
for name, value in _UPRIGHT_BAD:
    if (name, value) != ("threshold", "0.02"):              # a string threshold: its own case in test_upright_ref_cpu.py
        case("decode_points", (SCAN8,), {"device": "cpu", "upright": {name: value}}, "upright." + name)
        case("decode_points", (SCAN8,), {"device": "cpu", "pitch": 0.05, "upright": {name: value}}, "upright." + name)
case("decode_points", (SCAN8,), {"device": "cpu", "upright": {"threshold": "0.02"}}, "upright.threshold")

# ---- cloud.py --------------------------------------------------------------------------------------------------------------
for bad in _XYZ_BAD:
    case("knn_graph", (bad,), {"k": 2}, "xyz")
    case("point_normals", (bad, IDX), {}, "xyz")
    case("thin_points", (bad,), {}, "xyz")
    case("thin_points", (X, bad), {}, "colours")
for k in (0, 33, -1):
    case("knn_graph", (X,), {"k": k}, "k")
for cell in (0.0, -1.0, NAN):
    case("knn_graph", (X,), {"k": 2, "cell": cell}, "cell")
case("knn_graph", (X,), {"k": 2}, "device")
for bad in (IDX.long(), torch.zeros(5, 2, dtype=torch.int32), torch.zeros(8, dtype=torch.int32)):
    case("point_normals", (X, bad), {}, "idx")
case("point_normals", (X, IDX), {}, "device")
case("knn_edges", (torch.zeros(3, dtype=torch.int32),), {}, "idx")

NL = torch.zeros(4, 3)
for bad in (NL.numpy(), NL.double(), torch.zeros(4, 4), torch.zeros(12)):
    case("orient_normals", (bad, IDX), {}, "nl")
for bad in (IDX.numpy(), IDX.long(), torch.zeros(5, 2, dtype=torch.int32), torch.zeros(8, dtype=torch.int32)):
    case("orient_normals", (NL, bad), {}, "idx")
for k in (0, 33):
    case("orient_normals", (NL, torch.zeros(4, k, dtype=torch.int32)), {}, "k")
case("orient_normals", (NL, IDX), {}, "device")

for pitch in (0.0, -0.02, NAN, INF):
    case("thin_points", (X, None, pitch), {}, "pitch")
case("thin_points", (X, X8), {}, "colours")                  # one colour per point
case("thin_points", (X, None, 0.02), {}, "device")
for ratio in (-1.0, NAN, INF):
    case("outlier_mask", (D2, ratio), {}, "ratio")
for bad in (D2.double(), torch.zeros(12)):
    case("outlier_mask", (bad,), {}, "d2")
for k in (0, 33):
    case("outlier_mask", (torch.zeros(4, k),), {}, "k")
    case("raw_index", (INV, KEEP, torch.zeros(4, k, dtype=torch.int32)), {}, "k")
case("outlier_mask", (D2, 2.0), {}, "device")
for bad in (INV.long(), torch.zeros(3, 2, dtype=torch.int32)):
    case("raw_index", (bad, KEEP, IDX), {}, "inverse")
    case("radius_raw_index", (bad, KEEP, X, 1.0), {}, "inverse")
for bad in (KEEP.to(torch.uint8), torch.ones(2, 2, dtype=torch.bool)):
    case("raw_index", (INV, bad, IDX), {}, "keep")
    case("radius_raw_index", (INV, bad, X, 1.0), {}, "keep")
case("radius_raw_index", (INV, KEEP[:3], X, 1.0), {}, "keep")  # one flag per point
for bad in (IDX.long(), torch.zeros(5, 2, dtype=torch.int32), torch.zeros(8, dtype=torch.int32)):
    case("raw_index", (INV, KEEP, bad), {}, "idx")
case("raw_index", (INV, KEEP, IDX), {}, "device")

for radius in (0.0, -1.0, NAN, INF, 1e39):
    case("radius_count", (X, radius), {}, "radius")
    case("radius_outlier_mask", (X, radius, 4), {}, "radius")
    case("radius_raw_index", (INV, KEEP, X, radius), {}, "radius")
for cap in (0, -1, 1 << 31, 2.5, True):
    case("radius_count", (X, 1.0), {"cap": cap}, "cap")
    case("radius_outlier_mask", (X, 1.0, cap), {}, "min_pts")
case("radius_outlier_mask", (X, 1.0, None), {}, "min_pts")
for cell in (0.0, -1.0, NAN):
    case("radius_count", (X, 1.0), {"cell": cell}, "cell")
    case("radius_outlier_mask", (X, 1.0, 4), {"cell": cell}, "cell")
    case("radius_raw_index", (INV, KEEP, X, 1.0), {"cell": cell}, "cell")
for bad in _XYZ_BAD_NEW:
    case("radius_count", (bad, 1.0), {}, "xyz")
    case("radius_outlier_mask", (bad, 1.0, 4), {}, "xyz")
    case("radius_raw_index", (INV, KEEP, bad, 1.0), {}, "xyz")
case("radius_count", (X, 1.0), {}, "device")
case("radius_outlier_mask", (X, 1.0, 4), {}, "device")
case("radius_raw_index", (INV, KEEP, X, 1.0), {}, "device")

for fn in ("fit_plane", "upright"):
    for name, value in _UPRIGHT_BAD:
        case(fn, (X8,), _up(**{name: value}), name)
    for bad in (X8.double(), torch.zeros(8, 2), torch.zeros(24), np.zeros((8, 3), np.float32)):
        case(fn, (bad, 0.02), {}, "xyz")
    case(fn, (X8, 0.02), {}, "device")

case("carry_labels", (torch.zeros(3), i32(0, 1, 2)), {}, "labels")
case("carry_labels", (torch.zeros(3, dtype=torch.bool), i32(0, 1, 2)), {}, "labels")

case("vote_labels", (torch.zeros(3, dtype=torch.int64), i32(0, 0, 0)), {}, "rows")
case("vote_labels", (i32(0, 0, 0), torch.zeros(3)), {}, "sem")
case("vote_labels", (i32(0, 0, 0), i32(0, 0, 0), torch.zeros(3, 1, dtype=torch.int32)), {}, "ins")
case("vote_labels", (i32(0, 0, 0), i32(0, 0)), {}, "sem")
case("vote_labels", (i32(0, 0, 0), i32(0, 0, 0), i32(0, 0)), {}, "ins")
for nc in (0, 1024):
    case("vote_labels", (i32(0, 0), i32(0, 0)), {"n_classes": nc}, "n_classes")
case("vote_labels", (i32(0, 0), i32(0, 0)), {"m": -1}, "m")
case("vote_labels", (i32(0, 0), i32(0, 0)), {"m": 1}, "device")

# ---- ply.py ----------------------------------------------------------------------------------------------------------------
for fn in ("read_ply", "read_ply_points"):
    for path in (PLY_NOT, PLY_ASCII, PLY_NO_END, PLY_PROPERTY_FIRST, PLY_LINE):
        case(fn, (path,), {}, "path")
for path in (PLY_POINTS, PLY_DOUBLE, PLY_FACE_TYPE, PLY_SHORT, PLY_QUAD):
    case("read_ply", (path,), {}, "path")
for path in (PLY_MESH, PLY_DOUBLE, PLY_POINTS_SHORT):
    case("read_ply_points", (path,), {}, "path")
case("write_ply", (os.path.join(TMP, "w.ply"), NPX, NPX, np.zeros((1, 3))), {"index_type": "long"}, "index_type")
case("write_ply", (os.path.join(TMP, "w.ply"), np.zeros(4), NPX, np.zeros((1, 3))), {}, "xyz")


def case_id(i):
    fn, _, _, wrong = CASES[i]
    return "%03d %s %s" % (i, fn, wrong)


def outcome(call):
    """(exception class name, message) of call(), the temporary directory shown as <tmp>; ("", "") when nothing is raised."""
    try:
        call()
    except Exception as e:  # noqa: BLE001 -- the class is what is recorded
        return type(e).__name__, str(e).replace(TMP, "<tmp>")
    return "", ""


# ---- the status word ---------------------------------------------------------------------------------------------------
STATUS_BITS = (1, 2, 4, 8, 16)
# stage -> (args, kwargs of a valid call, the details its messages show)
STATUS_CALLS = {
    "knn_graph": ((X,), {"k": 2}, {}),
    "thin_points": ((X, None, 0.02), {}, {"pitch": 0.02}),
    "orient_normals": ((NL, IDX), {}, {}),
    "radius_count": ((X, 1.0), {}, {}),
    "radius_raw_index": ((INV, KEEP, X, 1.0), {}, {}),
    "fit_plane": ((X8, 0.02), {}, {}),
    "upright": ((X8, 0.02), {}, {}),
    "vote_labels": ((i32(0, 1, 2), i32(0, 0, 0)), {"m": 3, "n_classes": 20}, {"m": 3, "n_classes": 20}),
}
