"""GPU tier: csrc/mesh.hip through pbnet_amd.mesh on the designed inputs of tests/mesh_cases.py against tests/mesh_ref.py, with
int32 and with int64 indices.  vertex_normals must equal decode_normals bit for bit; segment_mesh / segment_point must give the
reference's sup under ascending tie order, element by element; a second run must give the same bytes; decode_mesh and the timed
entry must agree with the plain one.  Once through the C ABI: nl and sup sit inside sentinel-filled allocations, and a workspace
one byte short is refused before anything is written.  No tolerance anywhere.

The four large cases (mesh_cases.LARGE) run vertex_normals once per index type, or the segmentation once with int32."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import mesh_cases as MC
import mesh_ref as MR
from pbnet_amd import _native as N
from pbnet_amd import mesh
from pbnet_amd import selftest as S

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
INDEX = {"i32": np.int32, "i64": np.int64}


def _d(a, dtype=None):
    return torch.from_numpy(np.array(a, dtype=dtype, order="C", copy=True)).to(DEV)         # the cases' arrays are read-only


def _bits(t):
    return t.detach().cpu().numpy().view(np.uint32)


def test_constants_are_the_kernels():
    assert MC.sort_tile() == N.lib().pbn_selftest_sort_tile() > 0
    assert MC.SCAN_TILE == S.SCAN_TILE and (MC.MESH_GRID, MC.TPB) == (4096, 256)
    t = MC.sort_tile()
    assert [len(MC.case("O_sort_" + k)["edges"]) for k in ("Tm1", "T", "Tp1", "2T")] == [t - 1, t, t + 1, 2 * t]


def _segment(c, idx):
    if c["mode"] == "mesh":
        return mesh.segment_mesh(_d(c["xyz"]), _d(c["faces"], idx), c["k_thresh"], c["seg_min_verts"])
    return mesh.segment_point(_d(c["xyz"]), _d(c["normals"]), _d(c["edges"], idx), c["k_thresh"], c["seg_min_verts"])


@functools.lru_cache(maxsize=None)
def _centred_reference(name):
    """nl and sup of the reference for the case's vertices as decode_mesh centres them."""
    c = MC.case(name)
    xyz_c, _ = mesh.centre_and_scale(c["xyz"], np.zeros((len(c["xyz"]), 3), np.uint8))
    xyz_c = np.ascontiguousarray(xyz_c, np.float32)
    return MR.decode_normals(xyz_c, c["faces"]), MR.segment_mesh(xyz_c, c["faces"], c["k_thresh"], c["seg_min_verts"], ties="asc")


@pytest.mark.parametrize("idx", list(INDEX))
@pytest.mark.parametrize("name", MC.SMALL)
def test_case_equals_reference(name, idx):
    c, ref, idx = MC.case(name), MC.reference(name), INDEX[idx]
    if c["mode"] == "mesh":
        xyz, faces = _d(c["xyz"]), _d(c["faces"], idx)
        nl = mesh.vertex_normals(xyz, faces)
        assert np.array_equal(_bits(nl), ref["nl"].view(np.uint32)), "nl"
        assert torch.equal(mesh.vertex_normals(xyz, faces).view(torch.int32), nl.view(torch.int32)), "second run of vertex_normals"
    sup = _segment(c, idx)
    assert sup.dtype == torch.int64 and np.array_equal(sup.cpu().numpy(), ref["sup"]), "sup"
    assert torch.equal(_segment(c, idx), sup), "second run of the segmentation"
    if c["mode"] == "mesh":
        nl_t = torch.empty_like(nl)
        times = {}
        sup_t = mesh._segment_mesh(xyz, faces, c["k_thresh"], c["seg_min_verts"], nl=nl_t, times=times)
        assert torch.equal(sup_t, sup) and np.array_equal(_bits(nl_t), ref["nl"].view(np.uint32)) and set(times) == set(mesh.STAGES)
        # decode_mesh centres the vertices itself: its nl and sup are the reference's for the centred vertices
        col = np.zeros((len(c["xyz"]), 3), np.uint8)
        xyz_c, _ = mesh.centre_and_scale(c["xyz"], col)
        dec = mesh.decode_mesh((c["xyz"], col, c["faces"].astype(idx)), device=DEV, kThresh=c["k_thresh"], segMinVerts=c["seg_min_verts"])
        assert np.array_equal(_bits(dec["xyz"]), np.ascontiguousarray(xyz_c, np.float32).view(np.uint32))
        want_nl, want_sup = _centred_reference(name)
        assert np.array_equal(_bits(dec["nl"]), want_nl.view(np.uint32)) and np.array_equal(dec["sup"].cpu().numpy(), want_sup)
        xd, fd = dec["xyz"], dec["face"]
        assert torch.equal(dec["nl"].view(torch.int32), mesh.vertex_normals(xd, fd).view(torch.int32)), "decode_mesh nl"
        assert torch.equal(dec["sup"], mesh.segment_mesh(xd, fd, c["k_thresh"], c["seg_min_verts"])), "decode_mesh sup"


@pytest.mark.parametrize("idx", list(INDEX))
@pytest.mark.parametrize("name", [n for n in MC.LARGE if MC.ONLY[n] == "normals"])
def test_large_normals(name, idx):
    c, ref = MC.case(name), MC.reference(name)
    xyz, faces = _d(c["xyz"]), _d(c["faces"], INDEX[idx])
    nl = mesh.vertex_normals(xyz, faces)
    assert np.array_equal(_bits(nl), ref["nl"].view(np.uint32))
    assert torch.equal(mesh.vertex_normals(xyz, faces).view(torch.int32), nl.view(torch.int32))


@pytest.mark.parametrize("name", [n for n in MC.LARGE if MC.ONLY[n] == "segment"])
def test_large_segment_point(name):
    c, ref = MC.case(name), MC.reference(name)
    sup = _segment(c, np.int32)
    assert np.array_equal(sup.cpu().numpy(), ref["sup"])
    assert torch.equal(_segment(c, np.int32), sup)


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------------
PAD = 4096                      # sentinel elements either side of an output


def _guarded(n, dtype, fill):
    buf = torch.full((n + 2 * PAD,), fill, dtype=dtype, device=DEV)
    return buf, buf[PAD:PAD + n]


def _untouched(buf, n, fill):
    return bool((buf[:PAD] == fill).all()) and bool((buf[PAD + n:] == fill).all())


def test_outputs_stay_inside_their_arrays():
    """nl [V, 3] and sup [V] in the middle of sentinel-filled allocations, V no multiple of anything: nothing outside may change."""
    lib = N.lib()
    c, ref = MC.case("L_strip_v257"), MC.reference("L_strip_v257")
    v, f = len(c["xyz"]), len(c["faces"])
    xyz, faces = _d(c["xyz"]), _d(c["faces"], np.int32)
    for mode in (mesh.MESH_NORMALS, mesh.MESH_SEGMENT):
        nl_buf, nl = _guarded(3 * v, torch.float32, -7.5)
        sup_buf, sup = _guarded(v, torch.int64, -77)
        ws = torch.empty(lib.pbn_mesh_workspace_bytes(mode, v, f), dtype=torch.uint8, device=DEV)
        if mode == mesh.MESH_NORMALS:
            status = torch.zeros(1, dtype=torch.int32, device=DEV)
            rc = lib.pbn_mesh_vertex_normals(N.ptr(xyz), v, N.ptr(faces), 0, f, N.ptr(nl), N.ptr(status), N.ptr(ws), ws.numel(),
                                             N.current_stream())
        else:
            rc = lib.pbn_mesh_segment(N.ptr(xyz), v, N.ptr(faces), 0, f, c["k_thresh"], c["seg_min_verts"], N.ptr(sup), N.ptr(nl),
                                      N.ptr(ws), ws.numel(), None, N.current_stream())
        torch.cuda.synchronize()
        assert rc == N.PBN_OK
        assert np.array_equal(_bits(nl).reshape(v, 3), ref["nl"].view(np.uint32)) and _untouched(nl_buf, 3 * v, -7.5)
        if mode == mesh.MESH_SEGMENT:
            assert np.array_equal(sup.cpu().numpy(), ref["sup"])
        else:
            assert bool((sup == -77).all()) and int(status.item()) == 0
        assert _untouched(sup_buf, v, -77)
    c, ref = MC.case("L_point_ve257"), MC.reference("L_point_ve257")
    v, e = len(c["xyz"]), len(c["edges"])
    sup_buf, sup = _guarded(v, torch.int64, -77)
    ws = torch.empty(lib.pbn_mesh_workspace_bytes(mesh.MESH_SEGMENT_POINT, v, e), dtype=torch.uint8, device=DEV)
    xyz, nrm, edges = _d(c["xyz"]), _d(c["normals"]), _d(c["edges"], np.int64)
    rc = lib.pbn_mesh_segment_point(N.ptr(xyz), N.ptr(nrm), v, N.ptr(edges), 1, e, c["k_thresh"], c["seg_min_verts"], N.ptr(sup),
                                    N.ptr(ws), ws.numel(), N.current_stream())
    torch.cuda.synchronize()
    assert rc == N.PBN_OK and np.array_equal(sup.cpu().numpy(), ref["sup"]) and _untouched(sup_buf, v, -77)


def test_short_workspace_is_refused_and_nothing_is_written():
    lib = N.lib()
    c = MC.case("L_strip_v257")
    v, f = len(c["xyz"]), len(c["faces"])
    xyz, faces = _d(c["xyz"]), _d(c["faces"], np.int32)
    p = MC.case("L_point_ve257")
    pv, pe = len(p["xyz"]), len(p["edges"])
    pxyz, pnrm, pedges = _d(p["xyz"]), _d(p["normals"]), _d(p["edges"], np.int32)
    for mode, n_v, n_e in ((mesh.MESH_NORMALS, v, f), (mesh.MESH_SEGMENT, v, f), (mesh.MESH_SEGMENT_POINT, pv, pe)):
        need = lib.pbn_mesh_workspace_bytes(mode, n_v, n_e)
        assert need > 0
        ws = torch.full((need,), 0x5a, dtype=torch.uint8, device=DEV)
        nl = torch.full((n_v, 3), -7.5, dtype=torch.float32, device=DEV)
        sup = torch.full((n_v,), -77, dtype=torch.int64, device=DEV)
        status = torch.full((1,), -3, dtype=torch.int32, device=DEV)
        if mode == mesh.MESH_NORMALS:
            rc = lib.pbn_mesh_vertex_normals(N.ptr(xyz), v, N.ptr(faces), 0, f, N.ptr(nl), N.ptr(status), N.ptr(ws), need - 1,
                                             N.current_stream())
        elif mode == mesh.MESH_SEGMENT:
            t = (ctypes.c_float * len(mesh.STAGES))(*([-1.0] * len(mesh.STAGES)))
            rc = lib.pbn_mesh_segment(N.ptr(xyz), v, N.ptr(faces), 0, f, c["k_thresh"], c["seg_min_verts"], N.ptr(sup), N.ptr(nl),
                                      N.ptr(ws), need - 1, t, N.current_stream())
            assert list(t) == [-1.0] * len(mesh.STAGES)
        else:
            rc = lib.pbn_mesh_segment_point(N.ptr(pxyz), N.ptr(pnrm), pv, N.ptr(pedges), 0, pe, p["k_thresh"], p["seg_min_verts"],
                                            N.ptr(sup), N.ptr(ws), need - 1, N.current_stream())
        torch.cuda.synchronize()
        assert rc == N.PBN_ERR_WORKSPACE
        assert bool((ws == 0x5a).all()) and bool((nl == -7.5).all()) and bool((sup == -77).all()) and int(status.item()) == -3
