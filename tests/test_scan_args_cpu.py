"""The scan decode's argument checks and status words, pinned to what they were before pbnet_amd/mesh.py was split into
mesh.py, cloud.py and ply.py: every call of tests/scan_arg_cases.py raises the class and the message recorded in
tests/golden/scan_arg_messages.json (tests/golden/make_scan_arg_messages.py), on CPU tensors, before a device or the
library is asked for anything; and every name tests and scripts reach through `mesh.` is the object of its new home."""
import json
import os

import pytest

import scan_arg_cases as S
from pbnet_amd import _native as N, cloud, mesh, ply

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "scan_arg_messages.json")) as fh:
    GOLDEN = json.load(fh)


def test_the_recording_covers_the_list():
    assert [c["id"] for c in GOLDEN["cases"]] == [S.case_id(i) for i in range(len(S.CASES))]
    assert [(s["stage"], s["status"]) for s in GOLDEN["status"]] == [(stage, bit) for stage in S.STATUS_CALLS
                                                                     for bit in S.STATUS_BITS]


@pytest.fixture
def no_library(monkeypatch):
    """A value check that fired only after the library had been asked would pass where the library is built and fail
    where it is not: here asking is an error of its own."""
    def lib():
        raise AssertionError("the library was asked before the arguments were checked")
    monkeypatch.setattr(N, "lib", lib)


@pytest.mark.parametrize("i", range(len(S.CASES)), ids=S.case_id)
def test_single_fault_raises_what_it_raised(i, no_library):
    fn, args, kwargs, _ = S.CASES[i]
    want = GOLDEN["cases"][i]
    assert S.outcome(lambda: getattr(mesh, fn)(*args, **kwargs)) == (want["exception"], want["message"])


@pytest.mark.parametrize("want", GOLDEN["status"], ids=lambda s: "%s-%d" % (s["stage"], s["status"]))
def test_status_word_raises_what_the_stage_raised(want):
    details = S.STATUS_CALLS[want["stage"]][2]
    got = S.outcome(lambda: cloud._scan_status(want["stage"], want["status"], **details))
    assert got == (want["exception"], want["message"])


def test_status_zero_is_silent():
    for stage, (_, _, details) in S.STATUS_CALLS.items():
        cloud._scan_status(stage, 0, **details)


# every name tests/ and scripts/ reach through `mesh.` (the matches of mesh\.[A-Za-z_]+ that are not file names), and its home
MESH_NAMES = {
    mesh: ["SCENE_BOOKKEEPING", "centre_and_scale", "decode_mesh", "decode_points", "save_decoded", "segment_mesh",
           "segment_point", "vertex_normals"],
    ply: ["read_ply", "read_ply_points", "write_ply"],
    cloud: ["CLOUD_STAGES", "ORIENT_STAGES", "RADIUS_STAGES", "THIN_STAGES", "UPRIGHT_MAX_HYP", "UPRIGHT_STAGES",
            "VOTE_STAGES", "_upright", "carry_labels", "fit_plane", "knn_edges", "knn_graph", "orient_normals",
            "outlier_mask", "point_normals", "radius_count", "radius_outlier_mask", "radius_raw_index", "raw_index",
            "thin_points", "upright", "vote_labels"],
}


def test_every_name_reached_through_mesh_is_its_home_object():
    for home, names in MESH_NAMES.items():
        for name in names:
            assert getattr(mesh, name) is getattr(home, name), name
            if callable(getattr(home, name)):
                assert getattr(home, name).__module__ == home.__name__, name


def test_ply_needs_neither_torch_nor_the_library():
    src = open(ply.__file__).read()
    assert "_native" not in src and "import torch" not in src
