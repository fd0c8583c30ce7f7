"""GPU tier: every coordinate entry point on the designed inputs of tests/pyramid_cases.py against the plain numpy specification
tests/pyramid_ref.py.  The sorted pipeline (csrc/pyramid.hip behind pbn_coords_prepare / pbn_coords_prepare_dev) must give EVERY
array of the contract element for element -- the contract fixes the row order of every level --; the hash-table pipeline
(pbn_coords_prepare_hash) and the training path (pbn_coords_build, rows in external order) the same lineage in their own row
order, compared in the order-free form.  A box of more than 44 key bits must be refused by the sorted entry point and then be
served by the hash pipeline in the same arena, as MinkowskiEngine/core.py does.  All integers: no tolerance."""
import ctypes

import numpy as np
import pytest
import torch

import pyramid_cases as PC
import pyramid_ref as PR
from pbnet_amd import _native as N
from pyramid_ref import DEV, _arrays, _is_z_ordered, _prepare, _view, canonical

pytestmark = pytest.mark.gpu
PLANS_RUN = set()


def _assert_equal(got, want, what):
    assert set(got) == set(want), (what, sorted(set(got) ^ set(want)))
    for k in sorted(want):
        assert got[k].shape == want[k].shape, (what, k, got[k].shape, want[k].shape)
        assert np.array_equal(got[k], want[k]), (what, k)


def _device_input(c):
    coords = torch.from_numpy(c["coords"]).to(DEV).reshape(-1, 4)
    nd = None if c["n_valid"] is None else torch.tensor([c["n_valid"]], dtype=torch.int32, device=DEV)
    return coords, nd


def _check_sorted_then_hash(c, ref, coords, nd, into=None, n_cap=None, then_hash=True):
    """The sequence of the product path: the sorted entry point; where it refuses the box, the hash pipeline on the same arena."""
    n = len(c["coords"]) if n_cap is None else n_cap
    want = PR.contract(ref)
    arena, P = _prepare(coords, "sorted", nd, c["want_k5"], c["x_fastest"], into=into)
    a = _arrays(arena, P, n, c["n_valid"])
    if ref["plan"] is None and ref["n_unique"][0] > 0:
        assert a["counts"][0] == -1, "a box of %d key bits must be refused" % ref["nbits"]
    else:
        assert a["counts"][0] >= 0, "the sorted pipeline reports an error (counts %s)" % a["counts"]
        assert np.array_equal(a["inv_perm"][a["perm"]], np.arange(len(a["perm"]))) and _is_z_ordered(a)
        _assert_equal(a, want, "sorted pipeline")
    if not then_hash:
        return arena, P
    arena, P = _prepare(coords, "hash", nd, c["want_k5"], c["x_fastest"], into=(arena, P))
    h = _arrays(arena, P, n, c["n_valid"])
    assert _is_z_ordered(h)
    _assert_equal(canonical(h), canonical(want), "hash pipeline")
    return arena, P


@pytest.mark.parametrize("name", PC.NAMES)
def test_prepare_equals_reference(name):
    c, ref = PC.case(name), PC.reference(name)
    _check_sorted_then_hash(c, ref, *_device_input(c))
    if c["family"] == "D":
        PLANS_RUN.add(ref["plan"])


def test_family_d_ran_every_digit_plan():
    """After the cases above (file order): what family D put through the sort is all nine plans, and the refused box."""
    assert PLANS_RUN == {(1, 8), (2, 8), (3, 8), (3, 9), (3, 10), (3, 11), (4, 9), (4, 10), (4, 11), None}


@pytest.mark.parametrize("name", PC.NAMES)
def test_build_equals_reference(name):
    """pbn_coords_build (training path): de-duplication and maps in the external row order."""
    c, ref = PC.case(name), PC.reference(name)
    coords, nd = _device_input(c)
    lib = N.lib()
    n = len(c["coords"])
    L = N.CoordsLayout()
    nbytes = lib.pbn_coords_arena_bytes(n, c["want_k5"], ctypes.byref(L))
    arena = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    N.check(lib.pbn_coords_build(N.ptr(coords), None if nd is None else N.ptr(nd), n, c["want_k5"], c["x_fastest"], N.ptr(arena),
                                 nbytes, ctypes.byref(L), N.current_stream()), "pbn_coords_build")
    torch.cuda.synchronize()
    counts = _view(arena, L.counts, 5, torch.int32)
    assert np.array_equal(counts, ref["counts"])
    n1, n_in = int(counts[0]), n if c["n_valid"] is None else c["n_valid"]
    a = {"counts": counts, "n_unique": counts[:1], "unique_index": _view(arena, L.unique_index, n, torch.int32)[:n1],
         "inverse": _view(arena, L.inverse, n, torch.int32)[:n_in], "perm": np.arange(n1), "inv_perm": np.arange(n1)}
    for l in range(5):
        a["coords%d" % l] = _view(arena, L.coords[l], n * 4, torch.int32).reshape(n, 4)[:counts[l]]
        a["k3_%d" % l] = _view(arena, L.k3[l], n * 27, torch.int32).reshape(n, 27)[:counts[l]]
    if c["want_k5"]:
        a["k5"] = _view(arena, L.k5, n * 125, torch.int32).reshape(n, 125)[:n1]
    for l in range(4):
        a["parent_row%d" % l] = _view(arena, L.parent_row[l], n, torch.int32)[:counts[l]]
        a["child_k%d" % l] = _view(arena, L.child_k[l], n, torch.int32)[:counts[l]]
        a["nbr_down%d" % l] = _view(arena, L.nbr_down[l], n * 8, torch.int32).reshape(n, 8)[:counts[l + 1]]
        a["up%d" % l] = _view(arena, L.up[l], n * 8, torch.int32).reshape(n, 8)[:counts[l]]
    a["ucoords"] = a["coords0"]
    assert np.array_equal(a["coords0"], ref["ucoords"])                      # level 0 IS the external order
    _assert_equal(canonical(a), canonical(PR.contract(ref)), "pbn_coords_build")


def test_second_call_on_a_used_arena():
    """One arena and layout (capacity form, sized for the largest input), never cleared by the caller: a large case, then smaller
    ones with another box and another digit plan, then a box the sorted pipeline refuses followed by the hash pipeline, then a
    sortable case again (sorted call straight after sorted call, and after the hash pipeline has used the same scratch).  Every call
    must reset its own tickets, scan states, histograms and "no child" entries."""
    names = ("D_4x11", "N_minimum_unaligned", "D_1x8", "D_45_bits", "B_seams", "C_valid_0", "S_n1025")
    cap = max(len(PC.case(n)["coords"]) for n in names)
    plans = [PC.reference(n)["plan"] for n in names]
    assert len(set(plans)) >= 4 and plans[0] == (4, 11) and plans[3] is None
    into = None
    for name in names:
        c, ref = PC.case(name), PC.reference(name)
        n_valid = len(c["coords"]) if c["n_valid"] is None else c["n_valid"]
        padded = np.full((cap, 4), 77777, np.int32)                          # beyond the count: out of range, never read
        padded[:len(c["coords"])] = c["coords"]
        nd = torch.tensor([n_valid], dtype=torch.int32, device=DEV)
        into = _check_sorted_then_hash(dict(c, n_valid=n_valid), ref, torch.from_numpy(padded).to(DEV), nd, into=into, n_cap=cap,
                                       then_hash=name in ("D_45_bits", "B_seams"))
