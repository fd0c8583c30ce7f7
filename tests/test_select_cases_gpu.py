"""GPU tier: k_select_points (csrc/front.hip) through pbn_select_points on the designed inputs of tests/select_cases.py against
tests/select_ref.py.  sem_pred is int64 as the ABI states, the block histogram is the reference's (so a wrong position is the
selection's own), the offsets sit in a [n, ld_off] buffer of their type whose padding columns are poisoned, and every output lies
inside an allocation filled with the byte 0x5a on both sides: all four outputs must equal the reference bit for bit and every word
nobody is sent to -- rows >= total, the margins -- must still be the pattern.  Every case runs twice with the same bytes.  On three
cases the histogram comes from pbn_sem_argmax_table instead, and the call goes through stage_ops.select_points.  No tolerance."""
import ctypes

import numpy as np
import pytest
import torch

import select_cases as SC
import select_ref as SR
from pbnet_amd import _native as N
from pbnet_amd import stage_ops

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
PAT = 0x5A
TORCH = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
ROWS_BEHIND = 64                       # output rows allocated behind the reference's last one, besides the margins


class Guarded(object):
    """n elements of `dtype` (at least one) between two margins, everything filled with the byte pattern."""

    def __init__(self, n_elems, dtype, margin=256):
        self.n, self.m, self.es = int(n_elems), margin, torch.empty(0, dtype=dtype).element_size()
        self.buf = torch.full(((max(self.n, 1) + 2 * margin) * self.es,), PAT, dtype=torch.uint8, device=DEV).view(dtype)

    @property
    def ptr(self):
        return ctypes.c_void_p(self.buf.data_ptr() + self.m * self.es)

    def bits(self):
        """The whole allocation, margins included, as unsigned words."""
        a = self.buf.cpu().view(torch.uint8).numpy()
        return a.view({4: np.uint32, 8: np.uint64}[self.es])

    def untouched(self):
        return bool((self.buf.view(torch.uint8) == PAT).all())


def _expected(g, width, written, values):
    """The allocation of Guarded g as the reference leaves it: `values` in the written rows of the body, the pattern elsewhere."""
    word = {4: np.uint32, 8: np.uint64}[g.es]
    want = np.frombuffer(bytes([PAT]) * (len(g.bits()) * g.es), word).copy()
    body = want[g.m:g.m + len(written) * width].reshape(len(written), width)
    body[written] = np.ascontiguousarray(values).view(word).reshape(len(written), width)[written]
    return want


def _inputs(c):
    n = len(c["sem_pred"])
    return dict(n=n, sem=torch.from_numpy(np.array(c["sem_pred"])).to(DEV), base=torch.from_numpy(np.array(c["class_base"])).to(DEV),
                xyz=torch.from_numpy(np.array(c["xyz"])).to(DEV),
                off=torch.from_numpy(SC.offset_buffer(c)).to(DEV).to(TORCH[c["dtype"]]).contiguous())


def _select(c, inp, histogram, **over):
    ref = SC.reference(c)
    rows = len(ref["written"]) + ROWS_BEHIND
    out = dict(ins_ind=Guarded(rows, torch.int64), ins_orig=Guarded(3 * rows, torch.float32), ins_off=Guarded(3 * rows, torch.float32),
               ins_sem=Guarded(rows, torch.int32))
    a = dict(sem=N.ptr(inp["sem"]), n=inp["n"], n_cls=c["n_cls"], base=N.ptr(inp["base"]), hist=N.ptr(histogram), xyz=N.ptr(inp["xyz"]),
             off=ctypes.c_void_p(inp["off"].data_ptr()), ld=c["ld_off"], dtype=N.DT[TORCH[c["dtype"]]])
    a.update({k: o.ptr for k, o in out.items()})
    a.update(over)
    rc = N.lib().pbn_select_points(a["sem"], a["n"], a["n_cls"], a["base"], a["hist"], a["xyz"], a["off"], a["ld"], a["dtype"],
                                   a["ins_ind"], a["ins_orig"], a["ins_off"], a["ins_sem"], N.current_stream())
    torch.cuda.synchronize()
    return rc, out


def _check(c, out):
    ref = SC.reference(c)
    w = ref["written"]
    for key, width in (("ins_ind", 1), ("ins_orig", 3), ("ins_off", 3), ("ins_sem", 1)):
        got, want = out[key].bits(), _expected(out[key], width, w, ref[key])
        if not np.array_equal(got, want):
            bad = np.nonzero(got != want)[0]
            raise AssertionError("%s: %d words differ, first at word %d of the allocation (body starts at %d, %d rows written): got %#x, "
                                 "want %#x" % (key, len(bad), bad[0], out[key].m, len(w), got[bad[0]], want[bad[0]]))


@pytest.mark.parametrize("name", SC.NAMES)
def test_case_equals_reference(name):
    c = SC.case(name)
    assert N.lib().pbn_select_blocks(len(c["sem_pred"])) == -(-len(c["sem_pred"]) // SC.BLOCK)
    inp = _inputs(c)
    assert inp["sem"].dtype == torch.int64 and inp["off"].shape == (inp["n"], c["ld_off"])
    assert np.array_equal(inp["off"][:, :3].float().cpu().numpy().view(np.uint32), c["offset"].view(np.uint32))     # exact in the type
    hist = torch.from_numpy(SR.block_hist(c["sem_pred"], c["n_cls"], SC.BLOCK)).to(DEV)
    rc, out = _select(c, inp, hist)
    assert rc == N.PBN_OK
    _check(c, out)
    rc, again = _select(c, inp, hist)
    assert rc == N.PBN_OK and all(torch.equal(out[k].buf.view(torch.uint8), again[k].buf.view(torch.uint8)) for k in out), "second run"


@pytest.mark.parametrize("name", SC.CHAINED)
def test_chained_behind_the_argmax_kernel(name):
    """One-hot scores whose arg-max is the case's label: pbn_sem_argmax_table's sem_pred and block histogram feed the selection, once
    through the C ABI inside guarded buffers and once through stage_ops.select_points."""
    c = SC.case(name)
    lab = c["sem_pred"]
    assert (lab >= 0).all()
    ref = SC.reference(c)
    inp = _inputs(c)
    score = torch.zeros(len(lab), c["n_cls"], dtype=torch.float32, device=DEV)
    score[torch.arange(len(lab), device=DEV), inp["sem"]] = 1.0
    sem_pred, _, table, block_hist = stage_ops.sem_argmax_table(score, None, 1)
    assert torch.equal(sem_pred, inp["sem"]) and sem_pred.dtype == torch.int64
    assert np.array_equal(block_hist.cpu().numpy(), SR.block_hist(lab, c["n_cls"], SC.BLOCK))
    assert np.array_equal(table.cpu().numpy().reshape(-1), np.bincount(lab, minlength=c["n_cls"]))
    rc, out = _select(c, dict(inp, sem=sem_pred), block_hist)
    assert rc == N.PBN_OK
    _check(c, out)
    m = ref["total"]
    assert ref["written"].all() and m == len(ref["written"])
    ins_ind, ins_orig, ins_off, ins_sem = stage_ops.select_points(sem_pred, inp["base"], block_hist, inp["xyz"], inp["off"][:, :3], m)
    assert ins_ind.dtype == torch.int64 and ins_sem.dtype == torch.int32
    assert np.array_equal(ins_ind.cpu().numpy(), ref["ins_ind"]) and np.array_equal(ins_sem.cpu().numpy(), ref["ins_sem"])
    assert np.array_equal(ins_orig.cpu().numpy().view(np.uint32), ref["ins_orig"].view(np.uint32))
    assert np.array_equal(ins_off.cpu().numpy().view(np.uint32), ref["ins_off"].view(np.uint32))


def test_refusals_write_nothing():
    c = SC.case("N_n65")
    inp = _inputs(c)
    hist = torch.from_numpy(SR.block_hist(c["sem_pred"], c["n_cls"], SC.BLOCK)).to(DEV)
    for over in (dict(n=-1), dict(n_cls=0), dict(n_cls=33), dict(ld=2), dict(dtype=7), dict(sem=None), dict(base=None), dict(hist=None),
                 dict(xyz=None), dict(off=None), dict(ins_ind=None), dict(ins_orig=None), dict(ins_off=None), dict(ins_sem=None)):
        rc, out = _select(c, inp, hist, **over)
        assert rc == N.PBN_ERR_ARG and all(o.untouched() for o in out.values()), over
    rc, out = _select(c, inp, hist, n=0)                                    # no points: accepted, nothing to write
    assert rc == N.PBN_OK and all(o.untouched() for o in out.values())
