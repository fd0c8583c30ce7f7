"""Deliberately WRONG variants of tests/aug_ref.py, used to show that tests/aug_cases.py is sharp: at least one case must
reject each (tests/test_aug_cases_cpu.py).  aug_ref.py stays clean: it states every step a mutant needs as a small named
function, and `mutant(name)` swaps exactly one of them for the duration of a `with` block."""
import contextlib
import itertools

import numpy as np

import aug_ref as R


def _crop_le_upper(x, o, level):
    xo = x + o
    return (xo.min(1) >= 0) * ((xo <= level).sum(1) == 3)


def _crop_gt_lower(x, o, level):
    xo = x + o
    return (xo.min(1) > 0) * ((xo < level).sum(1) == 3)


def _ext_post_after_mask(xo, valid):
    return R.extent(xo[valid])


def _pre_min_f64(x32):
    return x32.astype(np.float64) - x32.min(0).astype(np.float64)


def _relabel_once(ins):
    j, moved = 0, False
    while j < ins.max() and not moved:
        if len(np.where(ins == j)[0]) == 0:
            ins[ins == ins.max()] = j
            moved = True
        j += 1
    return ins


def _shift_none_too(ins, shift_of_row):
    return np.asarray(ins, np.int32) + np.asarray(shift_of_row, np.int32)


def _interp_unclipped(ax, values, x):
    """merge_ref.interp without the upper clip of the cell index.  On the last axis value the cell is b-1 and its upper
    corner lies outside the grid: a kernel would read past the row with weight 0, numpy raises IndexError -- the only
    way this mistake shows, since a finite stray value times 0 changes nothing."""
    idx, nd = [], []
    oob = np.zeros(x.shape[0], bool)
    for d, a in enumerate(ax):
        xd = x[:, d]
        i = np.maximum(np.searchsorted(a, xd, side="right") - 1, 0)
        i = np.where(xd > a[-1], a.size - 2, i)                  # rows beyond the grid get the fill value anyway
        idx.append(i)
        nd.append((xd - a[i]) / (a[1] - a[0]))                   # uniform axes: a[i + 1] - a[i] without reading a[b]
        oob |= (xd < a[0]) | (xd > a[-1])
    value = np.zeros(x.shape[0])
    for h in itertools.product(*[((i, 1 - y), (i + 1, y)) for i, y in zip(idx, nd)]):
        e, w = zip(*h)
        weight = np.ones(x.shape[0])
        for wd in w:
            weight = weight * wd
        value = value + values[e].astype(np.float64) * weight
    value[oob] = 0.0
    return value


def _voxel_trunc(x, voxel):
    return np.trunc(x / np.float64(voxel)).astype(np.int32)


MUTANTS = {
    "crop_upper_le": ("crop_valid", _crop_le_upper),             # 1. x + o <= level
    "crop_lower_gt": ("crop_valid", _crop_gt_lower),             # 2. x + o > 0
    "ext_post_after_mask": ("offset_extent", _ext_post_after_mask),   # 3. minimum of the kept rows only
    "pre_min_f64": ("pre_subtract", _pre_min_f64),               # 4. float32 minimum subtracted after widening
    "relabel_once": ("relabel", _relabel_once),                  # 5. the maximum moves once
    "shift_none_too": ("shift_labels", _shift_none_too),         # 6. -100 shifted with the partner's labels
    "interp_unclipped": ("interp", _interp_unclipped),           # 7. cell index not clipped at the last node
    "voxel_trunc": ("voxel_index", _voxel_trunc),                # 8. truncation instead of floor
}


@contextlib.contextmanager
def mutant(name):
    attr, fn = MUTANTS[name]
    clean = getattr(R, attr)
    setattr(R, attr, fn)
    try:
        yield
    finally:
        setattr(R, attr, clean)
