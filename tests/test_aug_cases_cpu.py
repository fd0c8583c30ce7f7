"""CPU tier: the designed cases of tests/aug_cases.py reach the paths they are named for, the per-entry restatement
tests/aug_ref.py composed in the loader's order reproduces merge_ref.train_merge / val_merge on the golden batches, its
pieces agree with merge_ref's crop loop and instance statistics, and every deliberately wrong variant of
tests/aug_mutants.py is rejected by at least one case."""
import glob
import os

import numpy as np
import pytest

import aug_cases as C
import aug_mutants as M
import aug_ref as R
import merge_ref

GOLDEN = sorted(glob.glob(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "merge_*.npz")))
CASES = C.all_cases()


@pytest.mark.parametrize("name", sorted(CASES))
def test_case_reaches_its_path(name):
    assert CASES[name]()["reaches"]() is True


@pytest.mark.parametrize("path", GOLDEN, ids=[os.path.basename(p)[6:-4] for p in GOLDEN])
def test_entries_compose_to_the_merge(path):
    kind, scenes, names, ids, draws, cfg, _ = merge_ref.load_golden(path)
    if kind == "train":
        want = merge_ref.train_merge(scenes, names, ids, draws, cfg)
        units = []
        for i, idx in enumerate(ids):
            s = draws.scenes[i]
            units.append((names[idx], s.primary, i, True))
            units.append((names[int(np.floor(s.mix_u * len(names)))], s.partner, i, False))
        got = R.merge(scenes, units, 2, cfg, [s.crop for s in draws.scenes])
        assert np.array_equal(got["crop_used"], want["crop_used"])
    else:
        want = merge_ref.val_merge(scenes, names, ids, draws, cfg)
        ids3 = ids + ids + ids
        got = R.merge(scenes, [(names[idx], draws.copies[i], i, False) for i, idx in enumerate(ids3)], 1, cfg)
    merge_ref.assert_batch(got, want, os.path.basename(path))


@pytest.mark.parametrize("name", ["crop", "crop_boundary"])
def test_crop_agrees_with_the_crop_loop(name):
    """State words, mask and offset rows of every cropping scene against merge_ref.crop_loop (the reference's loop)."""
    from types import SimpleNamespace
    c = CASES[name]()
    r = C.crop_ref(c)
    cfg = SimpleNamespace(scale_size=50, max_crop_p=c["max_crop_p"], min_crop_p=c["min_crop_p"])
    for s in np.nonzero(c["mode"] == 0)[0]:
        x = c["xyz"][c["soff"][s]:c["soff"][s + 1]]
        xo, valid, used, ok = merge_ref.crop_loop(x, SimpleNamespace(crop=c["triples"][s]), cfg)
        st = r["state"][s]
        assert (used, ok) == (st[R.ST_USED], bool(st[R.ST_SUCCESS]))
        keep_all, o, level, offset = R.crop_view(s, c["mode"], c["triples"], c["levels"], r["state"], r["ext_pre"])
        assert not keep_all and offset == ok
        assert np.array_equal(R.crop_valid(x, o, level), valid)
        assert np.array_equal(x + o if offset else x, xo)
        assert np.array_equal(r["ext_post"][s], R.extent(xo))
        visited = r["counts"][:, s] >= 0
        assert visited.sum() == used and valid.sum() == r["counts"][st[R.ST_TRIES] - 1, s, st[R.ST_LAST_K]]


def test_instances_agree_with_instance_info():
    c = C.instances_case()
    r = C.instances_ref(c)
    for s in (0, 2):
        a, b = c["ostart"][s], c["ostart"][s + 1]
        num, info, pn = merge_ref.instance_info(c["xyz"][a:b], c["label"][a:b])
        assert num == c["inst_num"][s] and pn == r["pointnum"][r["inst_start"][s]:r["inst_start"][s + 1]].tolist()
        assert np.array_equal(info[:, 3:], r["inst_info"][a:b, 3:])
        assert (np.abs(info[:, :3].astype(np.float64) - r["inst_info"][a:b, :3]) <= np.spacing(np.abs(info[:, :3]))).all()


def test_matmul_versus_elementwise_product():
    """Recorded, not asserted: how many affine outputs a BLAS product would change in the last bit."""
    c = C.affine_case()
    differ = total = 0
    for u in range(len(c["uoff"]) - 1):
        x = c["xyz"][c["uoff"][u]:c["uoff"][u + 1]]
        x = R.pre_subtract(x) if c["pre_min"][u] else x.astype(np.float64)
        m = c["mats"][u].reshape(3, 3)
        el = np.stack([x[:, 0] * m[0, j] + x[:, 1] * m[1, j] + x[:, 2] * m[2, j] for j in range(3)], 1)
        differ += int((el != np.matmul(x, m)).sum())
        total += el.size
    print("affine: %d of %d elementwise products differ from np.matmul" % (differ, total))


def _evaluate(name):
    c = CASES[name]()
    if name == "affine":
        out = R.affine(c["xyz"], c["uoff"], c["pre_min"], c["mats"], c["scale"], c["has_scale"])
    elif name == "elastic":
        steps, last = C.elastic_ref(c)
        out = [last] + [a for st in steps for a in st]
    elif name.startswith("crop"):
        r = C.crop_ref(c)
        out = [r[k] for k in ("counts", "state", "ext_pre", "ext_post")]
    elif name.startswith("compact"):
        r = C.compact_ref(c)
        out = [r[k] for k in ("xyz", "feat", "sem", "label", "scene_info", "scan")]
    elif name.startswith("instances"):
        r = C.instances_ref(c)
        out = [r[k] for k in ("pointnum", "stats", "inst_info", "ins")]
    else:
        out = R.quantize(c["xyz"], c["ostart"], c["voxel"])
    return [np.asarray(a) for a in out]


def _same(a, b):
    return all(x.shape == y.shape and np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))


@pytest.fixture(scope="module")
def clean():
    return {name: _evaluate(name) for name in sorted(CASES) if name != "compact_second_tile"}


@pytest.mark.parametrize("name", sorted(M.MUTANTS))
def test_mutant_is_rejected(name, clean):
    killers = []
    for case in clean:
        try:
            with M.mutant(name):
                got = _evaluate(case)
        except IndexError:
            assert name == "interp_unclipped"        # reads past the grid on the last axis value: that is the rejection
            killers.append(case)
            continue
        if not _same(got, clean[case]):
            killers.append(case)
    print("%s rejected by %s" % (name, killers))
    assert killers, name
    assert _same(_evaluate(killers[0]), clean[killers[0]])       # the swap is undone: the restatement is clean again
