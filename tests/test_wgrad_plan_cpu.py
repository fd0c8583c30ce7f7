"""CPU tier: the launch plan of the weight gradient (csrc/wgrad_plan.h: one host function that pbn_spconv_wgrad follows and
pbn_spconv_wgrad_plan reports) against the answers recorded before that function existed
(tests/golden/make_wgrad_plan_golden.py -> wgrad_plans.json), and the independent Python statement of the same dispatch
(tests/wgrad_plan_ref.py) against the same record.  Host code only: the library loads and answers without a GPU.  Default
environment and PBN_WGRAD_FORM=32 (static per process: a child); every other PBN_WGRAD_* knob unset."""
import json
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, "golden")
sys.path.insert(0, GOLDEN)
import make_wgrad_plan_golden as G  # noqa: E402

KNOBS = ("PBN_WGRAD_FORM",) + G.KNOBS

with open(os.path.join(GOLDEN, "wgrad_plans.json")) as _f:
    WANT = json.load(_f)


def _default_environment():
    if any(os.environ.get(k) for k in KNOBS):
        pytest.fail("the record holds for the default environment; unset " + ", ".join(k for k in KNOBS if os.environ.get(k)))


def library_plans(cases):
    """[(answer, grid)] of pbn_spconv_wgrad_plan under this process's environment; every case must be accepted."""
    from pbnet_amd import _native
    lib = _native.lib()
    out = []
    for c in cases:
        rc, plan, grid = G.ask(lib, _native.WgradPlan, c)
        assert rc == 0, (c, rc)
        out.append((plan, grid))
    return out


def _compare(got, want, cases, who):
    bad = [(c, g, w) for c, g, w in zip(cases, got, want) if g != w]
    assert not bad, "%s: %d of %d plans changed; first (case, now, recorded): %r" % (who, len(bad), len(got), bad[:5])


def _check_library(got, want, cases, who):
    _compare([p for p, _ in got], want, cases, who)
    # the grid of a ring launch: strips x offsets x splits, the splits padded to the 8 XCDs from 8 on (wgrad_tile)
    for c, (p, grid) in zip(cases, got):
        if p[0].startswith("ring"):
            strips, splits, k = p[4], p[5], c[5]
            assert grid == strips * k * (splits if splits < 8 else (splits + 7) // 8 * 8), (c, p, grid)


def test_fixture_holds_the_table():
    assert WANT["fields"] == G.FIELDS and WANT["answer"] == G.ANSWER
    assert WANT["cases"] == G.cases()
    assert 2000 <= len(WANT["cases"]) <= 8000
    for key in ("default", "form32"):
        assert len(WANT["plans"][key]) == len(WANT["cases"])
    # every kernel is in the record: k_wgrad<T> and the 32 k_wgrad_ring<WA, WB, IDENT>; quarter tiles, splits up to the cap
    forms = set(p[0] for p in WANT["plans"]["default"])
    assert forms == {"w32"} | {"ring%d%d%s" % (a, b, i) for a in (1, 2, 3, 4) for b in (1, 2, 3, 4) for i in ("", "i")}
    assert set(p[0] for p in WANT["plans"]["form32"]) == {"w32"}
    assert any(p[3] for p in WANT["plans"]["default"]) and max(p[5] for p in WANT["plans"]["default"]) == 64
    for c, p in zip(WANT["cases"], WANT["plans"]["default"]):
        assert p[0] != "w32" or c[0] == "f32" or not (c[1] and c[2]), (c, p)


def test_python_statement_gives_the_recorded_plans():
    _default_environment()
    _compare(G.reference_plans(WANT["cases"], None), WANT["plans"]["default"], WANT["cases"], "wgrad_plan_ref")
    _compare(G.reference_plans(WANT["cases"], "32"), WANT["plans"]["form32"], WANT["cases"], "wgrad_plan_ref, PBN_WGRAD_FORM=32")


def test_library_gives_the_recorded_plans():
    _default_environment()
    _check_library(library_plans(WANT["cases"]), WANT["plans"]["default"], WANT["cases"], "pbn_spconv_wgrad_plan")


_CHILD = """
import json, sys
sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
import test_wgrad_plan_cpu as T
print("PLANS", json.dumps(T.library_plans(T.WANT["cases"])))
"""


def test_library_gives_the_recorded_plans_under_form_32():
    """PBN_WGRAD_FORM is read once per process: a child asks the library with it set."""
    _default_environment()
    env = dict(os.environ, PBN_WGRAD_FORM="32")
    p = subprocess.run([sys.executable, "-c", _CHILD.format(root=ROOT, tests=HERE)], env=env, timeout=300, capture_output=True,
                       text=True)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
    line = [l for l in p.stdout.splitlines() if l.startswith("PLANS ")][-1]
    got = [(plan, grid) for plan, grid in json.loads(line[len("PLANS "):])]
    _check_library(got, WANT["plans"]["form32"], WANT["cases"], "pbn_spconv_wgrad_plan, PBN_WGRAD_FORM=32")


def test_plan_refuses_what_the_launch_refuses():
    import ctypes
    from pbnet_amd import _native as N
    lib = N.lib()
    p = N.WgradPlan()

    def call(dtype=1, n_offsets=27, n_pairs=1000, cin=32, cout=32, identity=0, out=p):
        return lib.pbn_spconv_wgrad_plan(dtype, 32, 32, 1, identity, n_offsets, n_pairs, cin, cout, 1, 1 << 20,
                                         ctypes.byref(out) if out is not None else None)
    assert call() == N.PBN_OK and p.form == 1
    assert call(n_pairs=0) == N.PBN_OK
    for kw in (dict(dtype=3), dict(dtype=-1), dict(n_offsets=0), dict(cin=0), dict(cout=0), dict(n_pairs=-1),
               dict(identity=1), dict(out=None)):
        assert call(**kw) == N.PBN_ERR_ARG, kw
    assert call(identity=1, n_offsets=1) == N.PBN_OK
