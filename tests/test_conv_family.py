"""CPU tier: the automatic kernel-family choice of the convolutions (csrc/spconv.hip: one ordered table -- row-stationary, then
wave-autonomous, the workgroup-tile family behind it -- walked by the launch and reported by pbn_spconv_family) against the
answers recorded before that table existed (tests/golden/make_conv_family_golden.py -> conv_family.json).  Host code only:
the library loads and answers without a GPU.  Default environment: every PBN_* switch of the choice unset."""
import json
import os
import sys

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
sys.path.insert(0, GOLDEN)
import make_conv_family_golden as G  # noqa: E402

SWITCHES = ("PBN_CONV_FAMILY", "PBN_CONV_RS", "PBN_CONV_PC", "PBN_RS_MIN_ROWS", "PBN_RS_MIN_ROWS2", "PBN_RS_WIDE",
            "PBN_WAVE_MAX_ROWS", "PBN_WAVE_MAX_GMACS", "PBN_PC_MIN_ROWS")

with open(os.path.join(GOLDEN, "conv_family.json")) as _f:
    WANT = json.load(_f)


def test_fixture_holds_the_table():
    assert WANT["cases"] == G.cases()
    assert len(WANT["family"]) == len(WANT["cases"]) >= 2 * 2 * 4 * 10
    # every family is in the record, and the row-stationary one only where there is a map and 16-bit rows
    assert set(WANT["family"]) == {0, 1, 2}
    for (dn, has_map, k, vpo, cout_p, n), fam in zip(WANT["cases"], WANT["family"]):
        assert fam != 2 or (has_map == 1 and dn == "bf16" and n >= 20000)


def test_family_choice_is_the_recorded_one():
    if any(os.environ.get(k) for k in SWITCHES):
        pytest.fail("the record holds for the default environment; unset " + ", ".join(k for k in SWITCHES if os.environ.get(k)))
    from pbnet_amd import _native
    lib = _native.lib()
    got = [G.ask(lib, c) for c in WANT["cases"]]
    bad = [(c, g, w) for c, g, w in zip(WANT["cases"], got, WANT["family"]) if g != w]
    assert not bad, "%d of %d shapes changed family; first (case, now, recorded): %r" % (len(bad), len(got), bad[:5])
