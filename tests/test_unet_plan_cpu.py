"""CPU tier: the static plans of the MinkUNet body, as the two native executors receive them, against a fixture recorded
before the plans became consumers of one walk of the body (tests/golden/make_unet_plan_golden.py -> unet_plans.json).

MinkUNet._build_plan (csrc/executor.hip) and train_engine.TrainPlan (csrc/train_exec.hip) are rebuilt from the same seeds
and compared field for field, exactly: every non-pointer field of every op, the buffers, the output view, the layouts.  The
hashes of the packed weights, scales and shifts count only under the torch version that recorded them (the rule of
backbone_*.npz).  The inference plans build without the native library; the training plans need it, as
tests/test_train_plan_cpu.py does."""
import json
import os
import sys

import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
sys.path.insert(0, GOLDEN)
import make_unet_plan_golden as G  # noqa: E402

with open(os.path.join(GOLDEN, "unet_plans.json")) as _f:
    WANT = json.load(_f)


@pytest.fixture(scope="module")
def nets():
    cache = {}

    def get(arch, extreme=False):
        if (arch, extreme) not in cache:
            cache[(arch, extreme)] = G.build(arch, extreme)
        return cache[(arch, extreme)]
    return get


def _compare(got, want, what, skip=()):
    assert sorted(got) == sorted(want), what
    assert got["op_fields"] == want["op_fields"], what
    assert len(got["ops"]) == len(want["ops"]), "%s: %d ops, recorded %d" % (what, len(got["ops"]), len(want["ops"]))
    for i, (g, w) in enumerate(zip(got["ops"], want["ops"])):
        diff = {f: (a, b) for f, a, b in zip(want["op_fields"], g, w) if a != b}
        assert not diff, "%s: op %d differs, field: (rebuilt, recorded) = %r" % (what, i, diff)
    for key in want:
        if key not in ("ops", "op_fields") + tuple(skip):
            assert got[key] == want[key], "%s: %s" % (what, key)


def test_fixture_holds_the_cases():
    assert sorted(WANT["inference"]) == sorted(G.inference_cases()) and sorted(WANT["training"]) == sorted(G.training_cases())
    for arch in G.ARCHS:
        for dn in G.DTYPES:
            for fold in ("fold", "sep"):
                assert "%s-%s-%s" % (arch, dn, fold) in WANT["inference"]
    # anchor, counted by hand at the recording commit: MinkUNet14A is 26 ops over 23 buffers, 7 of them folded shortcuts
    for dn in G.DTYPES:
        p = WANT["inference"]["MinkUNet14A-%s-fold" % dn]
        assert (len(p["ops"]), len(p["bufs"]), len(p["folded_io"])) == (26, 23, 7)
    # the fp16 guard case holds both decisions
    p = WANT["inference"]["MinkUNet14A-f16-fold-extreme"]
    assert 0 < len(p["folded_io"]) < 7 and len(p["ops"]) == 26 + 7 - len(p["folded_io"])


@pytest.mark.parametrize("name", sorted(G.inference_cases()))
def test_inference_plan_is_the_recorded_one(name, nets):
    arch, extreme, dn, fold = G.inference_cases()[name]
    got = json.loads(json.dumps(G.inference_plan(nets(arch, extreme), G.DTYPES[dn], fold)))
    same_torch = WANT["torch_version"] == torch.__version__
    _compare(got, WANT["inference"][name], name, skip=() if same_torch else ("sha256",))
    if arch == "MinkUNet14A" and fold and not extreme:
        assert (len(got["ops"]), len(got["bufs"]), len(got["folded_io"])) == (26, 23, 7)


@pytest.mark.parametrize("name", sorted(G.training_cases()))
def test_training_plan_is_the_recorded_one(name, nets):
    arch, dn, dx = G.training_cases()[name]
    got = json.loads(json.dumps(G.training_plan(nets(arch), G.DTYPES[dn], dx)))
    _compare(got, WANT["training"][name], name)
