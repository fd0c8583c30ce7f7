"""GPU tier: the device AP table behind its two callers, on the small synthetic validation batches of
tests/test_validate_device_ap_gpu.py and tests/test_serving_association_gpu.py: `ValidationEpoch` with cfg.device_ap_table against
cfg.device_ap alone, and `evaluate_served(device_table=True)` against its default form.  The same dropped scenes; every AP cell
within one float32 ulp (the bound of tests/test_ap_table_gpu.py); mAP, AP_50 and AP_25 within 1e-6 -- the mean of cells that each
moved by at most one float32 ulp (6e-8 for values up to 1) cannot move further than that."""
import types

import numpy as np
import pytest

import test_serving_association_gpu as TS
import test_validate_device_ap_gpu as TD
from test_ap_table_gpu import ulps
from test_serving_association_gpu import world                          # noqa: F401  (the module's fixture)
from test_validate_device_ap_gpu import setup                          # noqa: F401  (the module's fixture)
from pbnet_amd import evaluate as E
from pbnet_amd import validate as V
from pbnet_amd.serving import SceneServer

pytestmark = pytest.mark.gpu
FLAGS = dict(device_post=True, device_meters=True, device_ap=True)


def same_cells(got, want):
    assert got.shape == want.shape and np.array_equal(np.isnan(got), np.isnan(want))
    live = ~np.isnan(want)
    assert int(ulps(got[live], want[live]).max(initial=0)) <= 1


def same_averages(a, b):
    for key in ("all_ap", "all_ap_50%", "all_ap_25%"):
        assert np.isnan(a[key]) == np.isnan(b[key]) and (np.isnan(a[key]) or abs(float(a[key]) - float(b[key])) <= 1e-6), key


def test_the_table_needs_device_ap(setup):                            # noqa: F811
    cfg, model, _, fn = setup
    with pytest.raises(ValueError):
        V.ValidationEpoch(model, TD.with_flags(cfg, device_post=True, device_ap_table=True), 1, model_fn=fn)


def test_validation_epoch_reports_the_same_from_the_table(setup, capsys):     # noqa: F811
    cfg, model, batches, fn = setup

    def fn_second_empty(batch, model_, epoch, cfg_, task="train"):      # the second scene keeps no instance: one dropped scene
        loss, pred, visual, meters = fn(batch, model_, epoch, cfg_, task)
        if batch is batches[1]:
            pred["clt_scores"] = pred["clt_scores"] * 0.0
        return loss, pred, visual, meters

    for model_fn, dropped in ((fn, 0), (fn_second_empty, 1)):
        ve_a, a, lines_a = TD.run(model, TD.with_flags(cfg, **FLAGS), batches, model_fn)
        printed_a = capsys.readouterr().out
        ve_b, b, lines_b = TD.run(model, TD.with_flags(cfg, device_ap_table=True, **FLAGS), batches, model_fn)
        printed_b = capsys.readouterr().out
        assert ve_b.device_ap_table and not ve_a.device_ap_table and b["matches"] is None and "ap" not in a
        assert a["no_cluster"] == b["no_cluster"] == dropped and printed_a == printed_b and printed_a.count("no cluster") == dropped
        same_cells(b["ap"], E.evaluate_matches(a["matches"]))
        same_averages(a["avgs"], b["avgs"])
        for key in ("mAP", "AP_50", "AP_25"):
            assert np.isnan(a[key]) == np.isnan(b[key]) and (np.isnan(a[key]) or abs(a[key] - b[key]) <= 1e-6), key
        assert a["losses"] == b["losses"] and len(lines_a) == len(lines_b)


def test_served_logs_give_the_same_table(world):                       # noqa: F811
    """The teacher-forced units served by two workers: `ap_table()` against `association()` + `evaluate_matches` on the very
    same logs."""
    model, units, thr = world
    server, _ = TS._serve(model, units, thr, workers=2, max_batch=2)
    matches, dropped, failed = server.association()
    ap, table_dropped, table_failed, cells = server.ap_table()
    assert table_dropped == dropped and table_failed == failed and len(matches) + len(dropped) + len(failed) == len(units)
    assert len(matches) > 0 and int(cells.sum()) > 0                  # entries, or at least missed instances
    same_cells(ap, E.evaluate_matches(matches))
    same_averages(E.compute_averages(ap), E.compute_averages(E.evaluate_matches(matches)))


def test_evaluate_served_from_the_table(world):                        # noqa: F811
    """`evaluate_served(device_table=True)` against its default form: the same lines and the same averages."""
    model, units, thr = world
    outs = []
    for device_table in (False, True):
        lines = []
        server = SceneServer(model, max_batch=2, forwards_in_flight=1, refine=thr, tta=3, paused=True, association=True)
        avgs = E.evaluate_served(server, [("unit%d" % i, u, g) for i, (u, _, g) in enumerate(units)], thr,
                                 logger=types.SimpleNamespace(info=lines.append), device_table=device_table)
        outs.append((avgs, [line for line in lines if "left out" in line or "not served" in line]))
    same_averages(outs[0][0], outs[1][0])
    assert outs[0][1] == outs[1][1] and set(outs[1][0]) == {"all_ap", "all_ap_50%", "all_ap_25%", "classes"}
