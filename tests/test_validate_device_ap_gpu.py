"""GPU tier: validate.ValidationEpoch with cfg.device_post + cfg.device_meters + cfg.device_ap (association log and loss meter on
the device, read back once by finish()) against cfg.device_post alone, over the two smallest scenes tests/test_validate_gpu.py
builds: the same matches, AP averages, loss averages (with ==), `no_cluster` count and logged lines."""
import copy

import numpy as np
import pytest
import torch

import test_validate_gpu as TV
from pbnet_amd import evaluate, validate as V
from pbnet_amd.config import get_config

pytestmark = pytest.mark.gpu


class Log(object):
    def __init__(self):
        self.lines = []

    def info(self, line):
        self.lines.append(line.split(",  time:")[0])            # the epoch line ends in its wall time


def run(model, cfg, batches, fn, gt=None, epoch=1, progress=False):
    log = Log()
    ve = V.ValidationEpoch(model, cfg, epoch, model_fn=fn, logger=log, gt=gt, progress=progress)
    for batch in batches:
        ve.step(batch)
    return ve, ve.finish(), log.lines


def with_flags(cfg, **flags):
    c = copy.copy(cfg)
    for k, v in flags.items():
        setattr(c, k, v)
    return c


@pytest.fixture(scope="module")
def setup():
    from pbnet_amd.network.PBNet import PBNet
    cfg = get_config(batch_size=1, cluster_epoch=0)
    assert cfg.device_ap is False
    torch.manual_seed(22)
    model = PBNet(cfg).to(TV.DEV)
    data = sorted((TV.make_scene(i) for i in range(TV.N_SCENES)), key=lambda bt: bt[0]["xyz_original"].shape[0])[:2]
    batches = [b for b, _ in data]
    return cfg, model, batches, TV.forced({b["fn"][0]: t for b, t in data})


def test_device_ap_needs_device_post(setup):
    cfg, model, _, fn = setup
    with pytest.raises(ValueError):
        V.ValidationEpoch(model, with_flags(cfg, device_ap=True), 1, model_fn=fn)


@pytest.mark.parametrize("gt_form", ["batch_labels", "callable"])
def test_device_ap_changes_nothing_the_epoch_reports(setup, capsys, gt_form):
    cfg, model, batches, fn = setup
    gt = None
    if gt_form == "callable":
        ids = {b["fn"][0]: evaluate.encode_gt_ids(b["sem"].numpy()[:b["xyz_original"].shape[0] // 3],
                                                  b["ins"].numpy()[:b["xyz_original"].shape[0] // 3]) for b in batches}
        gt = ids.__getitem__
    ve_a, a, lines_a = run(model, with_flags(cfg, device_post=True), batches, fn, gt)
    printed_a = capsys.readouterr().out
    ve_b, b, lines_b = run(model, with_flags(cfg, device_post=True, device_meters=True, device_ap=True), batches, fn, gt)
    printed_b = capsys.readouterr().out
    assert ve_a.device_post and not ve_a.device_ap and ve_b.device_ap and ve_b._ap_log is not None
    assert len(a["matches"]) == 2 and list(a["matches"]) == list(b["matches"])
    TV.same_matches(a["matches"], b["matches"])
    for key in ("mAP", "AP_50", "AP_25"):
        assert np.array_equal(a[key], b[key], equal_nan=True), key
    assert a["no_cluster"] == b["no_cluster"] == 0 and a["scenes"] == b["scenes"] == 2
    assert set(a["losses"]) == set(b["losses"]) and len(a["losses"]) == 5
    for key in a["losses"]:
        print(key, repr(a["losses"][key]), repr(b["losses"][key]))
        assert a["losses"][key] == b["losses"][key], key
    assert lines_a == lines_b and len(lines_a) > 2 and printed_a == printed_b


def test_a_scene_without_clusters_is_counted_at_the_end(setup, capsys):
    """Thresholds nothing passes: both forms count one `no cluster` scene, print the line once and leave losses and matches
    empty; the device form prints it from finish()."""
    cfg, model, batches, fn = setup
    cfg = with_flags(cfg, TEST_SCORE_THRESH=2.0)
    outs = []
    for flags in (dict(device_post=True), dict(device_post=True, device_meters=True, device_ap=True)):
        _, out, lines = run(model, with_flags(cfg, **flags), batches[:1], fn)
        outs.append((out["no_cluster"], out["losses"], out.get("matches"), lines, capsys.readouterr().out))
    assert outs[0][0] == outs[1][0] == 1 and outs[0][1] == outs[1][1] == {} and outs[0][2] == outs[1][2] == {}
    assert outs[0][3] == outs[1][3] and outs[0][4] == outs[1][4] and outs[0][4].count("no cluster") == 1


def test_a_dropped_scene_stays_out_of_the_loss_averages(setup, capsys):
    """One scene with clusters and one without (its scores scaled below the threshold): the averages are the first scene's."""
    cfg, model, batches, fn = setup
    flags = dict(device_post=True, device_meters=True, device_ap=True)
    _, alone, _ = run(model, with_flags(cfg, **flags), batches[:1], fn)

    def fn_second_empty(batch, model_, epoch, cfg_, task="train"):
        loss, pred, visual, meters = fn(batch, model_, epoch, cfg_, task)
        if batch is batches[1]:
            pred["clt_scores"] = pred["clt_scores"] * 0.0
        return loss, pred, visual, meters
    _, both, _ = run(model, with_flags(cfg, **flags), batches, fn_second_empty)
    assert both["no_cluster"] == 1 and both["scenes"] == 2 and list(both["matches"]) == [batches[0]["fn"][0]]
    assert both["losses"] == alone["losses"] and capsys.readouterr().out.count("no cluster") == 1


def test_progress_lines_are_the_host_form_s(setup, capsys):
    """progress=True over one scene with clusters and one without: both forms log the `iter:` line for the first scene only."""
    cfg, model, batches, fn = setup

    def fn_second_empty(batch, model_, epoch, cfg_, task="train"):
        loss, pred, visual, meters = fn(batch, model_, epoch, cfg_, task)
        if batch is batches[1]:
            pred["clt_scores"] = pred["clt_scores"] * 0.0
        return loss, pred, visual, meters
    lines = []
    for flags in (dict(device_post=True), dict(device_post=True, device_meters=True, device_ap=True)):
        _, out, logged = run(model, with_flags(cfg, **flags), batches, fn_second_empty, progress=True)
        assert out["no_cluster"] == 1
        lines.append(logged)
    assert lines[0] == lines[1] and sum(line.startswith("iter:") for line in lines[0]) == 1
    capsys.readouterr()
