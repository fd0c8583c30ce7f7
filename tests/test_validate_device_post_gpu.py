"""GPU tier: validate.ValidationEpoch with cfg.device_post (postprocess.refine_instances_device, n_keep read back together with
the loss-meter weights) against the default path, over the two smallest scenes tests/test_validate_gpu.py builds: the same matches,
AP averages, `no_cluster` count and logged lines."""
import copy

import numpy as np
import pytest
import torch

import test_validate_gpu as TV
from pbnet_amd import validate as V
from pbnet_amd.config import get_config

pytestmark = pytest.mark.gpu


class Log(object):
    def __init__(self):
        self.lines = []

    def info(self, line):
        self.lines.append(line.split(",  time:")[0])            # the epoch line ends in its wall time


def run(model, cfg, batches, fn, epoch=1):
    log = Log()
    ve = V.ValidationEpoch(model, cfg, epoch, model_fn=fn, logger=log)
    for batch in batches:
        ve.step(batch)
    return ve, ve.finish(), log.lines


def test_device_post_changes_nothing_the_epoch_reports(capsys):
    from pbnet_amd.network.PBNet import PBNet
    cfg = get_config(batch_size=1, cluster_epoch=0)
    assert cfg.device_post is False
    torch.manual_seed(22)
    model = PBNet(cfg).to(TV.DEV)
    data = sorted((TV.make_scene(i) for i in range(TV.N_SCENES)), key=lambda bt: bt[0]["xyz_original"].shape[0])[:2]
    batches = [b for b, _ in data]
    fn = TV.forced({b["fn"][0]: t for b, t in data})
    dev_cfg = copy.copy(cfg)
    dev_cfg.device_post = True
    ve_a, a, lines_a = run(model, cfg, batches, fn)
    printed_a = capsys.readouterr().out
    ve_b, b, lines_b = run(model, dev_cfg, batches, fn)
    printed_b = capsys.readouterr().out
    assert not ve_a.device_post and ve_b.device_post and ve_b._post_ws is not None
    assert len(a["matches"]) == 2
    TV.same_matches(a["matches"], b["matches"])
    for key in ("mAP", "AP_50", "AP_25"):
        assert np.array_equal(a[key], b[key], equal_nan=True), key
    assert a["no_cluster"] == b["no_cluster"] and a["losses"] == b["losses"] and a["scenes"] == b["scenes"] == 2
    assert lines_a == lines_b and len(lines_a) > 2 and printed_a == printed_b


def test_a_scene_without_clusters_takes_the_same_branch(capsys):
    """Thresholds nothing passes: both paths print `no cluster`, count the scene and leave it out of the loss averages."""
    from pbnet_amd.network.PBNet import PBNet
    cfg = get_config(batch_size=1, cluster_epoch=0, TEST_SCORE_THRESH=2.0)
    torch.manual_seed(22)
    model = PBNet(cfg).to(TV.DEV)
    batch, teacher = TV.make_scene(0)
    fn = TV.forced({batch["fn"][0]: teacher})
    outs = []
    for flag in (False, True):
        c = copy.copy(cfg)
        c.device_post = flag
        _, out, lines = run(model, c, [batch], fn)
        outs.append((out["no_cluster"], out["losses"], out.get("matches"), lines, capsys.readouterr().out))
    assert outs[0][0] == outs[1][0] == 1 and outs[0][1] == outs[1][1] == {} and outs[0][2] == outs[1][2] == {}
    assert outs[0][3] == outs[1][3] and outs[0][4] == outs[1][4] and "no cluster" in outs[0][4]
