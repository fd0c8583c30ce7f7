"""GPU tier: model_fn with cfg.device_meters against its default path (same terms, one read-back fewer) and
pbnet_amd.train_epoch.TrainEpoch end to end against a hand-written loop (model_fn's default path, the same optimizer class,
AverageMeter's arithmetic on host floats), on the small synthetic training batch of scripts/train_step.py."""
import io
import re
import types
from contextlib import redirect_stdout

import pytest
import torch

from pbnet_amd import synth
from pbnet_amd.config import get_config

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SMALL = dict(room=(1.6, 1.3, 1.2), n_boxes=4, pitch=0.03, classes=(17, 10))        # run_training(small=True)


@pytest.fixture(scope="module")
def setup():
    """One PBNet with seeded weights, teacher-forced heads, and the small batch; `reset()` puts the weights back."""
    from pbnet_amd.network.PBNet import PBNet
    cfg = get_config(batch_size=1, cluster_epoch=0)
    torch.manual_seed(22)
    model = PBNet(cfg).to(DEV).train()
    batch_np, teacher_np, _ = synth.make_train_batch(seed=10, copies=1, **SMALL)
    batch = {k: torch.from_numpy(v).to(DEV) for k, v in batch_np.items()}
    batch["feat_voxel"] = batch["feat_voxel"].to(torch.bfloat16)
    teacher = {k: torch.from_numpy(v).to(DEV) for k, v in teacher_np.items()}
    fwd = model.forward
    model.forward = lambda *a, **k: fwd(*a, teacher=teacher, **k)
    state = {k: v.detach().clone() for k, v in model.state_dict().items()}

    def reset():
        model.load_state_dict(state)
        model.train()
        for p in model.parameters():
            p.grad = None
        return model
    return types.SimpleNamespace(model=model, batch=batch, reset=reset, state=state)


def _d2h_copies(fn):
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        out = fn()
        torch.cuda.synchronize()
    return out, len([e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and "dtoh" in e.name.lower()])


@pytest.mark.parametrize("native_losses", [False, True])
@pytest.mark.parametrize("epoch", [0, 1])
def test_model_fn_device_meters(setup, native_losses, epoch):
    """Same tensors, only the read-back differs: the device terms and weights equal the default path's floats exactly, on
    both loss paths and on both sides of cluster_epoch (0 here), and the call has one device-to-host copy fewer."""
    from pbnet_amd.network.PBNet import model_fn
    model = setup.reset()
    base = get_config(batch_size=1, cluster_epoch=0, native_losses=native_losses)
    dev = get_config(batch_size=1, cluster_epoch=0, native_losses=native_losses, device_meters=True)
    with torch.no_grad():
        model_fn(setup.batch, model, epoch, base, "train")                       # warm-up: plans, workspaces
        (_, _, visual, meter), n_base = _d2h_copies(lambda: model_fn(setup.batch, model, epoch, base, "train"))
        (_, _, visual_d, meter_d), n_dev = _d2h_copies(lambda: model_fn(setup.batch, model, epoch, dev, "train"))
    names = ["loss", "semantic_loss", "offset_norm_loss", "offset_dir_loss"] + (["mask_loss"] if epoch > 0 else [])
    assert list(meter) == list(meter_d) == names and list(visual) == list(visual_d) == names
    for k in names:
        assert isinstance(visual[k], float) and isinstance(meter[k][0], float)
        for t in (visual_d[k], meter_d[k][0]):
            assert torch.is_tensor(t) and t.is_cuda and t.dim() == 0 and t.dtype == torch.float32
        assert torch.is_tensor(meter_d[k][1]) and meter_d[k][1].is_cuda
        assert visual_d[k].item() == visual[k] == meter[k][0] == meter_d[k][0].item(), k
        assert float(meter_d[k][1]) == float(meter[k][1]), k
    print("device-to-host copies: default %d, device_meters %d" % (n_base, n_dev))
    assert n_dev == n_base - 1


class _Recorder(object):
    def __init__(self):
        self.lines, self.scalars = [], []

    def info(self, line):
        self.lines.append(str(line))

    def add_scalar(self, tag, value, step):
        self.scalars.append((tag, float(value), int(step)))


def _cfg(tmp, **kw):
    return get_config(batch_size=1, cluster_epoch=0, lr=1e-3, step_epoch=50, epochs=520, logpath=str(tmp) + "/", save_freq=4, **kw)


def _hand_loop(setup, cfg, steps=3):
    """train.py:47-65 by hand: model_fn's default path (host floats), pbnet_amd.optim.Adam, AverageMeter in float64."""
    from pbnet_amd.network.PBNet import model_fn
    from pbnet_amd.optim import Adam
    from pbnet_amd.train_epoch import cosine_lr_after_step
    from pbnet_amd.validate import AverageMeter
    model = setup.reset()
    opt = Adam(model.parameters(), lr=cfg.lr)
    am = {}
    for _ in range(steps):
        cosine_lr_after_step(opt, cfg.lr, 1, cfg.step_epoch, cfg.epochs, clip=1e-6)
        loss, _, visual, meter = model_fn(setup.batch, model, 1, cfg, task="train")
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
        for k, v in meter.items():
            am.setdefault(k, AverageMeter()).update(float(v[0]), float(v[1]))
    torch.cuda.synchronize()
    return [p.detach().clone() for p in model.parameters()], {k: m.avg for k, m in am.items()}


def _epoch_loop(setup, cfg, log_every, rec, steps=3, save=True):
    from pbnet_amd.optim import Adam
    from pbnet_amd.train_epoch import TrainEpoch
    model = setup.reset()
    opt = Adam(model.parameters(), lr=123.0)                                   # the schedule sets the rate
    out = io.StringIO()
    with redirect_stdout(out):
        ep = TrainEpoch(model, cfg, 1, opt, steps, logger=rec, writer=rec, log_every=log_every, save=save)
        for _ in range(steps):
            ep.step(setup.batch)
        averages = ep.finish()
    torch.cuda.synchronize()
    return [p.detach().clone() for p in model.parameters()], averages, out.getvalue(), opt, ep


def test_train_epoch_end_to_end(setup, tmp_path):
    from pbnet_amd import checkpoint
    from pbnet_amd.network.PBNet import PBNet
    from pbnet_amd.train_epoch import LossMeter
    host_cfg = _cfg(tmp_path)
    p1, avg1 = _hand_loop(setup, host_cfg)
    p2, avg2 = _hand_loop(setup, host_cfg)
    # two hand loops repeat to the last bit (as tests/test_train_engine_gpu.py finds for its paths); were torch-side glue not
    # to repeat, the comparisons below would have to allow 4 x the spread of these two, and this assertion says so first
    assert all(torch.equal(a, b) for a, b in zip(p1, p2)) and avg1 == avg2
    assert any(not torch.equal(a, b) for a, b in zip(p1, setup.state.values())), "three steps moved nothing"

    rec = _Recorder()
    cfg = _cfg(tmp_path, device_meters=True)
    p3, avg3, printed, opt, ep = _epoch_loop(setup, cfg, 0, rec)
    assert isinstance(ep.meter, LossMeter) and not ep.meter.host and ep.meter.updates == 3
    for k, (a, b) in enumerate(zip(p3, p1)):
        assert torch.equal(a, b), "parameter %d differs from the hand loop" % k
    assert list(avg3) == list(avg1)
    for k in avg1:
        print("%s: epoch %.17g hand %.17g" % (k, avg3[k], avg1[k]))
        assert abs(avg3[k] - avg1[k]) <= 1e-12 * abs(avg1[k]), k
    # log_every = 0: no progress line; the epoch line and the checkpoint line in the recorded format (train_lines.json)
    assert printed == ""
    assert len(rec.lines) == 2
    assert re.fullmatch(r"epoch: 1/520, train loss: -?\d+\.\d{4}, mask_loss: -?\d+\.\d{4},  time: \d+\.\d+(e-?\d+)?s", rec.lines[0])
    assert rec.lines[0].startswith("epoch: 1/520, train loss: {:.4f}, mask_loss: {:.4f},  time: ".format(avg3["loss"], avg3["mask_loss"]))
    path = cfg.logpath + "%09d.pth" % 1
    assert rec.lines[1] == "Saving " + path
    tags = [s[0] for s in rec.scalars]
    assert tags == [k + "_train" for k in avg1] + ["train/learning_rate"] and rec.scalars[-1][1] == 1e-3
    assert opt.param_groups[0]["lr"] == 1e-3
    # the checkpoint loads into a fresh model and a fresh torch.optim.Adam
    fresh = PBNet(cfg).to(DEV)
    topt = torch.optim.Adam(fresh.parameters(), lr=1.0)
    start, loaded = checkpoint.checkpoint_restore(fresh, topt, cfg.logpath)
    assert (start, loaded) == (2, path)
    for a, b in zip(fresh.parameters(), p3):
        assert torch.equal(a, b)
    mine_state = opt.state_dict()["state"]
    assert len(topt.state) == len(mine_state) > 0
    for i, p in enumerate(topt.param_groups[0]["params"]):
        if i in mine_state:
            assert float(topt.state[p]["step"]) == 3.0
            assert torch.equal(topt.state[p]["exp_avg"], mine_state[i]["exp_avg"])
            assert torch.equal(topt.state[p]["exp_avg_sq"], mine_state[i]["exp_avg_sq"])

    # log_every = 1: three progress lines, the same parameters
    rec1 = _Recorder()
    p4, avg4, printed1, _, _ = _epoch_loop(setup, cfg, 1, rec1, save=False)
    assert all(torch.equal(a, b) for a, b in zip(p4, p1)) and avg4 == avg3
    lines = printed1.splitlines()
    assert len(lines) == 4 and lines[3] == ""
    for i, line in enumerate(lines[:3]):
        assert re.fullmatch(r"epoch: 1/520 iter: %d/3 loss: -?\d+\.\d{4}\(-?\d+\.\d{4}\)  mask_loss: -?\d+\.\d{4}\(-?\d+\.\d{4}\)   "
                            r" data_time: \d+\.\d\d\(\d+\.\d\d\) iter_time: \d+\.\d\d\(\d+\.\d\d\) remain_time: \d\d+:\d\d:\d\d"
                            % (i + 1), line), line
    assert len(rec1.lines) == 1                                               # save=False: no checkpoint line

    # host floats are accepted too (model_fn's default path): the same parameters, the averages of the hand loop exactly
    p5, avg5, _, _, ep5 = _epoch_loop(setup, host_cfg, 0, _Recorder(), save=False)
    assert ep5.meter.host and all(torch.equal(a, b) for a, b in zip(p5, p1)) and avg5 == avg1


def test_train_epoch_without_steps(setup, tmp_path):
    from pbnet_amd.optim import Adam
    from pbnet_amd.train_epoch import TrainEpoch
    model = setup.reset()
    rec = _Recorder()
    ep = TrainEpoch(model, _cfg(tmp_path, device_meters=True), 1, Adam(model.parameters()), 0, logger=rec, log_every=0, save=False)
    assert ep.finish() == {"loss": 0.0, "mask_loss": 0.0}                      # n_iters = 0: no division by zero
    assert len(rec.lines) == 1 and rec.lines[0].startswith("epoch: 1/520, train loss: 0.0000, mask_loss: 0.0000,  time: ")
