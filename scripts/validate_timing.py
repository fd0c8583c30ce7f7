"""Per-scene cost of the validation meters on the bench scene (seed 2, 3 x 161 517 points) with the `pred` tensors of a real
task='eval' forward: SemanticMeter.update + MaskAccuracyMeter.update against the reference's formulation
(tests/metrics_ref.py: reference_form_torch = train.py:146-147 + tools/mIOU.py:18-31, reference_mask_form_torch =
train.py:153-165).  Host clock around work that ends in a synchronise, warmed up, the two forms alternated, at least
`seconds` of timed work each.  Recorded in DESIGN.md section 10, not gated.

    python scripts/validate_timing.py [out.json] [seconds=2.0]
    rocprofv3 --kernel-trace --stats -d DIR -- python scripts/validate_timing.py --kernels-only      (the kernels' own time)"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

import metrics_ref as R  # noqa: E402
from pbnet_amd import synth, validate as V  # noqa: E402
from pbnet_amd.config import get_config  # noqa: E402
from pbnet_amd.network.PBNet import PBNet, model_fn  # noqa: E402

kernels_only = "--kernels-only" in sys.argv
args = [a for a in sys.argv[1:] if not a.startswith("--")]
out_path = args[0] if args else None
seconds = float(args[1]) if len(args) > 1 else 2.0
dev = torch.device("cuda:0")
cfg = get_config(batch_size=1, cluster_epoch=0)
torch.manual_seed(22)
model = PBNet(cfg).to(dev).eval()
batch_np, teacher_np, info = synth.make_train_batch(seed=2, copies=3)
batch = {k: torch.from_numpy(v) for k, v in batch_np.items()}
teacher = {k: torch.from_numpy(v).to(dev) for k, v in teacher_np.items()}
forward = model.forward
model.forward = lambda *a, **kw: forward(*a, teacher=teacher, **kw)
with torch.no_grad():
    _, pred, _, _ = model_fn(batch, model, 1, cfg, task="eval")
pred_sem, sem_label = pred["sem"], batch["sem"].to(dev)
pred_mask, gt_mask = pred["mask_scores"]
K = cfg.sem_num
print("points %d, mask rows %d (%s)" % (pred_sem.numel(), gt_mask.numel(), pred_mask.dtype))

sem, mask = V.SemanticMeter(K), V.MaskAccuracyMeter(capacity=1 << 16)


def new_form():
    sem.update(pred_sem, sem_label)
    mask.update(pred_mask, gt_mask)
    torch.cuda.synchronize()


def reference_form(scores):
    R.reference_form_torch(pred_sem, sem_label, K)
    R.reference_mask_form_torch(scores, gt_mask)
    torch.cuda.synchronize()


if kernels_only:
    for _ in range(50):
        mask._n = 0
        new_form()
    sys.exit(0)

# the two formulations count the same things on these tensors
want = np.stack(R.sem_counts(pred_sem.cpu().numpy(), sem_label.cpu().numpy(), K))
ref = np.stack(R.reference_form_torch(pred_sem, sem_label, K)).astype(np.int64)
assert np.array_equal(np.stack([want[0], want[1] + want[2] - want[0], want[2]]), ref)     # every count below 2^24 here
new_form()
got = sem.result()
assert np.array_equal(np.stack([got["intersection"], got["output"], got["target"]]), want)
assert np.array_equal(mask.rows()[0], R.mask_row(pred_mask.float().cpu().numpy(), gt_mask.cpu().numpy()))

times = {"new": [], "reference": []}
for i in range(5):
    new_form()
    reference_form(pred_mask.float().clone())
while sum(times["new"]) < seconds or sum(times["reference"]) < seconds:
    mask._n = 0                                            # keep writing row 0: the buffer does not grow while timing
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    new_form()
    times["new"].append(time.perf_counter() - t0)
    scores = pred_mask.float().clone()                     # the reference binarises its input in place: a fresh copy, untimed
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    reference_form(scores)
    times["reference"].append(time.perf_counter() - t0)

res = {"what": "per-scene wall time of the validation meters, bench scene (seed 2, 3 copies), real eval-forward pred tensors",
       "points": int(pred_sem.numel()), "mask_rows": int(gt_mask.numel()), "mask_dtype": str(pred_mask.dtype),
       "device": torch.cuda.get_device_name(0), "seconds_per_form": seconds}
for k, v in times.items():
    a = np.array(v) * 1e3
    res[k] = {"iterations": len(v), "median_ms": float(np.median(a)), "mean_ms": float(a.mean()), "min_ms": float(a.min()),
              "p90_ms": float(np.percentile(a, 90))}
res["speedup_median"] = res["reference"]["median_ms"] / res["new"]["median_ms"]
print(json.dumps(res))
if out_path:
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
