"""The grouping stage on the bench scene's selected points, called eagerly 12 times as PBNet.forward calls it: run under
`rocprofv3 --kernel-trace` and summarise with scripts/grouping_trace_summary.py (PBNET_HIP_LIB selects the build)."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import bench as B
from pbnet_amd import pbnet_ops

dev = torch.device("cuda", 0)
cfg, model, b, t, info, raw = B.build_workload(0, 1, torch.bfloat16, dev, "c2", 1)
calls = []
orig = pbnet_ops.cluster_device
def spy(*a, **k):
    calls.append((a, k))
    return orig(*a, **k)
pbnet_ops.cluster_device = spy
B.one_step(model, b, t)
torch.cuda.synchronize()
pbnet_ops.cluster_device = orig
a, k = calls[0]
print("points", a[0].shape[0], "kw", k)
for _ in range(12):
    r = orig(*a, **k)
torch.cuda.synchronize()
print("clusters", int(r.n_clusters.item()), "largest", int((r.member_start[1:int(r.n_clusters.item()) + 1] - r.member_start[:int(r.n_clusters.item())]).max().item()))
