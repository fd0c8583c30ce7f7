"""Python face of csrc/front.hip, csrc/heads.hip and csrc/plan.hip: the fused glue between the big kernels of PBNet.forward on
the inference path (/root/reference/network/PBNet.py:113-280), and the ONLY module that marshals those entry points.  Device
tensors in, device tensors out, no host synchronisation; every function is one launch.  (With autograd enabled PBNet.forward
keeps the differentiable tensor-op form.)  Given a device-side count (`n_dev`: an int32 device tensor whose FIRST word is the
count, e.g. the one-element view counts[k:k + 1] -- no launch, no allocation, no synchronisation, and it captures into a HIP
graph) the sizes are CAPACITIES; without one they are exact."""
from types import SimpleNamespace

import numpy as np
import torch

from . import _native as N

_DT = N.DT
# include/pbnet_hip.h PBN_CNT_* / PBN_OVF_*: the words of the device-side counts and the bits of counts[OVERFLOW]
CNT = SimpleNamespace(POINTS=0, CLUSTERS=1, ENTRIES=2, ROWS=3, SCENES=4, PROPOSAL_ROWS=5, PROPOSALS=6, OVERFLOW=7, WORDS=16)
OVF_NAMES = {1: "selected points", 2: "clusters", 4: "local-scene entries", 8: "local-scene rows",
             16: "clusters of one (class, batch) segment", 32: "batch index outside [0, cluster_batch)", 64: "rows of a level",
             128: "a segment of more than 25 clusters (torch.cdist ranks through its matrix-multiply path: host plan)"}


def reciprocal_f32(x):
    """fp32 reciprocal of a host scalar: what a device tensor divided by a host scalar is multiplied by."""
    return float(np.float32(1.0) / np.float32(x))


class EntryTable(object):
    """The entry table of the local scenes: ONE int32 device buffer [row_start (n + 1) | member_start n | scene n | weight bits n]
    for n entries (a capacity when planned on the device).  The kernels take four addresses and ask no alignment of them."""

    def __init__(self, buf, n):
        assert buf.dtype == torch.int32 and buf.numel() == 4 * n + 1 and buf.is_contiguous()
        self.buf, self.n = buf, int(n)

    row_start = property(lambda self: self.buf[:self.n + 1])
    member_start = property(lambda self: self.buf[self.n + 1:2 * self.n + 1])
    scene = property(lambda self: self.buf[2 * self.n + 1:3 * self.n + 1])
    weight = property(lambda self: self.buf[3 * self.n + 1:].view(torch.float32))

    def pointers(self):
        base, n = self.buf.data_ptr(), self.n
        return tuple(N.c_vp(base + 4 * (k * n + 1)) if k else N.c_vp(base) for k in range(4))

    def compact(self, n_ent):
        """The buffer of the first n_ent entries (one concatenation on the device)."""
        return torch.cat([self.buf[:n_ent + 1]] + [self.buf[k * self.n + 1:k * self.n + 1 + n_ent] for k in (1, 2, 3)])


def local_scene_rows(packed, n_ent, n_rows, member_idx, ins_ind, xyz, voxel, point_feat, sem_score, sem_pred, ld_out=None,
                     n_ent_dev=None, n_rows_dev=None):
    """PBNet.py:182-247 in one launch.  packed: an EntryTable of n_ent entries, or its buffer i32[4*n_ent+1] on the device;
    n_ent_dev / n_rows_dev: device-side counts.  Returns (point_idx i64[R], row_scene i64[R], coords i32[R,4], feat [R, C+2])."""
    ent = packed if isinstance(packed, EntryTable) else EntryTable(packed, n_ent)
    N.require_cuda(ent.buf, member_idx, ins_ind, xyz, point_feat, sem_score)
    dev = point_feat.device
    c = int(point_feat.shape[1])
    ld_out = c + 2 if ld_out is None else int(ld_out)
    assert ent.n == n_ent and (n_ent_dev is None) == (n_rows_dev is None)
    assert point_feat.stride(1) == 1 and sem_score.stride(1) == 1 and sem_score.dtype == point_feat.dtype
    assert xyz.dtype == torch.float32 and xyz.is_contiguous() and ins_ind.dtype == torch.int64
    assert member_idx.dtype == torch.int32 and (sem_pred is None or sem_pred.dtype == torch.int64)
    point_idx = torch.empty(n_rows, dtype=torch.int64, device=dev)
    row_scene = torch.empty(n_rows, dtype=torch.int64, device=dev)
    coords = torch.empty(n_rows, 4, dtype=torch.int32, device=dev)
    feat = torch.empty(n_rows, ld_out, dtype=point_feat.dtype, device=dev)
    vp = N.c_vp
    rc = N.lib().pbn_local_scene_rows(*(ent.pointers() + (
        int(n_ent), int(n_rows), N.ptr(n_ent_dev), N.ptr(n_rows_dev), N.ptr(member_idx), N.ptr(ins_ind), N.ptr(xyz),
        reciprocal_f32(voxel), vp(point_feat.data_ptr()), point_feat.stride(0), c, vp(sem_score.data_ptr()),
        sem_score.stride(0), N.ptr(sem_pred), _DT[point_feat.dtype], N.ptr(point_idx), N.ptr(row_scene), N.ptr(coords),
        vp(feat.data_ptr()), ld_out, N.current_stream())))
    N.check(rc, "pbn_local_scene_rows")
    return point_idx, row_scene, coords, feat


def gather_pad_rows(feats, width, idx=None, idx2=None, n=None, n_dev=None):
    """out[i, :] = feats[idx2[idx[i]], :] (either index None = identity) zero-padded to `width` columns, in one launch.  n: output
    rows (default: those of idx, else of feats); n_dev: their device-side count."""
    N.require_cuda(feats, idx, idx2)
    es = feats.element_size()
    if n is None:
        n = int(idx.shape[0]) if idx is not None else int(feats.shape[0])
    assert feats.stride(1) == 1 and feats.shape[1] <= width
    out = torch.empty(n, width, dtype=feats.dtype, device=feats.device)
    vp = N.c_vp
    rc = N.lib().pbn_gather_pad_rows(vp(feats.data_ptr()), feats.stride(0) * es, int(feats.shape[1]) * es, N.ptr(idx),
                                     N.ptr(idx2), int(n), N.ptr(n_dev), vp(out.data_ptr()), width * es, N.current_stream())
    N.check(rc, "pbn_gather_pad_rows")
    return out


class _HeadParams(object):
    """fp32 device copies of one two-layer head (Linear, BatchNorm(eval), PReLU, Linear[, Sigmoid]) in the layout
    pbn_mlp_rows reads; rebuilt when any parameter / running statistic changes."""

    def __init__(self):
        self.key = None

    def get(self, head):
        lin1, bn, act, lin2 = head[0].linear, head[1].bn, head[2].module, head[3].linear
        tensors = [lin1.weight, bn.weight, bn.bias, bn.running_mean, bn.running_var, act.weight, lin2.weight, lin2.bias]
        key = tuple((t.data_ptr(), t._version) for t in tensors if t is not None)
        if key != self.key:
            with torch.no_grad():
                f = lambda t: t.detach().float().contiguous()
                scale = f(bn.weight) / torch.sqrt(f(bn.running_var) + bn.eps)
                shift = f(bn.bias) - f(bn.running_mean) * scale
                hidden = lin1.weight.shape[0]
                self.w1 = f(lin1.weight)
                self.scale, self.shift = scale.contiguous(), shift.contiguous()
                self.slope = f(act.weight).expand(hidden).contiguous()
                self.w2 = f(lin2.weight)
                self.b2 = f(lin2.bias) if lin2.bias is not None else None
                self.hidden, self.n_out, self.channels = int(hidden), int(lin2.weight.shape[0]), int(lin1.weight.shape[1])
                self.sigmoid = len(head) > 4
                assert lin1.bias is None
            self.key = key
        return self


_HEADS = {}


def mlp_rows(head, feats, idx_a=None, idx_b=None, n=None, n_dev=None, in_rows=None):
    """head(x) for the rows feats[idx_b[idx_a[i]]] (PBNet.py:43-82 heads, eval mode) in one launch; returns [n, n_out].
    n_dev: device-side count of the rows; a row index outside [0, in_rows) (default: the rows of feats) then reads as zeros."""
    hp = _HEADS.setdefault(id(head), _HeadParams()).get(head)
    N.require_cuda(feats)
    assert feats.stride(1) == 1 and feats.shape[1] == hp.channels
    if n is None:
        n = int(idx_a.shape[0]) if idx_a is not None else int(feats.shape[0])
    out = torch.empty(n, hp.n_out, dtype=feats.dtype, device=feats.device)
    vp = N.c_vp
    if n_dev is None:
        in_rows = -1             # exact sizes: the rows are not bounded
    elif in_rows is None:
        in_rows = feats.shape[0]
    rc = N.lib().pbn_mlp_rows(vp(feats.data_ptr()), feats.stride(0), int(in_rows), hp.channels, N.ptr(idx_a), N.ptr(idx_b), int(n),
                              N.ptr(n_dev), N.ptr(hp.w1), N.ptr(hp.scale), N.ptr(hp.shift), N.ptr(hp.slope), hp.hidden,
                              N.ptr(hp.w2), N.ptr(hp.b2), hp.n_out, int(hp.sigmoid), vp(out.data_ptr()), hp.n_out,
                              _DT[feats.dtype], N.current_stream())
    N.check(rc, "pbn_mlp_rows")
    return out


def sem_argmax_table(score, batch, nb):
    """PBNet.py:134,151-163: (sem_pred i64[N], sem_prob [N] own-class softmax score, table i32[S, nb], block_hist)."""
    N.require_cuda(score)
    n, s = int(score.shape[0]), int(score.shape[1])
    dev = score.device
    assert score.stride(1) == 1 and (batch is None or (batch.dtype == torch.int32 and batch.is_contiguous()))
    lib = N.lib()
    sem_pred = torch.empty(n, dtype=torch.int64, device=dev)
    sem_prob = torch.empty(n, dtype=score.dtype, device=dev)
    table = torch.empty(s, nb, dtype=torch.int32, device=dev)
    block_hist = torch.empty(max(lib.pbn_select_blocks(n), 1), s, dtype=torch.int32, device=dev)
    rc = lib.pbn_sem_argmax_table(N.c_vp(score.data_ptr()), score.stride(0), s, N.ptr(batch), int(nb), n, _DT[score.dtype],
                                  N.ptr(sem_pred), N.c_vp(sem_prob.data_ptr()), N.ptr(table), N.ptr(block_hist),
                                  N.current_stream())
    N.check(rc, "pbn_sem_argmax_table")
    return sem_pred, sem_prob, table, block_hist


def select_points(sem_pred, class_base, block_hist, xyz, offset, m):
    """PBNet.py:151-170: class-major stable selection; class_base i32[S] on the device (-1 drops a class), m = number of
    selected points (host).  Returns (ins_ind i64[m], ins_orig f32[m,3], ins_offseted f32[m,3], ins_sem i32[m])."""
    N.require_cuda(sem_pred, class_base, block_hist, xyz, offset)
    dev = xyz.device
    n, s = int(sem_pred.shape[0]), int(class_base.shape[0])
    assert xyz.dtype == torch.float32 and xyz.is_contiguous() and offset.stride(1) == 1 and class_base.dtype == torch.int32
    ins_ind = torch.empty(m, dtype=torch.int64, device=dev)
    ins_orig = torch.empty(m, 3, dtype=torch.float32, device=dev)
    ins_off = torch.empty(m, 3, dtype=torch.float32, device=dev)
    ins_sem = torch.empty(m, dtype=torch.int32, device=dev)
    rc = N.lib().pbn_select_points(N.ptr(sem_pred), n, s, N.ptr(class_base), N.ptr(block_hist), N.ptr(xyz),
                                   N.c_vp(offset.data_ptr()), offset.stride(0), _DT[offset.dtype], N.ptr(ins_ind),
                                   N.ptr(ins_orig), N.ptr(ins_off), N.ptr(ins_sem), N.current_stream())
    N.check(rc, "pbn_select_points")
    return ins_ind, ins_orig, ins_off, ins_sem


def class_gate(table, thr05, nb, m_cap, n_points, counts):
    """PBNet.py:151-163 on the device: which classes enter the grouping (population gate thr05 f32[S]) and where.  Writes
    counts[POINTS] and the overflow bits; returns (class_base i32[S] for select_points, seg_len i32[(S-2)*nb])."""
    N.require_cuda(table, thr05, counts)
    s = int(table.shape[0])
    assert table.dtype == torch.int32 and thr05.dtype == torch.float32 and thr05.shape[0] == s and counts.numel() == CNT.WORDS
    class_base = torch.empty(s, dtype=torch.int32, device=table.device)
    seg_len = torch.empty((s - 2) * nb, dtype=torch.int32, device=table.device)
    rc = N.lib().pbn_class_gate(N.ptr(table), N.ptr(thr05), s, int(nb), int(m_cap), int(n_points), N.ptr(class_base),
                                N.ptr(seg_len), N.ptr(counts), N.current_stream())
    N.check(rc, "pbn_class_gate")
    return class_base, seg_len


def local_plan(res, nb, thr02, kmax, c_cap, e_cap, r_cap, counts):
    """PBNet.py:182-234 over CLUSTERS on the device: the EntryTable (at its capacity e_cap) of the local scenes of a capacity-mode
    grouping result (pbnet_ops.cluster_device).  Writes counts[CLUSTERS, ENTRIES, ROWS, SCENES] and the overflow bits."""
    N.require_cuda(res.cluster_num, thr02, kmax, counts)
    assert thr02.dtype == torch.float32 and kmax.dtype == torch.int32 and counts.dtype == torch.int32
    dev, lib = counts.device, N.lib()
    ent = EntryTable(torch.empty(4 * e_cap + 1, dtype=torch.int32, device=dev), e_cap)
    ws_bytes = int(lib.pbn_local_plan_workspace_bytes(int(c_cap)))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    rc = lib.pbn_local_plan(N.ptr(res.cluster_num), int(res.cluster_num.shape[0]), int(nb), N.ptr(res.member_start),
                            N.ptr(res.centers), N.ptr(res.n_clusters), N.ptr(thr02), N.ptr(kmax), int(c_cap), int(e_cap),
                            int(r_cap), *(ent.pointers() + (N.ptr(counts), N.ptr(ws), ws_bytes, N.current_stream())))
    N.check(rc, "pbn_local_plan")
    return ent


def mask_count(mask_score, thd, row_scene, n_scenes, n_dev=None):
    """First half of get_proposal (PBNet.py:317-333): kept rows per local scene and per row block (device tensors); n_dev:
    device-side count of the rows."""
    N.require_cuda(mask_score, row_scene)
    n = int(row_scene.shape[0])
    dev = mask_score.device
    lib = N.lib()
    ms = mask_score.view(n, -1) if n else mask_score.view(0, 1)
    assert ms.stride(1) == 1 and row_scene.dtype == torch.int64
    per_scene = torch.empty(max(n_scenes, 1), dtype=torch.int32, device=dev)
    block_cnt = torch.empty(max(lib.pbn_select_blocks(n), 1), dtype=torch.int32, device=dev)
    rc = lib.pbn_mask_count(N.c_vp(ms.data_ptr()), ms.stride(0), float(thd), N.ptr(row_scene), n, N.ptr(n_dev), int(n_scenes),
                            _DT[ms.dtype], N.ptr(per_scene), N.ptr(block_cnt), N.current_stream())
    N.check(rc, "pbn_mask_count")
    return per_scene[:n_scenes], block_cnt


def proposal_offsets(per_scene, counts):
    """PBNet.py:330-345 on the device: from the kept rows per local scene (a capacity's worth; counts[SCENES] of them exist) the
    (proposals_offset i64[S+1], surviving scene ids i64[S], dense renumbering i32[S]); writes counts[PROPOSALS, PROPOSAL_ROWS]."""
    N.require_cuda(per_scene, counts)
    s_cap, dev = int(per_scene.shape[0]), per_scene.device
    assert per_scene.dtype == torch.int32 and counts.numel() == CNT.WORDS
    proposals_offset = torch.zeros(s_cap + 1, dtype=torch.int64, device=dev)
    alive_ids = torch.zeros(s_cap, dtype=torch.int64, device=dev)
    dense_of = torch.empty(s_cap, dtype=torch.int32, device=dev)
    rc = N.lib().pbn_proposal_offsets(N.ptr(per_scene), s_cap, N.ptr(proposals_offset), N.ptr(alive_ids), N.ptr(dense_of),
                                      N.ptr(counts), N.current_stream())
    N.check(rc, "pbn_proposal_offsets")
    return proposals_offset, alive_ids, dense_of


def proposal_rows(mask_score, thd, row_scene, point_idx, dense_of, block_cnt, total, xyz=None, scale=1.0, voxel=1.0,
                  point_feat=None, n_dev=None):
    """Second half of get_proposal (+ PBNet.py:240-252 when xyz / point_feat are given); n_dev: device-side count of the input
    rows (`total` is then a capacity).  Returns (proposals_idx i64[P,2], proposals_ms [P], coords i32[P,4] or None, feat [P,C] or None)."""
    n = int(row_scene.shape[0])
    dev = mask_score.device
    ms = mask_score.view(n, -1) if n else mask_score.view(0, 1)
    prop_idx = torch.empty(total, 2, dtype=torch.int64, device=dev)
    prop_ms = torch.empty(total, dtype=ms.dtype, device=dev)
    coords = torch.empty(total, 4, dtype=torch.int32, device=dev) if xyz is not None else None
    feat = None
    c = ld_feat = 0
    if point_feat is not None:
        assert point_feat.stride(1) == 1 and point_feat.dtype == ms.dtype
        c, ld_feat = int(point_feat.shape[1]), point_feat.stride(0)
        feat = torch.empty(total, c, dtype=point_feat.dtype, device=dev)
    if total == 0:               # no row passed the threshold: nothing to launch (empty tensors have no address)
        return prop_idx, prop_ms, coords, feat
    vp = N.c_vp
    rc = N.lib().pbn_proposal_rows(
        vp(ms.data_ptr()), ms.stride(0), float(thd), N.ptr(row_scene), N.ptr(point_idx), n, N.ptr(n_dev), N.ptr(dense_of),
        N.ptr(block_cnt), N.ptr(xyz), float(np.float32(scale)), reciprocal_f32(voxel),
        None if point_feat is None else vp(point_feat.data_ptr()), ld_feat, c, _DT[ms.dtype], N.ptr(prop_idx),
        vp(prop_ms.data_ptr()), N.ptr(coords), None if feat is None else vp(feat.data_ptr()), N.current_stream())
    N.check(rc, "pbn_proposal_rows")
    return prop_idx, prop_ms, coords, feat


def batch_starts(coords, n_cap, n_dev, n_segments):
    """seg_start i32[n_segments + 1]: first row of the batch-sorted coordinate list coords i32[., 4] whose batch index is >= s --
    the segments MinkowskiEngine.nn.segment_pool reduces.  Rows read: min(n_dev, n_cap); n_dev, the rows that exist, never exceeds
    the list, while n_cap (the row capacity of the consumer) may when capacities were chosen inconsistently."""
    N.require_cuda(coords)
    assert coords.dtype == torch.int32 and coords.shape[1] == 4
    seg_start = torch.empty(n_segments + 1, dtype=torch.int32, device=coords.device)
    rc = N.lib().pbn_batch_starts(N.ptr(coords), N.ptr(n_dev), int(n_cap), int(n_segments), N.ptr(seg_start),
                                  N.current_stream())
    N.check(rc, "pbn_batch_starts")
    return seg_start
