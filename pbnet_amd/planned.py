"""Capacity-planned inference: PBNet.forward (task 'test', /root/reference/network/PBNet.py:113-280) as a FIXED launch
sequence with no host synchronisation inside.

The reference -- and the size-exact path of pbnet_amd.network.PBNet -- learn every data-dependent size on the host (class
populations, number of clusters, their centres and sizes, rows per local scene, proposal rows, the row counts of three
coordinate pyramids: six to seven device->host copies per forward).  Here every such size stays on the device:

  * buffers are allocated at CAPACITIES (Capacities, normally measured once on a scene of the same size class by
    `measure_capacities` and padded by a slack factor);
  * the decisions the reference takes on the host are three small device launches (csrc/plan.hip: class gate, local-scene
    plan with the kNN of the cluster centres, proposal offsets);
  * every kernel bounds itself by a device-side count and the launch grids are sized by the capacities;
  * an overflow of any capacity raises a flag in the device-side counts instead of writing out of bounds; `finish` (the ONE
    read-back of the forward) reports it and the caller falls back to the size-exact path.

Because the sequence is fixed it can be captured in a HIP graph (`PlannedForward.capture`) and replayed: BASELINE configs[4].
Results are bit-identical to the size-exact path whenever the same kernel configurations are chosen (capacities equal to
the true sizes); with slack the convolution tiles / pooling splits of a level may differ, which changes fp32 summation
order only (tests/test_planned_gpu.py)."""
import ctypes
import os
import sys

import torch

from . import _native as N
from . import stage_ops
from .MinkowskiEngine import conventions as CV
from .MinkowskiEngine.conv import SPLITK_WORKSPACE_BYTES
from .MinkowskiEngine.core import table_arrays
from .MinkowskiEngine.nn import segment_pool
from .network.PBNet import LOCAL_VOXEL, MASK_THD
from .network.mink_unet import alloc_arena, input_slab
from .stage_ops import CNT, OVF_NAMES          # (re-exported: the names callers of this module use)

_DEBUG = os.environ.get("PBN_PLANNED_DEBUG", "0") == "1"
HINTS = os.environ.get("PBN_PLANNED_HINTS", "1") != "0"      # kernel choice by the rows expected, not by the capacities
_STOP = os.environ.get("PBN_PLANNED_STOP", "")      # debugging: end the launch sequence after the named stage
_TRACE = _DEBUG or bool(_STOP)


def _stage_done(stage, counts, live):
    """End of a stage of the launch sequence.  PBN_PLANNED_DEBUG=1: synchronise and say where the forward is (hang / fault
    localisation).  PBN_PLANNED_STOP=<stage>: returns what `run` returns instead of going on -- the counts and, kept alive, the
    tensors and lineages among `live` (the caller's locals)."""
    if _DEBUG:
        torch.cuda.synchronize()
        sys.stderr.write("[planned] %s done counts=%s\n" % (stage, counts.tolist()[:8]))
        sys.stderr.flush()
    if _STOP == stage:
        return {"counts": counts, "_keep": {k: v for k, v in live.items() if torch.is_tensor(v) or isinstance(v, _Lineage)}}
    return None


class Capacities(object):
    """Buffer sizes of one planned forward.  lv1 / lv2 / lv3: rows per tensor stride (1..16) of the backbone, mask-branch
    and score-branch coordinate pyramids; points: points entering the grouping; clusters; entries / rows of the local scenes."""
    FIELDS = ("n_points", "n_voxels", "lv1", "lv2", "lv3", "points", "clusters", "entries", "rows")

    def __init__(self, **kw):
        for k in self.FIELDS:
            setattr(self, k, kw[k])
        # rows EXPECTED per level (the measured ones): the kernels' family / tile choice follows these, the grids the capacities
        # (round 5: choosing by the 1.25 x capacities picked slower kernels -- pbn_unet_forward_dev's rows_expected)
        self.expect = kw.get("expect") or {"lv1": list(self.lv1), "lv2": list(self.lv2), "lv3": list(self.lv3)}

    def padded(self, slack=1.25, quantum=256):
        """The same plan with head room: every data-dependent size x slack, rounded up to a multiple of `quantum`."""
        def up(v, lo=quantum):
            return int(max(lo, -(-int(v * slack) // quantum) * quantum))
        return Capacities(n_points=self.n_points, n_voxels=self.n_voxels,
                          lv1=[self.n_voxels] + [up(v) for v in self.lv1[1:]], lv2=[up(v) for v in self.lv2],
                          lv3=[up(v) for v in self.lv3], points=min(self.n_points, up(self.points)),
                          clusters=up(self.clusters, 64), entries=up(self.entries, 64), rows=up(self.rows), expect=self.expect)

    def __repr__(self):
        return "Capacities(%s)" % ", ".join("%s=%r" % (k, getattr(self, k)) for k in self.FIELDS)


def measure_capacities(model, feat_voxel, xyz_voxel, xyz_original, v2p_index, teacher=None):
    """One size-exact forward that records every data-dependent size (PBNet._last_sizes)."""
    with torch.no_grad():
        model(feat_voxel, xyz_voxel, xyz_original, v2p_index, None, 1, "test", teacher=teacher)
    s = model._last_sizes
    return Capacities(n_points=int(xyz_original.shape[0]), n_voxels=int(feat_voxel.shape[0]), lv1=list(s["lv1"]),
                      lv2=list(s.get("lv2", [1] * 5)), lv3=list(s.get("lv3", [1] * 5)), points=int(s.get("points", 1)),
                      clusters=int(s.get("clusters", 1)), entries=int(s.get("entries", 1)), rows=int(s.get("rows", 1)))


class _Lineage(object):
    """pbn_coords_prepare(_dev) of one SparseTensor lineage into a private arena; views of what the forward needs.
    n_dev: device-side count of the coordinate rows (a one-element int32 view; n_cap is then their capacity) or None."""

    def __init__(self, coords, n_cap, n_dev, dev):
        lib = N.lib()
        self.P = N.PrepareLayout()
        nbytes = lib.pbn_coords_prepare_bytes(int(n_cap), 1, ctypes.byref(self.P))
        self.arena = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        if n_dev is None:
            rc = lib.pbn_coords_prepare(N.ptr(coords), int(n_cap), 1, int(CV.X_FASTEST), N.ptr(self.arena), nbytes,
                                        ctypes.byref(self.P), N.current_stream())
        else:
            rc = lib.pbn_coords_prepare_dev(N.ptr(coords), N.ptr(n_dev), int(n_cap), 1, int(CV.X_FASTEST),
                                            N.ptr(self.arena), nbytes, ctypes.byref(self.P), N.current_stream())
        N.check(rc, "pbn_coords_prepare")
        self.n_cap = int(n_cap)
        L = self.P.pyramid
        self.counts = self.view(L.counts, 5, torch.int32)                       # rows per level (device)
        self.perm = self.view(self.P.perm, n_cap, torch.int64)                  # unique row at Z-order position p
        self.inv_perm = self.view(self.P.inv_perm, n_cap, torch.int64)
        self.unique_index = self.view(self.P.unique_index, n_cap, torch.int64)  # input row of unique row u
        self.inverse = self.view(self.P.inverse, n_cap, torch.int64)            # unique row of input row i
        self.ucoords = self.view(self.P.ucoords, n_cap * 4, torch.int32).view(n_cap, 4)

    def view(self, offset, count, dtype):
        nbytes = int(count) * torch.empty(0, dtype=dtype).element_size()
        return self.arena[offset:offset + nbytes].view(dtype)

    def tables(self):
        return table_arrays(self.arena.data_ptr(), self.P.pyramid)


class PlannedForward(object):
    def __init__(self, model, cap, dtype=torch.bfloat16, device=None):
        self.model, self.cap, self.dtype = model, cap, dtype
        self.dev = device or next(model.parameters()).device
        model._front_consts(self.dev)                                  # built here, not inside a capture
        self.nb = 3                                                    # PBNet.py:167-170: cluster_batch outside training
        self.graph = None
        # level capacities on the device (compared with the row counts of each pyramid; built here, not inside a capture)
        self._caps_t = {id(lv): torch.tensor([int(v) for v in lv], dtype=torch.int32, device=self.dev)
                        for lv in (cap.lv1, cap.lv2, cap.lv3)}

    # ---- helpers ----------------------------------------------------------------------------------------------------
    def _unet(self, net, lin, cap_levels, feats, expect=None):
        """Fused U-Net on a lineage: feats are the INPUT rows (before de-duplication); returns the output slab in Z-order
        [cap_levels[0], cout] and flags a level whose row count exceeds its capacity."""
        lib = N.lib()
        dt, dev = self.dtype, self.dev
        plan = net._plan(dt)
        cin_p = plan["cin_p"]
        n0 = int(cap_levels[0])
        padded = input_slab(feats, cin_p, lin.perm, lin.unique_index, n0, lin.counts)
        arena, nbytes, offs, n_rows = alloc_arena(plan["bufs"], plan["n_bufs"], cap_levels, dt, dev)
        k3, k5, down, up = lin.tables()
        # split-K scratch of THIS forward: the per-stream cache of the size-exact path must not be used here -- every graph
        # capture of a process runs on torch's one shared capture stream, so a cached block would be handed from the private
        # pool of one captured graph to the next and dangle once the first graph is released
        ws = self._splitk_ws
        vp = ctypes.c_void_p
        hint = None
        if expect is not None and HINTS:
            hint = (ctypes.c_int32 * 5)(*[max(1, min(int(e), int(c))) for e, c in zip(expect, cap_levels)])
        N.check(lib.pbn_unet_forward_dev(plan["ops"], plan["n_ops"], plan["bufs"], plan["n_bufs"], n_rows,
                                         vp(lin.counts.data_ptr()), hint, vp(padded.data_ptr()), cin_p, k3, k5, down, up,
                                         vp(arena.data_ptr()), nbytes, N.DT[dt], vp(ws.data_ptr()), ws.numel(),
                                         N.current_stream()), "pbn_unet_forward_dev")
        self._level_overflow.append((lin.counts > self._caps_t[id(cap_levels)]).any())
        return net._output_rows(plan, arena, offs, n0, dt)

    # ---- the forward: launches only -------------------------------------------------------------------------------------
    def run(self, feat_voxel, xyz_voxel, xyz_original, v2p_index, teacher=None):
        """Returns capacity-sized device tensors + the device-side counts; nothing is read back."""
        m, cap, dev, dt = self.model, self.cap, self.dev, self.dtype
        n_pts, n_vox, nb = cap.n_points, cap.n_voxels, self.nb
        assert feat_voxel.shape[0] == n_vox and xyz_original.shape[0] == n_pts and feat_voxel.dtype == dt
        self._level_overflow = []
        self._splitk_ws = torch.empty(SPLITK_WORKSPACE_BYTES, dtype=torch.uint8, device=dev)
        counts = torch.zeros(CNT.WORDS, dtype=torch.int32, device=dev)
        n_ent_d, n_rows_d, n_prop_rows_d = (counts[k:k + 1] for k in (CNT.ENTRIES, CNT.ROWS, CNT.PROPOSAL_ROWS))
        xyz = xyz_original.float().contiguous()

        # ---- backbone + heads (PBNet.py:117-136) ----
        coords1 = xyz_voxel.to(torch.int32).contiguous()
        lin1 = _Lineage(coords1, n_vox, None, dev)
        if _STOP == "prepare1":
            return {"counts": counts, "_keep": {"lin1": lin1, "coords1": coords1}}
        f = self._unet(m.MEUnet, lin1, cap.lv1, feat_voxel.contiguous(), cap.expect["lv1"])
        if _TRACE and (stop := _stage_done("backbone", counts, locals())):
            return stop
        v2p = v2p_index.long()
        v2p_z = lin1.inv_perm[v2p]                                   # Z-order row of every point's voxel
        point_feat_p = f[v2p_z]
        sem_score = stage_ops.mlp_rows(m.linear_sem, f, v2p_z)
        offset_p = stage_ops.mlp_rows(m.linear_offset, f, v2p_z)
        batch_head = coords1[:, 0][v2p]
        if teacher is not None:
            sem_score = teacher["sem_score"].to(dev, sem_score.dtype)
            offset_p = teacher["offset"].to(dev, offset_p.dtype)
        sem_pred, sem_prob, table, block_hist = stage_ops.sem_argmax_table(sem_score, batch_head.contiguous(), nb)
        out = {"sem_pred_p": sem_pred, "sem_pred_score_p": sem_score, "offset_pred_p": offset_p, "counts": counts}
        if _TRACE and (stop := _stage_done("heads", counts, locals())):
            return stop

        # ---- class gate -> selection -> grouping -> local-scene plan (PBNet.py:151-234), sizes on the device ----
        c_cap, r_cap = int(cap.clusters), int(cap.rows)
        ins_ind, res, ent = m._front_launches(table, sem_pred, block_hist, xyz, offset_p, nb, int(cap.points), c_cap,
                                              int(cap.entries), r_cap, counts)
        if _TRACE and (stop := _stage_done("grouping", counts, locals())):
            return stop
        # ---- rows of the local scenes by one launch ----
        point_idx, row_scene, coords2, feat2 = stage_ops.local_scene_rows(
            ent, ent.n, r_cap, res.member_idx, ins_ind, xyz, LOCAL_VOXEL, point_feat_p, sem_prob.view(-1, 1), None,
            n_ent_dev=n_ent_d, n_rows_dev=n_rows_d)
        if _TRACE and (stop := _stage_done("local scene rows", counts, locals())):
            return stop

        # ---- mask branch (PBNet.py:236-252) ----
        lin2 = _Lineage(coords2, r_cap, n_rows_d, dev)
        f2 = self._unet(m.D_Unet, lin2, cap.lv2, feat2, cap.expect["lv2"])
        mask_score = stage_ops.mlp_rows(m.linear_binary, f2, lin2.inverse, lin2.inv_perm, r_cap, n_dev=n_rows_d)     # [r_cap, 1]
        if _TRACE and (stop := _stage_done("mask branch", counts, locals())):
            return stop

        # ---- proposals (PBNet.py:317-347) ----
        per_scene, block_cnt = stage_ops.mask_count(mask_score, MASK_THD, row_scene, c_cap, n_dev=n_rows_d)
        proposals_offset, alive_ids, dense_of = stage_ops.proposal_offsets(per_scene, counts)
        prop_idx, prop_ms, coords3, feat3 = stage_ops.proposal_rows(
            mask_score, MASK_THD, row_scene, point_idx, dense_of, block_cnt, r_cap, xyz, m.scale_size, m.voxel_size,
            point_feat_p, n_dev=n_rows_d)
        if _TRACE and (stop := _stage_done("proposals", counts, locals())):
            return stop

        # ---- score branch (PBNet.py:255-279) ----
        lin3 = _Lineage(coords3, r_cap, n_prop_rows_d, dev)
        f3 = self._unet(m.score_Unet, lin3, cap.lv3, feat3, cap.expect["lv3"])
        n3 = int(cap.lv3[0])
        iou_feat = stage_ops.mlp_rows(m.linear_IOU_feat, f3, lin3.inv_perm, None, n3, n_dev=lin3.counts)     # external row order
        seg_start = stage_ops.batch_starts(lin3.ucoords, n3, lin3.counts, c_cap)
        mx, av = segment_pool(iou_feat, None, c_cap, seg_start=seg_start)
        pooled = (mx + av).to(dt)
        clt_scores = stage_ops.mlp_rows(m.linear_IOU, pooled).view(-1)
        if _TRACE and (stop := _stage_done("score branch", counts, locals())):
            return stop
        # a level of one of the three pyramids that outgrew its capacity (rows were dropped): flag it
        ovf = torch.stack(self._level_overflow).any().to(torch.int32) * 64
        counts[CNT.OVERFLOW:CNT.OVERFLOW + 1] |= ovf
        out.update(proposals_idx=prop_idx, proposals_offset=proposals_offset, alive_ids=alive_ids, proposals_ms=prop_ms,
                   clt_scores=clt_scores, _keep=(lin1, lin2, lin3, res, feat2, feat3, point_feat_p, self._splitk_ws))
        return out

    # ---- the one read-back ------------------------------------------------------------------------------------------------
    def finish(self, out):
        """Slice the capacity-sized outputs to their true sizes (one device->host copy of 16 ints).  Returns the dict of
        PBNet.forward, or raises CapacityOverflow."""
        return self._slice(out, clone=False)

    @staticmethod
    def _slice(out, clone):
        c = out["counts"].cpu().tolist()
        if c[CNT.OVERFLOW]:
            raise CapacityOverflow(c[CNT.OVERFLOW])
        n_prop, n_rows = c[CNT.PROPOSALS], c[CNT.PROPOSAL_ROWS]
        f = (lambda t: t.clone()) if clone else (lambda t: t)
        return {"sem_pred_p": f(out["sem_pred_p"]), "sem_pred_score_p": f(out["sem_pred_score_p"]),
                "offset_pred_p": f(out["offset_pred_p"]),
                "proposals": (f(out["proposals_idx"][:n_rows]), f(out["proposals_offset"][:n_prop + 1]),
                              f(out["alive_ids"][:n_prop]), f(out["proposals_ms"][:n_rows])),
                "clt_scores": f(out["clt_scores"][:n_prop]), "counts": c}

    def __call__(self, feat_voxel, xyz_voxel, xyz_original, v2p_index, teacher=None):
        with torch.no_grad():
            return self.finish(self.run(feat_voxel, xyz_voxel, xyz_original, v2p_index, teacher))

    # ---- HIP graph ---------------------------------------------------------------------------------------------------------
    def capture(self, feat_voxel, xyz_voxel, xyz_original, v2p_index, teacher=None):
        """Capture the forward into a HIP graph over STATIC input buffers (copies of the arguments); `replay` copies new
        inputs of the same shapes in and launches the graph.  Warm-up runs first (weight packing, allocator pools)."""
        self.static_in = [feat_voxel.clone(), xyz_voxel.clone(), xyz_original.clone(), v2p_index.clone()]
        self.static_teacher = None if teacher is None else {k: v.clone() for k, v in teacher.items()}
        with torch.no_grad():
            s = torch.cuda.Stream(self.dev)
            s.wait_stream(torch.cuda.current_stream(self.dev))
            with torch.cuda.stream(s):
                for _ in range(2):
                    self.run(*self.static_in, teacher=self.static_teacher)
            torch.cuda.current_stream(self.dev).wait_stream(s)
            torch.cuda.synchronize(self.dev)
            self.graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.graph):
                self.static_out = self.run(*self.static_in, teacher=self.static_teacher)
        return self

    def replay(self, feat_voxel=None, xyz_voxel=None, xyz_original=None, v2p_index=None, teacher=None):
        """Copy new inputs (same shapes) into the static buffers and launch the graph on the caller's current stream.
        Replays may be interleaved with anything (eager kernels on the outputs, read-backs, synchronisations): every fill
        the launch sequence needs is a kernel node (csrc/common.hip fill_ranges) -- hipMemsetAsync nodes turned out not to
        re-execute after an explicit stream / device synchronisation between two replays on this ROCm runtime, which used to
        leave hash tables full (endless probe loops) and count tables accumulating."""
        new = (feat_voxel, xyz_voxel, xyz_original, v2p_index)
        for dst, src in zip(self.static_in, new):
            if src is not None:
                dst.copy_(src)
        if teacher is not None:
            for k, v in teacher.items():
                self.static_teacher[k].copy_(v)
        self.graph.replay()          # on the caller's current stream (a private replay stream per graph doubles the
                                     # number of HIP streams of a serving loop: 4 graphs in flight fell from 281 to 179 scenes/s)
        return self.static_out


class CapacityOverflow(RuntimeError):
    def __init__(self, flags):
        self.flags = int(flags)
        what = [name for bit, name in OVF_NAMES.items() if self.flags & bit]
        super().__init__("planned forward: capacity exceeded for " + ", ".join(what) + " -- rerun on the size-exact path")
