"""MinkUNet family on the MI355X kernels: the backbone of /root/reference/network/Mink.py (MinkUNetBase
:202-354 and its variants :357-419; factory Mink_unet :502-526).  Module and parameter names match the reference so
a state dict moves across unchanged (conv0p1s1.kernel, bn0.bn.weight, block1.0.conv1.kernel,
block2.0.downsample.0.kernel, convtr4p16s2.kernel, final_sematic.bias, ...).

Two execution paths over the same parameters:
  * module path  -- one kernel launch per ME module, BatchNorm/ReLU as separate feature passes; used in training
    mode and as the unfused cross-check;
  * fused path   -- eval mode only: BatchNorm folded into a per-channel scale/shift that the convolution applies in
    its epilogue together with ReLU and the residual add; skip concatenations are written in place (the encoder
    block stores its result directly into the right-hand columns of the decoder's concat slab, the transposed
    convolution into the left-hand columns), so no activation is touched twice.

The body's topology is stated twice: _forward_modules (the reference-shaped one) and walk_body, the one walk that the
inference plan (_build_plan), the training plan (train_engine.TrainPlan) and the Python-issued cross-check
(_forward_fused_py) all consume.
"""
import ctypes
import operator
import os

import torch
import torch.nn as nn

from .. import _native as N
from .. import stage_ops
from .. import MinkowskiEngine as ME
from ..MinkowskiEngine.conv import spconv_forward, pack_weight, _pad_vec, _vpo, _workspace
from ..MinkowskiEngine.modules.resnet_block import BasicBlock
from ..MinkowskiEngine.fused_train import conv_bn_act
from ..prof import section

# arch -> (blocks per stage, planes)   (Mink.py:357-419; BasicBlock families only)
SPECS = {
    "MinkUNet14A": ((1,) * 8, (32, 64, 128, 256, 128, 128, 96, 96)),
    "MinkUNet14B": ((1,) * 8, (32, 64, 128, 256, 128, 128, 128, 128)),
    "MinkUNet14C": ((1,) * 8, (32, 64, 128, 256, 192, 192, 128, 128)),
    "MinkUNet14D": ((1,) * 8, (32, 64, 128, 256, 384, 384, 384, 384)),
    "MinkUNet18A": ((2,) * 8, (32, 64, 128, 256, 128, 128, 96, 96)),
    "MinkUNet18B": ((2,) * 8, (32, 64, 128, 256, 128, 128, 128, 128)),
    "MinkUNet18D": ((2,) * 8, (32, 64, 128, 256, 384, 384, 384, 384)),
    "MinkUNet34A": ((2, 3, 4, 6, 2, 2, 2, 2), (32, 64, 128, 256, 256, 128, 64, 64)),
    "MinkUNet34B": ((2, 3, 4, 6, 2, 2, 2, 2), (32, 64, 128, 256, 256, 128, 64, 32)),
    "MinkUNet34C": ((2, 3, 4, 6, 2, 2, 2, 2), (32, 64, 128, 256, 256, 128, 96, 96)),
}
INIT_DIM = 32          # Mink.py:208
_DOWN = ("conv1p1s2", "conv2p2s2", "conv3p4s2", "conv4p8s2")
_DOWN_BN = ("bn1", "bn2", "bn3", "bn4")
_UP = ("convtr4p16s2", "convtr5p8s2", "convtr6p4s2", "convtr7p2s2")
_UP_BN = ("bntr4", "bntr5", "bntr6", "bntr7")


def _group_steps(spo):
    """Steps per barrier group of the workgroup-tile kernel: the largest divisor <= 4 of the steps per offset (spconv.hip)."""
    for c in (4, 3, 2, 1):
        if spo % c == 0:
            return c
    return 1


_VERSION_OF = operator.attrgetter("_version")

# map kind of a plan op (include/pbnet_hip.h) -> (kernel volume, slot in pbn_pair_lists[14] of (level_in, level_out), the map of a
# pyramid or coordinate manager for (level_in, level_out)); levels 0..4 are tensor strides 1..16.  csrc/unet_plan.h: op_tables
MAP_KINDS = {
    0: (1, None, lambda pyr, lin, lout: None),                                                  # 1x1: identity pairs
    1: (27, lambda lin, lout: lout, lambda pyr, lin, lout: pyr.kernel_map(1 << lout, 3)),
    2: (125, lambda lin, lout: 5, lambda pyr, lin, lout: pyr.kernel_map(1, 5)),
    3: (8, lambda lin, lout: 6 + lin, lambda pyr, lin, lout: pyr.down_map(1 << lin)),           # k2s2: level_in = fine level
    4: (8, lambda lin, lout: 10 + lout, lambda pyr, lin, lout: pyr.up_map(2 << lout)),          # transposed: level_out = fine
}


def walk_body(net, src, slab, conv, shortcut_block=None):
    """The body of a MinkUNet (Mink.py:291-350: everything but the final 1x1 convolution) as one sequence of convolutions
    over views the caller defines -- symbolic (buffer, column) pairs for the two native plans, tensors for the Python-issued
    cross-check.  Owns the order of the ops and where results go, nothing else:
      * the decoder slab of level l is [up | skip]: the stem and the encoder stages 1-3 write the right-hand columns, the
        transposed convolution of level l+1 the left-hand ones, the decoder stage reads the whole slab;
      * the last block of a stage writes into the view the stage was asked for.
    src: the input view.  slab(level, up_channels, skip_channels) -> (up view, skip view, whole slab), called for levels 0..3
    before any op.  conv(conv, norm, map_kind, level_in, level_out, src, residual, out, relu) -> the view it wrote (out =
    None: wherever the caller likes).  shortcut_block(blk, h, cur, level, out), optional, is offered every block with a 1x1
    shortcut after its first convolution (h = conv1's output, cur = the block's input): it may issue
    relu(bn2(conv2(h)) + bn_d(conv_d(cur))) its own way and return the view, or return None for the two separate ops.
    Returns the view of the body's output."""
    P = net.PLANES
    skip_c, up_c = (INIT_DIM, P[0], P[1], P[2]), (P[7], P[6], P[5], P[4])
    slabs = [slab(l, up_c[l], skip_c[l]) for l in range(4)]

    def stage(blocks, cur, l, out=None):
        for bi, blk in enumerate(blocks):
            h = conv(blk.conv1, blk.norm1, 1, l, l, cur, None, None, True)
            last_out = out if bi == len(blocks) - 1 else None
            nxt = None
            if blk.downsample is not None and shortcut_block is not None:
                nxt = shortcut_block(blk, h, cur, l, last_out)
            if nxt is None:
                res = cur
                if blk.downsample is not None:
                    res = conv(blk.downsample[0], blk.downsample[1], 0, l, l, cur, None, None, False)
                nxt = conv(blk.conv2, blk.norm2, 1, l, l, h, res, last_out, True)
            cur = nxt
        return cur

    cur = conv(net.conv0p1s1, net.bn0, 2, 0, 0, src, None, slabs[0][1], True)
    for l in range(1, 5):
        cur = conv(getattr(net, _DOWN[l - 1]), getattr(net, _DOWN_BN[l - 1]), 3, l - 1, l, cur, None, None, True)
        cur = stage(getattr(net, "block%d" % l), cur, l, out=slabs[l][1] if l < 4 else None)
    for i, l in enumerate((3, 2, 1, 0)):
        conv(getattr(net, _UP[i]), getattr(net, _UP_BN[i]), 4, l + 1, l, cur, None, slabs[l][0], True)
        cur = stage(getattr(net, "block%d" % (i + 5)), slabs[l][2], l)
    return cur


class MinkUNet(nn.Module):
    FUSE_EVAL = True
    # round 4: a BasicBlock's 1x1 shortcut (Mink.py:77-87) runs as extra reduction steps of the block's second convolution
    # (pbn_spconv_forward_dual): 7 launches fewer per network and no residual slab.  PBNET_FOLD_SHORTCUT=0: separate launches.
    FOLD_SHORTCUT = os.environ.get("PBNET_FOLD_SHORTCUT", "1") != "0"

    def _fold_is_safe(self, blk, dtype):
        """The folded form multiplies the BatchNorm scales gamma / sqrt(var + eps) into the 16-bit weights (the separate launches
        apply them in the fp32 epilogue).  In fp16 a very small running variance can push |w * scale| past 65504 and a very large
        one can push the bulk of the products into the subnormals: fold only when the scaled weights stay inside fp16's normal
        range (largest magnitude below 3e4, and at most 1 % of the non-zero products below 6.1e-5); bf16 and fp32 have fp32's
        exponent range.  (tests/test_backbone_gpu.py::test_fold_guard_extreme_batchnorm_statistics)"""
        if dtype != torch.float16:
            return True
        for conv, bn in ((blk.conv2, blk.norm2), (blk.downsample[0], blk.downsample[1])):
            cout = int(conv.kernel.shape[-1])
            s, _ = self._fold(bn, (cout + 15) // 16 * 16)
            w = (conv.kernel.detach().float() * s[:cout]).abs()
            nz = w[w > 0]
            if nz.numel() == 0:
                continue
            if float(nz.max()) > 3.0e4 or float((nz < 6.1e-5).float().mean()) > 0.01:
                return False
        return True
    MORTON = os.environ.get("PBNET_MORTON", "1") != "0"   # fused path runs the lineage in Z-order (L2-local gathers)
    OP_TIMING_SINK = None   # callable(model, plan, rows, cm, esz, op_ms) installed by bench.py's roofline probe

    def __init__(self, in_channels, out_channels, D=3, arch="MinkUNet34C"):
        super().__init__()
        assert D == 3
        self.arch = arch
        self.LAYERS, self.PLANES = SPECS[arch]
        P, L = self.PLANES, self.LAYERS
        self.inplanes = INIT_DIM
        self.conv0p1s1 = ME.MinkowskiConvolution(in_channels, self.inplanes, kernel_size=5, dimension=D)
        self.bn0 = ME.MinkowskiBatchNorm(self.inplanes)
        # encoder: k2s2 down convolution + residual stage, four times (Mink.py:226-251)
        for i in range(4):
            setattr(self, _DOWN[i], ME.MinkowskiConvolution(self.inplanes, self.inplanes, kernel_size=2, stride=2,
                                                            dimension=D))
            setattr(self, _DOWN_BN[i], ME.MinkowskiBatchNorm(self.inplanes))
            setattr(self, "block%d" % (i + 1), self._make_layer(P[i], L[i], D))
        # decoder: transposed k2s2 + skip concat + residual stage (Mink.py:253-280)
        skips = (P[2], P[1], P[0], INIT_DIM)
        for i in range(4):
            setattr(self, _UP[i], ME.MinkowskiConvolutionTranspose(self.inplanes, P[4 + i], kernel_size=2, stride=2,
                                                                   dimension=D))
            setattr(self, _UP_BN[i], ME.MinkowskiBatchNorm(P[4 + i]))
            self.inplanes = P[4 + i] + skips[i]
            setattr(self, "block%d" % (i + 5), self._make_layer(P[4 + i], L[4 + i], D))
        self.final_sematic = ME.MinkowskiConvolution(P[7], out_channels, kernel_size=1, bias=True, dimension=D)
        self.relu = ME.MinkowskiReLU(inplace=True)
        self.weight_initialization()
        self._fold_cache = {}
        self._plans = {}
        # load_state_dict(assign=True) -- also through a parent module -- replaces the Parameter objects
        self.register_load_state_dict_post_hook(lambda module, incompatible: module._forget_state_tensors())

    def _make_layer(self, planes, blocks, D):
        """Mink.py:75-107 with stride 1: a 1x1 conv + BN shortcut iff the channel count changes."""
        downsample = None
        if self.inplanes != planes:
            downsample = nn.Sequential(ME.MinkowskiConvolution(self.inplanes, planes, kernel_size=1, stride=1, dimension=D),
                                       ME.MinkowskiBatchNorm(planes))
        layers = [BasicBlock(self.inplanes, planes, stride=1, downsample=downsample, dimension=D)]
        self.inplanes = planes
        layers += [BasicBlock(planes, planes, stride=1, dimension=D) for _ in range(1, blocks)]
        return nn.Sequential(*layers)

    def weight_initialization(self):
        """Mink.py:66-73: kaiming-normal(fan_out) on MinkowskiConvolution kernels (transposed ones keep ME's default
        uniform init: they are a different class), BN weight 1 / bias 0."""
        for m in self.modules():
            if isinstance(m, ME.MinkowskiConvolution):
                ME.utils.kaiming_normal_(m.kernel, mode="fan_out", nonlinearity="relu")
            if isinstance(m, ME.MinkowskiBatchNorm):
                nn.init.constant_(m.bn.weight, 1)
                nn.init.constant_(m.bn.bias, 0)

    # ---------------------------------------------------------------------------------------------------------
    def forward(self, x):
        if self.FUSE_EVAL and not self.training and not torch.is_grad_enabled():
            return self._forward_fused(x)
        return self._forward_modules(x)

    def _forward_modules(self, x):
        """Mink.py:291-354, module by module -- or, on the native training path, the whole body as one autograd node
        (network/train_engine.py) followed by the final 1x1 convolution."""
        from .train_engine import forward_body
        body = forward_body(self, x)
        if body is not None:
            return self.final_sematic(body)
        out = conv_bn_act(self.conv0p1s1, self.bn0, x)                # = self.relu(self.bn0(self.conv0p1s1(x))), one node when training natively
        skips = [out]
        for i in range(4):
            out = conv_bn_act(getattr(self, _DOWN[i]), getattr(self, _DOWN_BN[i]), out)
            out = getattr(self, "block%d" % (i + 1))(out)
            if i < 3:
                skips.append(out)
        for i in range(4):
            out = conv_bn_act(getattr(self, _UP[i]), getattr(self, _UP_BN[i]), out)
            out = ME.cat(out, skips[3 - i])
            out = getattr(self, "block%d" % (i + 5))(out)
        return self.final_sematic(out)

    # ---------------------------------------------------------------------------------------------------------
    def _fold(self, bn, cout_p):
        """Eval-mode BatchNorm as y = x*scale + shift (fp32, padded to the kernel's channel tile)."""
        b = bn.bn
        key = (id(bn), b.weight._version, b.bias._version, b.running_mean._version, b.running_var._version, cout_p)
        hit = self._fold_cache.get(id(bn))
        if hit is None or hit[0] != key:
            scale = b.weight.detach().float() / torch.sqrt(b.running_var.float() + b.eps)
            shift = b.bias.detach().float() - b.running_mean.float() * scale
            hit = (key, _pad_vec(scale, cout_p, 1.0), _pad_vec(shift, cout_p, 0.0))
            self._fold_cache[id(bn)] = hit
        return hit[1], hit[2]

    def _cbr(self, conv, bn, feats, nbr, n_out, relu=True, residual=None, out=None):
        packed = conv._cache.get(conv.kernel, feats.dtype)
        scale, shift = self._fold(bn, packed[3])
        return spconv_forward(feats, nbr, n_out, packed, scale=scale, shift=shift, residual=residual, relu=relu, out=out)

    # ---- native executor: the fused forward as ONE C call (csrc/executor.hip) ------------------------------------
    def _build_plan(self, dtype):
        """Static list of fused convolution ops over symbolic buffers: walk_body in eval mode (BatchNorm folded into the
        epilogue, a 1x1 shortcut folded into its block's second convolution where that is safe) plus the final 1x1.
        Buffer 0 is the input slab; levels 0..4 are tensor strides 1..16."""
        keep, ops, bufs, true_io, folded_io = [], [], [(0, 0)], [], []

        def new_buf(level, width):
            bufs.append((level, width))
            return len(bufs) - 1

        def slab(level, up, skip):
            b = new_buf(level, up + skip)
            return (b, 0), (b, up), (b, 0)

        def emit(map_kind, lin, lout, src, res, out, packed, scale, shift, relu, src2=(-1, 0), vpo2=0):
            w, vpo, n_steps, cout_p = packed
            keep.extend([w, scale, shift])
            if out is None:
                out = (new_buf(lout, cout_p), 0)
            op = N.UnetOp()
            op.map_kind, op.level_in, op.level_out = map_kind, lin, lout
            op.in_buf, op.in_col = src
            op.res_buf, op.res_col = res if res is not None else (-1, 0)
            op.out_buf, op.out_col = out
            op.vpo, op.n_steps, op.cout_p, op.relu = vpo, n_steps, cout_p, int(relu)
            op.in2_buf, op.in2_col = src2
            op.vpo2 = vpo2
            op.w = w.data_ptr()
            op.scale = scale.data_ptr() if scale is not None else None
            op.shift = shift.data_ptr() if shift is not None else None
            ops.append(op)
            return out

        def add(conv, bn, map_kind, lin, lout, src, res, out, relu):
            packed = conv._cache.get(conv.kernel, dtype)
            if bn is not None:
                scale, shift = self._fold(bn, packed[3])
            else:
                scale = None
                shift = _pad_vec(conv.bias.detach(), packed[3], 0.0) if conv.bias is not None else None
            true_io.append((int(conv.kernel.shape[-2]), int(conv.kernel.shape[-1])))   # un-padded (C_in, C_out)
            return emit(map_kind, lin, lout, src, res, out, packed, scale, shift, relu)

        def add_folded(blk, h, cur, l, out):
            """relu(bn2(conv2(h)) + bn_d(conv_d(cur))) as ONE convolution over two sources: both BatchNorm scales go into the
            weights (they differ per branch), the shifts add up, the 1x1 kernel becomes the reduction steps behind the map's.
            None (the two separate ops) when folding is off, the channel counts do not fill whole barrier groups or the scaled
            weights would leave the dtype's range."""
            conv2, convd = blk.conv2, blk.downsample[0]
            if not (self.FOLD_SHORTCUT and _vpo(int(conv2.kernel.shape[-2]), dtype) % 4 == 0
                    and _vpo(int(convd.kernel.shape[-2]), dtype) % 4 == 0 and self._fold_is_safe(blk, dtype)):
                return None
            cout = int(conv2.kernel.shape[-1])
            cout_p = (cout + 15) // 16 * 16
            s2, b2 = self._fold(blk.norm2, cout_p)
            sd, bd = self._fold(blk.downsample[1], cout_p)
            k2 = conv2.kernel.detach().float() * s2[:cout]
            kd = convd.kernel.detach().float()
            kd = (kd if kd.dim() == 3 else kd.unsqueeze(0)) * sd[:cout]
            w2, vpo, n_main, cp2 = pack_weight(k2, dtype)
            wd, vpo2, n2, cpd = pack_weight(kd, dtype)
            assert cp2 == cpd == cout_p and vpo % 4 == 0 and vpo2 % 4 == 0
            cg = _group_steps(vpo // 4)
            pad = (-n2) % cg                           # whole barrier groups of the first source: zero weights behind the real ones
            parts = [w2, wd] + ([torch.zeros(pad, *wd.shape[1:], dtype=wd.dtype, device=wd.device)] if pad else [])
            w = torch.cat(parts, 0).contiguous()
            true_io.append((int(conv2.kernel.shape[-2]), cout))
            folded_io.append((len(ops), int(kd.shape[-2]), cout))
            return emit(1, l, l, h, None, out, (w, vpo, n_main + n2 + pad, cout_p), None, (b2 + bd).contiguous(), True, cur, vpo2)

        cur = walk_body(self, (0, 0), slab, add, add_folded)
        final = add(self.final_sematic, None, 0, 0, 0, cur, None, None, False)
        cin_p = self.conv0p1s1._cache.get(self.conv0p1s1.kernel, dtype)[1] * (16 // torch.empty(0, dtype=dtype).element_size())
        bufs[0] = (0, cin_p)
        ops_arr = (N.UnetOp * len(ops))(*ops)
        bufs_arr = (N.UnetBuf * len(bufs))(*[N.UnetBuf(lv, w) for lv, w in bufs])
        return dict(ops=ops_arr, n_ops=len(ops), bufs=bufs_arr, n_bufs=len(bufs), out_buf=final[0], cin_p=cin_p,
                    out_width=bufs[final[0]][1], keep=keep, true_io=true_io, folded_io=folded_io)

    def _forget_state_tensors(self):
        self.__dict__.pop("_state_tensors", None)
        self.__dict__.pop("_train_plans", None)
        self.__dict__.pop("_train_engine_ok", None)
        self.__dict__.pop("_train_engine_norms", None)
        self._plans.clear()

    def _apply(self, fn, *args, **kwargs):
        # .to() / .half() / .cuda() may swap the storage behind parameters: drop the tensor list and the packed plans
        self._forget_state_tensors()
        return super()._apply(fn, *args, **kwargs)

    def _plan(self, dtype):
        # in-place updates (optimizer steps, load_state_dict copies) bump ._version; walking the module tree for the
        # tensors costs ~1 ms of host time per call, so the list is kept (a forward is ~2.5 ms of device time)
        tensors = self.__dict__.get("_state_tensors")
        if tensors is None:
            tensors = list(self.parameters()) + list(self.buffers())
            self.__dict__["_state_tensors"] = tensors
        # versions only grow, so their SUM changes whenever any of them does: one C-level pass, no list / tuple per forward
        # (round 5: the walk was 0.23 ms of the ~3 ms of Python per forward that the in-flight rate is bound by)
        ver = sum(map(_VERSION_OF, tensors))
        hit = self._plans.get(dtype)
        if hit is None or hit[0] != ver:
            hit = (ver, self._build_plan(dtype))
            self._plans[dtype] = hit
        return hit[1]

    def _output_rows(self, plan, arena, offs, n, dtype):
        """The fused forward's output [n, out_channels]: a view of the arena."""
        out = arena_rows(arena, offs[plan["out_buf"]], n, plan["out_width"], dtype)
        cout = self.final_sematic.kernel.shape[-1]
        return out if out.shape[1] == cout else out[:, :cout]

    def _forward_fused(self, x):
        cm = x.coordinate_manager
        assert x.tensor_stride == 1
        sv = cm.sorted() if self.MORTON else None      # the lineage in Z-order: compact tiles, L2-local gathers
        pyr = sv.pyramid if sv is not None else cm.plain()
        dt, dev = x.F.dtype, x.F.device
        plan = self._plan(dt)
        feats = input_slab(x.F, plan["cin_p"], None if sv is None else sv.perm)
        rows = list(pyr.n)
        arena, nbytes, offs, n_rows = alloc_arena(plan["bufs"], plan["n_bufs"], rows, dt, dev)
        lib = N.lib()
        vp = ctypes.c_void_p
        ws = _workspace(dev)
        args = (plan["ops"], plan["n_ops"], plan["bufs"], plan["n_bufs"], n_rows, vp(feats.data_ptr()), feats.stride(0)) \
            + pyr.native_tables() + (vp(arena.data_ptr()), nbytes, N.DT[dt], vp(ws.data_ptr()), ws.numel(), N.current_stream())
        if MinkUNet.OP_TIMING_SINK is None:
            rc = lib.pbn_unet_forward(*args)
        else:  # bench.py's roofline probe: per-op HIP-event durations (synchronises)
            op_ms = (ctypes.c_float * plan["n_ops"])()
            rc = lib.pbn_unet_forward_timed(*(args + (op_ms,)))
            MinkUNet.OP_TIMING_SINK(self, plan, rows, pyr, feats.element_size(), list(op_ms))
        N.check(rc, "pbn_unet_forward")
        out = self._output_rows(plan, arena, offs, rows[0], dt)
        if sv is not None:                                 # rows are in Z-order: external row i = out[inv_perm[i]]
            return ME.SparseTensor._from_stored_rows(out, sv.inv_perm, cm)
        return ME.SparseTensor(out, coordinate_manager=cm, tensor_stride=1)

    def _forward_fused_py(self, x):
        """The fused forward issued from Python: walk_body with real tensors -- torch allocates the slabs, every op is one
        _cbr / spconv_forward launch, no pbn_unet_forward, no folded shortcuts.  It shares the walk with _build_plan on purpose:
        what it cross-checks is csrc/executor.hip's sequencing and pointer arithmetic, bit for bit
        (tests/test_backbone_gpu.py::test_unet_matches_golden_and_oracle).  The independent statements of the topology are
        _forward_modules, oracle/sparse_ref.py and the golden files."""
        cm = x.coordinate_manager
        assert x.tensor_stride == 1
        dt, dev = x.F.dtype, x.F.device
        n = [cm.num_rows(1 << l) for l in range(5)]

        def slab(level, up, skip):
            t = torch.empty(n[level], up + skip, dtype=dt, device=dev)
            return t[:, :up], t[:, up:], t

        def conv(conv, bn, map_kind, lin, lout, src, res, out, relu):
            return self._cbr(conv, bn, src, MAP_KINDS[map_kind][2](cm, lin, lout), n[lout], relu=relu, residual=res, out=out)

        cur = walk_body(self, x.F, slab, conv)
        fs = self.final_sematic
        packed = fs._cache.get(fs.kernel, dt)
        out = spconv_forward(cur, None, n[0], packed, shift=_pad_vec(fs.bias, packed[3], 0.0))
        cout = fs.kernel.shape[-1]
        return ME.SparseTensor(out if out.shape[1] == cout else out[:, :cout], coordinate_manager=cm, tensor_stride=1)


def input_slab(feats, cin_p, perm=None, perm2=None, n=None, n_dev=None):
    """Input rows -> the slab the native executors read: row i = feats[perm2[perm[i]]] (either index None = identity) in cin_p
    zero-padded columns (whole 16-byte vectors) at a 16-byte-aligned address; n / n_dev as stage_ops.gather_pad_rows.  Rows
    that already have that form pass through: the test is width == cin_p, for cin_p is the first convolution's input width
    rounded up to whole vectors (_build_plan, train_engine.TrainPlan) and x.F carries exactly that width -- a wider row cannot
    occur.  Otherwise one launch pads and permutes; rows it cannot address (not 4-byte granular) take torch ops."""
    es, width = feats.element_size(), int(feats.shape[1])
    assert width <= cin_p, "input rows of %d channels for a network of at most %d" % (width, cin_p)
    if perm is None and n_dev is None and width == cin_p and feats.stride(1) == 1 and (feats.stride(0) * es) % 16 == 0 \
            and feats.data_ptr() % 16 == 0:
        return feats
    if feats.stride(1) == 1 and (width * es) % 4 == 0 and (feats.stride(0) * es) % 4 == 0 and feats.data_ptr() % 4 == 0:
        return stage_ops.gather_pad_rows(feats, cin_p, perm, perm2, n, n_dev)
    assert perm2 is None and n_dev is None, "rows the padding launch cannot address have no capacity form"
    padded = torch.zeros(feats.shape[0], cin_p, dtype=feats.dtype, device=feats.device)
    padded[:, :width] = feats if perm is None else feats[perm]
    return padded


def alloc_arena(bufs, n_bufs, rows, dtype, device):
    """The activation arena of a plan's buffers for `rows` per level: (arena, nbytes, byte offsets of the buffers, rows as int32[5])."""
    n_rows = (ctypes.c_int32 * 5)(*[int(v) for v in rows])
    offs = (ctypes.c_int64 * n_bufs)()
    nbytes = N.lib().pbn_unet_arena_bytes(bufs, n_bufs, n_rows, N.DT[dtype], offs)
    return torch.empty(max(nbytes, 16), dtype=torch.uint8, device=device), nbytes, offs, n_rows


def arena_rows(arena, offset, n, width, dtype):
    """View of one arena buffer as [n, width] rows."""
    return arena[offset:offset + n * width * torch.empty(0, dtype=dtype).element_size()].view(dtype).view(n, width)


def _variant(name):
    def init(self, in_channels, out_channels, D=3):
        MinkUNet.__init__(self, in_channels, out_channels, D, arch=name)
    return type(name, (MinkUNet,), {"__init__": init})


for _n in SPECS:
    globals()[_n] = _variant(_n)


def Mink_unet(in_channels=3, out_channels=20, D=3, arch="MinkUNet18A"):
    """Factory with the reference's signature (Mink.py:502-526)."""
    if arch not in SPECS:
        raise Exception("architecture not supported yet: {}".format(arch))
    return globals()[arch](in_channels, out_channels, D)
