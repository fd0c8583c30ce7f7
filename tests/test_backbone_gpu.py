"""GPU tier: sparse-voxel backbone (coords.hip + spconv.hip through the C ABI) against the CPU oracle
(oracle/sparse_ref.py) and the committed golden fixtures.  Tolerance: 1e-4 absolute on fp32 features
(BASELINE.json north_star); bf16/f16 slabs of single convolutions are checked per element against the float64 result of the
same rounded operands: |got - ref| <= ulp_T(ref) + 2^-20 S (tests/conv_exact.py)."""
import os

import numpy as np
import pytest
import torch

from oracle import sparse_ref as R
import pbnet_amd.MinkowskiEngine as ME
from pbnet_amd import synth
from pbnet_amd.network.Mink import Mink_unet
import conv_exact as X

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-4          # ABSOLUTE, on fp32 features (BASELINE.json north_star) -- no scaling by the magnitude of the output


def _close(got, want, what, tol=TOL):
    """max |got - want| <= tol in absolute terms; prints the observed figure (pytest -s / failure reports)."""
    err = (got.float() - want.float()).abs().max().item()
    print("%s: max |diff| %.3e (|want| max %.2f, tol %.1e abs)" % (what, err, want.abs().max().item(), tol))
    assert err <= tol, "%s: max |diff| %.3e > %.1e" % (what, err, tol)


def _check16(got, want64, dtype, what):
    """16-bit slabs: one rounding to T plus fp32 accumulation, per element (tests/conv_exact.py)."""
    worst = X.check_bounded(got.cpu(), want64[0], want64[1], dtype, what)
    print("%s: worst err / (ulp + 2^-20 S) %.3f" % (what, worst))


def _scene_coords(seed, room=(0.6, 0.5, 0.4), n_boxes=1, batch=2):
    sc = synth.synth_room(seed=seed, pitch=0.0225, room=room, n_boxes=n_boxes)
    q, _, _ = synth.voxelize_numpy(sc["xyz"], 0.02)
    parts = []
    for b in range(batch):
        c = np.concatenate([np.full((len(q), 1), b, np.int32), q + np.array([5 * b, -3 * b, b], np.int32)], 1)
        parts.append(c[: len(c) if b == 0 else len(c) // 2])
    return np.concatenate(parts, 0).astype(np.int32)


def test_coordinate_pyramid_matches_oracle():
    coords = _scene_coords(41)
    cm_ref = R.CoordinateManager(coords)
    cm = ME.CoordinateManager(torch.from_numpy(coords).to(DEV))
    for s in (1, 2, 4, 8, 16):
        want = cm_ref.get_coords(s)
        got = cm.coordinates(s).cpu().numpy()
        assert got.shape == want.shape
        assert np.array_equal(got, want), "stride %d coordinates / first-occurrence order" % s
    # kernel maps: same (in,out) pair sets as the oracle's per-offset maps
    for s, k in ((1, 3), (2, 3), (8, 3), (1, 5)):
        nbr = cm.kernel_map(s, k).cpu().numpy()
        maps = cm_ref.get_map(s, s, k)
        assert nbr.shape[1] == k ** 3
        for kk, (in_rows, out_rows) in enumerate(maps):
            col = nbr[:, kk]
            assert np.array_equal(np.nonzero(col >= 0)[0], out_rows)
            assert np.array_equal(col[out_rows], in_rows)
    # strided maps: every fine row appears exactly once in its parent's child table at its own k
    for s in (1, 2, 4, 8):
        down = cm.down_map(s).cpu().numpy()
        up = cm.up_map(2 * s).cpu().numpy()
        maps = cm_ref.get_map(s, 2 * s, 2)
        for kk, (fine_rows, coarse_rows) in enumerate(maps):
            assert np.array_equal(down[coarse_rows, kk], fine_rows)
            assert np.array_equal(up[fine_rows, kk], coarse_rows)
        assert (up >= 0).sum() == cm.num_rows(s) and (down >= 0).sum() == cm.num_rows(s)


def test_duplicate_coordinates_first_occurrence():
    """B5: ME.SparseTensor dedupe + inverse_mapping (PBNet.py:240-247) and sparse_quantize."""
    rng = np.random.default_rng(0)
    base = rng.integers(-20, 20, (500, 3)).astype(np.int32)
    coords = np.concatenate([np.zeros((1500, 1), np.int32), base[rng.integers(0, 500, 1500)]], 1)
    feats = torch.randn(1500, 8)
    st = ME.SparseTensor(feats, torch.from_numpy(coords), device=DEV)
    f_ref, c_ref, inv_ref = R.sparse_tensor(feats, coords)
    assert np.array_equal(st.C.cpu().numpy(), c_ref)
    assert torch.equal(st.F.cpu(), f_ref)
    assert torch.equal(st.inverse_mapping.cpu(), inv_ref)
    # unique input keeps its order
    st2 = ME.SparseTensor(f_ref, torch.from_numpy(c_ref), device=DEV)
    assert np.array_equal(st2.C.cpu().numpy(), c_ref) and torch.equal(st2.inverse_mapping.cpu(), torch.arange(len(c_ref)))
    # sparse_quantize on raw points (dataset_preprocess.py:269-272)
    xyz = rng.uniform(-1, 3, (4000, 3))
    pf = rng.normal(size=(4000, 6)).astype(np.float32)
    qc, qf, idx, inv = ME.utils.sparse_quantize(xyz, pf, quantization_size=0.02, return_index=True, return_inverse=True)
    rc, rf, ridx, rinv = R.sparse_quantize(xyz, pf, 0.02)
    assert np.array_equal(qc, rc) and np.array_equal(qf, rf) and np.array_equal(idx, ridx) and np.array_equal(inv, rinv)
    # out-of-range coordinates are reported, not wrapped
    bad = torch.tensor([[0, 0, 0, 0], [0, 40000, 0, 0]], dtype=torch.int32)
    with pytest.raises(ValueError):
        ME.SparseTensor(torch.zeros(2, 4), bad, device=DEV)
    # the inference constructor (one native call: de-duplication + Z-order + pyramid, pbn_coords_prepare) must agree
    with torch.no_grad():
        st3 = ME.SparseTensor(feats, torch.from_numpy(coords), device=DEV)
        assert st3.coordinate_manager._native is not None
        assert np.array_equal(st3.C.cpu().numpy(), c_ref)
        assert torch.equal(st3.F.cpu(), f_ref)
        assert torch.equal(st3.inverse_mapping.cpu(), inv_ref)
        sv = st3.coordinate_manager.sorted()
        assert torch.equal(sv.inv_perm[sv.perm].cpu(), torch.arange(len(c_ref)))
        assert np.array_equal(sv.pyramid.coordinates(1).cpu().numpy(), c_ref[sv.perm.cpu().numpy()])
        for s_ in (2, 4, 8, 16):      # coarser levels hold the same voxel sets as the external-order pyramid
            a = {tuple(r) for r in sv.pyramid.coordinates(s_).cpu().numpy().tolist()}
            b = {tuple(r) for r in st.coordinate_manager.coordinates(s_).cpu().numpy().tolist()}
            assert a == b
        with pytest.raises(ValueError):
            ME.SparseTensor(torch.zeros(2, 4), bad, device=DEV)


@pytest.mark.parametrize("dtype,tol", [(torch.float32, TOL), (torch.bfloat16, 6e-2), (torch.float16, 1e-2)])
@pytest.mark.parametrize("cin,cout,k", [(32, 32, 3), (6, 32, 5), (96, 96, 3), (128, 256, 3), (384, 256, 3), (34, 32, 5),
                                        (256, 256, 1), (32, 16, 1), (16, 20, 1)])
def test_single_convolution(dtype, tol, cin, cout, k):
    """B1: one convolution = oracle gather-mm-index_add (both kernel tile shapes)."""
    coords = _scene_coords(43, batch=1)
    torch.manual_seed(cin * 1000 + cout + k)
    feats = torch.randn(len(coords), cin)
    conv = ME.MinkowskiConvolution(cin, cout, kernel_size=k, bias=(k == 1), dimension=3)
    cm_ref = R.CoordinateManager(coords)
    want = R.conv(feats, conv.kernel.detach(), None if k == 1 else cm_ref.get_map(1, 1, k), len(coords),
                  bias=conv.bias.detach() if conv.bias is not None else None)
    conv = conv.to(DEV)
    x = ME.SparseTensor(feats.to(dtype), torch.from_numpy(coords), device=DEV)
    with torch.no_grad():
        got = conv(x).F.float().cpu()
    assert got.shape == want.shape
    # fp32 slabs: the parity bar, absolute 1e-4; bf16 / f16 slabs: per element against float64 on the rounded operands
    if dtype == torch.float32:
        _close(got, want, "conv %d->%d k=%d %s" % (cin, cout, k, dtype), tol)
    else:
        q = (lambda t: t.to(dtype).float())
        want64 = X.oracle_reference(q(feats), q(conv.kernel.detach().cpu()), None if k == 1 else cm_ref.get_map(1, 1, k),
                                    len(coords), shift=None if conv.bias is None else conv.bias.detach().cpu().reshape(-1))
        _check16(got, want64, dtype, "conv %d->%d k=%d %s" % (cin, cout, k, dtype))
    if dtype == torch.float32 and k == 3:
        # explicit tile shapes: 16 and 32 rows per wave
        from pbnet_amd.MinkowskiEngine.conv import spconv_forward
        packed = conv._cache.get(conv.kernel, dtype)
        nbr = x.coordinate_manager.kernel_map(1, 3)
        for rw in (16, 32):
            o = spconv_forward(x.F, nbr, len(coords), packed, rows_per_wave=rw)[:, :cout].cpu()
            _close(o, want, "rows_per_wave=%d" % rw)


def test_down_up_round_trip():
    """B2: k2s2 down then transposed up lands on the original coordinates; values equal the oracle's."""
    coords = _scene_coords(44)
    torch.manual_seed(3)
    feats = torch.randn(len(coords), 32)
    down = ME.MinkowskiConvolution(32, 64, kernel_size=2, stride=2, dimension=3)
    up = ME.MinkowskiConvolutionTranspose(64, 32, kernel_size=2, stride=2, dimension=3)
    cm_ref = R.CoordinateManager(coords)
    m = cm_ref.get_map(1, 2, 2)
    mid = R.conv(feats, down.kernel.detach(), m, cm_ref.get_coords(2).shape[0])
    want = R.conv_transpose(mid, up.kernel.detach(), m, len(coords))
    x = ME.SparseTensor(feats, torch.from_numpy(coords), device=DEV)
    with torch.no_grad():
        y = down.to(DEV)(x)
        z = up.to(DEV)(y)
    assert y.tensor_stride == 2 and z.tensor_stride == 1
    _close(y.F.cpu(), mid, "k2s2 down")
    _close(z.F.cpu(), want, "k2s2 transposed up")
    assert np.array_equal(z.C.cpu().numpy(), coords)


@pytest.mark.parametrize("arch", ["MinkUNet14A", "MinkUNet34C"])
def test_unet_matches_golden_and_oracle(arch, golden_dir):
    """B3/B4: whole U-Net, seeded weights, eval-mode BN (fused and module paths) and train-mode BN (module path)."""
    import sys
    sys.path.insert(0, golden_dir)
    import make_backbone_golden as G
    g = dict(np.load(os.path.join(golden_dir, "backbone_%s.npz" % arch)))
    cin = g["feats"].shape[1]
    m = G.build(arch, cin)
    feats = torch.from_numpy(g["feats"])
    coords = g["coords"]
    same_torch = str(g["torch_version"]) == torch.__version__
    want_eval = torch.from_numpy(g["out_eval"]) if same_torch else R.minkunet_forward(m.state_dict(), arch, feats, coords)
    want_train = (torch.from_numpy(g["out_train"]) if same_torch
                  else R.minkunet_forward(m.state_dict(), arch, feats, coords, training=True))
    m = m.to(DEV)
    x = ME.SparseTensor(feats, torch.from_numpy(coords), device=DEV)
    # level sizes and rule-pair counts
    cm = x.coordinate_manager
    assert [cm.num_rows(s) for s in (1, 2, 4, 8, 16)] == g["counts"].tolist()
    assert [int((cm.kernel_map(s, 3) >= 0).sum().item()) for s in (1, 2, 4, 8, 16)] == g["pairs"].tolist()
    m.eval()
    with torch.no_grad():
        fused = m(x).F.cpu()
        fused_py = m._forward_fused_py(x).F.cpu()  # same plan issued launch by launch from Python
        m.FUSE_EVAL = False
        unfused = m(x).F.cpu()
        m.FUSE_EVAL = True
    # Z-order changes which tiles split their reduction (split-K slices), not what is summed: same values up to fp32
    # re-association; with the external row order the native executor is bit-identical to the Python-issued plan
    _close(fused, fused_py, "Z-order vs external-order fused path", 1e-5)
    with torch.no_grad():
        type(m).MORTON = False
        fused_plain = m(x).F.cpu()
        # the Python-issued plan launches the 1x1 shortcuts separately: bit-identity holds against the executor doing the same
        from pbnet_amd.network import mink_unet as U_
        U_.MinkUNet.FOLD_SHORTCUT = False
        m._plans.clear()
        fused_plain_sep = m(x).F.cpu()
        U_.MinkUNet.FOLD_SHORTCUT = True
        m._plans.clear()
        type(m).MORTON = True
    assert torch.equal(fused_plain_sep, fused_py), "native executor and Python-issued fused path must be bit-identical"
    _close(fused_plain, fused_py, "shortcuts folded into the second convolutions vs separate launches", 1e-5)
    _close(fused, want_eval, arch + " fused eval path")
    _close(unfused, want_eval, arch + " module eval path")
    m.train()
    with torch.no_grad():
        tr = m(x).F.cpu()
    _close(tr, want_train, arch + " train-mode BN")
    # reduced precision slabs stay close to the fp32 result (sanity, not the parity bar)
    m.eval()
    with torch.no_grad():
        xb = ME.SparseTensor(feats.to(torch.bfloat16), torch.from_numpy(coords), device=DEV)
        ob = m(xb).F.float().cpu()
    rel = (ob - want_eval).norm() / want_eval.norm()
    assert rel < 0.05, "bf16 relative error %.4f" % rel


def test_linear_heads_and_pooling():
    """PBNet.py:43-82,274-276: MinkowskiLinear / BN / PReLU / Sigmoid / Softmax on .F, global avg + max pooling."""
    coords = _scene_coords(45, batch=3)
    torch.manual_seed(5)
    feats = torch.randn(len(coords), 32)
    head = torch.nn.Sequential(ME.MinkowskiLinear(32, 16, bias=False), ME.MinkowskiBatchNorm(16), ME.MinkowskiPReLU(),
                               ME.MinkowskiLinear(16, 20, bias=True))
    head.eval()
    lin0, bn, pr, lin1 = head[0].linear, head[1].bn, head[2].module, head[3].linear
    with torch.no_grad():
        want = lin1(pr(bn(lin0(feats))))
        want_sm = torch.softmax(want, 1)
    head = head.to(DEV)
    x = ME.SparseTensor(feats, torch.from_numpy(coords), device=DEV)
    with torch.no_grad():
        y = head(x)
        sm = ME.MinkowskiSoftmax()(y)
        avg = ME.MinkowskiGlobalAvgPooling()(y)
        mx = ME.MinkowskiGlobalMaxPooling()(y)
    _close(y.F.cpu(), want, "linear head")
    _close(sm.F.cpu(), want_sm, "softmax")
    b = coords[:, 0]
    _close(avg.F.cpu(), R.global_pool(want, b, 3, "avg"), "global avg pool")
    _close(mx.F.cpu(), R.global_pool(want, b, 3, "max"), "global max pool")
    assert ((mx + avg).F.cpu() - (R.global_pool(want, b, 3, "avg") + R.global_pool(want, b, 3, "max"))).abs().max() <= 1e-3


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_segment_pool_long_and_ragged_segments(dtype):
    """Score-branch pooling (PBNet.py:274-276) at proposal-sized segments: one long, several short, one empty; the
    two-pass kernel must agree with a per-segment fp32 reduction and be run-to-run identical."""
    from pbnet_amd.MinkowskiEngine.nn import segment_pool
    torch.manual_seed(9)
    lens = [20011, 3, 0, 777, 1, 4096, 130]
    feats = torch.randn(sum(lens), 32).to(dtype)
    batch = torch.repeat_interleave(torch.arange(len(lens)), torch.tensor(lens)).to(torch.int32)
    mx, av = segment_pool(feats.to(DEV), batch.to(DEV), len(lens))
    mx2, av2 = segment_pool(feats.to(DEV), batch.to(DEV), len(lens))
    assert torch.equal(mx, mx2) and torch.equal(av.nan_to_num(), av2.nan_to_num())
    f32 = feats.float()
    o = 0
    for i, n in enumerate(lens):
        seg = f32[o:o + n]
        o += n
        if n == 0:
            assert torch.isinf(mx[i]).all() and torch.isnan(av[i]).all()
            continue
        assert torch.equal(mx[i].cpu(), seg.max(0)[0])
        assert (av[i].cpu() - seg.double().mean(0).float()).abs().max().item() <= 1e-5


def test_full_size_scene_linearity_and_determinism():
    """BASELINE configs[1] size (145k voxels): convolution is linear in its input, independent of row-tile shape,
    and bit-reproducible run to run (fixed summation order)."""
    sc = synth.synth_room(seed=2, pitch=0.0225, room=(4.0, 3.2, 2.6), n_boxes=12)
    q, _, _ = synth.voxelize_numpy(sc["xyz"], 0.02)
    coords = np.concatenate([np.zeros((len(q), 1), np.int32), q], 1).astype(np.int32)
    assert len(coords) > 140000
    torch.manual_seed(0)
    conv = ME.MinkowskiConvolution(96, 96, kernel_size=3, dimension=3).to(DEV)
    a = torch.randn(len(coords), 96, device=DEV)
    b = torch.randn(len(coords), 96, device=DEV)
    x = ME.SparseTensor(a, torch.from_numpy(coords), device=DEV)
    with torch.no_grad():
        ya = conv(x).F
        yb = conv(x.replace_feature(b)).F
        yab = conv(x.replace_feature(a + 2 * b)).F
        ya2 = conv(x).F
    assert torch.equal(ya, ya2)
    assert (yab - (ya + 2 * yb)).abs().max().item() < 1e-3
    nbr = x.coordinate_manager.kernel_map(1, 3)
    pairs = int((nbr >= 0).sum().item())
    assert 6.0 < pairs / len(coords) < 8.5
    # spot-check 2000 random rows against a direct gather on the GPU tensors
    rows = torch.randint(0, len(coords), (2000,), device=DEV)
    nb = nbr[rows].long()
    ref = torch.zeros(2000, 96, device=DEV, dtype=torch.float64)
    for k in range(27):
        valid = nb[:, k] >= 0
        ref[valid] += a[nb[valid, k]].double() @ conv.kernel[k].double()
    assert (ya[rows].double() - ref).abs().max().item() < 1e-4


def test_loader_voxelize_batch_matches_per_scene_quantize_and_collate():
    """dataset_preprocess.py:345-375 ('Voxel and Batch' of valMerge): one batched device de-duplication == per-scene
    sparse_quantize + v2p offsets + sparse_collate (oracle restatement of the ME rules, fixture B5)."""
    from pbnet_amd import loader_ops
    rng = np.random.default_rng(11)
    xyz_list = [rng.uniform(-1, 3, (n, 3)) for n in (4000, 2500, 3300)]
    feat_list = [rng.normal(size=(len(x), 6)).astype(np.float32) for x in xyz_list]
    xv, fv, v2p = loader_ops.voxelize_batch(xyz_list, feat_list, 0.02, device=DEV)
    want_c, want_f, want_v2p, total = [], [], [], 0
    for b, (x, f) in enumerate(zip(xyz_list, feat_list)):
        qc, qf, idx, inv = R.sparse_quantize(x, f, 0.02)
        want_c.append(np.concatenate([np.full((len(qc), 1), b, np.int32), qc.astype(np.int32)], 1))
        want_f.append(qf)
        want_v2p.append(inv + total)
        total += len(qc)
    assert np.array_equal(xv.cpu().numpy(), np.concatenate(want_c))
    assert np.array_equal(fv.cpu().numpy(), np.concatenate(want_f))
    assert np.array_equal(v2p.cpu().numpy(), np.concatenate(want_v2p))


def _brute_kernel_map(coords, stride, k):
    """nbr[row, kk] by dictionary lookup, ME conventions (x fastest, odd kernels centred, even not)."""
    index = {tuple(c): i for i, c in enumerate(coords.tolist())}
    c0 = k // 2 if k % 2 else 0
    out = np.full((len(coords), k ** 3), -1, np.int64)
    for kk in range(k ** 3):
        d = np.array([0, (kk % k - c0) * stride, (kk // k % k - c0) * stride, (kk // (k * k) - c0) * stride])
        for i, c in enumerate(coords):
            out[i, kk] = index.get(tuple((c + d).tolist()), -1)
    return out


@pytest.mark.parametrize("mode", ["sorted", "plain"])
def test_kernel_maps_in_z_order_and_external_order(mode):
    """pbn_kernel_map_cube on the Z-ordered lineage and on the external order against a dictionary look-up: every level,
    odd and even kernels, negative coordinates, batch seams, a tensor stride the rows are not multiples of."""
    coords = _scene_coords(43, room=(0.7, 0.6, 0.5), n_boxes=2, batch=3)
    coords[:, 1:] -= np.array([9, 4, 2], np.int32)                    # part of the scene at negative coordinates
    cm = ME.CoordinateManager(torch.from_numpy(coords).to(DEV))
    pyr = cm.sorted().pyramid if mode == "sorted" else cm.plain()
    for s in (1, 2, 4, 8, 16):
        lvl = pyr.coordinates(s).cpu().numpy()
        assert (lvl[:, 1:] % s == 0).all()
        for k in ((3, 5) if s == 1 else (3,)):
            got = pyr.kernel_map(s, k).cpu().numpy()
            assert np.array_equal(got, _brute_kernel_map(lvl, s, k)), (mode, s, k)
    # the C entry point on its own: even kernels, and a tensor stride the rows are NOT multiples of; rows in blocked or
    # external order
    from pbnet_amd import _native as N
    lib = N.lib()
    order = np.lexsort((coords[:, 3], coords[:, 2], coords[:, 1], coords[:, 3] >> 3, coords[:, 2] >> 3, coords[:, 1] >> 3,
                        coords[:, 0])) if mode == "sorted" else np.arange(len(coords))
    blocked = np.ascontiguousarray(coords[order])
    p0 = ME.CoordinateManager(torch.from_numpy(blocked).to(DEV)).plain()
    p0.finalize()
    lvl0 = p0.coordinates(1)
    assert np.array_equal(lvl0.cpu().numpy(), blocked)
    n, L = int(lvl0.shape[0]), p0.layout
    for k, stride in ((2, 1), (4, 1), (3, 2), (2, 3)):
        nbr = torch.full((n, k ** 3), -7, dtype=torch.int32, device=DEV)
        N.check(lib.pbn_kernel_map_cube(N.ptr(lvl0), None, n, k, stride, 1, N.c_vp(p0.ptr(L.keys[0])),
                                        N.c_vp(p0.ptr(L.vals[0])), L.capacity[0], N.ptr(nbr), N.current_stream()),
                "pbn_kernel_map_cube")
        assert np.array_equal(nbr.cpu().numpy(), _brute_kernel_map(blocked, stride, k)), (mode, k, stride)


def test_unet_forward_is_graph_capturable_fp16(golden_dir):
    """BASELINE configs[4]: fp16 feature slabs, int32 coordinates, the U-Net forward captured in a HIP graph.  With the
    coordinate pyramid built (its row counts on the host) the fused forward is a fixed sequence of launches on the
    current stream -- no allocation-by-size decision, no read-back -- so it captures, and a replay reproduces the
    eagerly launched result bit for bit; fp16 stays close to the fp32 golden."""
    import sys
    sys.path.insert(0, golden_dir)
    import make_backbone_golden as G
    g = dict(np.load(os.path.join(golden_dir, "backbone_MinkUNet34C.npz")))
    m = G.build("MinkUNet34C", g["feats"].shape[1]).to(DEV).eval()
    x = ME.SparseTensor(torch.from_numpy(g["feats"]).to(torch.float16), torch.from_numpy(g["coords"]), device=DEV)
    assert x.C.dtype == torch.int32
    with torch.no_grad():
        eager = m(x).F.clone()                       # also builds the pyramid, packs the weights, sizes the scratch
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = m(x).F
        for _ in range(3):
            out.zero_()
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(out, eager)
    want = torch.from_numpy(g["out_eval"])
    assert ((out.float().cpu() - want).norm() / want.norm()).item() < 5e-3


WAVE_CFGS = (401, 402, 404, 406, 408, 204, 206, 208, 1401, 1402, 1404, 1201, 1202, 1204, 2201, 2202)


@pytest.mark.parametrize("dtype,tol", [(torch.float32, TOL), (torch.bfloat16, 6e-2), (torch.float16, 1e-2)])
@pytest.mark.parametrize("cin,cout,k", [(32, 96, 3), (64, 128, 3), (6, 32, 5), (40, 64, 5), (96, 128, 1), (16, 16, 1)])
def test_wave_family_configurations(dtype, tol, cin, cout, k):
    """Every built configuration of the wave-autonomous family (csrc/spconv_wave.hip: row-split and K-split modes, 16-row
    fragment counts, channel-tile counts) against the oracle on the same convolution, with the full fused epilogue
    (scale, shift, residual, ReLU); run-to-run bit-identical; all configurations agree with each other to fp32
    re-association."""
    from pbnet_amd.MinkowskiEngine.conv import spconv_forward, _pad_vec
    from pbnet_amd import _native as N
    coords = _scene_coords(47, room=(1.0, 0.8, 0.6), batch=1)
    n = len(coords)
    torch.manual_seed(cin * 100 + cout + k)
    feats = torch.randn(n, cin)
    conv = ME.MinkowskiConvolution(cin, cout, kernel_size=k, dimension=3)
    cm_ref = R.CoordinateManager(coords)
    scale, shift = torch.rand(cout) + 0.5, torch.randn(cout) * 0.1
    res = torch.randn(n, cout)
    q = (lambda t: t.to(dtype).float())
    want = R.conv(q(feats), q(conv.kernel.detach()), None if k == 1 else cm_ref.get_map(1, 1, k), n)
    want = torch.relu(want * scale + shift + q(res))
    want64 = X.oracle_reference(q(feats), q(conv.kernel.detach()), None if k == 1 else cm_ref.get_map(1, 1, k), n, scale, shift,
                                q(res), relu=True)
    conv = conv.to(DEV)
    x = ME.SparseTensor(feats.to(dtype), torch.from_numpy(coords), device=DEV)
    packed = conv._cache.get(conv.kernel, dtype)
    cout_p = packed[3]
    nbr = None if k == 1 else x.coordinate_manager.kernel_map(1, k)
    sc, sh = _pad_vec(scale.to(DEV), cout_p, 1.0), _pad_vec(shift.to(DEV), cout_p, 0.0)
    resd = torch.zeros(n, cout_p, dtype=dtype, device=DEV)
    resd[:, :cout] = res.to(dtype).to(DEV)
    ran = 0
    for cfg in WAVE_CFGS:
        nt = cfg % 100
        if (cout_p // 16) % nt:
            continue
        try:
            o1 = spconv_forward(x.F, nbr, n, packed, scale=sc, shift=sh, residual=resd, relu=True, rows_per_wave=cfg)
        except RuntimeError as e:                 # e.g. K = 125 with a 256-row tile: more LDS than a CU has
            assert "UNSUPPORTED" in str(e), e
            continue
        o2 = spconv_forward(x.F, nbr, n, packed, scale=sc, shift=sh, residual=resd, relu=True, rows_per_wave=cfg)
        assert torch.equal(o1, o2), "cfg %d not deterministic" % cfg
        if dtype == torch.float32:
            _close(o1[:, :cout].float().cpu(), want, "wave cfg %d %d->%d k=%d %s" % (cfg, cin, cout, k, dtype), tol)
        else:
            _check16(o1, want64, dtype, "wave cfg %d %d->%d k=%d %s" % (cfg, cin, cout, k, dtype))
        ran += 1
    assert ran >= 3


@pytest.mark.parametrize("dtype,tol", [(torch.float32, TOL), (torch.bfloat16, 6e-2), (torch.float16, 1e-2)])
@pytest.mark.parametrize("cin,cin2,cout", [(64, 32, 64), (96, 128, 96), (128, 192, 128), (256, 384, 256)])
def test_shortcut_folded_into_the_second_convolution(dtype, tol, cin, cin2, cout):
    """pbn_spconv_forward_dual (round 4): relu(bn2(conv2(h)) + bn_d(conv1x1(x))) of a BasicBlock with a shortcut
    (/root/reference/network/Mink.py:77-87,140-160) as ONE convolution over two sources, in every kernel family, against
    the oracle's two convolutions."""
    from pbnet_amd.MinkowskiEngine.conv import spconv_forward_dual, pack_weight, _pad_vec
    from pbnet_amd.network.mink_unet import _group_steps
    coords = _scene_coords(49, room=(1.0, 0.8, 0.6), batch=1)
    n = len(coords)
    torch.manual_seed(cin + cin2 + cout)
    h, x = torch.randn(n, cin), torch.randn(n, cin2)
    k2, kd = torch.randn(27, cin, cout) * (2.0 / (27 * cin)) ** 0.5, torch.randn(1, cin2, cout) * (1.0 / cin2) ** 0.5
    s2, b2, sd, bd = torch.rand(cout) + 0.5, torch.randn(cout) * 0.1, torch.rand(cout) + 0.5, torch.randn(cout) * 0.1
    q = (lambda t: t.to(dtype).float())
    cm_ref = R.CoordinateManager(coords)
    want = torch.relu(R.conv(q(h), q(k2 * s2), cm_ref.get_map(1, 1, 3), n) + b2 + q(x) @ q(kd[0] * sd) + bd)
    want64 = X.oracle_reference(q(h), q(k2 * s2), cm_ref.get_map(1, 1, 3), n, shift=b2 + bd, relu=True, x2=q(x), w2=q(kd[0] * sd))
    st = ME.SparseTensor(torch.zeros(n, 1), torch.from_numpy(coords), device=DEV)
    nbr = st.coordinate_manager.kernel_map(1, 3)
    w2, vpo, n_main, cout_p = pack_weight((k2 * s2).to(DEV), dtype)
    wd, vpo2, n2, _ = pack_weight((kd * sd).to(DEV), dtype)
    pad = (-n2) % _group_steps(vpo // 4)
    w = torch.cat([w2, wd] + ([torch.zeros(pad, *wd.shape[1:], dtype=wd.dtype, device=DEV)] if pad else []), 0).contiguous()
    e = 16 // torch.empty(0, dtype=dtype).element_size()
    hd = torch.zeros(n, vpo * e, dtype=dtype, device=DEV); hd[:, :cin] = h.to(dtype).to(DEV)
    xd = torch.zeros(n, vpo2 * e, dtype=dtype, device=DEV); xd[:, :cin2] = x.to(dtype).to(DEV)
    shift = _pad_vec((b2 + bd).to(DEV), cout_p, 0.0)
    lim = tol if dtype == torch.float32 else tol * max(1.0, want.abs().max().item())
    ran = 0
    for cfg in (0, 16, 32, 64, 401, 402, 404, 406, 408, 204, 206, 208, 1401, 1402, 1404, 1201, 1202, 1204, 1208, 2201, 2202):
        if cfg >= 100 and (cout_p // 16) % (cfg % 100):
            continue
        try:
            o1 = spconv_forward_dual(hd, nbr, n, xd, (w, vpo, n_main + n2 + pad, cout_p), vpo2, shift=shift, relu=True, rows_per_wave=cfg)
        except RuntimeError as ex:
            assert "UNSUPPORTED" in str(ex), ex
            continue
        o2 = spconv_forward_dual(hd, nbr, n, xd, (w, vpo, n_main + n2 + pad, cout_p), vpo2, shift=shift, relu=True, rows_per_wave=cfg)
        assert torch.equal(o1, o2), "cfg %d not deterministic" % cfg
        if dtype == torch.float32:
            _close(o1[:, :cout].float().cpu(), want, "dual cfg %d %d+%d->%d %s" % (cfg, cin, cin2, cout, dtype), lim)
        else:
            _check16(o1, want64, dtype, "dual cfg %d %d+%d->%d %s" % (cfg, cin, cin2, cout, dtype))
        ran += 1
    assert ran >= 5


@pytest.mark.parametrize("arch", ["MinkUNet14A", "MinkUNet34C"])
def test_folded_shortcuts_equal_separate_launches(arch):
    """The fused forward with the 1x1 shortcuts folded (default) against the same network with separate launches: fp32, 1e-4;
    7 convolution launches fewer per network."""
    from pbnet_amd.network import mink_unet as U
    coords = _scene_coords(45, room=(0.9, 0.7, 0.5), batch=2)
    torch.manual_seed(3)
    feats = torch.randn(len(coords), 6)
    net = Mink_unet(6, 20, arch=arch).to(DEV).eval()
    g = torch.Generator().manual_seed(7)
    for mod in net.modules():
        if isinstance(mod, torch.nn.BatchNorm1d):
            mod.running_mean.copy_(torch.randn(mod.num_features, generator=g) * 0.1)
            mod.running_var.copy_(torch.rand(mod.num_features, generator=g) * 0.5 + 0.75)
            mod.weight.data.copy_(torch.rand(mod.num_features, generator=g) + 0.5)
            mod.bias.data.copy_(torch.randn(mod.num_features, generator=g) * 0.1)
    outs, nops = {}, {}
    for fold in (True, False):
        U.MinkUNet.FOLD_SHORTCUT = fold
        try:
            net._plans.clear()
            with torch.no_grad():
                outs[fold] = net(ME.SparseTensor(feats, torch.from_numpy(coords), device=DEV)).F.float().cpu()
            nops[fold] = net._plan(torch.float32)["n_ops"]
        finally:
            U.MinkUNet.FOLD_SHORTCUT = True
    net._plans.clear()
    assert nops[False] - nops[True] == 7, nops
    _close(outs[True], outs[False], "%s folded vs separate shortcuts" % arch)


def test_fold_guard_extreme_batchnorm_statistics():
    """the folded shortcut multiplies BatchNorm scales into 16-bit weights.  With a huge gamma (scale ~1e7) or a
    running variance of 1e12 (scale ~1e-6) the products leave fp16's normal range: the planner must keep such a block on the separate launches (scales in the fp32
    epilogue) -- the fp16 forward stays finite and equals the forward with folding switched off, bit for bit; bf16 keeps folding."""
    from pbnet_amd.network.mink_unet import MinkUNet
    coords = _scene_coords(53, room=(0.8, 0.6, 0.5), batch=1)
    torch.manual_seed(7)
    net = Mink_unet(in_channels=3, out_channels=20, arch="MinkUNet14A").to(DEV).eval()
    blocks = [b for m in net.modules() if hasattr(m, "downsample") and m.downsample is not None for b in [m]]
    assert blocks
    with torch.no_grad():
        for i, blk in enumerate(blocks):
            bn = (blk.norm2 if i % 2 == 0 else blk.downsample[1]).bn
            if i % 4 < 2:
                bn.weight.fill_(3e6)                 # gamma / sqrt(var + eps) ~ 1e9: the scaled weights overflow fp16
                bn.running_var.fill_(1e-2)
            else:
                bn.running_var.fill_(1e12)           # scale ~ 1e-6: the scaled weights are fp16 subnormals
    for blk in blocks:
        assert not net._fold_is_safe(blk, torch.float16)
        assert net._fold_is_safe(blk, torch.bfloat16)
    feats = torch.randn(len(coords), 3) * 1e-3
    x = ME.SparseTensor(feats.to(torch.float16), torch.from_numpy(coords), device=DEV)
    with torch.no_grad():
        a = net(x).F.float()
        old = MinkUNet.FOLD_SHORTCUT
        try:
            MinkUNet.FOLD_SHORTCUT = False
            net._plans.clear()
            b = net(x).F.float()
        finally:
            MinkUNet.FOLD_SHORTCUT = old
            net._plans.clear()
    assert torch.equal(a, b), "guarded blocks must run the separate launches"
