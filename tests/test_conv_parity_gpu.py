"""GPU tier: the three forward convolution families pinned to a float64 reference (tests/conv_exact.py), through the C ABI.

k_spconv (+ its split-K pass k_spconv_reduce, csrc/spconv.hip), k_spconv_wave (csrc/spconv_wave.hip) and k_spconv_rs
(csrc/spconv_rs.hip), in bf16 and fp16 everywhere and in fp32 where an instantiation is built:
  * exact mode (integer-valued operands: every fp32 sum is exact) -- the output must equal RNE_T(float64 reference) bit for
    bit, padding columns included;
  * bounded mode (Gaussian operands) on a subset -- |got - ref| <= ulp_T(ref) + 2^-20 S per element;
  * every launch writes into a strided view of a sentinel-filled buffer (rows past the count, columns either side): nothing
    outside the rows written x cout_p columns may change;
  * every launch runs twice: bit-identical.
Each family must actually run a minimum number of configurations (PBN_ERR_UNSUPPORTED everywhere fails).  Run with -s for
the per-case lines: family, configuration, dtype, rows, and the worst bounded-mode err / bound."""
import numpy as np
import pytest
import torch

import conv_exact as X
from oracle import sparse_ref as R
import pbnet_amd.MinkowskiEngine as ME
from pbnet_amd import _native as N
from pbnet_amd import synth
from pbnet_amd.MinkowskiEngine.conv import _DT, _ELEMS, _pad_vec, _vpo, _workspace, pack_weight
from pbnet_amd.network.mink_unet import INIT_DIM, SPECS, _group_steps

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = (torch.bfloat16, torch.float16, torch.float32)
WAVE_CFGS = (401, 402, 404, 406, 408, 204, 206, 208, 1401, 1402, 1404, 1201, 1202, 1204, 1208, 1408, 2201, 2202)
RS_PAIRS = {(2, 1): (32, 32), (2, 2): (64, 32), (4, 1): (32, 64), (4, 2): (64, 64), (6, 3): (96, 96), (6, 4): (128, 96),
            (8, 2): (64, 128), (8, 3): (192, 128), (8, 4): (128, 128)}          # (nt, cg) -> (cin, cout) in 16-bit slabs
UNSUPPORTED = "UNSUPPORTED"
_WORST = {}                                   # family -> worst bounded-mode err / bound seen in this process


def rs_cfg(nf, tile_rows=0):
    """rows_per_wave code of an explicit row-stationary configuration (include/pbnet_hip.h)."""
    return 10000 + 2000 + nf + 100000 * (tile_rows // 16)


def rs_nf_max(nt, cg):
    """csrc/spconv_rs.hip: fragments per wave an instantiation is built for."""
    return 3 if nt >= 8 else (4 if (nt == 6 and cg == 4) else 5)


def family_of(cfg):
    if cfg >= 10000:
        return "rs"
    if cfg >= 100:
        return "wave"
    return "tile" if cfg else "auto"


def _coords(seed, room, batch=1):
    sc = synth.synth_room(seed=seed, pitch=0.0225, room=room, n_boxes=1)
    q, _, _ = synth.voxelize_numpy(sc["xyz"], 0.02)
    return np.concatenate([np.concatenate([np.full((len(q), 1), b, np.int32), q], 1) for b in range(batch)], 0).astype(np.int32)


def random_nbr(g, n_out, n_in, K, empty=0.4):
    nbr = torch.randint(0, n_in, (n_out, K), generator=g, dtype=torch.int32)
    nbr[torch.rand(n_out, K, generator=g) < empty] = -1
    return nbr


class Conv(object):
    """One convolution's operands on the device (slabs padded as the ABI wants them) and its float64 reference."""

    def __init__(self, dtype, nbr, n_in, cin, cout, mode="exact", seed=0, relu=False, cin2=0, identity=False, epilogue=True):
        self.dtype, self.mode, self.relu, self.cin, self.cout, self.cin2 = dtype, mode, relu, cin, cout, cin2
        n_out, K = nbr.shape
        self.n_in, self.n_out, self.K = n_in, n_out, K
        g = torch.Generator().manual_seed(seed)
        op = (X.exact_operands(g, n_in, cin, K, cout, n_out, dtype, cin2=cin2) if mode == "exact"
              else X.gaussian_operands(g, n_in, cin, K, cout, n_out, dtype, cin2=cin2))
        if not epilogue:
            op["scale"] = op["shift"] = op["res"] = None
        self.op = {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in op.items()}
        op = self.op
        self.nbr = None if identity else nbr.to(DEV).int().contiguous()
        nbr_ref = torch.arange(n_out, device=DEV, dtype=torch.int32)[:, None] if identity else self.nbr
        self.ref, self.S = X.reference(op["x"], op["w"], nbr_ref, op["scale"], op["shift"], op["res"], relu,
                                       op.get("x2"), op.get("w2"))
        if mode == "exact":
            X.assert_exact_premise(dtype, op["x"], op["w"], op["w_unit"], op["scale"], op["shift"], op["res"], self.ref, self.S,
                                   op.get("x2"), op.get("w2"))
        w, self.vpo, n_main, self.cout_p = pack_weight(op["w"], dtype)
        e = _ELEMS[dtype]
        self.xs = torch.zeros(n_in, self.vpo * e, dtype=dtype, device=DEV)
        self.xs[:, :cin] = op["x"].to(dtype)
        self.n_steps, self.w = n_main, w
        if cin2:
            wd, self.vpo2, n2, _ = pack_weight(op["w2"][None], dtype)
            pad = (-n2) % _group_steps(self.vpo // 4)
            self.w = torch.cat([w, wd] + ([torch.zeros(pad, *wd.shape[1:], dtype=dtype, device=DEV)] if pad else []), 0).contiguous()
            self.n_steps = n_main + n2 + pad
            self.x2s = torch.zeros(n_out, self.vpo2 * e, dtype=dtype, device=DEV)
            self.x2s[:, :cin2] = op["x2"].to(dtype)
        self.sc = None if op["scale"] is None else _pad_vec(op["scale"], self.cout_p, 1.0)
        self.sh = None if op["shift"] is None else _pad_vec(op["shift"], self.cout_p, 0.0)
        self.res = None
        if op["res"] is not None:
            self.res = torch.zeros(n_out, self.cout_p, dtype=dtype, device=DEV)
            self.res[:, :cout] = op["res"].to(dtype)

    def family(self):
        return int(N.lib().pbn_spconv_family(self.n_out, self.K, self.vpo, self.n_steps, self.cout_p, _DT[self.dtype],
                                             int(self.nbr is not None)))

    def launch(self, cfg, out, row_perm=None, count=None, ws=True):
        wsb = _workspace(torch.device(DEV)) if ws else None
        n_dev = None if count is None else torch.tensor([count], dtype=torch.int32, device=DEV)
        vp = lambda t: None if t is None else N.c_vp(t.data_ptr())
        common = (vp(self.w), self.vpo, self.n_steps, self.cout_p, vp(self.sc), vp(self.sh), vp(self.res),
                  0 if self.res is None else self.res.stride(0), int(self.relu), vp(out), out.stride(0), _DT[self.dtype], cfg,
                  vp(wsb), 0 if wsb is None else wsb.numel())
        if self.cin2:
            assert row_perm is None
            rc = N.lib().pbn_spconv_forward_dual(vp(self.xs), self.xs.stride(0), self.n_in, vp(self.nbr), self.K, vp(n_dev),
                                                 self.n_out, *common, vp(self.x2s), self.x2s.stride(0), self.n_out, self.vpo2,
                                                 N.current_stream())
        else:
            rc = N.lib().pbn_spconv_forward(vp(self.xs), self.xs.stride(0), self.n_in, vp(self.nbr), self.K, vp(row_perm),
                                            vp(n_dev), self.n_out, *common, N.current_stream())
        torch.cuda.synchronize()
        return rc

    def run(self, cfg, label="", row_perm=None, count=None, ws=True):
        """Launch twice into sentinel buffers and check everything; True when it ran, False when UNSUPPORTED."""
        what = "%-5s cfg %-7d %-14s %-8s rows %6d%s%s%s %s" % (
            family_of(cfg), cfg, "%d%s->%d k%d" % (self.cin, "+%d" % self.cin2 if self.cin2 else "", self.cout, self.K),
            str(self.dtype).replace("torch.", ""), self.n_out, "" if count is None else " count %d" % count,
            " perm" if row_perm is not None else "", "" if ws else " ws=0", label)
        outs = []
        for _ in range(2):
            o = X.SentinelOut(self.n_out, self.cout_p, self.dtype, DEV)
            rc = self.launch(cfg, o.view, row_perm, count, ws)
            if rc == N.PBN_ERR_UNSUPPORTED:
                print("%s: UNSUPPORTED" % what)
                return False
            N.check(rc, what)
            outs.append(o)
        a, b = outs
        assert torch.equal(a.buf.view(torch.int16 if self.dtype != torch.float32 else torch.int32),
                           b.buf.view(torch.int16 if self.dtype != torch.float32 else torch.int32)), "%s: not deterministic" % what
        n = self.n_out if count is None else count
        rows = torch.arange(n, device=DEV) if row_perm is None else row_perm[:n].long()
        a.check(rows if row_perm is not None else n, what)
        got = a.view[rows]
        if self.mode == "exact":
            X.check_exact(got, self.ref[rows], self.dtype, what)
            print("%s: exact, 0 mismatches" % what)
        else:
            worst = X.check_bounded(got, self.ref[rows], self.S[rows], self.dtype, what)
            fam = family_of(cfg)
            _WORST[fam] = max(_WORST.get(fam, 0.0), worst)
            print("%s: bounded, worst err/bound %.3f" % (what, worst))
        return True


def _geo(room, seed, k, batch=1):
    """A scene's coordinates and its k^3 map on the device (the production map builder, checked against the oracle elsewhere)."""
    coords = _coords(seed, room, batch)
    cm = ME.CoordinateManager(torch.from_numpy(coords).to(DEV))
    return cm, cm.kernel_map(1, k)


@pytest.fixture(scope="module")
def scene():
    return _geo((1.0, 0.8, 0.6), 47, 3)


def test_gpu_reference_statement_equals_the_oracle():
    """The device-side float64 statement against R.conv on the CPU (the oracle's maps) on one small scene."""
    coords = _coords(52, (0.5, 0.4, 0.3))
    cm_ref = R.CoordinateManager(coords)
    maps = cm_ref.get_map(1, 1, 3)
    nbr = X.maps_to_nbr(maps, len(coords))
    g = torch.Generator().manual_seed(0)
    x, w = torch.randn(len(coords), 40, generator=g).double(), torch.randn(27, 40, 24, generator=g).double()
    ref, S = X.reference(x.to(DEV), w.to(DEV), nbr.to(DEV))
    want = R.conv(x, w, maps, len(coords))
    assert torch.allclose(ref.cpu(), want, rtol=0, atol=1e-12 * float(S.max()))


# ---- k_spconv (workgroup tiles) and k_spconv_reduce (split-K) -----------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
def test_tile_family(dtype, scene):
    """rows_per_wave 16 / 32 / 64 (NF 1 / 2 / 4) x channel-tile counts NT 8 / 6 / 4 / 2 / 1; with and without the split-K
    workspace; one bounded-mode pass per shape."""
    cm, nbr = scene
    n = nbr.shape[0]
    ran = 0
    for cin, cout in ((96, 128), (64, 96), (32, 64), (96, 32), (40, 16), (34, 48), (32, 80)):
        c = Conv(dtype, nbr, n, cin, cout, seed=cin + cout)
        for rpw in (16, 32, 64):
            for ws in (True, False):
                ran += c.run(rpw, ws=ws)
        cb = Conv(dtype, nbr, n, cin, cout, mode="bounded", relu=True, seed=cin + cout)
        ran += cb.run(32)
    assert ran >= 7 * 7


@pytest.mark.parametrize("dtype", DTYPES)
def test_split_k_deep_reductions(dtype):
    """Few rows, deep reductions: the split-K launch (fp32 partial slabs + k_spconv_reduce) and the single-pass launch must
    both be exact, also under a device-side row count (k_spconv_reduce reads it) and a processing order."""
    g = torch.Generator().manual_seed(5)
    ran = 0
    for n, cin in ((300, 256), (1100, 384), (3000, 256)):
        nbr = random_nbr(g, n, n + 57, 27, empty=0.5)
        c = Conv(dtype, nbr, n + 57, cin, 256, seed=n)
        for rpw in (16, 32):
            ran += c.run(rpw, ws=True) + c.run(rpw, ws=False)
            ran += c.run(rpw, count=n // 3, ws=True) + c.run(rpw, count=0, ws=True)
            perm = torch.randperm(n, generator=g).int().to(DEV)
            ran += c.run(rpw, row_perm=perm, ws=True) + c.run(rpw, row_perm=perm, count=n - 5, ws=True)
        cb = Conv(dtype, nbr, n + 57, cin, 256, mode="bounded", relu=True, seed=n)
        ran += cb.run(16, ws=True) + cb.run(16, ws=False)
    assert ran == 3 * 14


# ---- k_spconv_wave ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
def test_wave_family(dtype):
    """Every code in WAVE_CFGS (row-split, K-split, K-split over the populated steps) on k = 1, 3, 5 and the k2s2 down /
    transposed-up maps."""
    cm, nbr3 = _geo((1.0, 0.8, 0.6), 48, 3)
    n = nbr3.shape[0]
    cases = [("k3", nbr3, n, 32, 96), ("k3", nbr3, n, 64, 128), ("k5", cm.kernel_map(1, 5), n, 6, 32),
             ("k5", cm.kernel_map(1, 5), n, 40, 64), ("k1", None, n, 96, 128), ("k1", None, n, 16, 16),
             ("down", cm.down_map(1), cm.num_rows(1), 96, 96), ("up", cm.up_map(2), cm.num_rows(2), 64, 32)]
    ran = {}
    for kind, nbr, n_in, cin, cout in cases:
        ident = nbr is None
        t = torch.arange(n, dtype=torch.int32)[:, None] if ident else nbr
        c = Conv(dtype, t, n_in, cin, cout, seed=cin * 7 + cout, identity=ident)
        for cfg in WAVE_CFGS:
            if (c.cout_p // 16) % (cfg % 100):
                continue
            ok = c.run(cfg, label=kind)
            ran[(kind, cin, cout)] = ran.get((kind, cin, cout), 0) + ok
        cb = Conv(dtype, t, n_in, cin, cout, mode="bounded", relu=True, seed=cin, identity=ident)
        cb.run(1202, label=kind)
    print("wave configurations run per map: %s" % ran)
    assert all(v >= 3 for v in ran.values()) and len(ran) == len(cases)


# ---- k_spconv_rs ----------------------------------------------------------------------------------------------------------

def rs_key(cin, cout, dtype):
    """(nt, cg) of a shape in launch_rs_t: channel tiles, and steps per barrier group (largest divisor <= 4 of vpo / 4)."""
    vpo = _vpo(cin, dtype)
    if vpo % 4:
        return None
    spo = vpo // 4
    return ((cout + 15) // 16, max(c for c in (1, 2, 3, 4) if spo % c == 0))


RS_BUILT_F32 = {(2, 1), (2, 2), (6, 3), (6, 4)}


@pytest.mark.parametrize("dtype", DTYPES)
def test_row_stationary_family(dtype, scene):
    """Every (nt, cg) instantiation of launch_rs_t, every fragment count up to rs_nf_max, tile heights that leave a ragged
    last tile.  fp32 builds (2, 1), (2, 2), (6, 3), (6, 4) only: every other shape must answer UNSUPPORTED."""
    cm, nbr = scene
    n = nbr.shape[0]
    ran = {}
    shapes = list(RS_PAIRS.values()) + ([(16, 32)] if dtype == torch.float32 else [])
    for cin, cout in shapes:
        nt, cg = key = rs_key(cin, cout, dtype)
        c = Conv(dtype, nbr, n, cin, cout, seed=nt * 10 + cg)
        got = 0
        for nf in range(1, rs_nf_max(nt, cg) + 1):
            for rows in (0, 128 * nf - 16 * (nf % 3)):
                got += c.run(rs_cfg(nf, rows), label="(nt %d, cg %d)" % key)
        got += c.run(rs_cfg(0), label="(nt %d, cg %d)" % key)
        for nf in (rs_nf_max(nt, cg) + 1, 6):         # past the built fragment counts: refused, nothing written
            o = X.SentinelOut(n, c.cout_p, dtype, DEV)
            assert c.launch(rs_cfg(nf), o.view) == N.PBN_ERR_UNSUPPORTED
            o.check(0, "refused rs nf %d" % nf)
        built = dtype != torch.float32 or key in RS_BUILT_F32
        assert got == ((2 * rs_nf_max(nt, cg) + 1) if built else 0), (key, got)
        ran[key] = got
        if built:
            cb = Conv(dtype, nbr, n, cin, cout, mode="bounded", relu=True, seed=nt)
            assert cb.run(rs_cfg(0), label="(nt %d, cg %d)" % key)
    print("row-stationary configurations run per (nt, cg) in %s: %s" % (dtype, ran))
    assert len([k for k, v in ran.items() if v]) == (9 if dtype != torch.float32 else 4)


def test_row_stationary_family_at_automatic_dispatch():
    """>= 20 k rows (two copies of a room: 56 k rows) with rows_per_wave = 0: pbn_spconv_family says 2 wherever
    rs_family_wanted takes the shape, and the launch is exact; bf16 and fp16."""
    cm, nbr = _geo((2.0, 1.6, 1.2), 47, 3, batch=2)
    n = nbr.shape[0]
    assert n >= 40000, n
    fams = {}
    for dtype in (torch.bfloat16, torch.float16):
        for (nt, cg), (cin, cout) in RS_PAIRS.items():
            c = Conv(dtype, nbr, n, cin, cout, seed=nt + cg)
            fams[(nt, cg)] = c.family()
            assert c.run(0, label="auto family %d" % fams[(nt, cg)])
        cb = Conv(dtype, nbr, n, 128, 96, mode="bounded", relu=True, seed=1)
        cb.run(0, label="auto")
    print("automatic family per (nt, cg) at %d rows: %s" % (n, fams))
    # (2, 2) -- 64 -> 32 -- is not a shape the automatic choice gives this family
    assert all(f == 2 for key, f in fams.items() if key != (2, 2)), fams


# ---- the folded shortcut -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
def test_folded_shortcut_every_family(dtype, scene):
    cm, nbr = scene
    n = nbr.shape[0]
    ran = {}
    for cin, cin2, cout in ((64, 32, 64), (96, 128, 96), (128, 192, 128)):
        c = Conv(dtype, nbr, n, cin, cout, cin2=cin2, seed=cin2)
        for cfg in (0, 16, 32, 64, 402, 404, 204, 1401, 1402, 1404, 1201, 1202, 1204, 1208, rs_cfg(0), rs_cfg(2, 240), rs_cfg(3)):
            if 100 <= cfg < 10000 and (c.cout_p // 16) % (cfg % 100):
                continue
            ok = c.run(cfg, label="dual")
            ran[family_of(cfg)] = ran.get(family_of(cfg), 0) + ok
            if ok and cfg in (32, 1202):
                assert c.run(cfg, count=n // 2, label="dual")
        cb = Conv(dtype, nbr, n, cin, cout, mode="bounded", cin2=cin2, seed=cin2)
        cb.run(32, label="dual")
    print("dual configurations run per family in %s: %s" % (dtype, ran))
    assert ran["tile"] >= 9 and ran["wave"] >= 9 and ran["auto"] == 3
    assert ran["rs"] >= (6 if dtype != torch.float32 else 1)


# ---- edges ---------------------------------------------------------------------------------------------------------------

def _edge_nbr(g, n_out, n_in, K):
    """Random map with: row 0 without any neighbour, offset 5 empty for every row, input row 3 gathered by every row at
    offset 7."""
    nbr = random_nbr(g, n_out, n_in, K)
    nbr[:, 5 % K] = -1
    if K > 7:
        nbr[:, 7] = 3 % n_in
    nbr[0] = -1
    return nbr


EDGE_CFGS = {"tile": ((32, 128), (64, 256), (16, 64)), "wave": ((1202, 32), (402, 256), (204, 128)),
             "rs": ((rs_cfg(1, 128), 128), (rs_cfg(2, 240), 240), (rs_cfg(0), 300))}
EDGE_NEED = {"tile": 100, "wave": 80, "rs": 60}


@pytest.mark.parametrize("family", ["tile", "wave", "rs"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_edges(family, dtype):
    """Row counts 1, 15, 16, 17 and TM - 1 / TM / TM + 1 of the family's tile heights; a row with no neighbour (exactly the
    epilogue of 0); an offset empty for every row; one input row gathered by every output row; n_in != n_out; channel
    tails (cin 6 / 34 / 40, cout 20); the k = 5 stem."""
    g = torch.Generator().manual_seed(11)
    ran = 0
    counts = sorted({1, 15, 16, 17} | {t + d for _, t in EDGE_CFGS[family] for d in (-1, 0, 1)})
    for cin, cout, K in ((40, 20, 27), (34, 32, 27), (6, 32, 125), (64, 64, 27), (32, 32, 27)):
        for n in counts:
            n_in = n + 23 if n % 2 else max(n // 2, 5)
            nbr = _edge_nbr(g, n, n_in, K)
            assert bool((nbr[0] < 0).all())          # row 0 has no neighbour: its output is exactly relu?(shift + res)
            c = Conv(dtype, nbr, n_in, cin, cout, seed=n + cin, relu=(n % 2 == 0))
            for cfg, _ in EDGE_CFGS[family]:
                ran += c.run(cfg, label="edge")
    print("%s edges in %s: %d launches ran" % (family, dtype, ran))
    # (rs: no k = 5 form, and fp32 builds only the (nt, cg) pairs this set reaches with 32 -> 32)
    need = EDGE_NEED[family] if not (family == "rs" and dtype == torch.float32) else len(counts) * 3
    assert ran >= need, ran


# ---- processing order and device-side row count -----------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
def test_row_perm_and_device_count(dtype, scene):
    """A random processing order on the families that take one (rs answers PBN_ERR_UNSUPPORTED), and device-side row counts
    below the capacity, 0 included, on every family: rows past the count stay untouched."""
    cm, nbr = scene
    n = nbr.shape[0]
    g = torch.Generator().manual_seed(3)
    perm = torch.randperm(n, generator=g).int().to(DEV)
    c = Conv(dtype, nbr, n, 96, 96, seed=9)
    ran = 0
    for cfg in (16, 32, 64, 402, 1202, 1402, 2202):
        for ws in (True, False):
            ran += c.run(cfg, row_perm=perm, ws=ws)
            ran += c.run(cfg, row_perm=perm, count=n // 3, ws=ws)
    assert ran == 28
    o = X.SentinelOut(n, c.cout_p, dtype, DEV)
    for cfg in (rs_cfg(0), rs_cfg(2, 256)):
        assert c.launch(cfg, o.view, row_perm=perm) == N.PBN_ERR_UNSUPPORTED
    o.check(0, "rs refused a processing order")
    ran = 0
    for cfg in (0, 16, 32, 64, 402, 1202, 1402, rs_cfg(0), rs_cfg(3, 304)):
        for count in (0, 1, n // 2 + 3, n - 1):
            ran += c.run(cfg, count=count)
    assert ran == 36, ran


# ---- MinkUNet34C at the bench scene's sizes, automatic dispatch -------------------------------------------------------

def _unet_shapes(arch="MinkUNet34C", in_channels=6, out_channels=32):
    """Every distinct convolution launch of the fused forward: (level_in, level_out, map, cin, cout, cin2 of the folded shortcut)."""
    L, P = SPECS[arch]
    out = [(1, 1, "k5", in_channels, INIT_DIM, 0)]
    inp, s = INIT_DIM, 1
    blocks = []
    for i in range(4):
        out.append((s, 2 * s, "down", inp, inp, 0))
        s *= 2
        blocks.append((s, inp, P[i], L[i]))
        inp = P[i]
    skips = (P[2], P[1], P[0], INIT_DIM)
    for i in range(4):
        out.append((s, s // 2, "up", inp, P[4 + i], 0))
        s //= 2
        blocks.append((s, P[4 + i] + skips[i], P[4 + i], L[4 + i]))
        inp = P[4 + i]
    for lvl, cin, planes, nb in blocks:
        out.append((lvl, lvl, "k3", cin, planes, 0))
        out.append((lvl, lvl, "k3", planes, planes, cin if cin != planes else 0))
        if nb > 1 or cin != planes:
            out.append((lvl, lvl, "k3", planes, planes, 0))
    out.append((1, 1, "k1", P[7], out_channels, 0))
    return sorted(set(out))


@pytest.fixture(scope="module")
def bench_pyramids():
    b, _, info = synth.make_val_batch(seed=2, copies=1)          # bench.py's default scene: 146 038 voxels
    one = b["xyz_voxel"].astype(np.int32)
    four = np.concatenate([np.concatenate([np.full((len(one), 1), j, np.int32), one[:, 1:]], 1) for j in range(4)], 0)
    return {1: ME.CoordinateManager(torch.from_numpy(one).to(DEV)), 4: ME.CoordinateManager(torch.from_numpy(four).to(DEV))}


_BENCH_FAMILIES = {}


@pytest.mark.parametrize("scenes", [1, 4])
def test_bench_shapes_at_automatic_dispatch(scenes, bench_pyramids):
    """Every distinct convolution shape of MinkUNet34C (bench.py's backbone) on the bench scene's pyramid, one scene and
    four merged scenes (the served leg's row counts), bf16, rows_per_wave = 0, exact mode.  The automatic choice must
    reach all three families."""
    cm = bench_pyramids[scenes]
    fams = {}
    for lin, lout, kind, cin, cout, cin2 in _unet_shapes():
        n_in, n_out = cm.num_rows(lin), cm.num_rows(lout)
        ident = kind == "k1"
        nbr = {"k5": lambda: cm.kernel_map(lin, 5), "k3": lambda: cm.kernel_map(lin, 3), "down": lambda: cm.down_map(lin),
               "up": lambda: cm.up_map(lin), "k1": lambda: torch.arange(n_out, dtype=torch.int32, device=DEV)[:, None]}[kind]()
        c = Conv(torch.bfloat16, nbr, n_in, cin, cout, cin2=cin2, seed=lin * 1000 + cin + cout, identity=ident,
                 relu=bool(cin2))
        f = c.family()
        fams[f] = fams.get(f, 0) + 1
        assert c.run(0, label="L%d->L%d %s family %d" % (lin, lout, kind, f))
        del c
    _BENCH_FAMILIES[scenes] = fams
    print("MinkUNet34C at %d scene(s): launches per automatic family %s" % (scenes, fams))
    assert fams.get(0, 0) >= 1 and fams.get(1, 0) >= 1
    if scenes == 4:
        assert fams.get(2, 0) >= 1
        # the 64- / 128-channel row-stationary forms engage at these row counts
        assert set(_BENCH_FAMILIES.get(1, {})) | set(fams) >= {0, 1, 2}


def test_worst_bounded_ratios_report():
    """(report) the worst bounded-mode err / bound per family seen by the tests above in this process."""
    print("worst bounded-mode err / bound per family: %s" % {k: round(v, 3) for k, v in sorted(_WORST.items())})
    assert all(v <= 1.0 for v in _WORST.values())
