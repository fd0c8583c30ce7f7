"""CPU tier for depth-frame fusion: the designed cases of tests/fuse_cases.py against the two statements of the contract
(tests/fuse_ref.py vectorised, tests/fuse_mutants.py block by block), the kill matrix of the mutants, the properties the
cases were designed for, and a check that does not go through the restatement's own formula: ray-cast planes come back on
their planes, with their normals, within bounds derived here, and fusing noisy frames beats one of them."""
import numpy as np
import pytest

import frames_ref as R
import fuse_cases as C
import fuse_mutants as M
import fuse_ref as FR

NAMES = list(C.CASES)
SMALL = [n for n in NAMES if n != "room"]
_REFS = {}


def _ref(name):
    if name not in _REFS:
        depth, pose, intr, colour, kw = C.arguments(C.CASES[name])
        _REFS[name] = FR.fuse_ref(depth, pose, intr, colour, **kw)
    return _REFS[name]


def _volume_ref(v):
    return FR.extract_ref(v["tsdf"], v["weight"], v["rgb"], v["block_key"], v["origin"], v["voxel"], v["min_weight"])


@pytest.mark.parametrize("name", SMALL)
def test_both_statements_agree(name):
    assert M.same(M.fuse(C.CASES[name]), _ref(name)), C.CASES[name]["why"]


@pytest.mark.parametrize("name", list(C.VOLUMES))
def test_both_statements_agree_on_the_volumes(name):
    v = C.VOLUMES[name]
    got = M.extract(v["tsdf"], v["weight"], v["rgb"], v["block_key"], v["origin"], v["voxel"], v["min_weight"])
    assert M.same(got, _volume_ref(v)), v["why"]


def test_the_room_agrees_where_the_second_statement_is_affordable():
    """The largest case block by block would take minutes: its first twelve blocks are integrated by the second statement."""
    depth, pose, intr, colour, kw = C.arguments(C.CASES["room"])
    ref = _ref("room")
    keys = ref["block_key"][:12]
    got = M.integrate(depth, pose, intr, colour, ref["origin"], keys, kw["voxel"], 4.0 * kw["voxel"], 1000.0, 0.0, kw["depth_max"],
                      kw["edge"])
    assert got[0].tobytes() == ref["tsdf"][:12].tobytes() and got[1].tobytes() == ref["vol_weight"][:12].tobytes()
    assert got[2].tobytes() == ref["vol_rgb"][:12].tobytes()


def test_every_mutant_is_killed():
    order = ["tie", "trunc_exact", "wall_x", "weights", "zero_d", "two_adjacent", "wall_z"] + \
            [n for n in SMALL if n not in ("tie", "trunc_exact", "wall_x", "weights", "zero_d", "two_adjacent", "wall_z")]
    matrix = {}
    for mutant in M.MUTANTS:
        if mutant in M.EXTRACT_MUTANTS:
            for name, v in C.VOLUMES.items():
                got = M.extract(v["tsdf"], v["weight"], v["rgb"], v["block_key"], v["origin"], v["voxel"], v["min_weight"], mutant)
                if not M.same(got, _volume_ref(v)):
                    matrix[mutant] = "volume " + name
                    break
            if mutant in matrix:
                continue
        for name in order:
            if not M.same(M.fuse(C.CASES[name], mutant), _ref(name)):
                matrix[mutant] = name
                break
    print("\n".join("%-20s killed by %s" % (m, matrix.get(m)) for m in M.MUTANTS))
    assert sorted(matrix) == sorted(M.MUTANTS), "survivors: %s" % sorted(set(M.MUTANTS) - set(matrix))


def _projection(name):
    """uf of every voxel against frame 0 of an identity-pose case, and the volume's weights."""
    ref = _ref(name)
    case = C.CASES[name]
    p = FR.centres(ref["origin"], ref["block_key"], case["kw"]["voxel"]).reshape(-1, 3)
    fx, _, cx, _ = np.broadcast_to(case["intr"], (case["depth"].shape[0], 4))[0]
    with np.errstate(all="ignore"):
        return (fx * p[:, 0]) / p[:, 2] + cx, p, ref["vol_weight"].reshape(-1)


def test_designed_cases_have_their_properties():
    assert _ref("one")["block_key"].shape[0] == 27 and _ref("one")["n_raw"] == 1
    assert _ref("two_adjacent")["block_key"].shape[0] == 36 and _ref("two_adjacent")["n_raw"] == 2
    B = 8.0 * 0.05
    assert (2.0 - (2.0 - B)) / B < 1.0 and _ref("min_rounding")["status"] == 0
    assert FR.unpack(_ref("min_rounding")["block_key"]).min() == 0 and _ref("min_rounding")["block_key"].shape[0] == 27
    for name in ("all_lost", "none_measured"):
        r = _ref(name)
        assert r["n_raw"] == 0 and r["block_key"].shape[0] == 0 and r["n"] == 0 and r["tsdf"].shape == (0, 512)
    assert np.array_equal(_ref("tie")["origin"], [-0.5, -0.5, 0.5])
    # ties: voxels of the layer zc = 33/32 with uf exactly 7.5 and 8.5 both land on pixel 8 (even), and are seen
    uf, p, w = _projection("tie")
    layer = (p[:, 2] == 1.03125) & (p[:, 1] == p[:, 1][np.argmin(np.abs(p[:, 1]))])
    assert set(uf[layer & (w > 0)].tolist()) >= {7.5, 8.5}
    assert not np.any(w[layer & ((uf == 6.5) | (uf == 9.5))])
    uf, p, w = _projection("tie_low")
    layer = p[:, 2] == 1.03125
    assert np.any(w[layer & (uf == -0.5)] > 0) and not np.any(w[layer & (uf == -1.5)])
    # the NaN frame adds nothing: the volume is the one-frame volume
    one = FR.fuse_ref(C.CASES["nan_cx"]["depth"][:1], C.CASES["nan_cx"]["pose"][:1], C.CASES["nan_cx"]["intr"][:1], voxel=C.VOXEL)
    assert one["tsdf"].tobytes() == _ref("nan_cx")["tsdf"].tobytes()
    # s = -trunc exactly is kept, one ulp below is not
    a, b = _ref("trunc_exact"), _ref("trunc_ulp")
    assert a["vol_weight"].sum() == b["vol_weight"].sum() + (a["tsdf"] == np.float32(-1.0)).sum() > b["vol_weight"].sum()
    assert np.float32(1.0) in _ref("trunc_small")["tsdf"] and C.CASES["trunc_max"]["kw"]["trunc"] == 8 * C.VOXEL
    assert set(np.unique(_ref("weights")["vol_weight"]).tolist()) == {0, 1, 2, 3, 4}
    assert _ref("weights")["weight"].min() >= 3
    for n, seen in ((63, 3), (64, 2), (65, 3), (130, 5)):
        r = _ref("frames%d" % n)
        assert C.CASES["frames%d" % n]["depth"].shape[0] == n and r["vol_weight"].max() <= seen and r["n_raw"] == seen
    z = _ref("zero_d")
    zero = np.flatnonzero((z["tsdf"].reshape(-1) == 0.0) & (z["vol_weight"].reshape(-1) > 0))
    assert zero.size and np.any(np.isin(z["voxel_id"] // 3, zero))               # a crossing that starts on D = 0
    inside = _ref("inside")
    assert inside["n_raw"] == 26 and inside["n"] > 0
    for name in ("wall_z", "wall_x", "wall_y", "wall_f32", "room"):
        r = _ref(name)
        local = (r["voxel_id"] // 3) % 512
        axis = r["voxel_id"] % 3
        coord = np.stack([local & 7, (local >> 3) & 7, local >> 6], axis=1)[np.arange(local.size), axis]
        assert r["n"] > 20 and np.all(np.isfinite(r["xyz"])) and np.all(np.diff(r["voxel_id"]) > 0)
        assert np.any(coord == 7) or name == "wall_f32"                           # a crossing into the next block
    room = _ref("room")
    assert room["block_key"].shape[0] > 300 and "rgb" in room
    v = _volume_ref(C.VOLUMES["zero_gradient"])
    assert v["n"] == 3 and v["nl"][1].tolist() == [0.0, 0.0, 0.0] and np.all(v["nl"][[0, 2], 0] != 0.0)
    rv = _volume_ref(C.VOLUMES["random"])
    assert rv["n"] > 500 and len(C.VOLUMES["random"]["block_key"]) < 18


# --------------------------------------------------------------------------------------------------------------- geometry
INTR = (60.0, 60.0, 31.5, 23.5)
H, W, SCALE, VOX = 48, 64, 1000.0, 0.04


def _depth_error(img, trunc):
    """e_z: how far the depth a voxel reads may lie from the depth at which the voxel's own ray meets its plane.  Derived:
    the stored depth is off by at most half a quantum q = 1 / depth_scale.  The voxel reads the pixel its centre rounds to,
    so its ray lies up to half a pixel from the pixel's along u and along v.  On a plane 1 / z is affine in (u, v), so
    along a row z(u + t) - z(u) = -a t z(u) z(u + t): the change over t <= 1/2 is at most
    (1/2) (z(u + 1/2) / z(u + 1)) times the full step to the neighbour, and at the image border, where the neighbour on
    that side is missing, (1/2) (z(u + 1/2) / z(u - 1)) times the step to the other one; with rho the largest ratio of
    two adjacent depths both factors are at most rho^1.5 / 2.  So e_z = q / 2 + (rho^1.5 / 2) (step_u + step_v), step_a
    the largest difference of two adjacent pixels of one surface along a, plus the float32 store of D (|D| <= 1, half a
    spacing at 1, times trunc)."""
    z, surface = img["z"], img["surface"]
    step, rho = [], 1.0
    for ax in (0, 1):
        lo = [slice(None)] * 2
        hi = [slice(None)] * 2
        lo[ax], hi[ax] = slice(None, -1), slice(1, None)
        za, zb = z[tuple(lo)], z[tuple(hi)]
        same = np.isfinite(za) & np.isfinite(zb) & (surface[tuple(lo)] == surface[tuple(hi)])
        step.append(float(np.abs(za - zb)[same].max()))
        rho = max(rho, float((np.maximum(za, zb) / np.minimum(za, zb))[same].max()))
    assert rho ** 1.5 <= 2.0
    return 0.5 / SCALE + 0.5 * rho ** 1.5 * (step[0] + step[1]) + trunc * 2.0 ** -24


class _Rows:
    """The geometry of every surface row, from voxel_id alone: the crossing's voxels q and n = q + e_a, the twelve voxels
    of their gradient stencils, the pixel each of the fourteen reads, whether it is observed, and its projective factor
    c(p) = |nrm . (p - eye)| / zc(p) for a plane of unit normal nrm.  The projective distance a voxel stores is its true
    distance d(p) to the plane divided by c(p): along the voxel's ray the plane is met at depth z*, p - x* = (zc - z*) ray
    with ray = (p - eye) / zc, so d = (z* - zc) (nrm . ray) up to sign."""

    def __init__(self, out, pose, voxel):
        vid = out["voxel_id"]
        self.axis = (vid % 3).astype(int)
        flat = vid // 3
        idx = flat % 512
        local = np.stack([idx & 7, (idx >> 3) & 7, idx >> 6], axis=1)
        q = 8 * FR.unpack(out["block_key"])[flat // 512] + local
        e = np.eye(3, dtype=np.int64)
        n = q + e[self.axis]
        self.cells = np.stack([q, n] + [x + sgn * e[b] for x in (q, n) for b in range(3) for sgn in (1, -1)], axis=1)   # [N, 14, 3]
        self.p = np.asarray(out["origin"])[None, None, :] + (self.cells + 0.5) * voxel
        key, w = out["block_key"], out["vol_weight"]
        bk = FR.pack(self.cells // 8)
        pos = np.minimum(np.searchsorted(key, bk), len(key) - 1)
        m = self.cells % 8
        self.observed = (key[pos] == bk) & (w[pos, (m[..., 2] * 8 + m[..., 1]) * 8 + m[..., 0]] >= 1)
        self.eye = pose[:3, 3]
        rel = self.p - self.eye
        self.zc = rel @ pose[:3, 2]
        with np.errstate(all="ignore"):
            self.u = np.rint(INTR[0] * (rel @ pose[:3, 0]) / self.zc + INTR[2])
            self.v = np.rint(INTR[1] * (rel @ pose[:3, 1]) / self.zc + INTR[3])
        self.rel = rel

    def pure(self, surface, which):
        """Per voxel: it reads a pixel inside the image whose 3 x 3 neighbourhood lies on surface `which` [N] only."""
        inside = (self.zc > 0) & (self.u >= 1) & (self.u <= W - 2) & (self.v >= 1) & (self.v <= H - 2)
        u, v = np.where(inside, self.u, 1).astype(int), np.where(inside, self.v, 1).astype(int)
        ok = inside
        for dv in (-1, 0, 1):
            for du in (-1, 0, 1):
                ok = ok & (surface[v + dv, u + du] == which[:, None])
        return ok

    def c(self, axis):
        """c(p) of the fourteen voxels for planes x[axis] = const, axis [N]."""
        return np.abs(self.rel[np.arange(len(axis)), :, axis]) / self.zc


def _check_rows(out, rows, plane_axis, offset, e_z, voxel, trunc, select):
    """The two bounds, per row, on the rows of `select` that the derivation covers; returns how many rows each covered.

    Distance.  Write s = trunc * D for the stored projective distance of a voxel: s_i = d_i / c_i + eps_i, |eps_i| <= e_z.
    The crossing lies at t = r = s_q / (s_q - s_n) between q and n, where the true distance, which is linear along the axis,
    is delta = (1 - r) d_q + r d_n.  With d_i = c_i (s_i - eps_i) and (1 - r) s_q + r s_n = 0:
        delta = r s_n (c_n - c_q) - ((1 - r) c_q eps_q + r c_n eps_n),   |r s_n| = |s_q s_n| / (|s_q| + |s_n|) <= s_max / 2,
    so |delta| <= |c_n - c_q| s_max / 2 + max(c_q, c_n) e_z: the first term is what the projective distance adds on a plane
    seen at a slant.  s_q and s_n have opposite signs, so d_q >= -c_q e_z and d_n <= c_n e_z (or the reverse), and
    |d_q - d_n| <= voxel, hence |d_i| <= voxel + c_max e_z and |s_i| <= s_max = (voxel + c_max e_z) / c_min + e_z.  The
    derivation needs s_max < trunc (neither value clamped or cut): rows where it is not are not covered.  The float32
    store of the point adds one spacing at the scene's extent.

    Normal.  Rows whose fourteen stencil voxels are all observed, with s_st = (2 voxel + c_max e_z) / c_min + e_z < trunc so
    that none is clamped.  For x in {q, n}: trunc G(x)[b] = d+ / c+ - d- / c- + (eps+ - eps-)
    = ((d+ - d-) + eta_b) / c_x with d+ - d- = 2 voxel nrm_b and |eta_b| <= c_x (|d+| + |d-|) kappa + 2 c_x e_z, kappa the
    largest difference of two 1 / c in the stencil and |d+-| <= 2 voxel + c_max e_z.  gv = (1 - r) G(q) + r G(n) is then
    A nrm + err with A >= 2 voxel / c_max and every component of err at most E = eta_max / c_min: the angle to nrm is at
    most atan(sqrt(2) E / (A - E)).  The float32 store of nl adds 1e-6 to the cosine's bound."""
    k = np.arange(len(plane_axis))
    c = rows.c(plane_axis)
    cq, cn = c[:, 0], c[:, 1]
    cmin2, cmax2 = np.minimum(cq, cn), np.maximum(cq, cn)
    s_max = (voxel + cmax2 * e_z) / cmin2 + e_z
    covered = select[:, :2].all(axis=1) & (s_max < trunc)
    xyz = out["xyz"].astype(np.float64)
    dist = np.abs(xyz[k, plane_axis] - offset)
    bound = np.abs(cn - cq) * s_max / 2 + cmax2 * e_z + float(np.spacing(np.float32(np.abs(xyz).max())))
    print("distance: %d of %d rows covered, worst %.3e of its bound %.3e" %
          (covered.sum(), len(k), dist[covered][np.argmax((dist / bound)[covered])], bound[covered][np.argmax((dist / bound)[covered])]))
    assert np.all(dist[covered] <= bound[covered])
    cmin, cmax = c.min(axis=1), c.max(axis=1)
    s_st = (2 * voxel + cmax * e_z) / cmin + e_z
    kappa = (1.0 / c).max(axis=1) - (1.0 / c).min(axis=1)
    eta = cmax * (2 * (2 * voxel + cmax * e_z) * kappa + 2 * e_z)
    A, E = 2 * voxel / cmax, eta / cmin
    with np.errstate(all="ignore"):
        full = select.all(axis=1) & rows.observed.all(axis=1) & (s_st < trunc) & (A > E)
        lim = np.arctan(np.sqrt(2.0) * E / (A - E))
    want = np.zeros((len(k), 3))
    want[k, plane_axis] = -np.sign(rows.rel[k, 0, plane_axis])                    # from the plane towards the eye
    cos = np.sum(out["nl"].astype(np.float64) * want, axis=1)
    print("normals: %d of %d rows covered, largest allowed angle %.2f deg, largest found %.2f deg" %
          (full.sum(), len(k), np.degrees(lim[full].max()), np.degrees(np.arccos(np.clip(cos[full].min(), -1, 1)))))
    assert np.all(cos[full] >= np.cos(lim[full]) - 1e-6)
    return int(covered.sum()), int(full.sum())


@pytest.mark.parametrize("eye,target,plane", [((0.0, 0.0, 1.0), (0.0, 3.0, 1.0), (1, 2.0)),
                                              ((0.3, -0.2, 1.1), (0.5, 3.0, 0.9), (1, 2.5))])
def test_ray_cast_plane_comes_back_on_its_plane(eye, target, plane):
    """A fronto-parallel wall, and the same wall seen at a slant: every row the derivation covers lies within its distance
    bound, and every row with a fully observed stencil has its normal within the derived angle of the plane's."""
    pose = R.look_at(eye, target)
    img = R.render(pose, INTR, H, W, planes=[(plane[0], plane[1], (200, 10, 10))], depth_scale=SCALE)
    out = FR.fuse_ref(img["u16"][None], pose[None], INTR, voxel=VOX, depth_scale=SCALE)
    assert out["status"] == 0 and out["n"] > 500 and np.all(img["surface"] == 0)
    rows = _Rows(out, pose, VOX)
    n = out["n"]
    everything = np.ones((n, 14), bool)                                           # one surface fills the image
    covered, full = _check_rows(out, rows, np.full(n, plane[0]), plane[1], _depth_error(img, 4 * VOX), VOX, 4 * VOX, everything)
    assert covered == n and full > 0                                              # c >= 0.8 here: no row is left out of the distance


def test_box_room_comes_back_on_its_planes():
    """Five planes of a room.  A row is checked against the plane its voxels read: rows whose voxels read pixels within one
    pixel of another surface (a corner of the room) are the only ones set aside, by the rendered surface image; walls seen
    at a grazing angle drop out of the derivation where s_max reaches trunc, as _check_rows says."""
    planes = [(0, -1.5, (200, 60, 60)), (0, 1.5, (60, 200, 60)), (1, 2.0, (60, 60, 200)), (2, 0.0, (120, 120, 120)),
              (2, 2.4, (240, 240, 240))]
    pose = R.look_at((0.0, -0.5, 1.2), (0.0, 2.0, 1.1))
    img = R.render(pose, INTR, H, W, planes=planes, depth_scale=SCALE)
    out = FR.fuse_ref(img["u16"][None], pose[None], INTR, voxel=VOX, depth_scale=SCALE, edge=0.02)
    assert out["status"] == 0 and out["n"] > 1000
    rows = _Rows(out, pose, VOX)
    inside = (rows.zc[:, 0] > 0) & (rows.u[:, 0] >= 0) & (rows.u[:, 0] <= W - 1) & (rows.v[:, 0] >= 0) & (rows.v[:, 0] <= H - 1)
    assert np.all(inside)                                                         # q is observed: it read a pixel
    which = img["surface"][rows.v[:, 0].astype(int), rows.u[:, 0].astype(int)]
    assert which.min() >= 0
    axis = np.array([a for a, _, _ in planes])[which]
    offset = np.array([o for _, o, _ in planes])[which]
    covered, full = _check_rows(out, rows, axis, offset, _depth_error(img, 4 * VOX), VOX, 4 * VOX, rows.pure(img["surface"], which))
    assert covered > 0 and full > 0


def test_fusing_noisy_frames_beats_one_frame():
    """Zero-mean noise of one quantum per frame: the error of 16 fused frames is below the error of one."""
    rng = np.random.default_rng(5)
    pose = R.look_at((0.0, 0.0, 1.0), (0.0, 3.0, 1.0))
    img = R.render(pose, INTR, H, W, planes=[(1, 2.0, (90, 90, 90))], depth_scale=SCALE)
    noisy = np.stack([(img["u16"].astype(np.int64) + rng.integers(-1, 2, img["u16"].shape)).astype(np.uint16) for _ in range(16)])

    def error(frames):
        out = FR.fuse_ref(frames, np.tile(pose, (len(frames), 1, 1)), INTR, voxel=VOX, depth_scale=SCALE)
        d = out["xyz"][:, 1].astype(np.float64) - 2.0
        return float(np.sqrt(np.mean(d * d)))

    single, fused = error(noisy[:1]), error(noisy)
    print("rms error: one frame %.3e, sixteen frames %.3e" % (single, fused))
    assert fused < single
