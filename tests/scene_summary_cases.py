"""The shared case list of the scene-summary tests (not a test module).  A case is plain numpy: what pbn_scene_summary reads.
tests/test_scene_summary_ref_cpu.py runs every case through the restatement and a brute-force loop, tests/test_scene_summary_gpu.py
through the kernels and the restatement.

Scores are multiples of 1/4 below 8 in magnitude unless a case says otherwise: exact in float32, bfloat16 and float16, sums of a few
of them too, and ties between classes are frequent."""
import numpy as np

NO_LABEL = -100
LABELS = [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 14, 16, 24, 28, 33, 34, 36, 39]
MAX_CLASSES = 32           # SEL_MAX_CLASSES (csrc/pbn_common.h)


def make_case(name, sizes, copies=1, n_cls=20, pad=0, dtype="f32", n_keep=None, n_prop=None, seed=0, with_xyz=True, labels=None,
              unlabelled=0.2):
    """sizes: folded points per scene; n_keep: kept instances per scene (default 3 each); n_prop default sum(n_keep) + 3."""
    rng = np.random.default_rng(seed)
    b = len(sizes)
    starts = [0]
    for n in sizes:
        starts.append(starts[-1] + int(n))
    n_total = starts[-1]
    n_keep = [3] * b if n_keep is None else list(n_keep)
    n_prop = sum(n_keep) + 3 if n_prop is None else int(n_prop)
    scores = (rng.integers(-31, 32, size=(copies * n_total, n_cls)) / 4.0).astype(np.float32)
    inst = np.full(n_total, NO_LABEL, dtype=np.int32)
    for j in range(b):
        if n_keep[j] > 0 and sizes[j] > 0:
            v = rng.integers(0, n_keep[j], size=sizes[j]).astype(np.int32)
            v[rng.random(sizes[j]) < unlabelled] = NO_LABEL
            inst[starts[j]:starts[j + 1]] = v
    xyz = None
    if with_xyz:
        xyz = (rng.normal(size=(n_total, 3)) * 3.0).astype(np.float32)
    return dict(name=name, point_starts=starts, copies=copies, n_cls=n_cls, ld=n_cls + pad, dtype=dtype, scores=scores,
                point_instance=inst, n_keep=n_keep, n_prop=n_prop, xyz=xyz, labels=list(LABELS if labels is None else labels))


def _equal_sums():
    c = make_case("equal folded sums", (70,), copies=3, seed=11)
    n = 70
    s = c["scores"].reshape(3, n, -1)
    s[:, 0, :] = 1.0                                        # every class equal: class 0
    s[:, 1, :] = -2.0
    s[0, 1, 3], s[1, 1, 3], s[2, 1, 3] = 1.0, 0.5, 0.25     # classes 3 and 7 reach the same sum by different copies: class 3
    s[0, 1, 7], s[1, 1, 7], s[2, 1, 7] = 0.25, 0.5, 1.0
    return c


def _equal_votes():
    c = make_case("equal vote counts", (6,), n_keep=[1], seed=12)
    c["scores"][:] = 0.0
    for i, k in enumerate((5, 2, 5, 2, 9, 0)):              # instance 0: two points of class 5, two of class 2 -> class 2
        c["scores"][i, k] = 1.0
    c["point_instance"][:] = [0, 0, 0, 0, NO_LABEL, NO_LABEL]
    return c


def _copy_order():
    c = make_case("copy order", (5,), copies=3, n_cls=3, seed=13)
    s = c["scores"].reshape(3, 5, 3)
    s[:] = 0.0
    # in copy order class 0 sums to (1e8 + 1) - 1e8 = 0 and class 1 to (1e8 - 1e8) + 1 = 1; class 2 is 0.5 -> class 1.
    # Any order that adds the two large terms of class 0 first gives it 1 as well, and the tie would go to class 0.
    s[0, :, 0], s[1, :, 0], s[2, :, 0] = 1e8, 1.0, -1e8
    s[0, :, 1], s[1, :, 1], s[2, :, 1] = 1e8, -1e8, 1.0
    s[:, :, 2] = [[0.5], [0.0], [0.0]]
    return c


def _special_values():
    c = make_case("nan and inf scores", (9,), copies=3, n_cls=4, seed=14)
    s = c["scores"].reshape(3, 9, 4)
    s[:, 0, :] = np.nan                                     # all NaN: class 0
    s[:, 1, :] = 0.0
    s[1, 1, 0] = np.nan                                     # a NaN sum never wins: class 1 (first of the zeros)
    s[:, 2, :] = 0.0
    s[0, 2, 2], s[2, 2, 3] = np.inf, np.inf                 # two +inf sums: class 2
    s[:, 3, :] = 0.0
    s[0, 3, 1], s[1, 3, 1] = np.inf, -np.inf                # inf - inf = NaN: loses; the rest tie at 0: class 0
    s[:, 4, :] = -np.inf                                    # every sum -inf: nothing exceeds the start value: class 0
    s[:, 5, :] = -np.inf
    s[:, 5, 3] = -7.0                                       # one finite among -inf: class 3
    return c


def _bad_coordinates():
    c = make_case("invalid coordinates", (80, 40), n_keep=[3, 2], seed=15, unlabelled=0.0)
    x = c["xyz"]
    x[0] = [-0.0, 0.0, -1.5]
    x[1] = [0.0, -0.0, 2.5]
    c["point_instance"][:2] = 0
    x[5, 1] = np.nan                                        # scene 0: status 4, the points skipped
    x[6, 2] = 4e4
    x[7, 0] = -32768.0
    x[8, 0] = 32767.99609375                                # the largest float32 below the limit: taken
    c["point_instance"][80:] = 0                            # scene 1: instance 1 has no point at all, instance 0 only invalid ones
    x[80:, 0] = np.inf
    return c


def _bad_instances():
    c = make_case("point_instance out of range", (50, 30, 20), n_keep=[2, 3, 1], seed=16)
    c["point_instance"][3] = 2                              # = n_keep of scene 0: bit 8
    c["point_instance"][55] = -3                            # negative, not -100: bit 8
    return c                                                # scene 2 stays clean


def _class_outside():
    c = make_case("class outside the label table", (60, 40), n_keep=[2, 2], seed=17, labels=[7, 8, 9], unlabelled=0.0)
    c["scores"][:] = 0.0
    c["scores"][:60, 1] = 1.0                               # scene 0 votes class 1: inside
    c["scores"][60:, 5] = 1.0                               # scene 1 votes class 5: outside a table of 3
    return c


def _one_instance():
    c = make_case("every point in one instance", (700,), n_keep=[1], seed=18)
    c["point_instance"][:] = 0
    return c


def cases(lds_instances=None):
    """lds_instances: n_cls -> pbn_scene_summary_lds_instances(n_cls) (the GPU tier passes the library's; the CPU tier a stand-in:
    the restatement has one path)."""
    lds = (lambda k: 8) if lds_instances is None else lds_instances
    out = [make_case("n=%d" % n, (n,), seed=n) for n in (1, 63, 64, 65, 257)]
    out.append(make_case("an empty scene, workgroups across boundaries", (65, 0, 130), n_keep=[2, 0, 4], seed=2))
    out.append(make_case("tta layout", (97, 64), copies=3, n_keep=[4, 2], seed=3))
    out += [make_case("n_cls=%d ld=+3" % k, (130, 70), copies=2, n_cls=k, pad=3, labels=list(range(100, 100 + k)), seed=20 + k)
            for k in (1, 20, MAX_CLASSES)]
    out += [make_case("dtype %s" % d, (100, 45), copies=3, dtype=d, seed=4) for d in ("f32", "bf16", "f16")]
    out += [_equal_sums(), _equal_votes(), _copy_order(), _special_values()]
    for k in (20, MAX_CLASSES):
        edge = lds(k)
        for label, nk in [("0", 0), ("1", 1)] + ([("L", edge), ("L+1", edge + 1)] if edge > 0 else []):
            out.append(make_case("n_keep=%s n_cls=%d" % (label, k), (300, 520), n_cls=k, n_keep=[2, nk], n_prop=nk + 2, seed=30 + nk,
                                 labels=list(range(100, 100 + k)), unlabelled=0.05))
    out.append(make_case("no proposals", (70, 10), copies=2, n_keep=[0, 0], n_prop=0, seed=5))
    out.append(make_case("no coordinates", (90,), seed=6, with_xyz=False))
    out += [_one_instance(), _bad_coordinates(), _bad_instances(), _class_outside()]
    return out
