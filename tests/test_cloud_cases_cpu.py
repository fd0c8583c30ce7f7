"""The designed clouds that aim at csrc/cloud.hip's one shell walk (tests/cloud_cases.py) have the properties they are
there for; tests/test_cloud_gpu.py runs every one of them against the brute force."""
import numpy as np

import cloud_cases as C
import cloud_ref


def _grid(pts, cell):
    """k_cloud_grid for a caller-given cell: (h, cells per axis) after the widening to the table's cap."""
    mn, mx = pts.min(0).astype(np.float64), pts.max(0).astype(np.float64)
    t_cap = min(1 << 20, max(4096, 4 * pts.shape[0]))
    h = max(float(cell), (mx - mn).max() / 1023.0 * (1.0 + 1.0e-9))
    while True:
        dims = np.minimum(np.floor((mx - mn) / h), 1023).astype(np.int64) + 1
        if dims.prod() <= t_cap:
            return h, dims
        h *= 1.25


def test_collinear_has_two_axes_of_one_cell():
    pts, cell = C.CASES["collinear"]
    assert cell is None and pts.shape == (300, 3)
    assert np.ptp(pts[:, 1]) == 0 and np.ptp(pts[:, 2]) == 0 and np.ptp(pts[:, 0]) > 9


def test_face_tie_ties_the_kth_d2_with_the_bound_and_a_lower_index_across_the_face():
    pts, cell = C.CASES["face_tie"]
    h, dims = _grid(pts, cell)
    assert h == 1.0 and dims.tolist() == [5, 1, 1]
    cells = np.floor((pts[:, 0].astype(np.float64) - 0.0) / h).astype(int)
    assert cells.tolist() == [2, 1, 1, 0, 4]                 # the query and point 2 share cell 1; point 0 lies across the face
    keys = cloud_ref.knn_keys(pts, 2)
    idx, d2 = cloud_ref.split(keys)
    assert idx[1].tolist() == [0, 2] and d2[1].tolist() == [0.25, 0.25]
    # the bound after shell 0, as the kernel computes it: (gap - 2^-38) / inv * (1 - 2^-40), rounded to float32, squared
    bound = np.float32((0.5 - 2.0 ** -38) / 1.0 * (1.0 - 2.0 ** -40))
    assert np.float32(bound * bound) == np.float32(0.25)     # k-th d2 == bound2: `<` goes on, `<=` would keep point 2


def test_sparse_small_cell_needs_shells_beyond_the_first():
    pts, cell = C.CASES["sparse_small_cell"]
    h, dims = _grid(pts, cell)
    assert cell < h < 1.0 and dims.min() > 4
    d2 = cloud_ref.split(cloud_ref.knn_keys(pts, 6))[1]
    # after shell 1 no inner face is further than 2 h away: a k-th neighbour beyond that needs r >= 2
    assert np.sum(np.sqrt(d2[:, 5].astype(np.float64)) > 2.0 * h) >= 10


def test_one_cell_grid_has_no_inner_face():
    pts, cell = C.CASES["n257_one_cell"]
    assert _grid(pts, cell)[1].tolist() == [1, 1, 1] and pts.shape[0] == 257
