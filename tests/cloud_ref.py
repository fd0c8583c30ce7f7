"""numpy restatement of csrc/cloud.hip's two contracts (pbnet_amd.mesh.knn_graph / point_normals).

knn      brute force: d2(i, j) = ((dx*dx + dy*dy) + dz*dz), dx = x[j] - x[i], in float32 (numpy's element-wise float32
         arithmetic is IEEE-rounded per operation and never fused); row i = the k points j != i with the smallest key
         (bits of d2 as uint32, j), ascending; short rows end in idx = -1, d2 = +inf.
normals  S = i, then its valid neighbours in rank order; float64 mean and covariance sums accumulated in that order;
         numpy.linalg.eigh's eigenvector of the smallest eigenvalue, flipped when n . (viewpoint - p) < 0.
"""
import numpy as np

F32 = np.float32
PAD = (np.uint64(0x7f800000) << np.uint64(32)) | np.uint64(0xffffffff)       # d2 = +inf, idx = -1


def knn_keys(xyz, k, chunk=512):
    """uint64 [N, k]: (bits of d2 << 32) | j, ascending; PAD where a row has fewer than k other points."""
    xyz = np.ascontiguousarray(xyz, F32)
    n = xyz.shape[0]
    out = np.full((n, k), PAD, np.uint64)
    j = np.arange(n, dtype=np.uint64)
    take = min(k, max(n - 1, 0))
    for lo in range(0, n, chunk):
        q = xyz[lo:lo + chunk]
        dx = xyz[None, :, 0] - q[:, None, 0]
        dy = xyz[None, :, 1] - q[:, None, 1]
        dz = xyz[None, :, 2] - q[:, None, 2]
        d2 = (dx * dx + dy * dy) + dz * dz
        assert d2.dtype == F32
        key = (d2.view(np.uint32).astype(np.uint64) << np.uint64(32)) | j[None, :]
        rows = np.arange(q.shape[0])
        key[rows, lo + rows] = np.uint64(0xffffffffffffffff)                   # self: excluded by index
        key.sort(axis=1)
        out[lo:lo + chunk, :take] = key[:, :take]
    return out


def split(keys):
    idx = (keys & np.uint64(0xffffffff)).astype(np.uint32).view(np.int32)
    d2 = (keys >> np.uint64(32)).astype(np.uint32).view(F32)
    return idx, d2


def knn(xyz, k):
    """(idx int32 [N, k], d2 float32 [N, k])."""
    return split(knn_keys(xyz, k))


def knn_loop(xyz, k):
    """The same contract said a second way: a Python loop over rows, float32 scalars, the built-in sorted."""
    xyz = np.asarray(xyz, F32)
    n = xyz.shape[0]
    idx = np.full((n, k), -1, np.int32)
    d2 = np.full((n, k), np.inf, F32)
    for i in range(n):
        cand = []
        for j in range(n):
            if j == i:
                continue
            dx, dy, dz = xyz[j, 0] - xyz[i, 0], xyz[j, 1] - xyz[i, 1], xyz[j, 2] - xyz[i, 2]
            d = F32(F32(F32(dx * dx) + F32(dy * dy)) + F32(dz * dz))
            cand.append((int(np.array(d, F32).view(np.uint32)), j, d))
        for r, (_, j, d) in enumerate(sorted(cand)[:k]):
            idx[i, r], d2[i, r] = j, d
    return idx, d2


def normals(xyz, idx, viewpoint=None):
    """Returns (n float64 [N, 3], gap float64 [N] = (l1 - l0) / l2 (0 where l2 is 0), m int [N] = |S|).  Rows with
    |S| < 3 are zero."""
    p = np.asarray(xyz, F32).astype(np.float64)
    idx = np.asarray(idx)
    n, k = idx.shape
    vp = p.mean(0) if viewpoint is None else np.asarray(viewpoint, np.float64).reshape(3)
    vp = vp.astype(F32).astype(np.float64)                                    # uploaded as three floats
    valid = (idx >= 0) & (idx < n)
    safe = np.where(valid, idx, 0)
    s = p.copy()
    m = np.ones(n, np.int64)
    for r in range(k):
        s = s + np.where(valid[:, r, None], p[safe[:, r]], 0.0)
        m += valid[:, r]
    mean = s / m[:, None]
    d = p - mean
    cov = d[:, :, None] * d[:, None, :]
    for r in range(k):
        d = p[safe[:, r]] - mean
        cov = cov + np.where(valid[:, r, None, None], d[:, :, None] * d[:, None, :], 0.0)
    lam, vec = np.linalg.eigh(cov)
    nrm = vec[:, :, 0].copy()
    flip = np.einsum("ij,ij->i", nrm, vp[None, :] - p) < 0
    nrm[flip] = -nrm[flip]
    with np.errstate(invalid="ignore", divide="ignore"):
        gap = np.where(lam[:, 2] > 0, (lam[:, 1] - lam[:, 0]) / lam[:, 2], 0.0)
    nrm[m < 3] = 0.0
    return nrm, gap, m


def edges(idx):
    """mesh.knn_edges: rows (i, idx[i, r]), i-major and rank-minor, -1 dropped."""
    idx = np.asarray(idx)
    n, k = idx.shape
    src = np.repeat(np.arange(n, dtype=np.int64), k)
    dst = idx.reshape(-1).astype(np.int64)
    keep = dst >= 0
    return np.stack([src[keep], dst[keep]], axis=1)
