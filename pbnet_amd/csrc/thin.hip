// thin.hip -- a raw sensor scan brought to the network's pitch, and the answer carried back to the raw points.
//
//   thin      one point per occupied cell of a grid of `pitch`: the float64 centroid of the cell's members;
//   outliers  statistical outlier removal over the d2 table pbn_cloud_knn already wrote;
//   raw index for every raw point the row, among the kept points, that speaks for it.
//
// Every result is a pure function of the input, stated so that numpy can restate it (tests/thin_ref.py): no float atomics,
// no order left to the scheduler.  -ffp-contract=off, as cloud.hip: mu + ratio * sigma is a product, then a sum.
//
// Thinning.  Origin o[a] = the float32 minimum of axis a (cloud.hip's box kernel, with its non-finite flag).  Cell
// c[a] = floor((double(p[a]) - double(o[a])) / pitch), one subtraction and one correctly rounded division; the quotient is
// never negative.  c >= 2^21 on any axis raises SCAN_EXTENT.  key = cz << 42 | cy << 21 | cx (63 bits).  Order (key, index):
// radix_sort_u32 is stable and sorts 32-bit keys, so the low word goes first with values 0..n-1, then the high word with
// the first sort's order as values; ties of the second keep the first's order, ties of both keep the index order.  Runs of
// equal keys in that order are the cells: head flags, scan_exclusive_i32, and output row t is the t-th occupied cell in
// ascending key order.  One lane per cell walks its run from the head and adds the members' coordinates in float64 from 0.0
// in sorted = ascending index order; the quotient by double(count) is rounded once to float32.  The walk is as long as the
// fullest cell (a wave waits for its fullest); a run is never split over lanes, so the order of the additions is the
// contract's.  The number of cells lands next to the status word: result[0] = status, result[1] = M, one read-back.
//
// Outliers.  m_i = (the float64 sum, in rank order from 0.0, of sqrt(double(d2[i, r])) over the finite entries) / their
// number; a row without a finite entry has none.  Sums over points: blocks of 256 consecutive indices, inside a block the
// tree v[j] += v[j + s], s = 128 .. 1, absent entries 0.0, then the block partials added in block order by one thread.
// mu = sum m_i / n_valid; sigma = sqrt(sum (m_i - mu)^2 / n_valid), a second pass; keep_i = m_i <= mu + ratio * sigma.
#include <cmath>

#include "scan_dev.h"

namespace pbn {
namespace {

constexpr int THIN_AXIS_BITS = 21;
constexpr double THIN_AXIS_CELLS = 2097152.0;      // 2^21

__device__ __forceinline__ int in_rows(int j, int n) { return (unsigned)j < (unsigned)n ? j : 0; }   // only after a failed sort (flagged)

// ---- thinning ----------------------------------------------------------------------------------------------------------
// Keys are written whatever the status (0 for every point after a non-finite coordinate, 0 for a point outside the 2^21
// cells): the sorts below always see keys that match their histograms.
__global__ __launch_bounds__(TPB) void k_thin_keys(const float* __restrict__ xyz, int n, const unsigned* __restrict__ box,
                                                   int* __restrict__ status, double pitch, u64* __restrict__ cellkey,
                                                   u64* __restrict__ keys, int* __restrict__ vals, unsigned* __restrict__ ghist) {
    __shared__ unsigned s_hist[RADIX_U32_PASSES][RADIX];
    hist_clear(s_hist);
    __syncthreads();
    const bool bad = (*status & SCAN_NONFINITE) != 0;                        // the box kernel's word: final before this launch
    const double o0 = (double)okey32_val(box[0]), o1 = (double)okey32_val(box[1]), o2 = (double)okey32_val(box[2]);
    bool over = false;
    for (int i = blockIdx.x * TPB + threadIdx.x; i < n; i += gridDim.x * TPB) {
        u64 key = 0ull;
        if (!bad) {
            const double q0 = ((double)xyz[3 * (size_t)i] - o0) / pitch;
            const double q1 = ((double)xyz[3 * (size_t)i + 1] - o1) / pitch;
            const double q2 = ((double)xyz[3 * (size_t)i + 2] - o2) / pitch;
            if (q0 < THIN_AXIS_CELLS && q1 < THIN_AXIS_CELLS && q2 < THIN_AXIS_CELLS)      // q >= 0: p >= o and pitch > 0
                key = ((u64)floor(q2) << (2 * THIN_AXIS_BITS)) | ((u64)floor(q1) << THIN_AXIS_BITS) | (u64)floor(q0);
            else
                over = true;
        }
        cellkey[i] = key;
        keys[i] = key & 0xffffffffull;
        vals[i] = i;
        hist_add(s_hist, (unsigned)key);
    }
    if (over) atomicOr(status, SCAN_EXTENT);
    __syncthreads();
    hist_flush(s_hist, ghist);
}

// the high words in the order of the first sort, that order as their values
__global__ __launch_bounds__(TPB) void k_thin_high(const u64* __restrict__ cellkey, const int* __restrict__ order, int n,
                                                   u64* __restrict__ keys, int* __restrict__ vals, unsigned* __restrict__ ghist) {
    __shared__ unsigned s_hist[RADIX_U32_PASSES][RADIX];
    hist_clear(s_hist);
    __syncthreads();
    for (int s = blockIdx.x * TPB + threadIdx.x; s < n; s += gridDim.x * TPB) {
        const int j = in_rows(order[s], n);
        const unsigned hi = (unsigned)(cellkey[j] >> 32);
        keys[s] = (u64)hi;
        vals[s] = j;
        hist_add(s_hist, hi);
    }
    __syncthreads();
    hist_flush(s_hist, ghist);
}

__global__ __launch_bounds__(TPB) void k_thin_heads(const u64* __restrict__ cellkey, const int* __restrict__ order, int n,
                                                    int* __restrict__ head) {
    for (int s = blockIdx.x * TPB + threadIdx.x; s < n; s += gridDim.x * TPB)
        head[s] = (s == 0 || cellkey[in_rows(order[s], n)] != cellkey[in_rows(order[s - 1], n)]) ? 1 : 0;
}

// One lane per sorted position; the lane on a run's head owns the cell and walks the run.
__global__ __launch_bounds__(TPB) void k_thin_cells(const float* __restrict__ xyz, const float* __restrict__ rgb, int n,
                                                    const int* __restrict__ order, const int* __restrict__ head,
                                                    const int* __restrict__ before, const int* __restrict__ status,
                                                    float* __restrict__ out_xyz, float* __restrict__ out_rgb,
                                                    int* __restrict__ count, int* __restrict__ first, int* __restrict__ inverse) {
    if (*status != 0) return;                                                // nothing is written
    for (int s = blockIdx.x * TPB + threadIdx.x; s < n; s += gridDim.x * TPB) {
        const int j = order[s], h = head[s];
        const int row = before[s] + h - 1;                                   // heads before s, plus its own, minus one
        inverse[j] = row;
        if (!h) continue;
        double sx = 0.0, sy = 0.0, sz = 0.0, sr = 0.0, sg = 0.0, sb = 0.0;
        int t = s;
        do {
            const size_t m = 3 * (size_t)order[t];
            sx = sx + (double)xyz[m]; sy = sy + (double)xyz[m + 1]; sz = sz + (double)xyz[m + 2];
            if (rgb) { sr = sr + (double)rgb[m]; sg = sg + (double)rgb[m + 1]; sb = sb + (double)rgb[m + 2]; }
            ++t;
        } while (t < n && !head[t]);
        const double c = (double)(t - s);
        const size_t o = 3 * (size_t)row;
        out_xyz[o] = (float)(sx / c); out_xyz[o + 1] = (float)(sy / c); out_xyz[o + 2] = (float)(sz / c);
        if (rgb) { out_rgb[o] = (float)(sr / c); out_rgb[o + 1] = (float)(sg / c); out_rgb[o + 2] = (float)(sb / c); }
        count[row] = t - s;
        first[row] = j;                                                      // the run is in ascending index order
    }
}

struct ThinWs {
    unsigned* box; u64* cellkey; SortBufs sort; int* head; int* before; int* scan_tmp;      // sort 0: low word, sort 1: high word
};

ThinWs thin_carve(Carver& cv, int n) {
    ThinWs w{};
    const size_t N = (size_t)(n > 0 ? n : 1);
    w.box = cv.take<unsigned>(64);
    w.cellkey = cv.take<u64>(N);
    w.sort = sort_carve(cv, N, 2);
    w.head = cv.take<int>(N); w.before = cv.take<int>(N);
    w.scan_tmp = cv.take<int>(scan_tmp_ints((long long)N));
    return w;
}

size_t thin_ws_bytes(int n) {
    Carver cv(nullptr, 0);
    thin_carve(cv, n);
    return cv.off + 256;
}

constexpr int THIN_EVENTS = 6;      // around: box + keys | low sort | high keys + sort | heads + scan | cells

int thin_points(const float* xyz, const float* rgb, int n, double pitch, float* out_xyz, float* out_rgb, int32_t* count,
                int32_t* first, int32_t* inverse, int32_t* result, void* workspace, size_t workspace_bytes, hipStream_t st,
                hipEvent_t* ev) {
    Carver cv(workspace, workspace_bytes);
    const ThinWs w = thin_carve(cv, n);
    if (!cv.ok) return PBN_ERR_WORKSPACE;
    const FillRange fr[] = {{result, 2 * sizeof(int32_t), 0}, {w.box, 3 * sizeof(unsigned), 0xff},
                            {w.box + 3, 3 * sizeof(unsigned), 0}, sort_hist_fill(w.sort, 0), sort_hist_fill(w.sort, 1)};
    int rc = fill_ranges(fr, n > 0 ? 5 : 1, st);
    if (rc != PBN_OK) return rc;
    if (ev) PBN_HIP_CHECK(hipEventRecord(ev[0], st));
    if (n == 0) {
        if (ev) for (int i = 1; i < THIN_EVENTS; ++i) PBN_HIP_CHECK(hipEventRecord(ev[i], st));
        return PBN_OK;
    }
    int32_t* status = result;
    const dim3 grid(grid_for(n)), block(TPB);
    rc = cloud_box(xyz, n, w.box, status, st);
    if (rc != PBN_OK) return rc;
    hipLaunchKernelGGL(k_thin_keys, grid, block, 0, st, xyz, n, w.box, status, pitch, w.cellkey, w.sort.keys_a,
                       w.sort.vals_a, w.sort.ghist[0]);
    PBN_LAUNCH_CHECK();
    if (ev) PBN_HIP_CHECK(hipEventRecord(ev[1], st));
    rc = sort_run(w.sort, 0, n, status, st);
    if (rc != PBN_OK) return rc;
    if (ev) PBN_HIP_CHECK(hipEventRecord(ev[2], st));
    hipLaunchKernelGGL(k_thin_high, grid, block, 0, st, w.cellkey, w.sort.vals_b, n, w.sort.keys_a, w.sort.vals_a,
                       w.sort.ghist[1]);
    PBN_LAUNCH_CHECK();
    rc = sort_run(w.sort, 1, n, status, st);
    if (rc != PBN_OK) return rc;
    if (ev) PBN_HIP_CHECK(hipEventRecord(ev[3], st));
    hipLaunchKernelGGL(k_thin_heads, grid, block, 0, st, w.cellkey, w.sort.vals_b, n, w.head);
    PBN_LAUNCH_CHECK();
    rc = scan_exclusive_i32(w.head, w.before, n, w.scan_tmp, result + 1, st);
    if (rc != PBN_OK) return rc;
    if (ev) PBN_HIP_CHECK(hipEventRecord(ev[4], st));
    hipLaunchKernelGGL(k_thin_cells, grid, block, 0, st, xyz, rgb, n, w.sort.vals_b, w.head, w.before, status, out_xyz,
                       out_rgb, count, first, inverse);
    PBN_LAUNCH_CHECK();
    if (ev) PBN_HIP_CHECK(hipEventRecord(ev[5], st));
    return PBN_OK;
}

int thin_args(const float* xyz, const float* rgb, int n, double pitch, const float* out_xyz, const float* out_rgb,
              const int32_t* count, const int32_t* first, const int32_t* inverse, const int32_t* result, const void* workspace,
              size_t workspace_bytes) {
    if (n < 0 || n > SCAN_MAX_POINTS || !(pitch > 0.0) || !std::isfinite(pitch)) return PBN_ERR_ARG;
    if ((n && (!xyz || !out_xyz || !count || !first || !inverse)) || (n && rgb && !out_rgb) || !result || !workspace)
        return PBN_ERR_ARG;
    if (workspace_bytes < thin_ws_bytes(n)) return PBN_ERR_WORKSPACE;
    return PBN_OK;
}

// ---- outliers ----------------------------------------------------------------------------------------------------------
// SUM_BLOCK, tree_sum, ordered_total: scan_dev.h
__global__ __launch_bounds__(SUM_BLOCK) void k_outlier_mean(const float* __restrict__ d2, int n, int k, double* __restrict__ m,
                                                            unsigned char* __restrict__ valid, double* __restrict__ psum,
                                                            int* __restrict__ pcnt) {
    __shared__ double v[SUM_BLOCK];
    const long long i = (long long)blockIdx.x * SUM_BLOCK + threadIdx.x;
    double mi = 0.0;
    int cnt = 0;
    if (i < n) {
        double s = 0.0;
        for (int r = 0; r < k; ++r) {
            const float d = d2[(size_t)i * k + r];
            if ((__float_as_uint(d) & 0x7f800000u) == 0x7f800000u) continue;   // +-inf, NaN: no entry
            s = s + sqrt((double)d);
            ++cnt;
        }
        if (cnt) mi = s / (double)cnt;
        m[i] = mi;
        valid[i] = cnt ? 1 : 0;
    }
    v[threadIdx.x] = mi;                                                     // 0.0 where there is no m_i
    const int here = __syncthreads_count(cnt > 0);
    tree_sum(v);
    if (threadIdx.x == 0) { psum[blockIdx.x] = v[0]; pcnt[blockIdx.x] = here; }
}

__global__ __launch_bounds__(SUM_BLOCK) void k_outlier_dev(const double* __restrict__ m, const unsigned char* __restrict__ valid,
                                                           int n, const double* __restrict__ stats, double* __restrict__ psum) {
    __shared__ double v[SUM_BLOCK];
    const long long i = (long long)blockIdx.x * SUM_BLOCK + threadIdx.x;
    const double mu = stats[0];
    double e = 0.0;
    if (i < n && valid[i]) { const double d = m[i] - mu; e = d * d; }
    v[threadIdx.x] = e;
    tree_sum(v);
    if (threadIdx.x == 0) psum[blockIdx.x] = v[0];
}

// The block partials in block order, added by ONE thread (the block only stages them in LDS).  pass 0: stats[0] = mu,
// stats[2] = n_valid; pass 1: stats[1] = sigma.
__global__ __launch_bounds__(SUM_BLOCK) void k_outlier_total(const double* __restrict__ psum, const int* __restrict__ pcnt, int nb,
                                                             int pass, double* __restrict__ stats) {
    __shared__ double s_v[SUM_BLOCK];
    __shared__ int s_c[SUM_BLOCK];
    const double sum = ordered_total(psum, nb, s_v);
    const long long cnt = pass == 0 ? ordered_count(pcnt, nb, s_c) : 0;
    if (threadIdx.x != 0) return;
    if (pass == 0) {
        stats[0] = sum / (double)cnt;                                        // no valid row: 0 / 0 = NaN, and nothing is kept
        stats[2] = (double)cnt;
    } else {
        stats[1] = sqrt(sum / stats[2]);
    }
}

__global__ __launch_bounds__(TPB) void k_outlier_mask(const double* __restrict__ m, const unsigned char* __restrict__ valid, int n,
                                                      const double* __restrict__ stats, double ratio,
                                                      unsigned char* __restrict__ keep) {
    const double thr = stats[0] + ratio * stats[1];
    for (int i = blockIdx.x * TPB + threadIdx.x; i < n; i += gridDim.x * TPB) keep[i] = (valid[i] && m[i] <= thr) ? 1 : 0;
}

struct OutlierWs { double* m; unsigned char* valid; double* psum; int* pcnt; };

OutlierWs outlier_carve(Carver& cv, int n) {
    OutlierWs w{};
    const size_t N = (size_t)(n > 0 ? n : 1), nb = (size_t)cdiv((long long)N, SUM_BLOCK);
    w.m = cv.take<double>(N);
    w.valid = cv.take<unsigned char>(N);
    w.psum = cv.take<double>(nb);
    w.pcnt = cv.take<int>(nb);
    return w;
}

size_t outlier_ws_bytes(int n) {
    Carver cv(nullptr, 0);
    outlier_carve(cv, n);
    return cv.off + 256;
}

// ---- raw index ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TPB) void k_keep_flags(const unsigned char* __restrict__ keep, int m, int* __restrict__ flag) {
    for (int t = blockIdx.x * TPB + threadIdx.x; t < m; t += gridDim.x * TPB) flag[t] = keep[t] ? 1 : 0;
}

// before[t] = kept rows in front of t = t's row among the kept points when keep[t]
__global__ __launch_bounds__(TPB) void k_raw_index(const int* __restrict__ inverse, int n_raw, const unsigned char* __restrict__ keep,
                                                   const int* __restrict__ before, const int* __restrict__ idx, int m, int k,
                                                   int* __restrict__ out) {
    for (int i = blockIdx.x * TPB + threadIdx.x; i < n_raw; i += gridDim.x * TPB) {
        const int t = inverse[i];
        int row = -1;
        if ((unsigned)t < (unsigned)m) {
            if (keep[t]) row = before[t];
            else
                for (int r = 0; r < k; ++r) {                                // the first kept neighbour in rank order
                    const int j = idx[(size_t)t * k + r];
                    if ((unsigned)j < (unsigned)m && keep[j]) { row = before[j]; break; }
                }
        }
        out[i] = row;
    }
}

struct RawWs { int* flag; int* before; int* scan_tmp; };

RawWs raw_carve(Carver& cv, int m) {
    RawWs w{};
    const size_t M = (size_t)(m > 0 ? m : 1);
    w.flag = cv.take<int>(M); w.before = cv.take<int>(M);
    w.scan_tmp = cv.take<int>(scan_tmp_ints((long long)M));
    return w;
}

size_t raw_ws_bytes(int m) {
    Carver cv(nullptr, 0);
    raw_carve(cv, m);
    return cv.off + 256;
}

}  // namespace
}  // namespace pbn

using namespace pbn;

extern "C" size_t pbn_thin_workspace_bytes(int n_points) {
    if (n_points < 0 || n_points > SCAN_MAX_POINTS) return 0;
    return thin_ws_bytes(n_points);
}

extern "C" int pbn_thin_points(const float* xyz, const float* rgb, int n_points, double pitch, float* out_xyz, float* out_rgb,
                               int32_t* count, int32_t* first, int32_t* inverse, int32_t* result, void* workspace,
                               size_t workspace_bytes, pbn_stream_t stream) {
    const int rc = thin_args(xyz, rgb, n_points, pitch, out_xyz, out_rgb, count, first, inverse, result, workspace, workspace_bytes);
    if (rc != PBN_OK) return rc;
    return thin_points(xyz, rgb, n_points, pitch, out_xyz, out_rgb, count, first, inverse, result, workspace, workspace_bytes,
                       (hipStream_t)stream, nullptr);
}

extern "C" int pbn_thin_points_timed(const float* xyz, const float* rgb, int n_points, double pitch, float* out_xyz, float* out_rgb,
                                     int32_t* count, int32_t* first, int32_t* inverse, int32_t* result, void* workspace,
                                     size_t workspace_bytes, pbn_stream_t stream, float* times_ms) {
    const int rc = thin_args(xyz, rgb, n_points, pitch, out_xyz, out_rgb, count, first, inverse, result, workspace, workspace_bytes);
    if (rc != PBN_OK) return rc;
    if (!times_ms) return PBN_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    return timed_stages<THIN_EVENTS>(st, times_ms, [&](hipEvent_t* ev) {
        return thin_points(xyz, rgb, n_points, pitch, out_xyz, out_rgb, count, first, inverse, result, workspace, workspace_bytes, st,
                           ev);
    });
}

extern "C" size_t pbn_cloud_outlier_workspace_bytes(int n_points) {
    if (n_points < 0 || n_points > SCAN_MAX_POINTS) return 0;
    return outlier_ws_bytes(n_points);
}

extern "C" int pbn_cloud_outlier_mask(const float* d2, int n_points, int k, double ratio, uint8_t* keep, double* stats,
                                      void* workspace, size_t workspace_bytes, pbn_stream_t stream) {
    if (n_points < 0 || n_points > SCAN_MAX_POINTS || k < 1 || k > SCAN_MAX_K || !(ratio >= 0.0) || !std::isfinite(ratio))
        return PBN_ERR_ARG;
    if ((n_points && (!d2 || !keep)) || !stats || !workspace) return PBN_ERR_ARG;
    if (workspace_bytes < outlier_ws_bytes(n_points)) return PBN_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const int n = n_points;
    if (n == 0) return fill_bytes(stats, 0, 3 * sizeof(double), st);         // empty: mu = sigma = n_valid = 0
    Carver cv(workspace, workspace_bytes);
    const OutlierWs w = outlier_carve(cv, n);
    if (!cv.ok) return PBN_ERR_WORKSPACE;
    const int nb = cdiv(n, SUM_BLOCK);
    hipLaunchKernelGGL(k_outlier_mean, dim3(nb), dim3(SUM_BLOCK), 0, st, d2, n, k, w.m, w.valid, w.psum, w.pcnt);
    hipLaunchKernelGGL(k_outlier_total, dim3(1), dim3(SUM_BLOCK), 0, st, w.psum, w.pcnt, nb, 0, stats);
    hipLaunchKernelGGL(k_outlier_dev, dim3(nb), dim3(SUM_BLOCK), 0, st, w.m, w.valid, n, stats, w.psum);
    hipLaunchKernelGGL(k_outlier_total, dim3(1), dim3(SUM_BLOCK), 0, st, w.psum, w.pcnt, nb, 1, stats);
    hipLaunchKernelGGL(k_outlier_mask, dim3(grid_for(n)), dim3(TPB), 0, st, w.m, w.valid, n, stats, ratio, keep);
    PBN_LAUNCH_CHECK();
    return PBN_OK;
}

extern "C" size_t pbn_cloud_raw_index_workspace_bytes(int n_points) {
    if (n_points < 0 || n_points > SCAN_MAX_POINTS) return 0;
    return raw_ws_bytes(n_points);
}

extern "C" int pbn_cloud_raw_index(const int32_t* inverse, int n_raw, const uint8_t* keep, const int32_t* idx, int n_points, int k,
                                   int32_t* raw_index, void* workspace, size_t workspace_bytes, pbn_stream_t stream) {
    if (n_raw < 0 || n_raw > SCAN_MAX_POINTS || n_points < 0 || n_points > SCAN_MAX_POINTS || k < 1 || k > SCAN_MAX_K)
        return PBN_ERR_ARG;
    if ((n_raw && (!inverse || !raw_index)) || (n_points && (!keep || !idx)) || !workspace) return PBN_ERR_ARG;
    if (workspace_bytes < raw_ws_bytes(n_points)) return PBN_ERR_WORKSPACE;
    if (n_raw == 0) return PBN_OK;
    hipStream_t st = (hipStream_t)stream;
    Carver cv(workspace, workspace_bytes);
    const RawWs w = raw_carve(cv, n_points);
    if (!cv.ok) return PBN_ERR_WORKSPACE;
    if (n_points > 0) {
        hipLaunchKernelGGL(k_keep_flags, dim3(grid_for(n_points)), dim3(TPB), 0, st, keep, n_points, w.flag);
        PBN_LAUNCH_CHECK();
        const int rc = scan_exclusive_i32(w.flag, w.before, n_points, w.scan_tmp, nullptr, st);
        if (rc != PBN_OK) return rc;
    }
    hipLaunchKernelGGL(k_raw_index, dim3(grid_for(n_raw)), dim3(TPB), 0, st, inverse, n_raw, keep, w.before, idx, n_points, k,
                       raw_index);
    PBN_LAUNCH_CHECK();
    return PBN_OK;
}
