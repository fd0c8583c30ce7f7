// scan_dev.h -- what the stages of the scan-decode chain (mesh.hip, cloud.hip, thin.hip, vote.hip, orient.hip) share around
// radix_sort_u32 (sort_dev.h, which this includes): the chain's limits and status bits, the launch grid, the stage timing of
// the *_timed entry points, and the two float64 device helpers that more than one stage states its contract with: the
// fixed-shape sum (thin.hip, upright.hip) and the Jacobi eigenvector (cloud.hip, upright.hip).  Those two are one rounded
// operation per expression: every translation unit that calls them is built with -ffp-contract=off.
#pragma once
#include <cmath>

#include "sort_dev.h"

namespace pbn {
namespace {

// ---- limits and status bits ----------------------------------------------------------------------------------------------
constexpr int SCAN_MAX_POINTS = 1 << 28;          // points of a cloud, raw or kept
constexpr int SCAN_MAX_K = 32;                    // neighbours per point
// Bits of a stage's status word that mean the same in every stage (pbnet_amd/mesh.py mirrors them as CLOUD_*).
enum : int {
    SCAN_NONFINITE = 1,                           // k_cloud_box: a coordinate is NaN or infinite
    SCAN_EXTENT = 2,                              // k_thin_keys: an axis spans 2^21 cells or more
    SCAN_SORT_SPIN = SORT_SPIN,                   // radix_sort_u32: a chained scan gave up
    SCAN_WALK_CAP = 16,                           // k_orient_jump: a link chain did not end within n hops
};

// blocks of a striding grid over n items: at least one, at most cap
inline int grid_for(long long n, int cap = 1024) {
    const long long b = (n + TPB - 1) / TPB;
    return (int)(b < 1 ? 1 : b > cap ? cap : b);
}

// ---- the fixed-shape float64 sum ---------------------------------------------------------------------------------------
// Blocks of SUM_BLOCK consecutive indices; inside a block the tree v[j] += v[j + s], s = 128 .. 1, absent entries 0.0; then
// the block partials added in block order by one thread.
constexpr int SUM_BLOCK = 256;

// v[0] = the tree over the block's 256 entries; every thread of the block calls it
__device__ __forceinline__ void tree_sum(double* v) {
    __syncthreads();
#pragma unroll
    for (int s = SUM_BLOCK / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) v[threadIdx.x] = v[threadIdx.x] + v[threadIdx.x + s];
        __syncthreads();
    }
}

// The nb block partials in block order, added by ONE thread (the block only stages them in LDS, s_v[SUM_BLOCK]); every thread
// of a SUM_BLOCK-wide block calls it, thread 0's return value is the sum.
__device__ __forceinline__ double ordered_total(const double* __restrict__ psum, int nb, double* s_v) {
    double sum = 0.0;
    for (int base = 0; base < nb; base += SUM_BLOCK) {
        const int b = base + (int)threadIdx.x;
        s_v[threadIdx.x] = b < nb ? psum[b] : 0.0;
        __syncthreads();
        if (threadIdx.x == 0) {
            const int here = min(SUM_BLOCK, nb - base);
            for (int j = 0; j < here; ++j) sum = sum + s_v[j];
        }
        __syncthreads();
    }
    return sum;
}

// the same walk over the blocks' integer counts (their order does not matter; one thread keeps it simple)
__device__ __forceinline__ long long ordered_count(const int* __restrict__ pcnt, int nb, int* s_c) {
    long long cnt = 0;
    for (int base = 0; base < nb; base += SUM_BLOCK) {
        const int b = base + (int)threadIdx.x;
        s_c[threadIdx.x] = b < nb ? pcnt[b] : 0;
        __syncthreads();
        if (threadIdx.x == 0) {
            const int here = min(SUM_BLOCK, nb - base);
            for (int j = 0; j < here; ++j) cnt += s_c[j];
        }
        __syncthreads();
    }
    return cnt;
}

// ---- the eigenvector of a symmetric 3x3's smallest eigenvalue ----------------------------------------------------------
constexpr int JACOBI_SWEEPS = 10;

// one Jacobi rotation of the symmetric 3x3 (app, aqq, apq; apr, aqr the couplings to the third axis) and of the columns
// vp, vq of the eigenvector matrix (Numerical Recipes' jacobi, t = sgn(theta) / (|theta| + sqrt(theta^2 + 1)))
__device__ __forceinline__ void jacobi_rot(double& app, double& aqq, double& apq, double& apr, double& aqr, double& vp0,
                                           double& vp1, double& vp2, double& vq0, double& vq1, double& vq2) {
    if (apq == 0.0) return;
    const double theta = (aqq - app) / (2.0 * apq);
    const double tt = (theta < 0.0 ? -1.0 : 1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));   // an infinite theta gives 0
    const double c = 1.0 / sqrt(tt * tt + 1.0), s = tt * c;
    app = app - tt * apq;
    aqq = aqq + tt * apq;
    apq = 0.0;
    const double pr = c * apr - s * aqr, qr = s * apr + c * aqr;
    apr = pr; aqr = qr;
    double a, b;
    a = c * vp0 - s * vq0; b = s * vp0 + c * vq0; vp0 = a; vq0 = b;
    a = c * vp1 - s * vq1; b = s * vp1 + c * vq1; vp1 = a; vq1 = b;
    a = c * vp2 - s * vq2; b = s * vp2 + c * vq2; vp2 = a; vq2 = b;
}

// JACOBI_SWEEPS fixed sweeps (01, 02, 12) from V = I, then the column of the smallest diagonal entry (ties keep the lowest
// axis) divided by its length; (1, 0, 0) when that length is zero or not finite
__device__ __forceinline__ void jacobi_smallest(double a00, double a01, double a02, double a11, double a12, double a22,
                                                double& nx, double& ny, double& nz) {
    double v00 = 1.0, v10 = 0.0, v20 = 0.0, v01 = 0.0, v11 = 1.0, v21 = 0.0, v02 = 0.0, v12 = 0.0, v22 = 1.0;   // v[row][col]
    for (int sweep = 0; sweep < JACOBI_SWEEPS; ++sweep) {
        jacobi_rot(a00, a11, a01, a02, a12, v00, v10, v20, v01, v11, v21);
        jacobi_rot(a00, a22, a02, a01, a12, v00, v10, v20, v02, v12, v22);
        jacobi_rot(a11, a22, a12, a01, a02, v01, v11, v21, v02, v12, v22);
    }
    // blended with exact 0 / 1 weights: a chain of selects over nine doubles is turned into an indexed table in scratch
    const int col = a22 < fmin(a00, a11) ? 2 : a11 < a00 ? 1 : 0;
    const double w0 = col == 0 ? 1.0 : 0.0, w1 = col == 1 ? 1.0 : 0.0, w2 = col == 2 ? 1.0 : 0.0;
    nx = (w0 * v00 + w1 * v01) + w2 * v02; ny = (w0 * v10 + w1 * v11) + w2 * v12; nz = (w0 * v20 + w1 * v21) + w2 * v22;
    const double len = sqrt((nx * nx + ny * ny) + nz * nz);
    if (len > 0.0 && __builtin_isfinite(len)) { nx = nx / len; ny = ny / len; nz = nz / len; }
    else { nx = 1.0; ny = 0.0; nz = 0.0; }                                   // unreachable for finite input: stay a unit vector
}

// ---- stage timing ------------------------------------------------------------------------------------------------------
// N events, destroyed on every path out of the scope that holds them
template <int N>
struct StageEvents {
    hipEvent_t ev[N];
    int n = 0;
    StageEvents() = default;
    StageEvents(const StageEvents&) = delete;
    StageEvents& operator=(const StageEvents&) = delete;
    ~StageEvents() { for (int i = 0; i < n; ++i) (void)hipEventDestroy(ev[i]); }
    hipError_t make() {
        for (; n < N; ++n) { const hipError_t e = hipEventCreate(&ev[n]); if (e != hipSuccess) return e; }
        return hipSuccess;
    }
};

// A *_timed entry point: body(ev) runs the stage and records ev[0..N-1] around its N - 1 steps; times_ms takes their
// elapsed times after a synchronisation of the stream.
template <int N, typename Body>
int timed_stages(hipStream_t st, float* times_ms, Body body) {
    StageEvents<N> evs;
    PBN_HIP_CHECK(evs.make());
    const int rc = body(evs.ev);
    if (rc != PBN_OK) return rc;
    PBN_HIP_CHECK(hipStreamSynchronize(st));
    for (int i = 0; i + 1 < N; ++i) PBN_HIP_CHECK(hipEventElapsedTime(&times_ms[i], evs.ev[i], evs.ev[i + 1]));
    return PBN_OK;
}

}  // namespace
}  // namespace pbn
