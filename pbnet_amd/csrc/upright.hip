// upright.hip -- the floor plane of a raw scan and the rotation that turns the scan upright (PCL / Open3D's segment_plane,
// a RANSAC plane fit with a least-squares refit over the inliers, then the minimal rotation of the normal onto +z).
//
// Contract: include/pbnet_hip.h ("Floor plane and upright frame"); tests/upright_ref.py restates it in numpy, stage by
// stage.  -ffp-contract=off, as cloud.hip: every float32 and float64 expression below is one rounded operation per operator.
//
//   hypotheses  one lane per hypothesis: three indices from the splitmix64 stream, the float64 plane through the three
//               points, the hint's sign and tilt rules, the float32 rounding (a, b, c, d) and a live flag.
//   score       THE hot kernel: N x H point-plane tests.  Lanes own hypotheses, points are wave-uniform.  A workgroup of
//               UPR_HYP_BLOCK lanes holds that many planes in four VGPRs each and two integer counters per lane, and takes
//               one chunk of points: it stages the chunk's packed [n, 3] floats into LDS with coalesced loads (as float4
//               rows, so a point is one aligned read), then every lane reads the same LDS address -- a broadcast, no bank
//               conflict -- and does six float32 operations, two compares and two adds.  No cross-lane traffic; one integer
//               atomicAdd per lane and counter at the end.  Grid: chunks x hypothesis blocks.  (-DPBN_UPRIGHT_UNIFORM
//               builds the other staging form, wave-uniform global loads of each point and no LDS: DESIGN.md 9g has both
//               measurements.)  The workgroups of hypothesis block 0 also raise SCAN_NONFINITE.
//   select      one workgroup: the sign rule without a hint, the floor rule, and the arg-max over the keys
//               live << 62 | in << 12 | (4095 - h).
//   moments     the winner's inliers summed in float64 with scan_dev.h's fixed-shape sum: the centroid, then the six
//               centred second moments.
//   refit       one thread: the Jacobi eigenvector of scan_dev.h, the plane, the rotation and their float32 roundings.
//   apply       one lane per point: xyz_out = R32 . p, height and floor.
#include <cmath>

#include "scan_dev.h"

namespace pbn {
namespace {

constexpr int UPR_EVENTS = 5;                     // around: hypotheses | score | select + refit | apply
constexpr int UPR_MAX_HYP = 4096;
constexpr int UPR_HYP_BLOCK = 256;                // hypotheses (lanes) of a score workgroup
constexpr int UPR_CHUNK = 1024;                   // points of a score workgroup; tests/upright_ref.py: SCORE_CHUNK
constexpr int UPR_CHUNK_MAX = 2048;               // 32 KiB of LDS
constexpr u64 UPR_LIVE = 1ull << 62;

__device__ __forceinline__ bool nonfinite32(float v) { return (__float_as_uint(v) & 0x7f800000u) == 0x7f800000u; }

// s of the contract: the signed float32 distance of a point from a float32 plane
__device__ __forceinline__ float plane_s(float a, float b, float c, float d, float x, float y, float z) {
    return ((a * x + b * y) + c * z) + d;
}

// ---- hypotheses --------------------------------------------------------------------------------------------------------
struct UprHint { double x, y, z, cos_tilt; int on; };

__global__ __launch_bounds__(TPB) void k_upr_hyp(const float* __restrict__ xyz, int n, int n_hyp, u64 seed, UprHint hint,
                                                 float4* __restrict__ planes, unsigned char* __restrict__ live) {
    const int h = blockIdx.x * TPB + threadIdx.x;
    if (h >= n_hyp) return;
    float4 pl = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    bool ok = false;
    if (n >= 3) {
        int i[3];
#pragma unroll
        for (int j = 0; j < 3; ++j) i[j] = (int)(((mix64(seed + 3ull * (u64)h + (u64)j) >> 32) * (u64)n) >> 32);
        if (i[0] != i[1] && i[0] != i[2] && i[1] != i[2]) {
            const double p0x = (double)xyz[3 * (size_t)i[0]], p0y = (double)xyz[3 * (size_t)i[0] + 1], p0z = (double)xyz[3 * (size_t)i[0] + 2];
            const double e1x = (double)xyz[3 * (size_t)i[1]] - p0x, e1y = (double)xyz[3 * (size_t)i[1] + 1] - p0y,
                         e1z = (double)xyz[3 * (size_t)i[1] + 2] - p0z;
            const double e2x = (double)xyz[3 * (size_t)i[2]] - p0x, e2y = (double)xyz[3 * (size_t)i[2] + 1] - p0y,
                         e2z = (double)xyz[3 * (size_t)i[2] + 2] - p0z;
            const double nx = e1y * e2z - e1z * e2y, ny = e1z * e2x - e1x * e2z, nz = e1x * e2y - e1y * e2x;
            const double q = (nx * nx + ny * ny) + nz * nz;
            if (q > 0.0 && __builtin_isfinite(q)) {
                const double r = sqrt(q);
                double ux = nx / r, uy = ny / r, uz = nz / r;
                double d = -((ux * p0x + uy * p0y) + uz * p0z);
                ok = true;
                if (hint.on) {
                    const double dot = (ux * hint.x + uy * hint.y) + uz * hint.z;
                    if (dot < 0.0) { ux = -ux; uy = -uy; uz = -uz; d = -d; }
                    if (fabs(dot) < hint.cos_tilt) ok = false;
                }
                if (ok) pl = make_float4((float)ux, (float)uy, (float)uz, (float)d);
            }
        }
    }
    planes[h] = pl;
    live[h] = ok ? 1 : 0;
}

// ---- score -------------------------------------------------------------------------------------------------------------
// grid (chunks of `chunk` points, blocks of UPR_HYP_BLOCK hypotheses); dynamic LDS: chunk float4 rows
__global__ __launch_bounds__(UPR_HYP_BLOCK) void k_upr_score(const float* __restrict__ xyz, int n, int chunk,
                                                             const float4* __restrict__ planes,
                                                             const unsigned char* __restrict__ live, int n_hyp, float t,
                                                             int* __restrict__ cin, int* __restrict__ cabove,
                                                             int* __restrict__ status) {
    const long long base = (long long)blockIdx.x * chunk;
    const int here = (int)min((long long)chunk, (long long)n - base);
    const float* __restrict__ src = xyz + 3 * (size_t)base;
    bool bad = false;
#ifndef PBN_UPRIGHT_UNIFORM
    extern __shared__ float4 s_pts[];
    float* s_f = (float*)s_pts;
    for (int e = threadIdx.x; e < 3 * here; e += UPR_HYP_BLOCK) {            // consecutive lanes, consecutive floats
        const float v = src[e];
        bad |= nonfinite32(v);
        const int p = e / 3;
        s_f[4 * p + (e - 3 * p)] = v;                                        // row p, column e % 3; column 3 is never read
    }
    __syncthreads();
#else
    if (blockIdx.y == 0)
        for (int e = threadIdx.x; e < 3 * here; e += UPR_HYP_BLOCK) bad |= nonfinite32(src[e]);
#endif
    if (blockIdx.y == 0 && __any(bad) && lane_id() == 0) atomicOr(status, SCAN_NONFINITE);
    const int h = blockIdx.y * UPR_HYP_BLOCK + threadIdx.x;
    const bool on = h < n_hyp && live[h];
    if (!__any(on)) return;                                                  // a wave without a live hypothesis
    const float4 pl = on ? planes[h] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    int ci = 0, ca = 0;
#pragma unroll 8
    for (int p = 0; p < here; ++p) {
#ifndef PBN_UPRIGHT_UNIFORM
        const float4 q = s_pts[p];                                           // one address for the wave: a broadcast
        const float s = plane_s(pl.x, pl.y, pl.z, pl.w, q.x, q.y, q.z);
#else
        const float s = plane_s(pl.x, pl.y, pl.z, pl.w, src[3 * p], src[3 * p + 1], src[3 * p + 2]);   // wave-uniform loads
#endif
        ci += fabsf(s) <= t ? 1 : 0;
        ca += s > t ? 1 : 0;
    }
    if (on) {
        if (ci) atomicAdd(&cin[h], ci);
        if (ca) atomicAdd(&cabove[h], ca);
    }
}

// ---- select ------------------------------------------------------------------------------------------------------------
// info: found, winner h, its in / above / below, (refit inliers: k_upr_centroid), live hypotheses, 0
__global__ __launch_bounds__(SUM_BLOCK) void k_upr_select(const float4* __restrict__ planes, const unsigned char* __restrict__ live,
                                                          const int* __restrict__ cin, const int* __restrict__ cabove, int n_hyp,
                                                          int n, int hinted, int max_below, int* __restrict__ info,
                                                          float* __restrict__ plane0) {
    __shared__ u64 s_key[SUM_BLOCK];
    __shared__ int s_live[SUM_BLOCK];
    u64 best = 0ull;
    int alive = 0;
    for (int h = threadIdx.x; h < n_hyp; h += SUM_BLOCK) {
        if (!live[h]) continue;
        const int in = cin[h];
        int above = cabove[h], below = n - in - above;
        if (!hinted && below > above) below = above;                         // negated: the two counts swap
        if (max_below >= 0 && below > max_below) continue;                   // the floor rule
        ++alive;
        const u64 key = UPR_LIVE | ((u64)in << 12) | (u64)(UPR_MAX_HYP - 1 - h);
        if (key > best) best = key;
    }
    s_key[threadIdx.x] = best;
    s_live[threadIdx.x] = alive;
    __syncthreads();
    for (int s = SUM_BLOCK / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) {
            if (s_key[threadIdx.x + s] > s_key[threadIdx.x]) s_key[threadIdx.x] = s_key[threadIdx.x + s];
            s_live[threadIdx.x] += s_live[threadIdx.x + s];
        }
        __syncthreads();
    }
    if (threadIdx.x != 0) return;
    best = s_key[0];
    info[6] = s_live[0];
    if (best == 0ull) return;                                                // info and plane0 stay zero
    const int h = UPR_MAX_HYP - 1 - (int)(best & (u64)(UPR_MAX_HYP - 1));
    const int in = cin[h];
    int above = cabove[h], below = n - in - above;
    float4 pl = planes[h];
    if (!hinted && below > above) {
        const int sw = above; above = below; below = sw;
        pl = make_float4(-pl.x, -pl.y, -pl.z, -pl.w);
    }
    info[0] = 1; info[1] = h; info[2] = in; info[3] = above; info[4] = below;
    plane0[0] = pl.x; plane0[1] = pl.y; plane0[2] = pl.z; plane0[3] = pl.w;
}

// ---- refit -------------------------------------------------------------------------------------------------------------
// psum: row-major [6][nb] block partials, pcnt[nb]
__global__ __launch_bounds__(SUM_BLOCK) void k_upr_mom1(const float* __restrict__ xyz, int n, const int* __restrict__ info,
                                                        const float* __restrict__ plane0, float t, int nb,
                                                        double* __restrict__ psum, int* __restrict__ pcnt) {
    if (info[0] == 0) return;
    __shared__ double v[3][SUM_BLOCK];
    const long long i = (long long)blockIdx.x * SUM_BLOCK + threadIdx.x;
    double x = 0.0, y = 0.0, z = 0.0;
    bool in = false;
    if (i < n) {
        const float fx = xyz[3 * (size_t)i], fy = xyz[3 * (size_t)i + 1], fz = xyz[3 * (size_t)i + 2];
        in = fabsf(plane_s(plane0[0], plane0[1], plane0[2], plane0[3], fx, fy, fz)) <= t;
        if (in) { x = (double)fx; y = (double)fy; z = (double)fz; }
    }
    v[0][threadIdx.x] = x; v[1][threadIdx.x] = y; v[2][threadIdx.x] = z;     // 0.0 where there is no inlier
    const int here = __syncthreads_count(in);
#pragma unroll
    for (int a = 0; a < 3; ++a) tree_sum(v[a]);
    if (threadIdx.x == 0) {
        for (int a = 0; a < 3; ++a) psum[(size_t)a * nb + blockIdx.x] = v[a][0];
        pcnt[blockIdx.x] = here;
    }
}

// moments[0] = the inliers, moments[1..3] = their centroid, info[5] = the inliers
__global__ __launch_bounds__(SUM_BLOCK) void k_upr_centroid(const double* __restrict__ psum, const int* __restrict__ pcnt, int nb,
                                                            int* __restrict__ info, double* __restrict__ moments) {
    if (info[0] == 0) return;
    __shared__ double s_v[SUM_BLOCK];
    __shared__ int s_c[SUM_BLOCK];
    const long long cnt = ordered_count(pcnt, nb, s_c);
    double sum[3];
    for (int a = 0; a < 3; ++a) sum[a] = ordered_total(psum + (size_t)a * nb, nb, s_v);
    if (threadIdx.x != 0) return;
    moments[0] = (double)cnt;
    for (int a = 0; a < 3; ++a) moments[1 + a] = sum[a] / (double)cnt;
    info[5] = (int)cnt;
}

__global__ __launch_bounds__(SUM_BLOCK) void k_upr_mom2(const float* __restrict__ xyz, int n, const int* __restrict__ info,
                                                        const float* __restrict__ plane0, float t, int nb,
                                                        const double* __restrict__ moments, double* __restrict__ psum) {
    if (info[0] == 0) return;
    __shared__ double v[6][SUM_BLOCK];
    const long long i = (long long)blockIdx.x * SUM_BLOCK + threadIdx.x;
    double m[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (i < n) {
        const float fx = xyz[3 * (size_t)i], fy = xyz[3 * (size_t)i + 1], fz = xyz[3 * (size_t)i + 2];
        if (fabsf(plane_s(plane0[0], plane0[1], plane0[2], plane0[3], fx, fy, fz)) <= t) {
            const double dx = (double)fx - moments[1], dy = (double)fy - moments[2], dz = (double)fz - moments[3];
            m[0] = dx * dx; m[1] = dx * dy; m[2] = dx * dz; m[3] = dy * dy; m[4] = dy * dz; m[5] = dz * dz;
        }
    }
#pragma unroll
    for (int a = 0; a < 6; ++a) v[a][threadIdx.x] = m[a];
#pragma unroll
    for (int a = 0; a < 6; ++a) tree_sum(v[a]);
    if (threadIdx.x == 0)
        for (int a = 0; a < 6; ++a) psum[(size_t)a * nb + blockIdx.x] = v[a][0];
}

// The six totals, then ONE thread: the refit plane, R and the float32 roundings apply reads (rp: R32[9], plane32[4]).
// Without a winner: plane and moments stay zero, R = I.
__global__ __launch_bounds__(SUM_BLOCK) void k_upr_refit(const double* __restrict__ psum, int nb, const int* __restrict__ info,
                                                         const float* __restrict__ plane0, double* __restrict__ moments,
                                                         double* __restrict__ plane, double* __restrict__ R,
                                                         float* __restrict__ rp) {
    __shared__ double s_v[SUM_BLOCK];
    const bool found = info[0] != 0;
    double m[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (found)
        for (int a = 0; a < 6; ++a) m[a] = ordered_total(psum + (size_t)a * nb, nb, s_v);
    if (threadIdx.x != 0) return;
    double r[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0};
    if (found) {
        for (int a = 0; a < 6; ++a) moments[4 + a] = m[a];
        double a = (double)plane0[0], b = (double)plane0[1], c = (double)plane0[2], d = (double)plane0[3];
        if (moments[0] >= 3.0) {                                             // fewer: the hypothesis plane stands
            double nx, ny, nz;
            jacobi_smallest(m[0], m[1], m[2], m[3], m[4], m[5], nx, ny, nz);
            const double dot = (nx * a + ny * b) + nz * c;
            if (dot < 0.0) { nx = -nx; ny = -ny; nz = -nz; }
            a = nx; b = ny; c = nz;
            d = -((nx * moments[1] + ny * moments[2]) + nz * moments[3]);
        }
        plane[0] = a; plane[1] = b; plane[2] = c; plane[3] = d;
        const double k = 1.0 + c;
        if (k > 0.0) {
            const double ab = -((a * b) / k);
            r[0] = 1.0 - (a * a) / k; r[1] = ab; r[2] = -a;
            r[3] = ab; r[4] = 1.0 - (b * b) / k; r[5] = -b;
            r[6] = a; r[7] = b; r[8] = c;
        } else {
            r[4] = -1.0; r[8] = -1.0;                                        // the normal is -z: half a turn about x
        }
        for (int j = 0; j < 4; ++j) rp[9 + j] = (float)plane[j];
    }
    for (int j = 0; j < 9; ++j) { R[j] = r[j]; rp[j] = (float)r[j]; }
}

// ---- apply -------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TPB) void k_upr_apply(const float* __restrict__ xyz, int n, const int* __restrict__ info,
                                                   const float* __restrict__ rp, float t, float* __restrict__ xyz_out,
                                                   unsigned char* __restrict__ floor_out, float* __restrict__ height) {
    const bool found = info[0] != 0;
    float r[13];
#pragma unroll
    for (int j = 0; j < 13; ++j) r[j] = found ? rp[j] : 0.0f;
    for (long long i = (long long)blockIdx.x * TPB + threadIdx.x; i < n; i += (long long)gridDim.x * TPB) {
        const float x = xyz[3 * (size_t)i], y = xyz[3 * (size_t)i + 1], z = xyz[3 * (size_t)i + 2];
        float ox = x, oy = y, oz = z, hgt = 0.0f;
        unsigned char fl = 0;
        if (found) {
            ox = (r[0] * x + r[1] * y) + r[2] * z;
            oy = (r[3] * x + r[4] * y) + r[5] * z;
            oz = (r[6] * x + r[7] * y) + r[8] * z;
            hgt = plane_s(r[9], r[10], r[11], r[12], x, y, z);
            fl = fabsf(hgt) <= t ? 1 : 0;
        }
        if (xyz_out) { xyz_out[3 * (size_t)i] = ox; xyz_out[3 * (size_t)i + 1] = oy; xyz_out[3 * (size_t)i + 2] = oz; }
        floor_out[i] = fl;
        height[i] = hgt;
    }
}

// ---- host --------------------------------------------------------------------------------------------------------------
struct UprWs { float4* planes; unsigned char* live; int* cin; int* cabove; double* psum; int* pcnt; float* rp; };

UprWs upr_carve(Carver& cv, int n) {
    UprWs w{};
    const size_t nb = (size_t)cdiv(n > 0 ? n : 1, SUM_BLOCK);
    w.planes = cv.take<float4>(UPR_MAX_HYP);
    w.live = cv.take<unsigned char>(UPR_MAX_HYP);
    w.cin = cv.take<int>(UPR_MAX_HYP);
    w.cabove = cv.take<int>(UPR_MAX_HYP);
    w.psum = cv.take<double>(6 * nb);
    w.pcnt = cv.take<int>(nb);
    w.rp = cv.take<float>(16);
    return w;
}

size_t upr_ws_bytes(int n) {
    Carver cv(nullptr, 0);
    upr_carve(cv, n);
    return cv.off + 256;
}

struct UprArgs {
    const float* xyz; int n; float t; int n_hyp; u64 seed; const double* up_hint; double cos_tilt; int max_below;
    float* xyz_out; uint8_t* floor; float* height; double* plane; float* plane0; double* R; double* moments; int32_t* info;
    int32_t* status; void* ws; size_t ws_bytes;
};

int upr_check(const UprArgs& a, int chunk) {
    if (a.n < 0 || a.n > SCAN_MAX_POINTS || a.n_hyp < 1 || a.n_hyp > UPR_MAX_HYP || !(a.t > 0.0f) || !std::isfinite(a.t))
        return PBN_ERR_ARG;
    if (chunk < 1 || chunk > UPR_CHUNK_MAX || a.max_below < -1) return PBN_ERR_ARG;
    if (a.up_hint && !(std::isfinite(a.up_hint[0]) && std::isfinite(a.up_hint[1]) && std::isfinite(a.up_hint[2]) &&
                       std::isfinite(a.cos_tilt)))
        return PBN_ERR_ARG;
    if ((a.n && (!a.xyz || !a.floor || !a.height)) || !a.plane || !a.plane0 || !a.R || !a.moments || !a.info || !a.status || !a.ws)
        return PBN_ERR_ARG;
    if (a.ws_bytes < upr_ws_bytes(a.n)) return PBN_ERR_WORKSPACE;
    return PBN_OK;
}

// ev (optional): UPR_EVENTS events
int upr_run(const UprArgs& a, int chunk, hipStream_t st, hipEvent_t* ev) {
    Carver cv(a.ws, a.ws_bytes);
    const UprWs w = upr_carve(cv, a.n);
    if (!cv.ok) return PBN_ERR_WORKSPACE;
    const int n = a.n, H = a.n_hyp, nb = cdiv(n, SUM_BLOCK);
    const FillRange fr[] = {{a.status, sizeof(int32_t), 0}, {a.info, 8 * sizeof(int32_t), 0}, {a.moments, 10 * sizeof(double), 0},
                            {a.plane, 4 * sizeof(double), 0}, {a.plane0, 4 * sizeof(float), 0},
                            {w.cin, UPR_MAX_HYP * sizeof(int), 0}, {w.cabove, UPR_MAX_HYP * sizeof(int), 0}};
    const int rc = fill_ranges(fr, 7, st);
    if (rc != PBN_OK) return rc;
    if (ev) PBN_HIP_CHECK(hipEventRecord(ev[0], st));
    if (n == 0) {                                                            // nothing that indexes: R = I from found = 0
        hipLaunchKernelGGL(k_upr_refit, dim3(1), dim3(SUM_BLOCK), 0, st, w.psum, 0, a.info, a.plane0, a.moments, a.plane, a.R, w.rp);
        PBN_LAUNCH_CHECK();
        if (ev) for (int i = 1; i < UPR_EVENTS; ++i) PBN_HIP_CHECK(hipEventRecord(ev[i], st));
        return PBN_OK;
    }
    UprHint hint{0.0, 0.0, 0.0, 0.0, 0};
    if (a.up_hint) hint = UprHint{a.up_hint[0], a.up_hint[1], a.up_hint[2], a.cos_tilt, 1};
    hipLaunchKernelGGL(k_upr_hyp, dim3(cdiv(H, TPB)), dim3(TPB), 0, st, a.xyz, n, H, a.seed, hint, w.planes, w.live);
    PBN_LAUNCH_CHECK();
    if (ev) PBN_HIP_CHECK(hipEventRecord(ev[1], st));
#ifndef PBN_UPRIGHT_UNIFORM
    const size_t lds = (size_t)chunk * sizeof(float4);
#else
    const size_t lds = 0;
#endif
    hipLaunchKernelGGL(k_upr_score, dim3(cdiv(n, chunk), cdiv(H, UPR_HYP_BLOCK)), dim3(UPR_HYP_BLOCK), lds, st, a.xyz, n, chunk,
                       w.planes, w.live, H, a.t, w.cin, w.cabove, a.status);
    PBN_LAUNCH_CHECK();
    if (ev) PBN_HIP_CHECK(hipEventRecord(ev[2], st));
    hipLaunchKernelGGL(k_upr_select, dim3(1), dim3(SUM_BLOCK), 0, st, w.planes, w.live, w.cin, w.cabove, H, n, a.up_hint ? 1 : 0,
                       a.max_below, a.info, a.plane0);
    hipLaunchKernelGGL(k_upr_mom1, dim3(nb), dim3(SUM_BLOCK), 0, st, a.xyz, n, a.info, a.plane0, a.t, nb, w.psum, w.pcnt);
    hipLaunchKernelGGL(k_upr_centroid, dim3(1), dim3(SUM_BLOCK), 0, st, w.psum, w.pcnt, nb, a.info, a.moments);
    hipLaunchKernelGGL(k_upr_mom2, dim3(nb), dim3(SUM_BLOCK), 0, st, a.xyz, n, a.info, a.plane0, a.t, nb, a.moments, w.psum);
    hipLaunchKernelGGL(k_upr_refit, dim3(1), dim3(SUM_BLOCK), 0, st, w.psum, nb, a.info, a.plane0, a.moments, a.plane, a.R, w.rp);
    PBN_LAUNCH_CHECK();
    if (ev) PBN_HIP_CHECK(hipEventRecord(ev[3], st));
    hipLaunchKernelGGL(k_upr_apply, dim3(grid_for(n, 4096)), dim3(TPB), 0, st, a.xyz, n, a.info, w.rp, a.t, a.xyz_out, a.floor,
                       a.height);
    PBN_LAUNCH_CHECK();
    if (ev) PBN_HIP_CHECK(hipEventRecord(ev[4], st));
    return PBN_OK;
}

}  // namespace
}  // namespace pbn

using namespace pbn;

extern "C" size_t pbn_cloud_upright_workspace_bytes(int n_points, int n_hyp) {
    if (n_points < 0 || n_points > SCAN_MAX_POINTS || n_hyp < 1 || n_hyp > UPR_MAX_HYP) return 0;
    return upr_ws_bytes(n_points);
}

extern "C" int pbn_cloud_upright_max_hyp(void) { return UPR_MAX_HYP; }
extern "C" int pbn_cloud_upright_chunk(void) { return UPR_CHUNK; }
extern "C" int pbn_cloud_upright_hyp_block(void) { return UPR_HYP_BLOCK; }

extern "C" int pbn_cloud_upright_chunked(const float* xyz, int n_points, float threshold, int n_hyp, uint64_t seed,
                                         const double* up_hint, double cos_tilt, int max_below, int chunk, float* xyz_out,
                                         uint8_t* floor, float* height, double* plane, float* plane0, double* R, double* moments,
                                         int32_t* info, int32_t* status, void* workspace, size_t workspace_bytes,
                                         pbn_stream_t stream) {
    const UprArgs a{xyz, n_points, threshold, n_hyp, (u64)seed, up_hint, cos_tilt, max_below, xyz_out, floor, height, plane, plane0,
                    R, moments, info, status, workspace, workspace_bytes};
    const int rc = upr_check(a, chunk);
    if (rc != PBN_OK) return rc;
    return upr_run(a, chunk, (hipStream_t)stream, nullptr);
}

extern "C" int pbn_cloud_upright(const float* xyz, int n_points, float threshold, int n_hyp, uint64_t seed, const double* up_hint,
                                 double cos_tilt, int max_below, float* xyz_out, uint8_t* floor, float* height, double* plane,
                                 float* plane0, double* R, double* moments, int32_t* info, int32_t* status, void* workspace,
                                 size_t workspace_bytes, pbn_stream_t stream) {
    return pbn_cloud_upright_chunked(xyz, n_points, threshold, n_hyp, seed, up_hint, cos_tilt, max_below, UPR_CHUNK, xyz_out, floor,
                                     height, plane, plane0, R, moments, info, status, workspace, workspace_bytes, stream);
}

extern "C" int pbn_cloud_upright_timed(const float* xyz, int n_points, float threshold, int n_hyp, uint64_t seed,
                                       const double* up_hint, double cos_tilt, int max_below, float* xyz_out, uint8_t* floor,
                                       float* height, double* plane, float* plane0, double* R, double* moments, int32_t* info,
                                       int32_t* status, void* workspace, size_t workspace_bytes, pbn_stream_t stream,
                                       float* times_ms) {
    const UprArgs a{xyz, n_points, threshold, n_hyp, (u64)seed, up_hint, cos_tilt, max_below, xyz_out, floor, height, plane, plane0,
                    R, moments, info, status, workspace, workspace_bytes};
    const int rc = upr_check(a, UPR_CHUNK);
    if (rc != PBN_OK) return rc;
    if (!times_ms) return PBN_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    return timed_stages<UPR_EVENTS>(st, times_ms, [&](hipEvent_t* ev) { return upr_run(a, UPR_CHUNK, st, ev); });
}
