// tsdf.hip -- posed depth frames fused into a truncated signed distance volume and its surface points, on the device.
// include/pbnet_hip.h ("Depth-frame fusion") states the contract, tests/fuse_ref.py restates it in numpy.
//
//   blocks     the raw cloud's points -> their 8^3-voxel blocks (thin.hip's key with pitch B = 8 * voxel and an origin one
//              block below the minimum), unique by two radix sorts and run heads; every occupied block emits its 27
//              neighbours' keys into a padded array, unique again: the allocated blocks in ascending key order;
//   integrate  one workgroup per block, a voxel in one lane for ALL frames: S, Wt and C stay in registers and are stored
//              once, the volume is never read.  Frames are culled per block first: lanes own frames, 64 per ballot, the
//              block's bounding sphere against each frame's frustum; the waves then walk the set bits in ascending order;
//   extract    count | scan | write, as frames.hip: one workgroup per block, a lane owns two consecutive voxels, so lane
//              order is row order; neighbour blocks come from 27 binary searches per workgroup.
//
// No atomic touches an order or a float: two runs give the same bytes.  (The optional counters of the measurement entry are
// integer atomics beside the result.)
//
// Arithmetic contract (-ffp-contract=off): float64, one rounded operation per written operation; float32 on the store.
#include <cmath>
#include <vector>

#include "frames_dev.h"
#include "scan_dev.h"

namespace pbn {
namespace {

constexpr int FUSE_AXIS_BITS = 21;
constexpr double FUSE_AXIS_BLOCKS = 2097152.0;               // 2^21
constexpr int FUSE_MAX_BLOCKS = 1 << 21;
constexpr int FUSE_MAX_EXTRACT_BLOCKS = 1398101;             // floor((2^31 - 1) / 1536): the surface rows fit an int32
constexpr int FUSE_SIDE = 8, FUSE_VOXELS = 512;              // a block
constexpr int FUSE_PER_LANE = FUSE_VOXELS / TPB;             // voxels of a lane
constexpr int FUSE_TOO_MANY = 4;                             // status: more than 2^21 blocks
constexpr int FUSE_ROWS = 32;                                // status: a row at or beyond n_rows
constexpr u64 FUSE_PAD = ~0ull;                              // a slot of the padded key array that holds no block
constexpr int FUSE_BLOCKS_EVENTS = 4, FUSE_INTEGRATE_EVENTS = 2, FUSE_COUNT_EVENTS = 2, FUSE_WRITE_EVENTS = 2;
constexpr int FUSE_CAM = 16;                                 // doubles of a frame: Rt [9], tc [3], fx, fy, cx, cy

static_assert(FUSE_PER_LANE == 2, "the kernels below give a lane two voxels");

__device__ __forceinline__ int in_rows(int j, int n) { return (unsigned)j < (unsigned)n ? j : 0; }   // only after a failed sort (flagged)

// ---- blocks ------------------------------------------------------------------------------------------------------------
// key of every point's block; 0 after a non-finite coordinate, 0 and SCAN_EXTENT for a block whose +1 neighbour has no key
__global__ __launch_bounds__(TPB) void k_fuse_point_keys(const float* __restrict__ xyz, int n, const unsigned* __restrict__ box,
                                                         int* __restrict__ status, double B, u64* __restrict__ cellkey) {
    const bool bad = (*status & SCAN_NONFINITE) != 0;                        // the box kernel's word: final before this launch
    const double g0 = (double)okey32_val(box[0]) - B, g1 = (double)okey32_val(box[1]) - B, g2 = (double)okey32_val(box[2]) - B;
    bool over = false;
    for (int i = blockIdx.x * TPB + threadIdx.x; i < n; i += gridDim.x * TPB) {
        u64 key = 0ull;
        if (!bad) {
            // p >= min32, so the quotient is 1 up to its rounding: a point on the minimum may come out a last bit below 1 and
            // belongs to block 1 all the same.  The neighbour q + 1 needs a key too.
            const double q0 = fmax(floor(((double)xyz[3 * (size_t)i] - g0) / B), 1.0);
            const double q1 = fmax(floor(((double)xyz[3 * (size_t)i + 1] - g1) / B), 1.0);
            const double q2 = fmax(floor(((double)xyz[3 * (size_t)i + 2] - g2) / B), 1.0);
            // coordinate 2^21 - 1 stays free: a neighbour key is the key plus or minus 1, 2^21 or 2^42, and the borrow of
            // coordinate 0's lower neighbour lands on 2^21 - 1 of the next axis, which must never be a block
            if (q0 + 1.0 < FUSE_AXIS_BLOCKS - 1.0 && q1 + 1.0 < FUSE_AXIS_BLOCKS - 1.0 &&
                q2 + 1.0 < FUSE_AXIS_BLOCKS - 1.0)
                key = ((u64)q2 << (2 * FUSE_AXIS_BITS)) | ((u64)q1 << FUSE_AXIS_BITS) | (u64)q0;
            else
                over = true;
        }
        cellkey[i] = key;
    }
    if (over) atomicOr(status, SCAN_EXTENT);
}

// the 27 neighbour keys of every occupied block, in a padded array of `slots` keys
__global__ __launch_bounds__(TPB) void k_fuse_dilate(const u64* __restrict__ occ, const int* __restrict__ n_occ, int cap_occ,
                                                     const int* __restrict__ status, int slots, u64* __restrict__ cellkey) {
    const int m = *status != 0 ? 0 : min(*n_occ, cap_occ);
    for (int s = blockIdx.x * TPB + threadIdx.x; s < slots; s += gridDim.x * TPB) {
        const int i = s / 27, d = s % 27;
        u64 key = FUSE_PAD;
        if (i < m) {
            const long long dx = d % 3 - 1, dy = d / 3 % 3 - 1, dz = d / 9 - 1;
            key = (u64)((long long)occ[i] + dx + dy * (1ll << FUSE_AXIS_BITS) + dz * (1ll << (2 * FUSE_AXIS_BITS)));
        }
        cellkey[s] = key;
    }
}

// the low words with values 0..n-1; then the high words in the order of the first sort (thin.hip's two-word order)
__global__ __launch_bounds__(TPB) void k_fuse_low(const u64* __restrict__ cellkey, int n, u64* __restrict__ keys,
                                                  int* __restrict__ vals, unsigned* __restrict__ ghist) {
    __shared__ unsigned s_hist[RADIX_U32_PASSES][RADIX];
    hist_clear(s_hist);
    __syncthreads();
    for (int i = blockIdx.x * TPB + threadIdx.x; i < n; i += gridDim.x * TPB) {
        const unsigned lo = (unsigned)cellkey[i];
        keys[i] = (u64)lo;
        vals[i] = i;
        hist_add(s_hist, lo);
    }
    __syncthreads();
    hist_flush(s_hist, ghist);
}

__global__ __launch_bounds__(TPB) void k_fuse_high(const u64* __restrict__ cellkey, const int* __restrict__ order, int n,
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

__global__ __launch_bounds__(TPB) void k_fuse_heads(const u64* __restrict__ cellkey, const int* __restrict__ order, int n,
                                                    int* __restrict__ head) {
    for (int s = blockIdx.x * TPB + threadIdx.x; s < n; s += gridDim.x * TPB) {
        const u64 key = cellkey[in_rows(order[s], n)];
        head[s] = (key != FUSE_PAD && (s == 0 || key != cellkey[in_rows(order[s - 1], n)])) ? 1 : 0;
    }
}

// out[t] = the t-th distinct key, for t < cap
__global__ __launch_bounds__(TPB) void k_fuse_compact(const u64* __restrict__ cellkey, const int* __restrict__ order,
                                                      const int* __restrict__ head, const int* __restrict__ before, int n,
                                                      const int* __restrict__ status, u64* __restrict__ out, int cap) {
    if (*status != 0) return;
    for (int s = blockIdx.x * TPB + threadIdx.x; s < n; s += gridDim.x * TPB)
        if (head[s] && before[s] < cap) out[before[s]] = cellkey[in_rows(order[s], n)];
}

// result[2..4] = the bits of the float32 minimum per axis; the block limit
__global__ void k_fuse_blocks_result(const unsigned* __restrict__ box, const int* __restrict__ n_occ, int* __restrict__ result) {
    if (*n_occ > FUSE_MAX_BLOCKS || result[1] > FUSE_MAX_BLOCKS) result[0] |= FUSE_TOO_MANY;
    for (int a = 0; a < 3; ++a) result[2 + a] = (int)__float_as_uint(okey32_val(box[a]));
}

__global__ __launch_bounds__(TPB) void k_fuse_copy_keys(const u64* __restrict__ ukeys, int n_blocks, int* __restrict__ result,
                                                        long long* __restrict__ out) {
    if (result[0] != 0) return;
    if (result[1] != n_blocks) { if (blockIdx.x == 0 && threadIdx.x == 0) atomicOr(result, FUSE_ROWS); return; }
    for (int t = blockIdx.x * TPB + threadIdx.x; t < n_blocks; t += gridDim.x * TPB) out[t] = (long long)ukeys[t];
}

struct FuseBlocksWs {
    unsigned* box; u64* cellkey; SortBufs sort[2]; int* head; int* before; int* scan_tmp; u64* occ; u64* ukeys; int* n_occ;
    int cap_occ, slots;
};

FuseBlocksWs fuse_blocks_carve(Carver& cv, int n) {
    FuseBlocksWs w{};
    const size_t N = (size_t)(n > 0 ? n : 1);
    w.cap_occ = (int)(N < (size_t)FUSE_MAX_BLOCKS ? N : (size_t)FUSE_MAX_BLOCKS);
    w.slots = 27 * w.cap_occ;                                                // <= 27 * 2^21 < 2^28
    const size_t NS = N > (size_t)w.slots ? N : (size_t)w.slots;
    w.box = cv.take<unsigned>(64);
    w.cellkey = cv.take<u64>(NS);
    w.sort[0] = sort_carve(cv, NS, 2);                                       // the points' two sorts
    w.sort[1] = w.sort[0];                                                   // the blocks' two: the same buffers, own histograms
    for (int i = 0; i < 2; ++i) w.sort[1].ghist[i] = cv.take<unsigned>((size_t)RADIX_U32_PASSES * RADIX);
    w.head = cv.take<int>(NS); w.before = cv.take<int>(NS);
    w.scan_tmp = cv.take<int>(scan_tmp_ints((long long)NS));
    w.occ = cv.take<u64>((size_t)w.cap_occ);
    w.ukeys = cv.take<u64>((size_t)(w.slots < FUSE_MAX_BLOCKS ? w.slots : FUSE_MAX_BLOCKS));
    w.n_occ = cv.take<int>(1);
    return w;
}

size_t fuse_blocks_ws_bytes(int n) {
    Carver cv(nullptr, 0);
    fuse_blocks_carve(cv, n);
    return cv.off + 256;
}

// the distinct keys of cellkey[0..cnt) that are not FUSE_PAD, ascending, into out[0..cap); their number into *total
int fuse_unique(const FuseBlocksWs& w, const SortBufs& s, int cnt, int32_t* status, u64* out, int cap, int* total, hipStream_t st) {
    const dim3 grid(grid_for(cnt)), block(TPB);
    hipLaunchKernelGGL(k_fuse_low, grid, block, 0, st, w.cellkey, cnt, s.keys_a, s.vals_a, s.ghist[0]);
    PBN_LAUNCH_CHECK();
    PBN_TRY(sort_run(s, 0, cnt, status, st));
    hipLaunchKernelGGL(k_fuse_high, grid, block, 0, st, w.cellkey, s.vals_b, cnt, s.keys_a, s.vals_a, s.ghist[1]);
    PBN_LAUNCH_CHECK();
    PBN_TRY(sort_run(s, 1, cnt, status, st));
    hipLaunchKernelGGL(k_fuse_heads, grid, block, 0, st, w.cellkey, s.vals_b, cnt, w.head);
    PBN_LAUNCH_CHECK();
    PBN_TRY(scan_exclusive_i32(w.head, w.before, cnt, w.scan_tmp, total, st));
    hipLaunchKernelGGL(k_fuse_compact, grid, block, 0, st, w.cellkey, s.vals_b, w.head, w.before, cnt, status, out, cap);
    PBN_LAUNCH_CHECK();
    return PBN_OK;
}

int fuse_blocks_args(const float* xyz, int n, double voxel, const int32_t* result, const void* workspace, size_t workspace_bytes) {
    if (n < 0 || n > SCAN_MAX_POINTS || !(voxel > 0.0) || !std::isfinite(voxel) || !std::isfinite(8.0 * voxel)) return PBN_ERR_ARG;
    if ((n && !xyz) || !result || !workspace) return PBN_ERR_ARG;
    if (workspace_bytes < fuse_blocks_ws_bytes(n)) return PBN_ERR_WORKSPACE;
    return PBN_OK;
}

// ev (optional): FUSE_BLOCKS_EVENTS events around box + keys | the points' blocks | dilation + the allocated blocks
int fuse_blocks(const float* xyz, int n, double voxel, int32_t* result, void* workspace, size_t workspace_bytes, hipStream_t st,
                hipEvent_t* ev) {
    PBN_TRY(fuse_blocks_args(xyz, n, voxel, result, workspace, workspace_bytes));
    Carver cv(workspace, workspace_bytes);
    const FuseBlocksWs w = fuse_blocks_carve(cv, n);
    if (!cv.ok) return PBN_ERR_WORKSPACE;
    const FillRange fr[] = {{result, 8 * sizeof(int32_t), 0}, {w.box, 3 * sizeof(unsigned), 0xff}, {w.box + 3, 3 * sizeof(unsigned), 0},
                            {w.n_occ, sizeof(int), 0}, sort_hist_fill(w.sort[0], 0), sort_hist_fill(w.sort[0], 1),
                            sort_hist_fill(w.sort[1], 0), sort_hist_fill(w.sort[1], 1)};
    PBN_TRY(fill_ranges(fr, n > 0 ? 8 : 1, st));
    if (ev) PBN_HIP_CHECK(hipEventRecord(ev[0], st));
    if (n == 0) {
        if (ev) for (int i = 1; i < FUSE_BLOCKS_EVENTS; ++i) PBN_HIP_CHECK(hipEventRecord(ev[i], st));
        return PBN_OK;
    }
    int32_t* status = result;
    PBN_TRY(cloud_box(xyz, n, w.box, status, st));
    hipLaunchKernelGGL(k_fuse_point_keys, dim3(grid_for(n)), dim3(TPB), 0, st, xyz, n, w.box, status, 8.0 * voxel, w.cellkey);
    PBN_LAUNCH_CHECK();
    if (ev) PBN_HIP_CHECK(hipEventRecord(ev[1], st));
    PBN_TRY(fuse_unique(w, w.sort[0], n, status, w.occ, w.cap_occ, w.n_occ, st));
    if (ev) PBN_HIP_CHECK(hipEventRecord(ev[2], st));
    hipLaunchKernelGGL(k_fuse_dilate, dim3(grid_for(w.slots)), dim3(TPB), 0, st, w.occ, w.n_occ, w.cap_occ, status, w.slots,
                       w.cellkey);
    PBN_LAUNCH_CHECK();
    PBN_TRY(fuse_unique(w, w.sort[1], w.slots, status, w.ukeys, w.slots < FUSE_MAX_BLOCKS ? w.slots : FUSE_MAX_BLOCKS, result + 1,
                        st));
    hipLaunchKernelGGL(k_fuse_blocks_result, dim3(1), dim3(1), 0, st, w.box, w.n_occ, result);
    PBN_LAUNCH_CHECK();
    if (ev) PBN_HIP_CHECK(hipEventRecord(ev[3], st));
    return PBN_OK;
}

// ---- integration -------------------------------------------------------------------------------------------------------
struct FuseGrid {
    int height, width;
    double scale, z_min, z_max, edge, voxel, trunc, g0, g1, g2;
};

// the voxel centre's coordinate on one axis: block b, in-block i
__device__ __forceinline__ double fuse_centre(double g, int b, int i, double voxel) {
    return g + ((double)(FUSE_SIDE * b + i) + 0.5) * voxel;
}

// Can frame C (FUSE_CAM doubles) see any point of the sphere (c, rad)?  Conservative: the per-voxel test is the authority.
// A plane n . pc >= 0 of the frustum, n in the camera's frame: over the sphere n . pc is at most val + rad * |Rt^T n|, for
// any linear Rt; slack covers the rounding of val (1e-9 of the magnitudes that went into it, float64 rounds at 1e-16).
// Every comparison is false for NaN, which keeps the frame.
__device__ __forceinline__ bool fuse_may_see(const double* __restrict__ C, double c0, double c1, double c2, double rad,
                                             const FuseGrid& a) {
    double pc[3], apc[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        pc[r] = ((C[3 * r] * c0 + C[3 * r + 1] * c1) + C[3 * r + 2] * c2) + C[9 + r];
        apc[r] = ((fabs(C[3 * r] * c0) + fabs(C[3 * r + 1] * c1)) + fabs(C[3 * r + 2] * c2)) + fabs(C[9 + r]);
    }
    const double fx = C[12], fy = C[13], cx = C[14], cy = C[15];
    const double n[5][3] = {{0.0, 0.0, 1.0},                                   // zc > 0
                            {fx, 0.0, cx + 0.5}, {-fx, 0.0, ((double)a.width - 0.5) - cx},       // -0.5 <= uf <= W - 0.5
                            {0.0, fy, cy + 0.5}, {0.0, -fy, ((double)a.height - 0.5) - cy}};
    bool out = false;
#pragma unroll
    for (int p = 0; p < 5; ++p) {
        const double m0 = (C[0] * n[p][0] + C[3] * n[p][1]) + C[6] * n[p][2];
        const double m1 = (C[1] * n[p][0] + C[4] * n[p][1]) + C[7] * n[p][2];
        const double m2 = (C[2] * n[p][0] + C[5] * n[p][1]) + C[8] * n[p][2];
        const double ext = rad * sqrt((m0 * m0 + m1 * m1) + m2 * m2);
        const double val = (n[p][0] * pc[0] + n[p][1] * pc[1]) + n[p][2] * pc[2];
        const double mag = (fabs(n[p][0]) * apc[0] + fabs(n[p][1]) * apc[1]) + fabs(n[p][2]) * apc[2];
        out = out || (val + ext) + 1e-9 * (mag + ext) < 0.0;
    }
    {                                                                          // s >= -trunc: zc <= z + trunc <= z_max + trunc
        const double ext = rad * sqrt((C[6] * C[6] + C[7] * C[7]) + C[8] * C[8]);
        out = out || (((a.z_max + a.trunc) - pc[2]) + ext) + 1e-9 * (apc[2] + ext) < 0.0;
    }
    return !out;
}

// One voxel p against one frame: steps 1 to 6 of the contract.
template <typename D>
__device__ __forceinline__ void fuse_observe(const D* __restrict__ img, const unsigned char* __restrict__ col,
                                             const double* __restrict__ C, const FuseGrid& a, double p0, double p1, double p2,
                                             double& S, int& Wt, double& c0, double& c1, double& c2, unsigned& reads) {
    const double x = ((C[0] * p0 + C[1] * p1) + C[2] * p2) + C[9];
    const double y = ((C[3] * p0 + C[4] * p1) + C[5] * p2) + C[10];
    const double zc = ((C[6] * p0 + C[7] * p1) + C[8] * p2) + C[11];
    if (!(zc > 0.0)) return;
    const double uf = (C[12] * x) / zc + C[14], vf = (C[13] * y) / zc + C[15];
    const double ur = rint(uf), vr = rint(vf);
    if (!(ur >= 0.0 && ur <= (double)(a.width - 1) && vr >= 0.0 && vr <= (double)(a.height - 1))) return;
    const int u = (int)ur, v = (int)vr;
    double z;
    ++reads;
    if (!frames_depth_ok(img, a.height, a.width, u, v, a.scale, a.z_min, a.z_max, a.edge, z)) return;
    const double s = z - zc;
    if (s < -a.trunc) return;
    const double d = fmin(1.0, s / a.trunc);
    S = S + d;
    Wt += 1;
    if (col) {
        const unsigned char* __restrict__ cp = col + 3 * ((size_t)v * a.width + u);
        c0 = c0 + (double)cp[0]; c1 = c1 + (double)cp[1]; c2 = c2 + (double)cp[2];
    }
}

// One workgroup per block.  cam / fidx: the n_live frames that are not skipped, ascending.  stats (STATS): [0] block-frame
// pairs that survive the cull, [1] depth samples gathered (the centre pixel of step 3; the edge test's neighbours not counted).
template <typename D, bool STATS>
__global__ __launch_bounds__(TPB) void k_fuse_integrate(const D* __restrict__ depth, const unsigned char* __restrict__ colour,
                                                        const double* __restrict__ cam, const int* __restrict__ fidx, int n_live,
                                                        FuseGrid a, const long long* __restrict__ block_key, float* __restrict__ tsdf,
                                                        int* __restrict__ weight, float* __restrict__ rgb,
                                                        unsigned long long* __restrict__ stats) {
    __shared__ unsigned long long s_mask[TPB / WAVE];
    const long long key = block_key[blockIdx.x];
    const int bx = (int)(key & 0x1fffff), by = (int)((key >> FUSE_AXIS_BITS) & 0x1fffff), bz = (int)((key >> (2 * FUSE_AXIS_BITS)) & 0x1fffff);
    const int lane = lane_id(), wave = (int)threadIdx.x >> 6;
    double p0[FUSE_PER_LANE], p1[FUSE_PER_LANE], p2[FUSE_PER_LANE], S[FUSE_PER_LANE], C0[FUSE_PER_LANE], C1[FUSE_PER_LANE], C2[FUSE_PER_LANE];
    int Wt[FUSE_PER_LANE];
#pragma unroll
    for (int j = 0; j < FUSE_PER_LANE; ++j) {
        const int idx = (int)threadIdx.x + j * TPB;
        p0[j] = fuse_centre(a.g0, bx, idx & 7, a.voxel);
        p1[j] = fuse_centre(a.g1, by, (idx >> 3) & 7, a.voxel);
        p2[j] = fuse_centre(a.g2, bz, idx >> 6, a.voxel);
        S[j] = C0[j] = C1[j] = C2[j] = 0.0;
        Wt[j] = 0;
    }
    // the block's bounding sphere: its voxel centres lie within 3.5 voxels of the block's centre on every axis
    const double c0 = fuse_centre(a.g0, bx, 3, a.voxel) + 0.5 * a.voxel, c1 = fuse_centre(a.g1, by, 3, a.voxel) + 0.5 * a.voxel;
    const double c2 = fuse_centre(a.g2, bz, 3, a.voxel) + 0.5 * a.voxel;
    const double rad = 6.07 * a.voxel;                                       // > sqrt(3) * 3.5 voxels
    const size_t image = (size_t)a.height * a.width;
    unsigned reads = 0, seen = 0;
    for (int base = 0; base < n_live; base += TPB) {
        const int k = base + (int)threadIdx.x;
        const bool may = k < n_live && fuse_may_see(cam + FUSE_CAM * (size_t)k, c0, c1, c2, rad, a);
        const unsigned long long mine = __ballot(may);
        if (lane == 0) s_mask[wave] = mine;
        __syncthreads();
#pragma unroll 1
        for (int w = 0; w < TPB / WAVE; ++w) {
            const unsigned long long m = s_mask[w];
            unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)m), hi = __builtin_amdgcn_readfirstlane((unsigned)(m >> 32));
            unsigned long long mask = ((unsigned long long)hi << 32) | lo;   // uniform: the walk is scalar
            if (STATS) seen += (unsigned)__popcll(mask);
            while (mask) {
                const int kk = base + w * WAVE + (__ffsll((long long)mask) - 1);
                mask &= mask - 1;
                const double* __restrict__ C = cam + FUSE_CAM * (size_t)kk;
                const size_t f = (size_t)fidx[kk];
                const D* __restrict__ img = depth + f * image;
                const unsigned char* __restrict__ col = colour ? colour + 3 * f * image : nullptr;
#pragma unroll
                for (int j = 0; j < FUSE_PER_LANE; ++j)
                    fuse_observe(img, col, C, a, p0[j], p1[j], p2[j], S[j], Wt[j], C0[j], C1[j], C2[j], reads);
            }
        }
        __syncthreads();                                                     // s_mask is rewritten by the next round
    }
#pragma unroll
    for (int j = 0; j < FUSE_PER_LANE; ++j) {
        const size_t o = (size_t)blockIdx.x * FUSE_VOXELS + (size_t)((int)threadIdx.x + j * TPB);
        const double wt = (double)Wt[j];
        tsdf[o] = Wt[j] ? (float)(S[j] / wt) : 0.0f;
        weight[o] = Wt[j];
        if (rgb) {
            rgb[3 * o] = Wt[j] ? (float)(C0[j] / wt) : 0.0f;
            rgb[3 * o + 1] = Wt[j] ? (float)(C1[j] / wt) : 0.0f;
            rgb[3 * o + 2] = Wt[j] ? (float)(C2[j] / wt) : 0.0f;
        }
    }
    if (STATS) {
        const int r = wave_reduce_add((int)reads);
        if (lane == 0) atomicAdd(&stats[1], (unsigned long long)r);
        if (threadIdx.x == 0) atomicAdd(&stats[0], (unsigned long long)seen);
    }
}

struct FuseCall {
    const void* depth; int depth_is_f32; const uint8_t* colour; const double* pose; const double* intr;
    int n_frames, height, width; double depth_scale, depth_min, depth_max, edge, voxel, trunc; const double* origin;
};

struct FuseIntWs { double* cam; int* fidx; unsigned long long* stats; };

FuseIntWs fuse_int_carve(Carver& cv, int n_frames) {
    FuseIntWs w{};
    const size_t F = (size_t)(n_frames > 0 ? n_frames : 1);
    w.cam = cv.take<double>(FUSE_CAM * F);
    w.fidx = cv.take<int>(F);
    w.stats = cv.take<unsigned long long>(2);
    return w;
}

size_t fuse_int_ws_bytes(int n_frames) {
    Carver cv(nullptr, 0);
    fuse_int_carve(cv, n_frames);
    return cv.off + 256;
}

bool fuse_sizes_ok(int n_frames, int height, int width) {
    return n_frames >= 0 && height >= 0 && width >= 0 && (long long)n_frames * height * width <= 2147483647LL;
}

bool fuse_scalars_ok(double voxel, double trunc) {
    return voxel > 0.0 && std::isfinite(voxel) && std::isfinite(trunc) && trunc > 0.0 && trunc <= 8.0 * voxel;
}

// ev (optional): FUSE_INTEGRATE_EVENTS events around the upload and the kernel.  stats_out (host, optional): the counters.
int fuse_integrate(const FuseCall& c, const long long* block_key, int n_blocks, float* tsdf, int32_t* weight, float* rgb,
                   void* workspace, size_t workspace_bytes, hipStream_t st, hipEvent_t* ev, unsigned long long* stats_out) {
    if (!fuse_sizes_ok(c.n_frames, c.height, c.width) || (c.depth_is_f32 != 0 && c.depth_is_f32 != 1)) return PBN_ERR_ARG;
    if (!(c.depth_scale > 0.0) || !std::isfinite(c.depth_scale) || !(c.depth_min <= c.depth_max)) return PBN_ERR_ARG;
    if (!fuse_scalars_ok(c.voxel, c.trunc) || !c.origin || !workspace) return PBN_ERR_ARG;
    if (n_blocks < 0 || n_blocks > FUSE_MAX_BLOCKS) return PBN_ERR_ARG;
    if (c.n_frames && (!c.pose || !c.intr)) return PBN_ERR_ARG;
    if ((long long)c.n_frames * c.height * c.width > 0 && !c.depth) return PBN_ERR_ARG;
    if (n_blocks && (!block_key || !tsdf || !weight || (c.colour != nullptr) != (rgb != nullptr))) return PBN_ERR_ARG;
    for (int a = 0; a < 3; ++a) if (!std::isfinite(c.origin[a])) return PBN_ERR_ARG;
    for (int f = 0; f < c.n_frames; ++f) {
        const double fx = c.intr[4 * (size_t)f], fy = c.intr[4 * (size_t)f + 1];
        if (!(fx > 0.0) || !std::isfinite(fx) || !(fy > 0.0) || !std::isfinite(fy)) return PBN_ERR_ARG;
    }
    Carver cv(workspace, workspace_bytes);
    const FuseIntWs w = fuse_int_carve(cv, c.n_frames);
    if (!cv.ok) return PBN_ERR_WORKSPACE;
    if (ev) PBN_HIP_CHECK(hipEventRecord(ev[0], st));
    if (stats_out) stats_out[0] = stats_out[1] = 0;
    if (n_blocks == 0) {
        if (ev) PBN_HIP_CHECK(hipEventRecord(ev[1], st));
        return PBN_OK;
    }
    // world to camera of the frames that are not skipped: Rt = R transposed, tc[r] = -((Rt[r,0]*t0 + Rt[r,1]*t1) + Rt[r,2]*t2)
    std::vector<double> cam;
    std::vector<int> fidx;
    for (int f = 0; f < c.n_frames; ++f) {
        const double* P = c.pose + 16 * (size_t)f;
        bool ok = true;
        for (int i = 0; i < 12; ++i) ok = ok && std::isfinite(P[i]);
        if (!ok || (long long)c.height * c.width == 0) continue;
        double rec[FUSE_CAM];
        for (int r = 0; r < 3; ++r) {
            for (int q = 0; q < 3; ++q) rec[3 * r + q] = P[4 * q + r];
            rec[9 + r] = -((rec[3 * r] * P[3] + rec[3 * r + 1] * P[7]) + rec[3 * r + 2] * P[11]);   // -ffp-contract=off holds on the host too
        }
        for (int i = 0; i < 4; ++i) rec[12 + i] = c.intr[4 * (size_t)f + i];
        cam.insert(cam.end(), rec, rec + FUSE_CAM);
        fidx.push_back(f);
    }
    const int n_live = (int)fidx.size();
    if (n_live) {                                                            // pageable memory: both copies are staged before they return
        PBN_HIP_CHECK(hipMemcpyAsync(w.cam, cam.data(), cam.size() * sizeof(double), hipMemcpyHostToDevice, st));
        PBN_HIP_CHECK(hipMemcpyAsync(w.fidx, fidx.data(), fidx.size() * sizeof(int), hipMemcpyHostToDevice, st));
        PBN_HIP_CHECK(hipStreamSynchronize(st));                             // cam and fidx die with this scope
    }
    const FuseGrid a{c.height, c.width, c.depth_scale, c.depth_min, c.depth_max, c.edge, c.voxel, c.trunc, c.origin[0], c.origin[1],
                     c.origin[2]};
    const dim3 grid((unsigned)n_blocks), block(TPB);
    if (stats_out) {
        PBN_TRY(fill_bytes(w.stats, 0, 2 * sizeof(unsigned long long), st));
        if (c.depth_is_f32)
            hipLaunchKernelGGL((k_fuse_integrate<float, true>), grid, block, 0, st, (const float*)c.depth, c.colour, w.cam, w.fidx, n_live, a,
                               block_key, tsdf, weight, rgb, w.stats);
        else
            hipLaunchKernelGGL((k_fuse_integrate<unsigned short, true>), grid, block, 0, st, (const unsigned short*)c.depth, c.colour, w.cam,
                               w.fidx, n_live, a, block_key, tsdf, weight, rgb, w.stats);
    } else if (c.depth_is_f32) {
        hipLaunchKernelGGL((k_fuse_integrate<float, false>), grid, block, 0, st, (const float*)c.depth, c.colour, w.cam, w.fidx, n_live, a,
                           block_key, tsdf, weight, rgb, w.stats);
    } else {
        hipLaunchKernelGGL((k_fuse_integrate<unsigned short, false>), grid, block, 0, st, (const unsigned short*)c.depth, c.colour, w.cam,
                           w.fidx, n_live, a, block_key, tsdf, weight, rgb, w.stats);
    }
    PBN_LAUNCH_CHECK();
    if (ev) PBN_HIP_CHECK(hipEventRecord(ev[1], st));
    if (stats_out) {
        PBN_HIP_CHECK(hipStreamSynchronize(st));
        PBN_HIP_CHECK(hipMemcpy(stats_out, w.stats, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    }
    return PBN_OK;
}

// ---- extraction --------------------------------------------------------------------------------------------------------
struct FuseVolume {
    const float* tsdf; const int* weight; const float* rgb; const long long* block_key; int n_blocks, min_weight;
};

// the rank of `key` among the ascending block keys, -1 when it is not allocated
__device__ __forceinline__ int fuse_find(const long long* __restrict__ keys, int n, long long key) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (keys[mid] < key) lo = mid + 1; else hi = mid;
    }
    return (lo < n && keys[lo] == key) ? lo : -1;
}

// voxel (x, y, z) in the workgroup's block's coordinates, each in -8 .. 15: observed?  D as float64
__device__ __forceinline__ bool fuse_voxel(const FuseVolume& v, const int* s_rank, int x, int y, int z, double& D, int& wt, size_t& at) {
    const int nb = s_rank[(((z + 8) >> 3) * 3 + ((y + 8) >> 3)) * 3 + ((x + 8) >> 3)];
    if (nb < 0) return false;
    at = (size_t)nb * FUSE_VOXELS + (size_t)((((z & 7) * 8) + (y & 7)) * 8 + (x & 7));
    wt = v.weight[at];
    if (wt < v.min_weight) return false;
    D = (double)v.tsdf[at];
    return true;
}

// G(x)[b] = D'(x + e_b) - D'(x - e_b), an unobserved voxel reading as D(x) itself
__device__ __forceinline__ void fuse_gradient(const FuseVolume& v, const int* s_rank, int x, int y, int z, double Dx, double* G) {
#pragma unroll
    for (int b = 0; b < 3; ++b) {
        double Dp = Dx, Dm = Dx, t;
        int wt; size_t at;
        if (fuse_voxel(v, s_rank, x + (b == 0), y + (b == 1), z + (b == 2), t, wt, at)) Dp = t;
        if (fuse_voxel(v, s_rank, x - (b == 0), y - (b == 1), z - (b == 2), t, wt, at)) Dm = t;
        G[b] = Dp - Dm;
    }
}

struct FuseRows {
    float* xyz; float* rgb; float* nl; int* weight; long long* voxel_id; int n_rows; double voxel, g0, g1, g2;
};

// WRITE = false: counts[block] = its surface rows.  WRITE = true: the rows, from offs[block].
template <bool WRITE>
__global__ __launch_bounds__(TPB) void k_fuse_extract(FuseVolume v, int* __restrict__ counts, const int* __restrict__ offs, FuseRows o,
                                                      int* __restrict__ status) {
    __shared__ int s_rank[27];
    __shared__ int s_scan[TPB];
    __shared__ int s_status;
    const long long key = v.block_key[blockIdx.x];
    // one read, so the whole workgroup agrees; FUSE_ROWS is what other workgroups of THIS launch may be setting meanwhile, and
    // it stops no row below n_rows: only a status the count pass left does
    if (threadIdx.x == 0) s_status = WRITE ? (*status & ~FUSE_ROWS) : 0;
    if (threadIdx.x < 27) {
        const long long d = (long long)threadIdx.x;
        const long long nk = key + (d % 3 - 1) + (d / 3 % 3 - 1) * (1ll << FUSE_AXIS_BITS) + (d / 9 - 1) * (1ll << (2 * FUSE_AXIS_BITS));
        s_rank[threadIdx.x] = threadIdx.x == 13 ? (int)blockIdx.x : fuse_find(v.block_key, v.n_blocks, nk);
    }
    __syncthreads();
    if (s_status != 0) return;                                               // nothing is written
    // a lane's two voxels are consecutive in-block indices: lane order is row order
    bool cross[FUSE_PER_LANE][3];
    double Dq[FUSE_PER_LANE], Dn[FUSE_PER_LANE][3];
    int wq[FUSE_PER_LANE], wn[FUSE_PER_LANE][3];
    size_t aq[FUSE_PER_LANE], an[FUSE_PER_LANE][3];
    int mine = 0;
#pragma unroll
    for (int j = 0; j < FUSE_PER_LANE; ++j) {
        const int idx = FUSE_PER_LANE * (int)threadIdx.x + j, x = idx & 7, y = (idx >> 3) & 7, z = idx >> 6;
        const bool obs = fuse_voxel(v, s_rank, x, y, z, Dq[j], wq[j], aq[j]);
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            cross[j][a] = obs && fuse_voxel(v, s_rank, x + (a == 0), y + (a == 1), z + (a == 2), Dn[j][a], wn[j][a], an[j][a]) &&
                          ((Dq[j] < 0.0) != (Dn[j][a] < 0.0));
            mine += cross[j][a] ? 1 : 0;
        }
    }
    s_scan[threadIdx.x] = mine;
    __syncthreads();
    for (int s = 1; s < TPB; s <<= 1) {                                      // inclusive scan over the lanes
        const int t = (int)threadIdx.x >= s ? s_scan[threadIdx.x - s] : 0;
        __syncthreads();
        s_scan[threadIdx.x] += t;
        __syncthreads();
    }
    if (!WRITE) {
        if (threadIdx.x == TPB - 1) counts[blockIdx.x] = s_scan[TPB - 1];
        return;
    }
    int row = offs[blockIdx.x] + s_scan[threadIdx.x] - mine;
    bool over = false;
    const int bx = (int)(key & 0x1fffff), by = (int)((key >> FUSE_AXIS_BITS) & 0x1fffff), bz = (int)((key >> (2 * FUSE_AXIS_BITS)) & 0x1fffff);
#pragma unroll
    for (int j = 0; j < FUSE_PER_LANE; ++j) {
        const int idx = FUSE_PER_LANE * (int)threadIdx.x + j, x = idx & 7, y = (idx >> 3) & 7, z = idx >> 6;
        double Gq[3];
        bool have_gq = false;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            if (!cross[j][a]) continue;
            const int r_ = row++;
            if (r_ < 0 || r_ >= o.n_rows) { over = true; continue; }
            if (!have_gq) { fuse_gradient(v, s_rank, x, y, z, Dq[j], Gq); have_gq = true; }
            double Gn[3];
            fuse_gradient(v, s_rank, x + (a == 0), y + (a == 1), z + (a == 2), Dn[j][a], Gn);
            const double r = Dq[j] / (Dq[j] - Dn[j][a]);
            double p[3] = {fuse_centre(o.g0, bx, x, o.voxel), fuse_centre(o.g1, by, y, o.voxel), fuse_centre(o.g2, bz, z, o.voxel)};
            const double moved = p[a] + r * o.voxel;
            const double gv0 = Gq[0] + r * (Gn[0] - Gq[0]), gv1 = Gq[1] + r * (Gn[1] - Gq[1]), gv2 = Gq[2] + r * (Gn[2] - Gq[2]);
            const double len = sqrt((gv0 * gv0 + gv1 * gv1) + gv2 * gv2);
            const bool unit = len > 0.0 && __builtin_isfinite(len);
            const size_t at = 3 * (size_t)r_;
            o.xyz[at] = (float)(a == 0 ? moved : p[0]); o.xyz[at + 1] = (float)(a == 1 ? moved : p[1]);
            o.xyz[at + 2] = (float)(a == 2 ? moved : p[2]);
            o.nl[at] = unit ? (float)(gv0 / len) : 0.0f; o.nl[at + 1] = unit ? (float)(gv1 / len) : 0.0f;
            o.nl[at + 2] = unit ? (float)(gv2 / len) : 0.0f;
            if (o.rgb) {
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) {
                    const double cq = (double)v.rgb[3 * aq[j] + ch], cn = (double)v.rgb[3 * an[j][a] + ch];
                    o.rgb[at + ch] = (float)(cq + r * (cn - cq));
                }
            }
            o.weight[r_] = min(wq[j], wn[j][a]);
            o.voxel_id[r_] = ((long long)blockIdx.x * FUSE_VOXELS + idx) * 3 + a;
        }
    }
    if (over) atomicOr(status, FUSE_ROWS);
}

struct FuseExtWs { int* counts; int* offs; int* scan_tmp; };

FuseExtWs fuse_ext_carve(Carver& cv, int n_blocks) {
    FuseExtWs w{};
    const size_t M = (size_t)(n_blocks > 0 ? n_blocks : 1);
    w.counts = cv.take<int>(M); w.offs = cv.take<int>(M);
    w.scan_tmp = cv.take<int>(scan_tmp_ints((long long)M));
    return w;
}

size_t fuse_ext_ws_bytes(int n_blocks) {
    Carver cv(nullptr, 0);
    fuse_ext_carve(cv, n_blocks);
    return cv.off + 256;
}

int fuse_ext_args(const FuseVolume& v, const int32_t* result, const void* workspace, size_t workspace_bytes) {
    if (v.n_blocks < 0 || v.n_blocks > FUSE_MAX_EXTRACT_BLOCKS || v.min_weight < 1) return PBN_ERR_ARG;
    if ((v.n_blocks && (!v.tsdf || !v.weight || !v.block_key)) || !result || !workspace) return PBN_ERR_ARG;
    if (workspace_bytes < fuse_ext_ws_bytes(v.n_blocks)) return PBN_ERR_WORKSPACE;
    return PBN_OK;
}

int fuse_extract_count(const FuseVolume& v, int32_t* result, void* workspace, size_t workspace_bytes, hipStream_t st, hipEvent_t* ev) {
    PBN_TRY(fuse_ext_args(v, result, workspace, workspace_bytes));
    Carver cv(workspace, workspace_bytes);
    const FuseExtWs w = fuse_ext_carve(cv, v.n_blocks);
    if (!cv.ok) return PBN_ERR_WORKSPACE;
    PBN_TRY(fill_bytes(result, 0, 2 * sizeof(int32_t), st));
    if (ev) PBN_HIP_CHECK(hipEventRecord(ev[0], st));
    if (v.n_blocks) {
        hipLaunchKernelGGL((k_fuse_extract<false>), dim3((unsigned)v.n_blocks), dim3(TPB), 0, st, v, w.counts, w.offs, FuseRows{}, result);
        PBN_LAUNCH_CHECK();
        PBN_TRY(scan_exclusive_i32(w.counts, w.offs, v.n_blocks, w.scan_tmp, result + 1, st));
    }
    if (ev) PBN_HIP_CHECK(hipEventRecord(ev[1], st));
    return PBN_OK;
}

int fuse_extract_write(const FuseVolume& v, const FuseRows& o, const double* origin, int32_t* result, void* workspace,
                       size_t workspace_bytes, hipStream_t st, hipEvent_t* ev) {
    PBN_TRY(fuse_ext_args(v, result, workspace, workspace_bytes));
    if (o.n_rows < 0 || !(o.voxel > 0.0) || !std::isfinite(o.voxel) || !origin) return PBN_ERR_ARG;
    if (o.n_rows && (!o.xyz || !o.nl || !o.weight || !o.voxel_id || (v.rgb != nullptr) != (o.rgb != nullptr))) return PBN_ERR_ARG;
    Carver cv(workspace, workspace_bytes);
    const FuseExtWs w = fuse_ext_carve(cv, v.n_blocks);
    if (!cv.ok) return PBN_ERR_WORKSPACE;
    FuseRows rows = o;
    rows.g0 = origin[0]; rows.g1 = origin[1]; rows.g2 = origin[2];
    if (ev) PBN_HIP_CHECK(hipEventRecord(ev[0], st));
    if (v.n_blocks) {                                                        // the workspace still holds offs of the count pass
        hipLaunchKernelGGL((k_fuse_extract<true>), dim3((unsigned)v.n_blocks), dim3(TPB), 0, st, v, w.counts, w.offs, rows, result);
        PBN_LAUNCH_CHECK();
    }
    if (ev) PBN_HIP_CHECK(hipEventRecord(ev[1], st));
    return PBN_OK;
}

}  // namespace
}  // namespace pbn

using namespace pbn;

extern "C" int pbn_fuse_max_blocks(void) { return FUSE_MAX_BLOCKS; }

extern "C" size_t pbn_fuse_blocks_workspace_bytes(int n_points) {
    if (n_points < 0 || n_points > SCAN_MAX_POINTS) return 0;
    return fuse_blocks_ws_bytes(n_points);
}

extern "C" int pbn_fuse_blocks(const float* xyz, int n_points, double voxel, int32_t* result, void* workspace, size_t workspace_bytes,
                               pbn_stream_t stream) {
    return fuse_blocks(xyz, n_points, voxel, result, workspace, workspace_bytes, (hipStream_t)stream, nullptr);
}

extern "C" int pbn_fuse_blocks_timed(const float* xyz, int n_points, double voxel, int32_t* result, void* workspace,
                                     size_t workspace_bytes, pbn_stream_t stream, float* times_ms) {
    if (!times_ms) return PBN_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    return timed_stages<FUSE_BLOCKS_EVENTS>(st, times_ms, [&](hipEvent_t* ev) {
        return fuse_blocks(xyz, n_points, voxel, result, workspace, workspace_bytes, st, ev);
    });
}

extern "C" int pbn_fuse_block_keys(int n_points, int n_blocks, int64_t* block_key, int32_t* result, void* workspace,
                                   size_t workspace_bytes, pbn_stream_t stream) {
    if (n_points < 0 || n_points > SCAN_MAX_POINTS || n_blocks < 0 || n_blocks > FUSE_MAX_BLOCKS) return PBN_ERR_ARG;
    if ((n_blocks && !block_key) || !result || !workspace) return PBN_ERR_ARG;
    if (workspace_bytes < fuse_blocks_ws_bytes(n_points)) return PBN_ERR_WORKSPACE;
    Carver cv(workspace, workspace_bytes);
    const FuseBlocksWs w = fuse_blocks_carve(cv, n_points);
    if (!cv.ok) return PBN_ERR_WORKSPACE;
    if (n_blocks > (w.slots < FUSE_MAX_BLOCKS ? w.slots : FUSE_MAX_BLOCKS)) return PBN_ERR_ARG;
    hipLaunchKernelGGL(k_fuse_copy_keys, dim3(grid_for(n_blocks)), dim3(TPB), 0, (hipStream_t)stream, w.ukeys, n_blocks, result,
                       (long long*)block_key);
    PBN_LAUNCH_CHECK();
    return PBN_OK;
}

extern "C" size_t pbn_fuse_integrate_workspace_bytes(int n_frames) {
    if (n_frames < 0) return 0;
    return fuse_int_ws_bytes(n_frames);
}

extern "C" int pbn_fuse_integrate(const void* depth, int depth_is_f32, const uint8_t* colour, const double* pose, const double* intr,
                                  int n_frames, int height, int width, double depth_scale, double depth_min, double depth_max,
                                  double edge, double voxel, double trunc, const double* origin, const int64_t* block_key,
                                  int n_blocks, float* tsdf, int32_t* weight, float* rgb, void* workspace, size_t workspace_bytes,
                                  pbn_stream_t stream) {
    const FuseCall c{depth, depth_is_f32, colour, pose, intr, n_frames, height, width, depth_scale, depth_min, depth_max, edge, voxel,
                     trunc, origin};
    return fuse_integrate(c, (const long long*)block_key, n_blocks, tsdf, weight, rgb, workspace, workspace_bytes, (hipStream_t)stream,
                          nullptr, nullptr);
}

extern "C" int pbn_fuse_integrate_timed(const void* depth, int depth_is_f32, const uint8_t* colour, const double* pose,
                                        const double* intr, int n_frames, int height, int width, double depth_scale, double depth_min,
                                        double depth_max, double edge, double voxel, double trunc, const double* origin,
                                        const int64_t* block_key, int n_blocks, float* tsdf, int32_t* weight, float* rgb,
                                        void* workspace, size_t workspace_bytes, pbn_stream_t stream, float* times_ms,
                                        uint64_t* stats) {
    if (!times_ms) return PBN_ERR_ARG;
    const FuseCall c{depth, depth_is_f32, colour, pose, intr, n_frames, height, width, depth_scale, depth_min, depth_max, edge, voxel,
                     trunc, origin};
    hipStream_t st = (hipStream_t)stream;
    return timed_stages<FUSE_INTEGRATE_EVENTS>(st, times_ms, [&](hipEvent_t* ev) {
        return fuse_integrate(c, (const long long*)block_key, n_blocks, tsdf, weight, rgb, workspace, workspace_bytes, st, ev,
                              (unsigned long long*)stats);
    });
}

extern "C" size_t pbn_fuse_extract_workspace_bytes(int n_blocks) {
    if (n_blocks < 0 || n_blocks > FUSE_MAX_EXTRACT_BLOCKS) return 0;
    return fuse_ext_ws_bytes(n_blocks);
}

extern "C" int pbn_fuse_extract_count(const float* tsdf, const int32_t* weight, const int64_t* block_key, int n_blocks, int min_weight,
                                      int32_t* result, void* workspace, size_t workspace_bytes, pbn_stream_t stream) {
    const FuseVolume v{tsdf, weight, nullptr, (const long long*)block_key, n_blocks, min_weight};
    return fuse_extract_count(v, result, workspace, workspace_bytes, (hipStream_t)stream, nullptr);
}

extern "C" int pbn_fuse_extract_count_timed(const float* tsdf, const int32_t* weight, const int64_t* block_key, int n_blocks,
                                            int min_weight, int32_t* result, void* workspace, size_t workspace_bytes,
                                            pbn_stream_t stream, float* times_ms) {
    if (!times_ms) return PBN_ERR_ARG;
    const FuseVolume v{tsdf, weight, nullptr, (const long long*)block_key, n_blocks, min_weight};
    hipStream_t st = (hipStream_t)stream;
    return timed_stages<FUSE_COUNT_EVENTS>(st, times_ms, [&](hipEvent_t* ev) {
        return fuse_extract_count(v, result, workspace, workspace_bytes, st, ev);
    });
}

extern "C" int pbn_fuse_extract_write(const float* tsdf, const int32_t* weight, const float* vol_rgb, const int64_t* block_key,
                                      int n_blocks, int min_weight, double voxel, const double* origin, int n_rows, float* xyz,
                                      float* rgb, float* nl, int32_t* out_weight, int64_t* voxel_id, int32_t* result, void* workspace,
                                      size_t workspace_bytes, pbn_stream_t stream) {
    const FuseVolume v{tsdf, weight, vol_rgb, (const long long*)block_key, n_blocks, min_weight};
    const FuseRows o{xyz, rgb, nl, out_weight, (long long*)voxel_id, n_rows, voxel, 0.0, 0.0, 0.0};
    return fuse_extract_write(v, o, origin, result, workspace, workspace_bytes, (hipStream_t)stream, nullptr);
}

extern "C" int pbn_fuse_extract_write_timed(const float* tsdf, const int32_t* weight, const float* vol_rgb, const int64_t* block_key,
                                            int n_blocks, int min_weight, double voxel, const double* origin, int n_rows, float* xyz,
                                            float* rgb, float* nl, int32_t* out_weight, int64_t* voxel_id, int32_t* result,
                                            void* workspace, size_t workspace_bytes, pbn_stream_t stream, float* times_ms) {
    if (!times_ms) return PBN_ERR_ARG;
    const FuseVolume v{tsdf, weight, vol_rgb, (const long long*)block_key, n_blocks, min_weight};
    const FuseRows o{xyz, rgb, nl, out_weight, (long long*)voxel_id, n_rows, voxel, 0.0, 0.0, 0.0};
    hipStream_t st = (hipStream_t)stream;
    return timed_stages<FUSE_WRITE_EVENTS>(st, times_ms, [&](hipEvent_t* ev) {
        return fuse_extract_write(v, o, origin, result, workspace, workspace_bytes, st, ev);
    });
}
