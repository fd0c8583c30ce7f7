// frames.hip -- posed depth frames to one compacted cloud: what a depth camera hands over (depth images, colour images, a
// pose and intrinsics per frame) back-projected on the device.  include/pbnet_hip.h ("Posed depth frames") states the
// contract, tests/frames_ref.py restates it in numpy.
//
//   count    one lane per SAMPLED pixel (the pixels with u % stride == 0 and v % stride == 0, numbered row-major inside
//            their frame, which is the order of their pixel ids): the validity test, a wave64 ballot, a popcount; one count
//            per workgroup;
//   scan     scan_exclusive_i32 over the workgroup counts; its total is N;
//   starts   frame_start[f] = the offset of frame f's first workgroup, frame_start[F] = N;
//   -- the caller reads (status, N) back and allocates N rows --
//   write    the validity test again, the ballot again; a wave's survivors go to the workgroup's offset + the counts of the
//            64-pixel chunks before its own + the lane's rank in the ballot.
//
// A workgroup covers FRAMES_BLOCK consecutive sampled pixels of ONE frame (the last workgroup of a frame is short), in
// FRAMES_CHUNKS chunks of 64: chunk c is wave (c % 4)'s iteration c / 4, so chunk order is pixel order.  The pose and the
// intrinsics are then uniform over the workgroup (scalar loads), and frame_start falls out of the workgroup offsets.
//
// Validity is computed twice, flags are never stored: the second test reads 2 to 5 bytes per pixel again (the depth, and
// the colour only of survivors), a flag array would cost a byte written and a byte read per pixel plus the same depth read
// for z.  The neighbour depths of the edge test come straight from the cache: the four neighbours of a row-major run of
// 64 pixels are the same cache lines as the run itself and the rows above and below, which the neighbouring waves load
// as their own centres.
//
// Arithmetic contract (-ffp-contract=off): float64, one rounded operation per written operation; float32 on the store.
#include <cmath>

#include "frames_dev.h"
#include "scan_dev.h"

namespace pbn {
namespace {

constexpr int FRAMES_ITERS = 4;                              // sampled pixels per lane
constexpr int FRAMES_BLOCK = TPB * FRAMES_ITERS;             // sampled pixels per workgroup
constexpr int FRAMES_CHUNKS = FRAMES_BLOCK / WAVE;           // ballots per workgroup
constexpr int FRAMES_WAVES = TPB / WAVE;
constexpr int FRAMES_ROWS = 1;                               // status: the write pass met a row at or beyond n_rows
constexpr int FRAMES_COUNT_EVENTS = 3, FRAMES_WRITE_EVENTS = 2;

struct FramesCam {                                           // device copies of the host's pose [F,16] and intr [F,4]
    const double* pose;
    const double* intr;
};

struct FramesShape {
    int n_frames, height, width, stride;
    int hs, ws;                                              // sampled rows and columns
    int per_frame;                                           // hs * ws
    int blocks_per_frame;
    double scale, z_min, z_max, edge;
};

// One sampled pixel s of frame f (pose_ok = rule (a)): rules (b), (c), (d); the pixel id and the float32 world point.
template <typename D>
__device__ __forceinline__ bool frames_point(const D* __restrict__ depth, const FramesShape& a, const double* __restrict__ P,
                                             const double* __restrict__ K, bool pose_ok, int f, int s, int& id, float& X,
                                             float& Y, float& Z) {
    if (!pose_ok || s >= a.per_frame) return false;
    const int v = (s / a.ws) * a.stride, u = (s % a.ws) * a.stride;
    const D* __restrict__ img = depth + (size_t)f * a.height * a.width;
    id = (int)(((size_t)f * a.height + v) * a.width + u);    // F * H * W <= 2^31 - 1
    double z;
    if (!frames_depth_ok(img, a.height, a.width, u, v, a.scale, a.z_min, a.z_max, a.edge, z)) return false;   // rules (b), (c)
    const double xc = (((double)u - K[2]) * z) / K[0];
    const double yc = (((double)v - K[3]) * z) / K[1];
    X = (float)(((P[0] * xc + P[1] * yc) + P[2] * z) + P[3]);
    Y = (float)(((P[4] * xc + P[5] * yc) + P[6] * z) + P[7]);
    Z = (float)(((P[8] * xc + P[9] * yc) + P[10] * z) + P[11]);
    return __builtin_isfinite(X) && __builtin_isfinite(Y) && __builtin_isfinite(Z);
}

// WRITE = false: counts[workgroup] = its valid pixels.  WRITE = true: the rows, at offs[workgroup] + ...
template <typename D, bool WRITE>
__global__ __launch_bounds__(TPB) void k_frames(const D* __restrict__ depth, const unsigned char* __restrict__ colour,
                                                FramesCam cam, FramesShape a, int* __restrict__ counts,
                                                const int* __restrict__ offs, int n_rows, float* __restrict__ xyz,
                                                float* __restrict__ rgb, int* __restrict__ pixel, int* __restrict__ status) {
    __shared__ int s_cnt[FRAMES_CHUNKS];
    if (WRITE && *status != 0) return;                       // uniform: nothing is written
    const int f = (int)blockIdx.x / a.blocks_per_frame;
    const int base = ((int)blockIdx.x % a.blocks_per_frame) * FRAMES_BLOCK;
    const double* __restrict__ P = cam.pose + 16 * (size_t)f;
    const double* __restrict__ K = cam.intr + 4 * (size_t)f;
    const bool pose_ok = frames_pose_ok(P);
    const int lane = lane_id(), wave = (int)threadIdx.x >> 6;
    bool ok[FRAMES_ITERS];
    int id[FRAMES_ITERS];
    float X[FRAMES_ITERS], Y[FRAMES_ITERS], Z[FRAMES_ITERS];
    unsigned long long ballot[FRAMES_ITERS];
#pragma unroll
    for (int it = 0; it < FRAMES_ITERS; ++it) {
        id[it] = 0; X[it] = Y[it] = Z[it] = 0.0f;
        ok[it] = frames_point(depth, a, P, K, pose_ok, f, base + it * TPB + (int)threadIdx.x, id[it], X[it], Y[it], Z[it]);
        ballot[it] = __ballot(ok[it]);
        if (lane == 0) s_cnt[it * FRAMES_WAVES + wave] = __popcll(ballot[it]);
    }
    __syncthreads();
    if (!WRITE) {
        if (threadIdx.x == 0) {
            int total = 0;
            for (int c = 0; c < FRAMES_CHUNKS; ++c) total += s_cnt[c];
            counts[blockIdx.x] = total;
        }
        return;
    }
    int before = offs[blockIdx.x];                           // rows before chunk c, c walking with the loop below
    int c = 0;
    bool over = false;
#pragma unroll
    for (int it = 0; it < FRAMES_ITERS; ++it) {
        for (; c < it * FRAMES_WAVES + wave; ++c) before += s_cnt[c];
        if (!ok[it]) continue;
        const int r = before + __popcll(ballot[it] & ((1ull << lane) - 1ull));
        if (r < 0 || r >= n_rows) { over = true; continue; }
        xyz[3 * (size_t)r] = X[it]; xyz[3 * (size_t)r + 1] = Y[it]; xyz[3 * (size_t)r + 2] = Z[it];
        pixel[r] = id[it];
        if (colour) {
            const unsigned char* __restrict__ cp = colour + 3 * (size_t)id[it];
            rgb[3 * (size_t)r] = (float)cp[0]; rgb[3 * (size_t)r + 1] = (float)cp[1]; rgb[3 * (size_t)r + 2] = (float)cp[2];
        }
    }
    if (over) atomicOr(status, FRAMES_ROWS);
}

// frame_start[f] = the offset of frame f's first workgroup; frame_start[F] = N (result[1], the scan's total)
__global__ __launch_bounds__(TPB) void k_frames_starts(const int* __restrict__ offs, const int* __restrict__ result, int n_frames,
                                                       int blocks_per_frame, int* __restrict__ frame_start) {
    for (int f = blockIdx.x * TPB + threadIdx.x; f <= n_frames; f += gridDim.x * TPB)
        frame_start[f] = f < n_frames ? offs[(size_t)f * blocks_per_frame] : result[1];
}

// ---- host --------------------------------------------------------------------------------------------------------------
struct FramesWs {
    double* pose; double* intr; int* counts; int* offs; int* scan_tmp;
};

// false = out of range (the header's Limits on sizes)
bool frames_shape(int n_frames, int height, int width, int stride, FramesShape& a) {
    if (n_frames < 0 || height < 0 || width < 0 || stride < 1) return false;
    if ((long long)n_frames * height * width > 2147483647LL) return false;
    a.n_frames = n_frames; a.height = height; a.width = width; a.stride = stride;
    a.hs = height ? (height - 1) / stride + 1 : 0;
    a.ws = width ? (width - 1) / stride + 1 : 0;
    a.per_frame = a.hs * a.ws;                               // <= H * W
    if ((long long)n_frames * a.per_frame > (long long)SCAN_MAX_POINTS) return false;
    a.blocks_per_frame = cdiv(a.per_frame, FRAMES_BLOCK);
    return true;
}

long long frames_blocks(const FramesShape& a) { return (long long)a.n_frames * a.blocks_per_frame; }

FramesWs frames_carve(Carver& cv, const FramesShape& a) {
    FramesWs w{};
    const size_t F = (size_t)(a.n_frames > 0 ? a.n_frames : 1);
    const long long nb = frames_blocks(a) > 0 ? frames_blocks(a) : 1;
    w.pose = cv.take<double>(16 * F);
    w.intr = cv.take<double>(4 * F);
    w.counts = cv.take<int>((size_t)nb);
    w.offs = cv.take<int>((size_t)nb);
    w.scan_tmp = cv.take<int>(scan_tmp_ints(nb));
    return w;
}

struct FramesCall {
    const void* depth; int depth_is_f32; const uint8_t* colour; const double* pose; const double* intr;
    int n_frames, height, width; double depth_scale, depth_min, depth_max; int stride; double edge;
    void* workspace; size_t workspace_bytes;
};

// every host-side check of both passes; fills the shape and carves the workspace
int frames_args(const FramesCall& c, const int32_t* result, FramesShape& a, FramesWs& w) {
    if (!frames_shape(c.n_frames, c.height, c.width, c.stride, a)) return PBN_ERR_ARG;
    if (c.depth_is_f32 != 0 && c.depth_is_f32 != 1) return PBN_ERR_ARG;
    if (!(c.depth_scale > 0.0) || !std::isfinite(c.depth_scale) || !(c.depth_min <= c.depth_max)) return PBN_ERR_ARG;
    if (!result || !c.workspace) return PBN_ERR_ARG;
    if (c.n_frames && (!c.pose || !c.intr)) return PBN_ERR_ARG;
    if (frames_blocks(a) && !c.depth) return PBN_ERR_ARG;
    for (int f = 0; f < c.n_frames; ++f) {
        const double fx = c.intr[4 * (size_t)f], fy = c.intr[4 * (size_t)f + 1];
        if (!(fx > 0.0) || !std::isfinite(fx) || !(fy > 0.0) || !std::isfinite(fy)) return PBN_ERR_ARG;
    }
    a.scale = c.depth_scale; a.z_min = c.depth_min; a.z_max = c.depth_max; a.edge = c.edge;
    Carver cv(c.workspace, c.workspace_bytes);
    w = frames_carve(cv, a);
    return cv.ok ? PBN_OK : PBN_ERR_WORKSPACE;
}

template <bool WRITE>
void frames_launch(const FramesCall& c, const FramesShape& a, const FramesWs& w, int n_rows, float* xyz, float* rgb,
                   int32_t* pixel, int32_t* status, hipStream_t st) {
    const FramesCam cam{w.pose, w.intr};
    const dim3 grid((unsigned)frames_blocks(a));
    if (c.depth_is_f32)
        hipLaunchKernelGGL((k_frames<float, WRITE>), grid, dim3(TPB), 0, st, (const float*)c.depth, c.colour, cam, a, w.counts,
                           w.offs, n_rows, xyz, rgb, pixel, status);
    else
        hipLaunchKernelGGL((k_frames<unsigned short, WRITE>), grid, dim3(TPB), 0, st, (const unsigned short*)c.depth, c.colour,
                           cam, a, w.counts, w.offs, n_rows, xyz, rgb, pixel, status);
}

// ev (optional): FRAMES_COUNT_EVENTS events around count | scan + starts
int frames_count(const FramesCall& c, int32_t* frame_start, int32_t* result, hipStream_t st, hipEvent_t* ev) {
    FramesShape a{};
    FramesWs w{};
    PBN_TRY(frames_args(c, result, a, w));
    if (!frame_start) return PBN_ERR_ARG;
    const long long nb = frames_blocks(a);
    const FillRange fr[] = {{result, 2 * sizeof(int32_t), 0}, {frame_start, ((size_t)c.n_frames + 1) * sizeof(int32_t), 0}};
    PBN_TRY(fill_ranges(fr, nb ? 1 : 2, st));
    if (ev) PBN_HIP_CHECK(hipEventRecord(ev[0], st));
    if (nb == 0) {                                           // no frame, or frames without a pixel: N = 0, every start 0
        if (ev) for (int i = 1; i < FRAMES_COUNT_EVENTS; ++i) PBN_HIP_CHECK(hipEventRecord(ev[i], st));
        return PBN_OK;
    }
    PBN_HIP_CHECK(hipMemcpyAsync(w.pose, c.pose, 16 * (size_t)c.n_frames * sizeof(double), hipMemcpyHostToDevice, st));
    PBN_HIP_CHECK(hipMemcpyAsync(w.intr, c.intr, 4 * (size_t)c.n_frames * sizeof(double), hipMemcpyHostToDevice, st));
    frames_launch<false>(c, a, w, 0, nullptr, nullptr, nullptr, result, st);
    PBN_LAUNCH_CHECK();
    if (ev) PBN_HIP_CHECK(hipEventRecord(ev[1], st));
    PBN_TRY(scan_exclusive_i32(w.counts, w.offs, (int)nb, w.scan_tmp, result + 1, st));
    hipLaunchKernelGGL(k_frames_starts, dim3(grid_for(c.n_frames + 1)), dim3(TPB), 0, st, w.offs, result, c.n_frames,
                       a.blocks_per_frame, frame_start);
    PBN_LAUNCH_CHECK();
    if (ev) PBN_HIP_CHECK(hipEventRecord(ev[2], st));
    return PBN_OK;
}

// ev (optional): FRAMES_WRITE_EVENTS events around the write
int frames_write(const FramesCall& c, int n_rows, float* xyz, float* rgb, int32_t* pixel, int32_t* result, hipStream_t st,
                 hipEvent_t* ev) {
    FramesShape a{};
    FramesWs w{};
    PBN_TRY(frames_args(c, result, a, w));
    if (n_rows < 0 || n_rows > SCAN_MAX_POINTS) return PBN_ERR_ARG;
    if (n_rows && (!xyz || !pixel || (c.colour != nullptr) != (rgb != nullptr))) return PBN_ERR_ARG;
    if (ev) PBN_HIP_CHECK(hipEventRecord(ev[0], st));
    if (frames_blocks(a)) {                                  // the workspace still holds pose, intr and offs of the count pass
        frames_launch<true>(c, a, w, n_rows, xyz, rgb, pixel, result, st);
        PBN_LAUNCH_CHECK();
    }
    if (ev) PBN_HIP_CHECK(hipEventRecord(ev[1], st));
    return PBN_OK;
}

}  // namespace
}  // namespace pbn

using namespace pbn;

extern "C" size_t pbn_frames_workspace_bytes(int n_frames, int height, int width, int stride) {
    FramesShape a{};
    if (!frames_shape(n_frames, height, width, stride, a)) return 0;
    Carver cv(nullptr, 0);
    frames_carve(cv, a);
    return cv.off + 256;
}

extern "C" int pbn_frames_block_pixels(void) { return FRAMES_BLOCK; }

extern "C" int pbn_frames_count(const void* depth, int depth_is_f32, const uint8_t* colour, const double* pose, const double* intr,
                                int n_frames, int height, int width, double depth_scale, double depth_min, double depth_max,
                                int stride, double edge, int32_t* frame_start, int32_t* result, void* workspace,
                                size_t workspace_bytes, pbn_stream_t stream) {
    const FramesCall c{depth, depth_is_f32, colour, pose, intr, n_frames, height, width, depth_scale, depth_min, depth_max, stride,
                       edge, workspace, workspace_bytes};
    return frames_count(c, frame_start, result, (hipStream_t)stream, nullptr);
}

extern "C" int pbn_frames_count_timed(const void* depth, int depth_is_f32, const uint8_t* colour, const double* pose,
                                      const double* intr, int n_frames, int height, int width, double depth_scale, double depth_min,
                                      double depth_max, int stride, double edge, int32_t* frame_start, int32_t* result,
                                      void* workspace, size_t workspace_bytes, pbn_stream_t stream, float* times_ms) {
    if (!times_ms) return PBN_ERR_ARG;
    const FramesCall c{depth, depth_is_f32, colour, pose, intr, n_frames, height, width, depth_scale, depth_min, depth_max, stride,
                       edge, workspace, workspace_bytes};
    hipStream_t st = (hipStream_t)stream;
    return timed_stages<FRAMES_COUNT_EVENTS>(st, times_ms, [&](hipEvent_t* ev) { return frames_count(c, frame_start, result, st, ev); });
}

extern "C" int pbn_frames_write(const void* depth, int depth_is_f32, const uint8_t* colour, const double* pose, const double* intr,
                                int n_frames, int height, int width, double depth_scale, double depth_min, double depth_max,
                                int stride, double edge, int n_rows, float* xyz, float* rgb, int32_t* pixel, int32_t* result,
                                void* workspace, size_t workspace_bytes, pbn_stream_t stream) {
    const FramesCall c{depth, depth_is_f32, colour, pose, intr, n_frames, height, width, depth_scale, depth_min, depth_max, stride,
                       edge, workspace, workspace_bytes};
    return frames_write(c, n_rows, xyz, rgb, pixel, result, (hipStream_t)stream, nullptr);
}

extern "C" int pbn_frames_write_timed(const void* depth, int depth_is_f32, const uint8_t* colour, const double* pose,
                                      const double* intr, int n_frames, int height, int width, double depth_scale, double depth_min,
                                      double depth_max, int stride, double edge, int n_rows, float* xyz, float* rgb, int32_t* pixel,
                                      int32_t* result, void* workspace, size_t workspace_bytes, pbn_stream_t stream,
                                      float* times_ms) {
    if (!times_ms) return PBN_ERR_ARG;
    const FramesCall c{depth, depth_is_f32, colour, pose, intr, n_frames, height, width, depth_scale, depth_min, depth_max, stride,
                       edge, workspace, workspace_bytes};
    hipStream_t st = (hipStream_t)stream;
    return timed_stages<FRAMES_WRITE_EVENTS>(st, times_ms, [&](hipEvent_t* ev) {
        return frames_write(c, n_rows, xyz, rgb, pixel, result, st, ev);
    });
}
