// sort_dev.h -- what the stages of the scan-decode chain (mesh.hip, cloud.hip, thin.hip, vote.hip, orient.hip) share around
// radix_sort_u32: the digit histograms its caller fills, the buffers of a sort, the launch grid, the chain's limits and
// status bits, and the stage timing of the *_timed entry points.  Integer helpers and host code only: nothing here depends
// on a translation unit's -ffp-contract setting.
#pragma once
#include "coords_dev.h"

namespace pbn {
namespace {

typedef unsigned long long u64;

// ---- limits and status bits ----------------------------------------------------------------------------------------------
constexpr int SCAN_MAX_POINTS = 1 << 28;          // points of a cloud, raw or kept
constexpr int SCAN_MAX_K = 32;                    // neighbours per point
// Bits of a stage's status word that mean the same in every stage (pbnet_amd/mesh.py mirrors them as CLOUD_*).
enum : int {
    SCAN_NONFINITE = 1,                           // k_cloud_box: a coordinate is NaN or infinite
    SCAN_EXTENT = 2,                              // k_thin_keys: an axis spans 2^21 cells or more
    SCAN_SORT_SPIN = 8,                           // radix_sort_u32: a chained scan gave up
    SCAN_WALK_CAP = 16,                           // k_orient_jump: a link chain did not end within n hops
};

// blocks of a striding grid over n items: at least one, at most cap
inline int grid_for(long long n, int cap = 1024) {
    const long long b = (n + TPB - 1) / TPB;
    return (int)(b < 1 ? 1 : b > cap ? cap : b);
}

// ---- digit histograms of radix_sort_u32 ----------------------------------------------------------------------------------
// A keys kernel declares `__shared__ unsigned s_hist[RADIX_U32_PASSES][RADIX_U32]`, clears it, adds the low 32 bits of every
// key it writes and flushes the bins it touched to the sort's ghist; it puts a barrier after the clear and before the flush.
constexpr int RADIX_U32 = 1 << RADIX_U32_DIGIT_BITS;

__device__ __forceinline__ void hist_clear(unsigned (*s_hist)[RADIX_U32]) {
    for (int e = threadIdx.x; e < RADIX_U32_PASSES * RADIX_U32; e += TPB) (&s_hist[0][0])[e] = 0u;
}
__device__ __forceinline__ void hist_add(unsigned (*s_hist)[RADIX_U32], unsigned key) {
#pragma unroll
    for (int p = 0; p < RADIX_U32_PASSES; ++p) atomicAdd(&s_hist[p][(key >> (p * RADIX_U32_DIGIT_BITS)) & (RADIX_U32 - 1)], 1u);
}
__device__ __forceinline__ void hist_flush(unsigned (*s_hist)[RADIX_U32], unsigned* __restrict__ ghist) {
    for (int e = threadIdx.x; e < RADIX_U32_PASSES * RADIX_U32; e += TPB) {
        const unsigned v = (&s_hist[0][0])[e];
        if (v) atomicAdd(&ghist[e], v);
    }
}

// ---- the buffers of a sort ---------------------------------------------------------------------------------------------
// Pairs go in through keys_a / vals_a and come out in keys_b / vals_b.  A stage that orders by a two-word key sorts twice
// over the same buffers (least significant word first) and keeps one histogram per sort, both zeroed up front.
struct SortBufs {
    u64* keys_a; u64* keys_b; int* vals_a; int* vals_b; unsigned* ghist[2]; void* scratch; size_t scratch_bytes;
};

inline SortBufs sort_carve(Carver& cv, size_t n, int n_sorts) {             // n >= 1
    SortBufs s{};
    s.keys_a = cv.take<u64>(n); s.keys_b = cv.take<u64>(n);
    s.vals_a = cv.take<int>(n); s.vals_b = cv.take<int>(n);
    for (int i = 0; i < n_sorts; ++i) s.ghist[i] = cv.take<unsigned>((size_t)RADIX_U32_PASSES * RADIX_U32);
    s.scratch_bytes = radix_sort_u32_scratch_bytes((int)n);
    s.scratch = cv.take<char>(s.scratch_bytes);
    return s;
}

// the zeroing of one histogram, for the stage's fill_ranges call
inline FillRange sort_hist_fill(const SortBufs& s, int which) {
    return FillRange{s.ghist[which], (size_t)RADIX_U32_PASSES * RADIX_U32 * sizeof(unsigned), 0};
}

inline int sort_run(const SortBufs& s, int which, int n, int32_t* status, hipStream_t st) {
    return radix_sort_u32(s.keys_a, s.keys_b, s.vals_a, s.vals_b, n, s.ghist[which], status, s.scratch, s.scratch_bytes, st);
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
