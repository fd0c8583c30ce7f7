// scan_dev.h -- what the stages of the scan-decode chain (mesh.hip, cloud.hip, thin.hip, vote.hip, orient.hip) share around
// radix_sort_u32 (sort_dev.h, which this includes): the chain's limits and status bits, the launch grid, and the stage
// timing of the *_timed entry points.  Host code only: nothing here depends on a translation unit's -ffp-contract setting.
#pragma once
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
