// selftest.hip -- entry points that put the shared device primitives under a test of their own: fill_ranges and the two
// exclusive scans (common.hip), radix_sort_u32 behind sort_dev.h's SortBufs / sort_run and histogram helpers (sort.hip).
// Every entry is a shim: it checks its arguments on the host, carves its workspace with Carver and calls the primitive the
// way the stages do (thin.hip's carve / args / run split).  Nothing here computes, repairs or re-orders a result:
// tests/test_prims_gpu.py compares what comes back with tests/prims_ref.py byte for byte.
#include "scan_dev.h"

namespace pbn {
namespace {

enum : int { SELFTEST_SCAN = 0, SELFTEST_SCAN_CHAINED = 1, SELFTEST_SORT = 2 };
constexpr int SELFTEST_MAX_RANGES = 64;            // ranges of one pbn_selftest_fill call

// ---- scans ---------------------------------------------------------------------------------------------------------------
struct ScanWs { int* tmp; unsigned long long* state; size_t state_words; };

ScanWs scan_carve(Carver& cv, int n, int chained) {
    ScanWs w{};
    if (chained) {
        w.state_words = scan_chained_state_words((long long)n);
        w.state = cv.take<unsigned long long>(w.state_words);
    } else {
        w.tmp = cv.take<int>(scan_tmp_ints((long long)n));
    }
    return w;
}

size_t scan_ws_bytes(int n, int chained) {
    Carver cv(nullptr, 0);
    scan_carve(cv, n, chained);
    return cv.off + 256;
}

// ---- sort ----------------------------------------------------------------------------------------------------------------
// The keys kernel of a stage (k_edge_weights, k_thin_keys): the pair goes into keys_a / vals_a, the key into the histograms.
__global__ __launch_bounds__(TPB) void k_selftest_keys(const unsigned* __restrict__ key_in, const int* __restrict__ val_in, int n,
                                                       u64* __restrict__ keys, int* __restrict__ vals,
                                                       unsigned* __restrict__ ghist) {
    __shared__ unsigned s_hist[RADIX_U32_PASSES][RADIX];
    hist_clear(s_hist);
    __syncthreads();
    for (int i = blockIdx.x * TPB + threadIdx.x; i < n; i += gridDim.x * TPB) {
        const unsigned key = key_in[i];
        keys[i] = (u64)key;
        vals[i] = val_in[i];
        hist_add(s_hist, key);
    }
    __syncthreads();
    hist_flush(s_hist, ghist);
}

__global__ __launch_bounds__(TPB) void k_selftest_copy_out(const u64* __restrict__ keys_b, const int* __restrict__ vals_b, int n,
                                                           u64* __restrict__ keys_out, int* __restrict__ vals_out) {
    for (int i = blockIdx.x * TPB + threadIdx.x; i < n; i += gridDim.x * TPB) {
        keys_out[i] = keys_b[i];
        vals_out[i] = vals_b[i];
    }
}

size_t sort_ws_bytes(int n) {
    Carver cv(nullptr, 0);
    sort_carve(cv, (size_t)(n > 0 ? n : 1), 1);
    return cv.off + 256;
}

}  // namespace
}  // namespace pbn

using namespace pbn;

extern "C" size_t pbn_selftest_workspace_bytes(int what, int n) {
    if (n < 0 || n > SCAN_MAX_POINTS) return 0;
    if (what == SELFTEST_SCAN || what == SELFTEST_SCAN_CHAINED) return scan_ws_bytes(n, what == SELFTEST_SCAN_CHAINED);
    if (what == SELFTEST_SORT) return sort_ws_bytes(n);
    return 0;
}

extern "C" int pbn_selftest_sort_tile(void) { return radix_sort_u32_tile(); }

extern "C" int pbn_selftest_fill(uint8_t* base, const int64_t* offset, const int64_t* bytes, const uint8_t* value, int n_ranges,
                                 pbn_stream_t stream) {
    if (n_ranges < 0 || n_ranges > SELFTEST_MAX_RANGES) return PBN_ERR_ARG;
    if (n_ranges && (!base || !offset || !bytes || !value)) return PBN_ERR_ARG;
    FillRange fr[SELFTEST_MAX_RANGES];
    for (int i = 0; i < n_ranges; ++i) {
        if (offset[i] < -1 || bytes[i] < 0) return PBN_ERR_ARG;
        fr[i] = FillRange{offset[i] < 0 ? nullptr : (void*)(base + offset[i]), (size_t)bytes[i], value[i]};
    }
    return fill_ranges(fr, n_ranges, (hipStream_t)stream);
}

extern "C" int pbn_selftest_scan(const int32_t* in, int32_t* out, int n, int chained, int32_t* total, int32_t* status, void* ws,
                                 size_t ws_bytes, pbn_stream_t stream) {
    if (n < 0 || n > SCAN_MAX_POINTS || (chained != 0 && chained != 1)) return PBN_ERR_ARG;
    if ((n && (!in || !out)) || (chained && !status) || !ws) return PBN_ERR_ARG;
    if (ws_bytes < scan_ws_bytes(n, chained)) return PBN_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    Carver cv(ws, ws_bytes);
    const ScanWs w = scan_carve(cv, n, chained);
    if (!cv.ok) return PBN_ERR_WORKSPACE;
    if (!chained) return scan_exclusive_i32(in, out, n, w.tmp, total, st);
    // the caller's part of the chained form, as in cluster.hip: states, ticket and *total zeroed by the stage's fill
    const FillRange fr[] = {{w.state, w.state_words * sizeof(unsigned long long), 0}, {total, sizeof(int32_t), 0}};
    const int rc = fill_ranges(fr, 2, st);
    if (rc != PBN_OK) return rc;
    return scan_exclusive_i32_chained(in, out, n, w.state, total, status, st);
}

extern "C" int pbn_selftest_sort_u32(const uint32_t* keys, const int32_t* vals, int n, uint64_t* keys_out, int32_t* vals_out,
                                     int32_t* status, void* ws, size_t ws_bytes, pbn_stream_t stream) {
    if (n < 0 || n > SCAN_MAX_POINTS) return PBN_ERR_ARG;
    if ((n && (!keys || !vals || !keys_out || !vals_out)) || !status || !ws) return PBN_ERR_ARG;
    if (ws_bytes < sort_ws_bytes(n)) return PBN_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    Carver cv(ws, ws_bytes);
    const SortBufs s = sort_carve(cv, (size_t)(n > 0 ? n : 1), 1);
    if (!cv.ok) return PBN_ERR_WORKSPACE;
    const FillRange fr = sort_hist_fill(s, 0);
    int rc = fill_ranges(&fr, 1, st);
    if (rc != PBN_OK) return rc;
    if (n == 0) return PBN_OK;
    const dim3 grid(grid_for(n)), block(TPB);
    hipLaunchKernelGGL(k_selftest_keys, grid, block, 0, st, keys, vals, n, s.keys_a, s.vals_a, s.ghist[0]);
    PBN_LAUNCH_CHECK();
    rc = sort_run(s, 0, n, status, st);
    if (rc != PBN_OK) return rc;
    hipLaunchKernelGGL(k_selftest_copy_out, grid, block, 0, st, s.keys_b, s.vals_b, n, (u64*)keys_out, vals_out);
    PBN_LAUNCH_CHECK();
    return PBN_OK;
}
