// sort_dev.h -- the interface of sort.hip's LSD radix sort, for the coordinate pyramid (pyramid.hip) and for the callers of
// radix_sort_u32 (scan_dev.h's stages, selftest.hip): the digit constants, the spin status bit, the digit histograms a
// caller fills, the sort's own words, the host entry points and the buffers of a sort.  Integer helpers and host code
// only: nothing here depends on a translation unit's -ffp-contract setting.
#pragma once
#include "coords_dev.h"

namespace pbn {

// ---- host entry points (sort.hip) ------------------------------------------------------------------------------------------
size_t sort_state_bytes(int n, int passes);        // chained-scan state of `passes` digit passes over n keys (n <= 0: as 1 key)
// The pyramid's sort of (64-bit key, row): MAX_PASSES launches of k_sort_pass, which reads its digits from the plan
// (coords_dev.h) and returns at once in a pass the box does not need; the result lands in buffer (passes & 1).  The sort's
// words are the plan's SW_WORDS ints from PL_SORT (one pointer: a second one cost the ticket draw a scalar load, 0.2 us a
// pass); the caller zeroes them, state (sort_state_bytes(n_max, MAX_PASSES)) and ghist (MAX_PASSES x RADIX, then filled).
int radix_sort_planned(unsigned long long* keys_a, unsigned long long* keys_b, int32_t* vals_a, int32_t* vals_b,
                       const int32_t* n_dev, int n_max, int32_t* plan, int32_t* status, const unsigned* ghist,
                       unsigned long long* state, hipStream_t stream);
// The same digit pass for 32-bit keys in the low half of u64 keys, values carried; stable, so ties keep the input order.
// ghist: RADIX_U32_PASSES x RADIX digit histograms (digit p = key >> p * RADIX_BITS & RADIX - 1), filled by the caller; the
// result lands in keys_b / vals_b.  A chained scan that gives up ORs SORT_SPIN into *status.
size_t radix_sort_u32_scratch_bytes(int n);
int radix_sort_u32_tile();                         // keys per workgroup of a digit pass (SORT_TILE of this build)
int radix_sort_u32(unsigned long long* keys_a, unsigned long long* keys_b, int32_t* vals_a, int32_t* vals_b, int n,
                   const unsigned* ghist, int32_t* status, void* scratch, size_t scratch_bytes, hipStream_t stream);

namespace {

typedef unsigned long long u64;

// ---- digits ------------------------------------------------------------------------------------------------------------------
constexpr int RADIX_BITS = 11, RADIX = 1 << RADIX_BITS;   // the widest digit and its bins (sort.hip: why a digit may be narrower)
constexpr int MAX_PASSES = 4;                             // digits of the widest key the sort takes
constexpr int RADIX_U32_PASSES = 3;                       // digits of radix_sort_u32, each RADIX_BITS wide
constexpr int SORT_SPIN = 8;                              // status bit: a chained scan gave up waiting for a predecessor

// nbits key bits are cut into the fewest digits of at most RADIX_BITS bits, each as narrow as that allows (>= 8 bits)
struct SortPlan { int passes, dbits; };
__device__ __forceinline__ SortPlan sort_plan(int nbits) {
    SortPlan sp;
    sp.passes = nbits <= 3 * RADIX_BITS ? min(3, (nbits + 7) / 8) : MAX_PASSES;
    sp.dbits = max(8, (nbits + sp.passes - 1) / sp.passes);
    return sp;
}

// A word of chained-scan state (sort.hip's digit pass, k_pyramid's level scan): payload and flag in one 8-byte granule,
// written by ONE agent-scope atomic store and read by agent-scope atomic loads, so no fences; every poll is bounded
__device__ __forceinline__ u64 ld_state(const u64* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void st_state(u64* p, u64 v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
constexpr unsigned SPIN_LIMIT = 1u << 24;

// The sort's own words (int32, zeroed by the caller): one ticket per pass and, in a PBN_SORT_STAMPS build, the cycle
// stamps of two workgroups.  Words 4..7 are not the sort's: a caller that embeds the block may keep words of its own there.
enum { SW_TICKET0 = 0, SW_STAMPS = 8, SW_WORDS = SW_STAMPS + 32 };

// ---- digit histograms ----------------------------------------------------------------------------------------------------
// A keys kernel declares `__shared__ unsigned s_hist[passes][RADIX]`, clears it, adds every key it writes (`passes` digits
// of `dbits` bits) and flushes the bins it touched to the sort's ghist; it puts a barrier after the clear and before the
// flush.  The defaults are radix_sort_u32's digits.
__device__ __forceinline__ void hist_clear(unsigned (*s_hist)[RADIX], int passes = RADIX_U32_PASSES) {
    for (int e = threadIdx.x; e < passes * RADIX; e += TPB) (&s_hist[0][0])[e] = 0u;
}
__device__ __forceinline__ void hist_add(unsigned (*s_hist)[RADIX], u64 key, int passes = RADIX_U32_PASSES, int dbits = RADIX_BITS) {
    for (int p = 0; p < passes; ++p) atomicAdd(&s_hist[p][(unsigned)(key >> (p * dbits)) & ((1u << dbits) - 1u)], 1u);
}
__device__ __forceinline__ void hist_flush(unsigned (*s_hist)[RADIX], unsigned* __restrict__ ghist, int passes = RADIX_U32_PASSES) {
    for (int e = threadIdx.x; e < passes * RADIX; e += TPB) {
        const unsigned v = (&s_hist[0][0])[e];
        if (v) atomicAdd(&ghist[e], v);
    }
}

// ---- the buffers of a radix_sort_u32 -------------------------------------------------------------------------------------
// Pairs go in through keys_a / vals_a and come out in keys_b / vals_b.  A stage that orders by a two-word key sorts twice
// over the same buffers (least significant word first) and keeps one histogram per sort, both zeroed up front.
struct SortBufs {
    u64* keys_a; u64* keys_b; int* vals_a; int* vals_b; unsigned* ghist[2]; void* scratch; size_t scratch_bytes;
};

inline SortBufs sort_carve(Carver& cv, size_t n, int n_sorts) {             // n >= 1
    SortBufs s{};
    s.keys_a = cv.take<u64>(n); s.keys_b = cv.take<u64>(n);
    s.vals_a = cv.take<int>(n); s.vals_b = cv.take<int>(n);
    for (int i = 0; i < n_sorts; ++i) s.ghist[i] = cv.take<unsigned>((size_t)RADIX_U32_PASSES * RADIX);
    s.scratch_bytes = radix_sort_u32_scratch_bytes((int)n);
    s.scratch = cv.take<char>(s.scratch_bytes);
    return s;
}

// the zeroing of one histogram, for the stage's fill_ranges call
inline FillRange sort_hist_fill(const SortBufs& s, int which) {
    return FillRange{s.ghist[which], (size_t)RADIX_U32_PASSES * RADIX * sizeof(unsigned), 0};
}

inline int sort_run(const SortBufs& s, int which, int n, int32_t* status, hipStream_t st) {
    return radix_sort_u32(s.keys_a, s.keys_b, s.vals_a, s.vals_b, n, s.ghist[which], status, s.scratch, s.scratch_bytes, st);
}

}  // namespace
}  // namespace pbn
