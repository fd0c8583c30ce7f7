// sort.hip -- the stable LSD radix sort of (key, value) pairs behind sort_dev.h: one digit per launch, a chained (decoupled
// look-back) scan over the workgroups inside the launch.  Two kernels share one digit pass: k_sort_pass for the coordinate
// pyramid (64-bit Z-order keys, digits decided on the device from the pyramid's plan) and k_sort_pass_u32 for
// radix_sort_u32 (32-bit keys, three digits of RADIX_BITS bits).  The digit histograms come from the caller's keys kernel
// (sort_dev.h: hist_clear / hist_add / hist_flush).  Integer code: no -ffp-contract setting applies.
#include "sort_dev.h"

namespace pbn {
namespace {

#ifndef PBN_SORT_ITEMS
#define PBN_SORT_ITEMS 8
#endif
constexpr int SORT_ITEMS = PBN_SORT_ITEMS, SORT_TILE = TPB * SORT_ITEMS;   // keys per workgroup; a wave's are contiguous
constexpr size_t SORT_LDS_BYTES = (size_t)SORT_TILE * 12 + (size_t)(TPB / 64 + 2) * RADIX * 4;

// ---- one digit per launch, chained scan over the workgroups ------------------------------------------------------------------
// Digit width: the box needs nbits key bits; they are cut into the fewest digits of at most 11 bits (3 up to 33 bits, 4
// up to 44), each as NARROW as that allows (>= 8 bits): a workgroup's 4096 keys then fall into few enough bins that, after
// a local reorder through LDS, runs of keys leave for consecutive addresses (a 24-bit room: 256 bins, runs of 16 keys =
// whole cache lines; the scattered 8- and 4-byte stores of a direct scatter were 2/3 of a pass).
// state[blk][bins / 2]: two bins per 64-bit word, each  flag << 30 | count  (flag 1: the workgroup's own count, 2: the
// inclusive prefix over workgroups 0..blk); a word is written by ONE agent-scope atomic store and read by agent-scope
// atomic loads (the payload and its flag share the 8-byte granule: no fences).  Workgroup numbers are drawn from a ticket
// so that every predecessor of a running workgroup has started.
// ld_state (sort_dev.h) without the compiler's wait behind it: a batch of them is issued back to back and waited for once
// (ld_state_wait); the agent-scope atomic form costs one memory round trip PER load (measured: 8 of them 3.4 us)
__device__ __forceinline__ void ld_state_issue(u64& dst, const u64* p) {
    asm volatile("global_load_dwordx2 %0, %1, off sc1" : "=v"(dst) : "v"(p) : "memory");
}
__device__ __forceinline__ void ld_state_wait() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }

#ifdef PBN_SORT_STAMPS
#define SORT_STAMP(I) if (threadIdx.x == 0 && pass == 0 && (blk == 0 || blk == 20)) words[SW_STAMPS + (blk ? 16 : 0) + (I)] = (int)__builtin_readcyclecounter();
#else
#define SORT_STAMP(I)
#endif
struct SortShared {
    u64* s_key; int* s_val; unsigned (*s_cnt)[RADIX]; unsigned* s_base; unsigned* s_local;
};

// the dynamic LDS block of a digit pass (SORT_LDS_BYTES) as its arrays
__device__ __forceinline__ SortShared sort_shared() {
    extern __shared__ __attribute__((aligned(16))) unsigned char sort_smem[];
    SortShared sh;
    sh.s_key = reinterpret_cast<u64*>(sort_smem);                                   // SORT_TILE keys in the workgroup's sorted order
    sh.s_val = reinterpret_cast<int*>(sh.s_key + SORT_TILE);
    sh.s_cnt = reinterpret_cast<unsigned (*)[RADIX]>(sh.s_val + SORT_TILE);         // per wave and bin: counts, then wave bases
    sh.s_base = &sh.s_cnt[TPB / 64][0];          // where the bin's keys of this workgroup start in the output
    sh.s_local = sh.s_base + RADIX;              // ... and in the workgroup's own sorted order
    return sh;
}

// Start of a digit pass: draws the workgroup's number blk from the pass's ticket and clears s_cnt.  False: nothing to do
// (no keys, or the tile of this number lies past them); n is uniform over the workgroup.
__device__ __forceinline__ bool sort_begin(const SortShared& sh, int* ticket, int n, int& blk) {
    __shared__ int s_blk;
    if (n <= 0) return false;
    const int tid = threadIdx.x;
    if (tid == 0) s_blk = atomicAdd(ticket, 1);
    for (int e = tid; e < (TPB / 64) * RADIX; e += TPB) (&sh.s_cnt[0][0])[e] = 0u;
    __syncthreads();
    blk = s_blk;
    return (long long)blk * SORT_TILE < n;
}

// One digit of the sort for a workgroup, BPT = bins per thread (digit width 8 + log2(BPT) bits) as a compile-time constant:
// every register array below is indexed by constants.
template <int BPT>
__device__ __forceinline__ void sort_pass_body(const u64* __restrict__ kin, u64* __restrict__ kout, const int* __restrict__ vin,
                                               int* __restrict__ vout, int n, int pass, int* __restrict__ words,
                                               int* __restrict__ status, const unsigned* __restrict__ ghist,
                                               u64* __restrict__ state, const SortShared& sh, int blk, unsigned (*s_wtot)[TPB / 64]) {
    constexpr int DBITS = (BPT == 1 ? 8 : BPT == 2 ? 9 : BPT == 4 ? 10 : 11), R = 1 << DBITS;
    constexpr int W = BPT >= 2 ? BPT / 2 : 1;        // 64-bit state words of one workgroup this thread reads
    constexpr int LB = 32 / W;                       // predecessors per look-back batch (32 loads in flight per thread)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long base = (long long)blk * SORT_TILE;
    const int shift = pass * DBITS;
    constexpr unsigned dmask = (unsigned)R - 1u;
    SORT_STAMP(0);

    // A. stable rank of every key inside (wave, bin): a wave owns a run of consecutive keys, 64 per round.  Every key and
    // value of the thread is loaded first (independent loads, all in flight together): a load left inside the ranking
    // rounds would wait out its latency once per round.
    u64 key[SORT_ITEMS];
    int val[SORT_ITEMS];
    unsigned rank[SORT_ITEMS];
    unsigned* my_cnt = sh.s_cnt[wave];
    const u64 lt = (1ull << lane) - 1ull;
#pragma unroll
    for (int j = 0; j < SORT_ITEMS; ++j) {
        const long long i = base + wave * (SORT_ITEMS * 64) + j * 64 + lane;
        key[j] = i < n ? kin[i] : ~0ull;
        val[j] = i < n ? vin[i] : 0;
    }
#pragma unroll
    for (int j = 0; j < SORT_ITEMS; ++j) {
        const long long i = base + wave * (SORT_ITEMS * 64) + j * 64 + lane;
        const bool ok = i < n;
        const unsigned d = (unsigned)(key[j] >> shift) & dmask;
        u64 peers = __ballot(ok);
#pragma unroll
        for (int b = 0; b < DBITS; ++b) {
            const u64 m = __ballot((d >> b) & 1u);
            peers &= ((d >> b) & 1u) ? m : ~m;
        }
        unsigned old = 0;
        const int leader = ok ? __ffsll((long long)peers) - 1 : lane;
        if (ok && lane == leader) old = atomicAdd(&my_cnt[d], (unsigned)__popcll(peers));     // own row of s_cnt: wave-private
        old = (unsigned)__shfl((int)old, leader, 64);
        rank[j] = old + (unsigned)__popcll(peers & lt);
    }
    SORT_STAMP(1);
    __syncthreads();
    SORT_STAMP(2);

    // B. per bin: wave bases, the workgroup's count, the chained scan over the workgroups, the bin's global and local start
    const int b0 = tid * BPT;                        // BPT consecutive bins per thread (threads past the last bin idle: BPT >= 1)
    unsigned tot[BPT], gh[BPT], gsum = 0, lsum = 0;
#pragma unroll
    for (int q = 0; q < BPT; ++q) {
        unsigned run = 0;
#pragma unroll
        for (int w = 0; w < TPB / 64; ++w) {
            const unsigned c = sh.s_cnt[w][b0 + q];
            sh.s_cnt[w][b0 + q] = run;
            run += c;
        }
        tot[q] = run;
        gh[q] = ghist[pass * RADIX + b0 + q];
        gsum += gh[q];
        lsum += run;
    }
    // publish this workgroup's counts (or, for the first one, its prefixes); BPT == 1: lanes 2i, 2i+1 share a word
    u64* mine = state + (size_t)blk * (RADIX / 2);
    auto publish = [&](const unsigned* v, u64 flag) {
        if constexpr (BPT == 1) {
            const unsigned other = (unsigned)__shfl_xor((int)v[0], 1, 64);
            if (!(tid & 1)) st_state(mine + tid / 2, (flag << 30 | v[0]) | ((flag << 30 | other) << 32));
        } else {
#pragma unroll
            for (int q = 0; q < BPT; q += 2) st_state(mine + (b0 + q) / 2, (flag << 30 | v[q]) | ((flag << 30 | v[q + 1]) << 32));
        }
    };
    publish(tot, blk == 0 ? 2ull : 1ull);
    SORT_STAMP(3);
    // exclusive prefix over the workgroups in front of this one, in batches of LB predecessors: their words are loaded
    // together (32 independent loads, one round trip: the workgroups of a small sort all start at once, so a walk that
    // waited for one predecessor at a time would be as long as the grid), then consumed nearest first until a prefix flag
    // ends the bin's walk
    unsigned excl[BPT];
#pragma unroll
    for (int q = 0; q < BPT; ++q) excl[q] = 0;
    unsigned open = blk > 0 ? (1u << BPT) - 1u : 0u;                 // bins still looking back
    unsigned spins = 0;
    int p = blk - 1;
    while (p >= 0 && open) {
        u64 wq[LB][W];
#pragma unroll
        for (int d = 0; d < LB; ++d) {
            const int pp = p - d;
#pragma unroll
            for (int q2 = 0; q2 < W; ++q2) {
                wq[d][q2] = 0ull;
                ld_state_issue(wq[d][q2], state + (size_t)(pp >= 0 ? pp : 0) * (RADIX / 2) + b0 / 2 + q2);   // block 0 stands in for pp < 0
            }
        }
        ld_state_wait();
        int used = 0;                                                // predecessors of this batch consumed
#pragma unroll
        for (int d = 0; d < LB; ++d) {
#pragma unroll
            for (int q2 = 0; q2 < W; ++q2) asm volatile("" : "+v"(wq[d][q2]));
            if (p - d < 0 || !open || used != d) continue;
            unsigned v[BPT];
            if constexpr (BPT == 1) v[0] = (unsigned)(wq[d][0] >> ((tid & 1) * 32));
            else {
#pragma unroll
                for (int q = 0; q < BPT; q += 2) { v[q] = (unsigned)wq[d][q / 2]; v[q + 1] = (unsigned)(wq[d][q / 2] >> 32); }
            }
            bool ready = true;
#pragma unroll
            for (int q = 0; q < BPT; ++q)
                if ((open >> q) & 1u) ready &= ((v[q] >> 30) != 0u);
            if (!ready) continue;
#pragma unroll
            for (int q = 0; q < BPT; ++q) {
                if (!((open >> q) & 1u)) continue;
                excl[q] += v[q] & 0x3fffffffu;
                if ((v[q] >> 30) == 2u) open &= ~(1u << q);
            }
            used = d + 1;
        }
        p -= used;
        if (used == 0) {
            if (++spins > SPIN_LIMIT) { atomicOr(status, SORT_SPIN); break; }
            __builtin_amdgcn_s_sleep(1);
        }
    }
    SORT_STAMP(4);
    if (blk > 0) {
        unsigned incl[BPT];
#pragma unroll
        for (int q = 0; q < BPT; ++q) incl[q] = excl[q] + tot[q];
        publish(incl, 2ull);
    }
    // bucket starts (exclusive scan of the global histogram over the bins) and the bins' starts inside this workgroup
    const unsigned g_incl = (unsigned)wave_incl_scan_i((int)gsum), l_incl = (unsigned)wave_incl_scan_i((int)lsum);
    if (lane == 63) { s_wtot[0][wave] = g_incl; s_wtot[1][wave] = l_incl; }
    __syncthreads();
    unsigned gstart = g_incl - gsum, lstart = l_incl - lsum;
    for (int w = 0; w < wave; ++w) { gstart += s_wtot[0][w]; lstart += s_wtot[1][w]; }
#pragma unroll
    for (int q = 0; q < BPT; ++q) {
        sh.s_base[b0 + q] = gstart + excl[q];
        sh.s_local[b0 + q] = lstart;
        gstart += gh[q];
        lstart += tot[q];
    }
    __syncthreads();
    SORT_STAMP(5);

    // C. the workgroup's keys in sorted order through LDS, then out: consecutive threads write consecutive addresses of a bin
#pragma unroll
    for (int j = 0; j < SORT_ITEMS; ++j) {
        const long long i = base + wave * (SORT_ITEMS * 64) + j * 64 + lane;
        if (i < n) {
            const unsigned d = (unsigned)(key[j] >> shift) & dmask;
            const unsigned lp = sh.s_local[d] + sh.s_cnt[wave][d] + rank[j];
            sh.s_key[lp] = key[j];
            sh.s_val[lp] = val[j];
        }
    }
    __syncthreads();
    SORT_STAMP(6);
    const int here = (int)min((long long)SORT_TILE, (long long)n - base);
    for (int e = tid; e < here; e += TPB) {
        const u64 k = sh.s_key[e];
        const unsigned d = (unsigned)(k >> shift) & dmask;
        const unsigned pos = sh.s_base[d] + ((unsigned)e - sh.s_local[d]);
        kout[pos] = k;
        vout[pos] = sh.s_val[e];
    }
    SORT_STAMP(7);
}

// The pyramid's digit pass: the digits follow from the box in its plan; a pass the box does not need, or a box too wide
// for MAX_PASSES digits (k_unique_keys has flagged it), ends here
__global__ __launch_bounds__(TPB) void k_sort_pass(const u64* __restrict__ kin, u64* __restrict__ kout,
                                                  const int* __restrict__ vin, int* __restrict__ vout, int pass,
                                                  u64* __restrict__ state, const int* n_dev, int n_max, int* __restrict__ plan,
                                                  int* __restrict__ status, const unsigned* __restrict__ ghist) {
    __shared__ unsigned s_wtot[2][TPB / 64];
    const SortShared sh = sort_shared();
    int* words = plan + PL_SORT;                      // the sort's words inside the plan
    const KeyPlan kp = key_plan(plan);
    if (kp.nbits > MAX_PASSES * RADIX_BITS) return;
    const SortPlan sp = sort_plan(kp.nbits);
    if (pass >= sp.passes) return;                    // this digit does not exist
    const int n = real_n(n_dev, n_max);
    int blk;
    if (!sort_begin(sh, &words[SW_TICKET0 + pass], n, blk)) return;
    switch (sp.dbits) {
        case 8: sort_pass_body<1>(kin, kout, vin, vout, n, pass, words, status, ghist, state, sh, blk, s_wtot); break;
        case 9: sort_pass_body<2>(kin, kout, vin, vout, n, pass, words, status, ghist, state, sh, blk, s_wtot); break;
        case 10: sort_pass_body<4>(kin, kout, vin, vout, n, pass, words, status, ghist, state, sh, blk, s_wtot); break;
        default: sort_pass_body<8>(kin, kout, vin, vout, n, pass, words, status, ghist, state, sh, blk, s_wtot); break;
    }
}

// The same digit pass for a caller's 32-bit keys (radix_sort_u32 below): RADIX_U32_PASSES digits of RADIX_BITS bits
__global__ __launch_bounds__(TPB) void k_sort_pass_u32(const u64* __restrict__ kin, u64* __restrict__ kout,
                                                      const int* __restrict__ vin, int* __restrict__ vout, int pass,
                                                      u64* __restrict__ state, int n, int* __restrict__ words,
                                                      int* __restrict__ status, const unsigned* __restrict__ ghist) {
    __shared__ unsigned s_wtot[2][TPB / 64];
    const SortShared sh = sort_shared();
    int blk;
    if (!sort_begin(sh, &words[SW_TICKET0 + pass], n, blk)) return;
    sort_pass_body<8>(kin, kout, vin, vout, n, pass, words, status, ghist, state, sh, blk, s_wtot);
}

size_t sort_blocks(int n) { return (size_t)cdiv(n > 0 ? n : 1, SORT_TILE); }

// `passes` launches of one of the two kernels: pass p reads buffer p & 1 and takes its own slice of the scan state; `rest`
// are the kernel's arguments behind the state
template <auto Kernel, typename... Rest>
int sort_launch(int passes, int n, u64* keys_a, u64* keys_b, int* vals_a, int* vals_b, u64* state, hipStream_t st, Rest... rest) {
    static const bool lds_attr = (hipFuncSetAttribute((const void*)Kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                                      (int)SORT_LDS_BYTES) == hipSuccess);
    if (!lds_attr) return PBN_ERR_HIP;
    const size_t blocks = sort_blocks(n);
    for (int p = 0; p < passes; ++p)
        hipLaunchKernelGGL(Kernel, dim3((unsigned)blocks), dim3(TPB), SORT_LDS_BYTES, st, (p & 1) ? keys_b : keys_a,
                           (p & 1) ? keys_a : keys_b, (p & 1) ? vals_b : vals_a, (p & 1) ? vals_a : vals_b, p,
                           state + (size_t)p * blocks * (RADIX / 2), rest...);
    return PBN_OK;
}

}  // namespace

size_t sort_state_bytes(int n, int passes) { return (size_t)passes * sort_blocks(n) * (RADIX / 2) * sizeof(u64); }

int radix_sort_planned(unsigned long long* keys_a, unsigned long long* keys_b, int32_t* vals_a, int32_t* vals_b,
                       const int32_t* n_dev, int n_max, int32_t* plan, int32_t* status, const unsigned* ghist,
                       unsigned long long* state, hipStream_t st) {
    return sort_launch<k_sort_pass>(MAX_PASSES, n_max, keys_a, keys_b, vals_a, vals_b, state, st, n_dev, n_max, plan, status, ghist);
}

int radix_sort_u32_tile() { return SORT_TILE; }

// scratch: the sort's words, then the scan state
size_t radix_sort_u32_scratch_bytes(int n) {
    return align_up(SW_WORDS * sizeof(int), 256) + align_up(sort_state_bytes(n, RADIX_U32_PASSES), 256);
}

int radix_sort_u32(unsigned long long* keys_a, unsigned long long* keys_b, int32_t* vals_a, int32_t* vals_b, int n,
                   const unsigned* ghist, int32_t* status, void* scratch, size_t scratch_bytes, hipStream_t st) {
    if (n <= 0) return PBN_OK;
    if (scratch_bytes < radix_sort_u32_scratch_bytes(n)) return PBN_ERR_WORKSPACE;
    const int frc = fill_bytes(scratch, 0, radix_sort_u32_scratch_bytes(n), st);
    if (frc != PBN_OK) return frc;
    u64* state = (u64*)((char*)scratch + align_up(SW_WORDS * sizeof(int), 256));
    const int rc = sort_launch<k_sort_pass_u32>(RADIX_U32_PASSES, n, keys_a, keys_b, vals_a, vals_b, state, st, n, (int*)scratch,
                                                status, ghist);
    PBN_LAUNCH_CHECK();
    return rc;
}

}  // namespace pbn
