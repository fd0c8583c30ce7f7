// pairs.hip -- rulebook pairs, offset-major (training: the operands of the weight gradient, wgrad.hip).
// Pair lists of an output-stationary map nbr[n, K]: for every offset k the (input row, output row) pairs with
// nbr[o, k] >= 0, output rows ascending, cut into segments of `seg` pairs.  Three steps: per-block column counts,
// a column-wise exclusive scan over the blocks (+ column totals), the fill.  Positions are prefix counts, never atomics:
// the lists -- and with them the summation order of the weight gradient -- are the same on every run.
// Every step is stated once as a *_body; a single map passes its arguments to the kernels, several maps pass a job table.
#include <algorithm>
#include <initializer_list>
#include "pbn_common.h"

namespace pbn {
namespace {

constexpr int TPB = 256;
constexpr int PAIR_ROWS = 256;   // rows per block = TPB
constexpr int PAIR_KC = 32;      // offsets per LDS tile
constexpr int PAIR_PITCH = PAIR_KC + 1;
constexpr int PAIR_MAX_K = 512;  // offsets of a map the fill can take: s_seg

// A block owns 256 rows.  The [256 x 32-offset] piece of the table is read ONCE, along the rows (coalesced), into LDS
// (pitch 33: the column reads below are conflict-free); every wave then owns the columns w, w + 4, ... of the piece and walks
// its 256 rows as four ballots -- no barrier per offset (round 2 read the table column by column with two barriers each).
__device__ __forceinline__ void pair_tile_load(const int* __restrict__ nbr, int n, int K, int row0, int k0, int kc, int* s_tile) {
    for (int e = threadIdx.x; e < PAIR_ROWS * kc; e += TPB) {
        const int r = e / kc, cc = e - r * kc;
        s_tile[r * PAIR_PITCH + cc] = row0 + r < n ? nbr[(size_t)(row0 + r) * K + k0 + cc] : -1;
    }
}

// step 1: table[blk][k] <- pairs of column k in the rows of block blk
__device__ __forceinline__ void pair_count_body(const int* __restrict__ nbr, int n, int K, int* __restrict__ table, int blk, int* s_tile) {
    const int row0 = blk * PAIR_ROWS;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int k0 = 0; k0 < K; k0 += PAIR_KC) {
        const int kc = min(PAIR_KC, K - k0);
        pair_tile_load(nbr, n, K, row0, k0, kc, s_tile);
        __syncthreads();
        for (int cc = wave; cc < kc; cc += TPB / 64) {
            int cnt = 0;
#pragma unroll
            for (int sub = 0; sub < PAIR_ROWS / 64; ++sub) cnt += __popcll(__ballot(s_tile[(sub * 64 + lane) * PAIR_PITCH + cc] >= 0));
            if (lane == 0) table[(size_t)blk * K + k0 + cc] = cnt;
        }
        __syncthreads();
    }
}

// step 2, one wave per column k: table[b][k] <- pairs of column k in blocks before b; totals[k] <- column total
__device__ __forceinline__ void pair_scan_body(int k, int K, int n_blocks, int* __restrict__ table, int* __restrict__ totals) {
    const int lane = threadIdx.x;
    int run = 0;
    for (int b0 = 0; b0 < n_blocks; b0 += 64) {
        const int b = b0 + lane;
        const int v = b < n_blocks ? table[(size_t)b * K + k] : 0;
        int inc = v;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int t = __shfl_up(inc, o);
            if (lane >= o) inc += t;
        }
        if (b < n_blocks) table[(size_t)b * K + k] = run + inc - v;
        run += __shfl(inc, 63);
    }
    if (lane == 0) totals[k] = run;
}

// step 3.  seg_start NULL (device lists): every block derives the first segment of every offset from the totals itself (one
// wave, K <= a few hundred) and block 0 publishes them as seg_begin_out[K + 1] -- no separate launch, no read-back
__device__ __forceinline__ void pair_fill_body(const int* __restrict__ nbr, int n, int K, const int* __restrict__ table,
                                               const int* __restrict__ seg_start, const int* __restrict__ totals,
                                               int* __restrict__ seg_begin_out, int seg, int* __restrict__ in_idx,
                                               int* __restrict__ out_idx, long long* __restrict__ seg_offset, int blk,
                                               int* s_tile, int* s_seg) {
    const int row0 = blk * PAIR_ROWS;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (seg_start) {
        for (int k = threadIdx.x; k < K; k += TPB) s_seg[k] = seg_start[k];
    } else if (wave == 0) {
        int run = 0;
        for (int k0 = 0; k0 < K; k0 += 64) {
            const int k = k0 + lane;
            const int v = k < K ? (totals[k] + seg - 1) / seg : 0;
            int inc = v;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const int t = __shfl_up(inc, o);
                if (lane >= o) inc += t;
            }
            if (k < K) { s_seg[k] = run + inc - v; if (blk == 0) seg_begin_out[k] = run + inc - v; }
            run += __shfl(inc, 63);
        }
        if (lane == 0 && blk == 0) seg_begin_out[K] = run;
    }
    __syncthreads();
    for (int k0 = 0; k0 < K; k0 += PAIR_KC) {
        const int kc = min(PAIR_KC, K - k0);
        pair_tile_load(nbr, n, K, row0, k0, kc, s_tile);
        __syncthreads();
        for (int cc = wave; cc < kc; cc += TPB / 64) {
            const int k = k0 + cc;
            int pos0 = table[(size_t)blk * K + k];
            const int first = s_seg[k];
#pragma unroll
            for (int sub = 0; sub < PAIR_ROWS / 64; ++sub) {
                const int src = s_tile[(sub * 64 + lane) * PAIR_PITCH + cc];
                const unsigned long long m = __ballot(src >= 0);
                if (src >= 0) {
                    const int pos = pos0 + __popcll(m & ((1ULL << lane) - 1ULL));
                    const int q = pos / seg;
                    const long long slot = (long long)(first + q) * seg + (pos - q * seg);
                    in_idx[slot] = src;
                    out_idx[slot] = row0 + sub * 64 + lane;
                    if (pos == q * seg) seg_offset[first + q] = k;
                }
                pos0 += __popcll(m);
            }
        }
        __syncthreads();
    }
}

// ---- one map: the arguments are the kernel's -----------------------------------------------------------------------
__global__ __launch_bounds__(TPB) void k_pair_count(const int* __restrict__ nbr, int n, int K, int* __restrict__ table) {
    __shared__ int s_tile[PAIR_ROWS * PAIR_PITCH];
    pair_count_body(nbr, n, K, table, blockIdx.x, s_tile);
}
__global__ __launch_bounds__(64) void k_pair_scan(int* __restrict__ table, int n_blocks, int K, int* __restrict__ totals) {
    pair_scan_body(blockIdx.x, K, n_blocks, table, totals);
}
__global__ __launch_bounds__(TPB) void k_pair_fill(const int* __restrict__ nbr, int n, int K, const int* __restrict__ table,
                                                  const int* __restrict__ seg_start, const int* __restrict__ totals,
                                                  int* __restrict__ seg_begin_out, int seg, int* __restrict__ in_idx,
                                                  int* __restrict__ out_idx, long long* __restrict__ seg_offset) {
    __shared__ int s_tile[PAIR_ROWS * PAIR_PITCH];
    __shared__ int s_seg[PAIR_MAX_K];
    pair_fill_body(nbr, n, K, table, seg_start, totals, seg_begin_out, seg, in_idx, out_idx, seg_offset, blockIdx.x, s_tile, s_seg);
}

// ---- all maps of a pyramid in three launches (the training executor builds 14 lists per lineage; most maps are small and
// a launch costs more than their work): a job table by value, blocks -> jobs through the prefix of their block counts -------
constexpr int PAIR_MAX_JOBS = 16;
struct PairJobs {
    const int* nbr[PAIR_MAX_JOBS]; int* table[PAIR_MAX_JOBS]; int* totals[PAIR_MAX_JOBS]; int* seg_begin[PAIR_MAX_JOBS];
    int* in_idx[PAIR_MAX_JOBS]; int* out_idx[PAIR_MAX_JOBS]; long long* seg_offset[PAIR_MAX_JOBS];
    int n[PAIR_MAX_JOBS], K[PAIR_MAX_JOBS];
    int block_begin[PAIR_MAX_JOBS + 1];      // row blocks (count / fill)
    int col_begin[PAIR_MAX_JOBS + 1];        // columns (scan)
    int n_jobs, seg;
};
__device__ __forceinline__ int pair_job_of(const int* begin, int n_jobs, int b) {
    int j = 0;
    while (j + 1 < n_jobs && b >= begin[j + 1]) ++j;
    return j;
}

__global__ __launch_bounds__(TPB) void k_pair_count_multi(const PairJobs J) {
    __shared__ int s_tile[PAIR_ROWS * PAIR_PITCH];
    const int j = pair_job_of(J.block_begin, J.n_jobs, blockIdx.x);
    pair_count_body(J.nbr[j], J.n[j], J.K[j], J.table[j], blockIdx.x - J.block_begin[j], s_tile);
}
__global__ __launch_bounds__(64) void k_pair_scan_multi(const PairJobs J) {
    const int j = pair_job_of(J.col_begin, J.n_jobs, blockIdx.x);
    pair_scan_body(blockIdx.x - J.col_begin[j], J.K[j], J.block_begin[j + 1] - J.block_begin[j], J.table[j], J.totals[j]);
}
__global__ __launch_bounds__(TPB) void k_pair_fill_multi(const PairJobs J) {
    __shared__ int s_tile[PAIR_ROWS * PAIR_PITCH];
    __shared__ int s_seg[PAIR_MAX_K];
    const int j = pair_job_of(J.block_begin, J.n_jobs, blockIdx.x);
    pair_fill_body(J.nbr[j], J.n[j], J.K[j], J.table[j], nullptr, J.totals[j], J.seg_begin[j], J.seg, J.in_idx[j], J.out_idx[j],
                   J.seg_offset[j], blockIdx.x - J.block_begin[j], s_tile, s_seg);
}

// one map's arguments: its sizes, then every buffer of `bufs` exists; `fill`: the fill keeps a word per offset in LDS
int pair_map_check(int n, int K, int seg, bool fill, std::initializer_list<const void*> bufs) {
    if (n < 0 || K < 1 || seg < 1) return PBN_ERR_ARG;
    for (const void* p : bufs)
        if (!p) return PBN_ERR_ARG;
    return fill && K > PAIR_MAX_K ? PBN_ERR_UNSUPPORTED : PBN_OK;
}

}  // namespace
}  // namespace pbn

using namespace pbn;

// row blocks of a map; where the device sizes the lists an empty map keeps one (empty) block, which publishes seg_begin
extern "C" int pbn_rulebook_pair_blocks(int n) { return n > 0 ? cdiv(n, PAIR_ROWS) : 0; }
static int pair_fill_blocks(int n) { return std::max(pbn_rulebook_pair_blocks(n), 1); }

extern "C" int pbn_rulebook_pair_counts(const int32_t* nbr, int n, int n_offsets, int32_t* table, int32_t* totals,
                                        pbn_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    PBN_TRY(pair_map_check(n, n_offsets, 1, false, {totals}));
    if (n == 0) return fill_bytes(totals, 0, sizeof(int32_t) * n_offsets, stream);
    PBN_TRY(pair_map_check(n, n_offsets, 1, false, {nbr, table}));
    const int nb = pbn_rulebook_pair_blocks(n);
    hipLaunchKernelGGL(k_pair_count, dim3(nb), dim3(TPB), 0, stream, nbr, n, n_offsets, table);
    hipLaunchKernelGGL(k_pair_scan, dim3(n_offsets), dim3(64), 0, stream, table, nb, n_offsets, totals);
    PBN_LAUNCH_CHECK();
    return PBN_OK;
}

extern "C" int pbn_rulebook_pair_fill(const int32_t* nbr, int n, int n_offsets, const int32_t* table, const int32_t* seg_start,
                                      int seg, int n_segments, int32_t* in_idx, int32_t* out_idx, int64_t* seg_offset,
                                      pbn_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (n_segments < 0) return PBN_ERR_ARG;
    PBN_TRY(pair_map_check(n, n_offsets, seg, true, {}));
    if (n_segments == 0) return PBN_OK;
    PBN_TRY(pair_map_check(n, n_offsets, seg, true, {in_idx, out_idx, seg_offset}));
    if (n > 0) PBN_TRY(pair_map_check(n, n_offsets, seg, true, {nbr, table, seg_start}));    // every refusal before the first write
    // padding slots (and surplus segments) read as -1 / offset 0
    PBN_TRY(fill_bytes(in_idx, 0xff, sizeof(int32_t) * (size_t)n_segments * seg, stream));
    PBN_TRY(fill_bytes(out_idx, 0xff, sizeof(int32_t) * (size_t)n_segments * seg, stream));
    PBN_TRY(fill_bytes(seg_offset, 0, sizeof(int64_t) * (size_t)n_segments, stream));
    if (n == 0) return PBN_OK;
    hipLaunchKernelGGL(k_pair_fill, dim3(pbn_rulebook_pair_blocks(n)), dim3(TPB), 0, stream, nbr, n, n_offsets, table, seg_start,
                       (const int*)nullptr, (int*)nullptr, seg, in_idx, out_idx, (long long*)seg_offset);
    PBN_LAUNCH_CHECK();
    return PBN_OK;
}

extern "C" int pbn_rulebook_pair_fill_dev(const int32_t* nbr, int n, int n_offsets, const int32_t* table, const int32_t* totals,
                                          int seg, int32_t* seg_begin, int32_t* in_idx, int32_t* out_idx, int64_t* seg_offset,
                                          pbn_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    PBN_TRY(pair_map_check(n, n_offsets, seg, true, {totals, seg_begin, nbr, table, in_idx, out_idx, seg_offset}));
    // The tails of the last segments are NOT padded: the consumer bounds every offset by its pair count (pbn_spconv_wgrad's
    // pair_counts = `totals`)
    hipLaunchKernelGGL(k_pair_fill, dim3(pair_fill_blocks(n)), dim3(TPB), 0, stream, nbr, n, n_offsets, table,
                       (const int*)nullptr, totals, seg_begin, seg, in_idx, out_idx, (long long*)seg_offset);
    PBN_LAUNCH_CHECK();
    return PBN_OK;
}

// pbn_rulebook_pairs_multi: pbn_rulebook_pair_counts + pbn_rulebook_pair_fill_dev of up to 16 maps in three launches
extern "C" int pbn_rulebook_pairs_multi(const pbn_pair_job* jobs, int n_jobs, int segment, pbn_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!jobs || n_jobs < 1 || n_jobs > PAIR_MAX_JOBS || segment < 1) return PBN_ERR_ARG;
    PairJobs J;
    J.n_jobs = n_jobs; J.seg = segment;
    int blocks = 0, cols = 0;
    for (int j = 0; j < n_jobs; ++j) {
        const pbn_pair_job& q = jobs[j];
        PBN_TRY(pair_map_check(q.n, q.n_offsets, segment, true,
                               {q.totals, q.seg_begin, q.nbr, q.table, q.in_idx, q.out_idx, q.seg_offset}));
        J.nbr[j] = q.nbr; J.table[j] = q.table; J.totals[j] = q.totals; J.seg_begin[j] = q.seg_begin;
        J.in_idx[j] = q.in_idx; J.out_idx[j] = q.out_idx; J.seg_offset[j] = (long long*)q.seg_offset;
        J.n[j] = q.n; J.K[j] = q.n_offsets;
        J.block_begin[j] = blocks; J.col_begin[j] = cols;
        blocks += pair_fill_blocks(q.n);
        cols += q.n_offsets;
    }
    for (int j = n_jobs; j <= PAIR_MAX_JOBS; ++j) { J.block_begin[j] = blocks; J.col_begin[j] = cols; }
    hipLaunchKernelGGL(k_pair_count_multi, dim3(blocks), dim3(TPB), 0, stream, J);
    hipLaunchKernelGGL(k_pair_scan_multi, dim3(cols), dim3(64), 0, stream, J);
    hipLaunchKernelGGL(k_pair_fill_multi, dim3(blocks), dim3(TPB), 0, stream, J);
    PBN_LAUNCH_CHECK();
    return PBN_OK;
}
