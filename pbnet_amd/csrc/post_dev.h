// post_dev.h -- the device steps that the forms of the post-processing share (post.hip: one scene with the TTA fold,
// post_batch.hip: the scenes of a merged forward) and that summary.hip and the AP association (assoc_dev.h) use as well.  Each
// step is stated here once and inlined into its callers; the host-stepped kernels at the top of post.hip stay apart on purpose,
// as the independent yardstick of the device-resident forms.
#pragma once
#include "pbn_common.h"

namespace pbn {

constexpr int POST_TPB = 256;
constexpr int POST_MAX_PROPOSALS = 4096;        // the NMS keeps score, order and suppress flags of every survivor in LDS
constexpr int POST_STATUS_SUPERPOINT = 1;       // a superpoint id >= the capacity
constexpr int POST_STATUS_CLASS = 2;            // a proposal without a first member, or a class outside the label table
constexpr int POST_STRIDE_BLOCKS = 2048;        // cap of every striding grid

// blocks of a striding grid over n items: at least one, at most POST_STRIDE_BLOCKS
inline int stride_blocks(long long n) {
    const long long b = (n + POST_TPB - 1) / POST_TPB;
    return (int)(b < 1 ? 1 : (b > POST_STRIDE_BLOCKS ? POST_STRIDE_BLOCKS : b));
}

// exclusive position of `flag` among the 256 threads of the block, in thread order; *total = flags set.  s_wave: 4 ints.
__device__ __forceinline__ int block_flag_scan(bool flag, int* s_wave, int* total) {
    const unsigned long long b = __ballot(flag);
    const int lane = lane_id(), wave = (int)(threadIdx.x >> 6);
    __syncthreads();                               // the previous round's readers are done with s_wave
    if (lane == 0) s_wave[wave] = __popcll(b);
    __syncthreads();
    int before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < POST_TPB / 64; ++w) {
        before += w < wave ? s_wave[w] : 0;
        all += s_wave[w];
    }
    *total = all;
    return before + __popcll(b & ((1ull << lane) - 1ull));
}

// one add per distinct bin of a wave: lanes that hit the same bin are merged first (the leader adds the lane count) -- points
// that lie next to each other mostly share a bin.  Every lane of the wave must call this; bin < 0 takes no part.
__device__ __forceinline__ void wave_merged_add(int* bins, int bin) {
    unsigned long long todo = __ballot(bin >= 0);
    while (todo) {
        const int leader = __ffsll((long long)todo) - 1;
        const int lb = __shfl(bin, leader);
        const unsigned long long same = __ballot(bin == lb) & todo;
        if (lane_id() == leader) atomicAdd(&bins[lb], __popcll(same));
        todo &= ~same;
    }
}

// ---- a column of a by-value scene table (point_start or sp_start of pbn_scene_table / pbn_tta_table) --------------------------
// entry j, j uniform: selects over constant indices, so the by-value table stays in scalar registers
__device__ __forceinline__ int start_of(const int32_t (&start)[PBN_MAX_SCENES + 1], int j) {
    int v = start[0];
#pragma unroll
    for (int k = 1; k <= PBN_MAX_SCENES; ++k) v = k == j ? start[k] : v;
    return v;
}

// the scene whose range holds `at` (0 <= at < start[n_scenes]): the last j with start[j] <= at, so an empty scene is stepped over
__device__ __forceinline__ int scene_of_folded(const int32_t (&start)[PBN_MAX_SCENES + 1], int n_scenes, int at) {
    int s = 0;
#pragma unroll
    for (int j = 1; j < PBN_MAX_SCENES; ++j) s = (j < n_scenes && at >= start[j]) ? j : s;
    return s;
}

// ---- mask IoU of two bitset rows: |a & b| by one wave (every lane gets the count), then the fp32 quotient of
// eval_map.py:90-96 on exact integers
__device__ __forceinline__ int mask_pair_intersection(const unsigned* __restrict__ a, const unsigned* __restrict__ b, int words) {
    int c = 0;
    for (int w = threadIdx.x; w < words; w += 64) c += __popc(a[w] & b[w]);
    return wave_reduce_add(c);
}

__device__ __forceinline__ float mask_pair_iou(int intersection, int count_a, int count_b) {
    const float inter = (float)intersection;
    return inter / (((float)count_a + (float)count_b) - inter);
}

// ---- the greedy NMS of tools/mIOU.py:77-87 by one workgroup over the n survivors my_rows[0, n) ---------------------------------
// Order: score descending, among equal scores the LOWER survivor position first; rank[i] = #{j : s[j] > s[i] or (s[j] == s[i]
// and j < i)} is a permutation (scores that passed `> score_t` are not NaN), exact and stable, so the walk is the same on every
// run.  A survivor is picked when no earlier pick has iou[pick][it] > nms_t (fp32 `>`: an IoU equal to the threshold does not
// suppress); after a pick every lane marks what that pick suppresses.  iou: row 0 of the survivors' table, row stride cap.
// Writes pick_rows[0, cap) = the picked proposals in pick order and, if asked for, pick = their survivor positions; tails -1.
// Returns the number of picks.  The caller declares the three LDS arrays, POST_MAX_PROPOSALS entries each.
__device__ __forceinline__ int nms_walk(float* s_score, unsigned short* s_order, unsigned char* s_supp,
                                        const float* __restrict__ score, const int* __restrict__ my_rows, int n, int cap,
                                        const float* __restrict__ iou, float nms_t, int* __restrict__ pick,
                                        int* __restrict__ pick_rows) {
    for (int i = threadIdx.x; i < n; i += POST_TPB) {
        const int r = my_rows[i];
        s_score[i] = (r >= 0 && r < cap) ? score[r] : -INFINITY;
        s_order[i] = (unsigned short)i;            // every slot names a survivor even if the ranks were no permutation (NaN)
        s_supp[i] = 0;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < n; i += POST_TPB) {
        const float si = s_score[i];
        int rank = 0;
        for (int j = 0; j < n; ++j) {              // every lane reads the same word: an LDS broadcast
            const float sj = s_score[j];
            rank += (sj > si || (sj == si && j < i)) ? 1 : 0;
        }
        s_order[rank] = (unsigned short)i;
    }
    __syncthreads();
    int n_pick = 0;
    for (int k = 0; k < n; ++k) {
        const int it = s_order[k];
        if (s_supp[it]) continue;                  // uniform: every thread reads the same flag
        if (threadIdx.x == 0) {
            if (pick) pick[n_pick] = it;
            pick_rows[n_pick] = my_rows[it];
        }
        ++n_pick;
        // `it` itself is left alone: a thread that has not read its flag yet must still see it clear
        const float* row = iou + (size_t)it * cap;
        for (int j = threadIdx.x; j < n; j += POST_TPB)
            if (j != it && row[j] > nms_t) s_supp[j] = 1;
        __syncthreads();
    }
    for (int k = n_pick + threadIdx.x; k < cap; k += POST_TPB) {
        if (pick) pick[k] = -1;
        pick_rows[k] = -1;
    }
    return n_pick;
}

// the class of proposal p: that of its first member (eval_map.py:63-65) through the label table; -1 without a first member or
// with a member or a class out of range
__device__ __forceinline__ long long first_member_class(const long long* __restrict__ proposals_idx, int n_entries,
                                                        const void* __restrict__ offsets, int offsets_i64, int p,
                                                        const void* __restrict__ pred_sem, int sem_i64, long long n_sem,
                                                        const long long* __restrict__ label_table, int n_labels) {
    const long long e = load_index(offsets, offsets_i64, p);
    if (e < 0 || e >= n_entries) return -1;
    const long long pt = proposals_idx[2 * e + 1];
    if (pt < 0 || pt >= n_sem) return -1;
    const long long s = load_index(pred_sem, sem_i64, pt);
    return (s >= 0 && s < n_labels) ? label_table[s] : -1;
}

}  // namespace pbn
