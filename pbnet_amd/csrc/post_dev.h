// post_dev.h -- what the two device-resident forms of the post-processing share (post.hip: one scene with the TTA fold,
// post_batch.hip: the scenes of a merged forward).
#pragma once
#include "pbn_common.h"

namespace pbn {

constexpr int POST_TPB = 256;
constexpr int POST_MAX_PROPOSALS = 4096;        // the NMS keeps score, order and suppress flags of every survivor in LDS
constexpr int POST_STATUS_SUPERPOINT = 1;       // a superpoint id >= the capacity
constexpr int POST_STATUS_CLASS = 2;            // a proposal without a first member, or a class outside the label table

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

}  // namespace pbn
