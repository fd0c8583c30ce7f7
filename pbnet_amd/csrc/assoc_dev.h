// assoc_dev.h -- the device steps that the two forms of the AP association share (apassoc.hip: one validation scene,
// apassoc_batch.hip: the scenes of a merged forward): the ground-truth code, the numbering scan, and the epoch log's state machine
// and record layout.  Each step is stated here once and inlined into its callers, so both forms write the same log bytes.
#pragma once
#include "post_dev.h"

namespace pbn {

constexpr int GT_ID_CAP_MAX = 1 << 20;              // direct table of the ground-truth numbering
constexpr int SCAN_IDS = 4;                         // ids per thread and trip of gt_number_scan
constexpr int AP_HDR = PBN_AP_RECORD_HEADER;
// state block of the log: used | wanted | n_records | overflow | offset of the record being written (-1 = none) | 3 spare
constexpr int ST_USED = 0, ST_WANTED = 1, ST_RECORDS = 2, ST_OVERFLOW = 3, ST_OFFSET = 4;

struct GtCode { int code, status; };

// get_val_gt.py:26-37: the id is a thousand times the class table[sem], plus inst + 1, where sem is the semantic label of the instance's first point
// (-100 = class 0).  A label outside the table gives code 0 and the status bit to OR.
__device__ __forceinline__ GtCode gt_code(long long sem, long long inst, const int* __restrict__ label_table, int n_labels) {
    if (sem == -100) sem = 0;
    if (sem < 0 || sem >= n_labels) return GtCode{0, PBN_AP_STATUS_SEMANTIC_RANGE};
    return GtCode{label_table[sem] * 1000 + (int)inst + 1, 0};
}

// One workgroup walks the direct table in ascending id order: the ids with a count get consecutive slots (uid, gt_vert) and
// table[id] becomes the id's slot.  An id past u_cap slots gets -1 (its points take no part) and sets *over in its thread.
// Returns the live count, at most u_cap.  s_wave: POST_TPB / 64 ints of LDS.
__device__ __forceinline__ int gt_number_scan(int* __restrict__ table, int id_cap, int* __restrict__ uid,
                                              int* __restrict__ gt_vert, int u_cap, int* s_wave, bool* over) {
    const int lane = lane_id(), wave = (int)(threadIdx.x >> 6);
    int base = 0;
    for (int t0 = 0; t0 < id_cap; t0 += POST_TPB * SCAN_IDS) {                     // uniform trip count
        const int id0 = t0 + (int)threadIdx.x * SCAN_IDS;
        int c[SCAN_IDS], mine = 0;
#pragma unroll
        for (int k = 0; k < SCAN_IDS; ++k) {
            c[k] = id0 + k < id_cap ? table[id0 + k] : 0;
            mine += c[k] > 0 ? 1 : 0;
        }
        int incl = mine;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int v = __shfl_up(incl, o, 64);
            if (lane >= o) incl += v;
        }
        __syncthreads();                                   // the previous trip's readers are done with s_wave
        if (lane == 63) s_wave[wave] = incl;
        __syncthreads();
        int before = 0, all = 0;
#pragma unroll
        for (int w = 0; w < POST_TPB / 64; ++w) {
            before += w < wave ? s_wave[w] : 0;
            all += s_wave[w];
        }
        int pos = base + before + incl - mine;
#pragma unroll
        for (int k = 0; k < SCAN_IDS; ++k) {
            if (c[k] <= 0) continue;
            if (pos < u_cap) {
                uid[pos] = id0 + k;
                gt_vert[pos] = c[k];
                table[id0 + k] = pos;
            } else {
                table[id0 + k] = -1;
                *over = true;
            }
            ++pos;
        }
        base += all;
    }
    return base < u_cap ? base : u_cap;
}

// words of a record with nk predictions and ng ground-truth instances: header | uid | gt_vert | label_id | conf | inter[nk, ng]
__device__ __forceinline__ long long ap_record_words(int nk, int ng) {
    return nk == 0 ? AP_HDR : (long long)AP_HDR + 2LL * ng + 2LL * nk + (long long)nk * ng;
}

// The log's state machine, by ONE thread: counts the record's words as wanted, and if the log has not overflowed and the record
// fits, writes its header and returns its offset; else -1.
__device__ __forceinline__ int ap_record_reserve(int* __restrict__ state, int* __restrict__ log, int log_words, int tag, int nk,
                                                 int ng, int n_pts, int status) {
    const long long words = ap_record_words(nk, ng);
    const long long wanted = (long long)state[ST_WANTED] + words;
    state[ST_WANTED] = wanted > 0x7fffffffLL ? 0x7fffffff : (int)wanted;
    const int used = state[ST_USED];
    if (state[ST_OVERFLOW] || used < 0 || (long long)used + words > (long long)log_words) {
        state[ST_OVERFLOW] = 1;                             // sticky: nothing is written after the first record that did not fit
        state[ST_OFFSET] = -1;
        return -1;
    }
    int* rec = log + used;
    rec[0] = PBN_AP_RECORD_MAGIC;
    rec[1] = tag;
    rec[2] = nk;
    rec[3] = ng;
    rec[4] = n_pts;
    rec[5] = status;
    rec[6] = (int)words;
    rec[7] = 0;
    state[ST_USED] = used + (int)words;
    state[ST_RECORDS] += 1;
    state[ST_OFFSET] = used;
    return used;
}

// word e of a record's body before the overlap table (0 <= e < 2 ng + 2 nk): uid | gt_vert | label_id | conf bits.  A label
// that does not fit 32 bits sets LABEL_RANGE in the record's status word.
__device__ __forceinline__ int ap_record_head_word(long long e, int nk, int ng, int* rec,
                                                   const int* __restrict__ uid, const int* __restrict__ gt_vert,
                                                   const long long* __restrict__ semantic_id, const float* __restrict__ conf) {
    const long long a = ng, b = 2LL * ng, c = b + nk;
    if (e < a) return uid[e];
    if (e < b) return gt_vert[e - a];
    if (e >= c) return __float_as_int(conf[e - c]);
    const long long s = semantic_id[e - b];
    const int v = (int)s;
    if (s != (long long)v) atomicOr(&rec[5], PBN_AP_STATUS_LABEL_RANGE);
    return v;
}

}  // namespace pbn
