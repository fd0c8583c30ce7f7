// post.hip -- what follows PBNet.forward at evaluation time (/root/reference/eval_map.py:55-123), on the device:
// TTA fold of the proposal member lists, proposal sizes, pairwise mask IoU, per-point label of the picked clusters,
// superpoint vote (tools/getins.py:72-98) and the rebuilt cluster masks.  The reference builds dense [P, N] int masks
// and a [P, P] product with torch.mm; here a proposal is a BITSET over the N/3 folded points (32 points per word), so
// the IoU matrix is popcounts of ANDs and every step is integer work -- bit-exact by construction.
// In the first form (pbn_mask_iou .. pbn_bitmask_to_dense) the greedy NMS itself (tools/mIOU.py:77-87: a few hundred scalars)
// stays on the host, exactly as the reference runs it; the device-resident form further down (pbn_post_select ..
// pbn_post_compact) runs it in one workgroup and keeps every count in a device scalar.
#include "pbn_common.h"
#include "post_dev.h"

namespace pbn {
namespace {

constexpr int TPB = POST_TPB;

// bit (point % n_fold) of row proposal: eval_map.py:67-70 (the three rotated copies fold onto one index range)
__global__ __launch_bounds__(TPB) void k_set_bits(const long long* __restrict__ proposals_idx, int n_entries, int n_fold,
                                                 int n_prop, int words, unsigned* __restrict__ masks) {
    const int e = blockIdx.x * TPB + threadIdx.x;
    if (e >= n_entries) return;
    const long long p = proposals_idx[2 * (size_t)e + 0];
    const long long pt = proposals_idx[2 * (size_t)e + 1] % n_fold;
    if (p < 0 || p >= n_prop || pt < 0) return;
    atomicOr(&masks[(size_t)p * words + (pt >> 5)], 1u << (pt & 31));
}

// counts[p] = popcount of row p (one wave per row)
__global__ __launch_bounds__(64) void k_row_popcount(const unsigned* __restrict__ masks, int words, int* __restrict__ counts) {
    const unsigned* row = masks + (size_t)blockIdx.x * words;
    int c = 0;
    for (int w = threadIdx.x; w < words; w += 64) c += __popc(row[w]);
    c = wave_reduce_add(c);
    if (threadIdx.x == 0) counts[blockIdx.x] = c;
}

// iou[i][j] = |Mi & Mj| / (|Mi| + |Mj| - |Mi & Mj|) in fp32, the arithmetic of eval_map.py:90-96 on exact integers
__global__ __launch_bounds__(64) void k_mask_iou(const unsigned* __restrict__ masks, const int* __restrict__ rows, int n_rows,
                                                int words, const int* __restrict__ counts, float* __restrict__ iou) {
    const int i = blockIdx.x, j = blockIdx.y;
    const int ri = rows ? rows[i] : i, rj = rows ? rows[j] : j;
    const int c = mask_pair_intersection(masks + (size_t)ri * words, masks + (size_t)rj * words, words);
    if (threadIdx.x == 0) iou[(size_t)i * n_rows + j] = mask_pair_iou(c, counts[ri], counts[rj]);
}

// seg[pt] = the LAST picked cluster that contains the point (eval_map.py:104-107 overwrites in order), else -100
__global__ __launch_bounds__(TPB) void k_point_labels(const unsigned* __restrict__ masks, const int* __restrict__ pick,
                                                     int n_pick, int words, int n_fold, long long* __restrict__ seg) {
    const int pt = blockIdx.x * TPB + threadIdx.x;
    if (pt >= n_fold) return;
    long long lab = -100;
    for (int c = n_pick - 1; c >= 0; --c)
        if ((masks[(size_t)pick[c] * words + (pt >> 5)] >> (pt & 31)) & 1u) { lab = c; break; }
    seg[pt] = lab;
}

// histogram of point labels per superpoint (tools/getins.py:88-92: negative labels go to bucket n_label)
__global__ __launch_bounds__(TPB) void k_sp_hist(const long long* __restrict__ seg, const long long* __restrict__ superpoint,
                                                int n, int n_sp, int n_label, int* __restrict__ hist) {
    const int pt = blockIdx.x * TPB + threadIdx.x;
    if (pt >= n) return;
    const long long sp = superpoint[pt];
    if (sp < 0 || sp >= n_sp) return;
    long long l = seg[pt];
    if (l < 0 || l > n_label) l = n_label;
    atomicAdd(&hist[(size_t)sp * (n_label + 1) + l], 1);
}

// sp_label = first arg-max bucket (np.argmax), bucket n_label -> -100 (tools/getins.py:93-94)
__global__ __launch_bounds__(TPB) void k_sp_argmax(const int* __restrict__ hist, int n_sp, int n_label,
                                                  long long* __restrict__ sp_label) {
    const int sp = blockIdx.x * TPB + threadIdx.x;
    if (sp >= n_sp) return;
    const int* h = hist + (size_t)sp * (n_label + 1);
    int best = h[0], arg = 0;
    for (int l = 1; l <= n_label; ++l)
        if (h[l] > best) { best = h[l]; arg = l; }
    sp_label[sp] = arg == n_label ? -100 : arg;
}

// seg2 = sp_label[superpoint]; cluster bitsets rebuilt from it (eval_map.py:109-116)
__global__ __launch_bounds__(TPB) void k_relabel_points(const long long* __restrict__ sp_label,
                                                       const long long* __restrict__ superpoint, int n, int n_sp,
                                                       int n_label, int words, long long* __restrict__ seg2,
                                                       unsigned* __restrict__ masks_out) {
    const int pt = blockIdx.x * TPB + threadIdx.x;
    if (pt >= n) return;
    const long long sp = superpoint[pt];
    const long long l = (sp >= 0 && sp < n_sp) ? sp_label[sp] : -100;
    seg2[pt] = l;
    if (l >= 0 && l < n_label) atomicOr(&masks_out[(size_t)l * words + (pt >> 5)], 1u << (pt & 31));
}

// dense int32 [rows, n_fold] view of selected bitset rows (the reference's `clusters` tensor)
__global__ __launch_bounds__(TPB) void k_bits_to_dense(const unsigned* __restrict__ masks, const int* __restrict__ rows,
                                                      int n_rows, int words, int n_fold, int* __restrict__ dense) {
    const long long e = (long long)blockIdx.x * TPB + threadIdx.x;
    if (e >= (long long)n_rows * n_fold) return;
    const int r = (int)(e / n_fold), pt = (int)(e - (long long)r * n_fold);
    const int src = rows ? rows[r] : r;
    dense[e] = (masks[(size_t)src * words + (pt >> 5)] >> (pt & 31)) & 1u;
}

// ---- the device-resident form (pbn_post_select .. pbn_post_compact) ------------------------------------------------------
// The same arithmetic with every count (n_rows, n_pick, n_keep) kept in device scalars: grids are sized by the capacity P and
// work items past the live count leave, so nothing between the first and the last launch waits for the host.

// rows = ascending proposals with score > score_t (fp32) and count > npoint_t (eval_map.py:74-84); the tail of rows is -1.
// The first launch of a call: it also clears the status word.
__global__ __launch_bounds__(TPB) void k_post_select(const float* __restrict__ score, const int* __restrict__ counts, int n_prop,
                                                    float score_t, int npoint_t, int* __restrict__ rows,
                                                    int* __restrict__ n_rows, int* __restrict__ status) {
    __shared__ int s_wave[TPB / 64];
    int base = 0;
    for (int p0 = 0; p0 < n_prop; p0 += TPB) {     // uniform trip count: the scan needs whole blocks
        const int p = p0 + threadIdx.x;
        const bool flag = p < n_prop && score[p] > score_t && counts[p] > npoint_t;
        int total;
        const int pos = block_flag_scan(flag, s_wave, &total);
        if (flag) rows[base + pos] = p;
        base += total;
    }
    for (int p = base + threadIdx.x; p < n_prop; p += TPB) rows[p] = -1;
    if (threadIdx.x == 0) { *n_rows = base; *status = 0; }
}

// k_mask_iou with the row count on the device: a fixed grid of one-wave workgroups strides over the n_rows^2 LIVE pairs, so the
// cost follows n_rows, not the capacity; table row stride cap; entries outside [n_rows, n_rows) stay
__global__ __launch_bounds__(64) void k_mask_iou_dev(const unsigned* __restrict__ masks, const int* __restrict__ rows,
                                                    const int* __restrict__ n_rows_dev, int cap, int words,
                                                    const int* __restrict__ counts, float* __restrict__ iou) {
    const int n_rows = min(*n_rows_dev, cap);
    const int n_pairs = n_rows * n_rows;           // cap <= 4096: fits
    for (int e = blockIdx.x; e < n_pairs; e += gridDim.x) {      // uniform per wave: one pair per wave and trip
        const int i = e / n_rows, j = e - i * n_rows;
        const int ri = rows[i], rj = rows[j];
        if (ri < 0 || ri >= cap || rj < 0 || rj >= cap) continue;
        const int c = mask_pair_intersection(masks + (size_t)ri * words, masks + (size_t)rj * words, words);
        if (threadIdx.x == 0) iou[(size_t)i * cap + j] = mask_pair_iou(c, counts[ri], counts[rj]);
    }
}

// nms_walk (post_dev.h) in one workgroup over the survivors of k_post_select: pick = survivor positions in pick order,
// pick_rows = their proposal indices, tails -1
__global__ __launch_bounds__(TPB) void k_post_nms(const float* __restrict__ score, const int* __restrict__ rows,
                                                 const int* __restrict__ n_rows_dev, int cap, const float* __restrict__ iou,
                                                 float nms_t, int* __restrict__ pick, int* __restrict__ pick_rows,
                                                 int* __restrict__ n_pick_dev) {
    __shared__ float s_score[POST_MAX_PROPOSALS];
    __shared__ unsigned short s_order[POST_MAX_PROPOSALS];
    __shared__ unsigned char s_supp[POST_MAX_PROPOSALS];
    const int n_pick = nms_walk(s_score, s_order, s_supp, score, rows, min(*n_rows_dev, cap), cap, iou, nms_t, pick, pick_rows);
    if (threadIdx.x == 0) *n_pick_dev = n_pick;
}

// zero what the vote accumulates into: hist columns [0, n_pick] of every row and the n_pick rebuilt bitsets
__global__ __launch_bounds__(TPB) void k_refine_clear(const int* __restrict__ n_pick_dev, int cap, int n_sp, int words,
                                                     int* __restrict__ hist, unsigned* __restrict__ masks_out) {
    const int n_pick = min(*n_pick_dev, cap);
    const long long n_hist = (long long)n_sp * (n_pick + 1), n_mask = (long long)n_pick * words;
    const long long step = (long long)gridDim.x * TPB;
    for (long long e = (long long)blockIdx.x * TPB + threadIdx.x; e < n_hist; e += step) {
        const long long sp = e / (n_pick + 1);
        hist[sp * (cap + 1) + (e - sp * (n_pick + 1))] = 0;
    }
    for (long long e = (long long)blockIdx.x * TPB + threadIdx.x; e < n_mask; e += step) masks_out[e] = 0u;
}

__global__ __launch_bounds__(TPB) void k_point_labels_dev(const unsigned* __restrict__ masks, const int* __restrict__ pick_rows,
                                                         const int* __restrict__ n_pick_dev, int cap, int words, int n_fold,
                                                         long long* __restrict__ seg) {
    const int pt = blockIdx.x * TPB + threadIdx.x;
    if (pt >= n_fold) return;
    const int n_pick = min(*n_pick_dev, cap);
    long long lab = -100;
    for (int c = n_pick - 1; c >= 0; --c)
        if ((masks[(size_t)pick_rows[c] * words + (pt >> 5)] >> (pt & 31)) & 1u) { lab = c; break; }
    seg[pt] = lab;
}

// k_sp_hist on the table hist[n_sp, cap + 1] (bucket n_pick = unlabelled); an id >= n_sp is reported, never counted
__global__ __launch_bounds__(TPB) void k_sp_hist_dev(const long long* __restrict__ seg, const long long* __restrict__ superpoint,
                                                    int n, int n_sp, const int* __restrict__ n_pick_dev, int cap,
                                                    int* __restrict__ hist, int* __restrict__ status) {
    const int pt = blockIdx.x * TPB + threadIdx.x;
    if (pt >= n) return;
    const long long sp = superpoint[pt];
    if (sp >= n_sp) { atomicOr(status, POST_STATUS_SUPERPOINT); return; }
    if (sp < 0) return;
    const int n_label = min(*n_pick_dev, cap);
    long long l = seg[pt];
    if (l < 0 || l > n_label) l = n_label;
    atomicAdd(&hist[(size_t)sp * (cap + 1) + l], 1);
}

__global__ __launch_bounds__(TPB) void k_sp_argmax_dev(const int* __restrict__ hist, int n_sp, const int* __restrict__ n_pick_dev,
                                                      int cap, long long* __restrict__ sp_label) {
    const int sp = blockIdx.x * TPB + threadIdx.x;
    if (sp >= n_sp) return;
    const int n_label = min(*n_pick_dev, cap);
    const int* h = hist + (size_t)sp * (cap + 1);
    int best = h[0], arg = 0;
    for (int l = 1; l <= n_label; ++l)
        if (h[l] > best) { best = h[l]; arg = l; }
    sp_label[sp] = arg == n_label ? -100 : arg;
}

__global__ __launch_bounds__(TPB) void k_relabel_points_dev(const long long* __restrict__ sp_label,
                                                           const long long* __restrict__ superpoint, int n, int n_sp,
                                                           const int* __restrict__ n_pick_dev, int cap, int words,
                                                           long long* __restrict__ seg2, unsigned* __restrict__ masks_out) {
    const int pt = blockIdx.x * TPB + threadIdx.x;
    if (pt >= n) return;
    const int n_label = min(*n_pick_dev, cap);
    const long long sp = superpoint[pt];
    const long long l = (sp >= 0 && sp < n_sp) ? sp_label[sp] : -100;
    seg2[pt] = l;
    if (l >= 0 && l < n_label) atomicOr(&masks_out[(size_t)l * words + (pt >> 5)], 1u << (pt & 31));
}

// counts[c] = popcount of rebuilt row c for c < n_pick, 0 above (grid = cap rows, one wave each)
__global__ __launch_bounds__(64) void k_row_popcount_dev(const unsigned* __restrict__ masks, int words,
                                                        const int* __restrict__ n_rows_dev, int cap, int* __restrict__ counts) {
    int c = 0;
    if ((int)blockIdx.x < min(*n_rows_dev, cap)) {
        const unsigned* row = masks + (size_t)blockIdx.x * words;
        for (int w = threadIdx.x; w < words; w += 64) c += __popc(row[w]);
        c = wave_reduce_add(c);
    }
    if (threadIdx.x == 0) counts[blockIdx.x] = c;
}

// keep = the picked clusters that still own a point, in order (eval_map.py:113-118), with their score and the class of the
// proposal's first member (:63-65) through the label table; tails: keep -1, score 0, class -1
__global__ __launch_bounds__(TPB) void k_post_compact(const int* __restrict__ counts2, const int* __restrict__ pick_rows,
                                                     const int* __restrict__ n_pick_dev, int cap, const float* __restrict__ score,
                                                     const long long* __restrict__ proposals_idx, int n_entries,
                                                     const void* __restrict__ offsets, int offsets_i64,
                                                     const void* __restrict__ pred_sem, int sem_i64, long long n_sem,
                                                     const long long* __restrict__ label_table, int n_labels,
                                                     int* __restrict__ keep, float* __restrict__ scores_out,
                                                     long long* __restrict__ sem_out, int* __restrict__ n_keep_dev,
                                                     int* __restrict__ status) {
    __shared__ int s_wave[TPB / 64];
    const int n_pick = min(*n_pick_dev, cap);
    int base = 0;
    for (int c0 = 0; c0 < n_pick; c0 += TPB) {
        const int c = c0 + threadIdx.x;
        const bool flag = c < n_pick && counts2[c] > 0;
        int total;
        const int pos = block_flag_scan(flag, s_wave, &total);
        if (flag) {
            const int p = pick_rows[c];
            const long long cls = first_member_class(proposals_idx, n_entries, offsets, offsets_i64, p, pred_sem, sem_i64, n_sem,
                                                     label_table, n_labels);
            if (cls < 0) atomicOr(status, POST_STATUS_CLASS);
            keep[base + pos] = c;
            scores_out[base + pos] = score[p];
            sem_out[base + pos] = cls;
        }
        base += total;
    }
    for (int k = base + threadIdx.x; k < cap; k += TPB) {
        keep[k] = -1;
        scores_out[k] = 0.f;
        sem_out[k] = -1;
    }
    if (threadIdx.x == 0) *n_keep_dev = base;
}

// k_bits_to_dense over the whole capacity: rows below n_keep are the kept bitsets, the rest zero
__global__ __launch_bounds__(TPB) void k_bits_to_dense_dev(const unsigned* __restrict__ masks, const int* __restrict__ keep,
                                                          const int* __restrict__ n_keep_dev, int cap, int words, int n_fold,
                                                          int* __restrict__ dense) {
    const long long e = (long long)blockIdx.x * TPB + threadIdx.x;
    if (e >= (long long)cap * n_fold) return;
    const int r = (int)(e / n_fold), pt = (int)(e - (long long)r * n_fold);
    int v = 0;
    if (r < min(*n_keep_dev, cap)) v = (masks[(size_t)keep[r] * words + (pt >> 5)] >> (pt & 31)) & 1u;
    dense[e] = v;
}

}  // namespace
}  // namespace pbn

using namespace pbn;

extern "C" int pbn_post_words(int n_fold) { return n_fold > 0 ? (n_fold + 31) / 32 : 0; }

extern "C" int pbn_proposal_bitmask(const int64_t* proposals_idx, int n_entries, int n_fold, int n_prop, uint32_t* masks,
                                    int32_t* counts, pbn_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (n_entries < 0 || n_fold < 1 || n_prop < 0) return PBN_ERR_ARG;
    if (n_prop == 0) return PBN_OK;
    if (!masks || !counts || (n_entries > 0 && !proposals_idx)) return PBN_ERR_ARG;
    const int words = pbn_post_words(n_fold);
    PBN_TRY(fill_bytes(masks, 0, sizeof(uint32_t) * (size_t)n_prop * words, stream));
    if (n_entries > 0)
        hipLaunchKernelGGL(k_set_bits, dim3(cdiv(n_entries, TPB)), dim3(TPB), 0, stream, (const long long*)proposals_idx,
                           n_entries, n_fold, n_prop, words, masks);
    hipLaunchKernelGGL(k_row_popcount, dim3(n_prop), dim3(64), 0, stream, masks, words, counts);
    PBN_LAUNCH_CHECK();
    return PBN_OK;
}

extern "C" int pbn_mask_iou(const uint32_t* masks, const int32_t* rows, int n_rows, int n_fold, const int32_t* counts,
                            float* iou, pbn_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (n_rows < 0 || n_fold < 1) return PBN_ERR_ARG;
    if (n_rows == 0) return PBN_OK;
    if (!masks || !counts || !iou) return PBN_ERR_ARG;
    hipLaunchKernelGGL(k_mask_iou, dim3(n_rows, n_rows), dim3(64), 0, stream, masks, rows, n_rows, pbn_post_words(n_fold),
                       counts, iou);
    PBN_LAUNCH_CHECK();
    return PBN_OK;
}

extern "C" int pbn_superpoint_refine(const uint32_t* masks, const int32_t* pick, int n_pick, int n_fold,
                                     const int64_t* superpoint, int n_sp, int64_t* seg, int32_t* hist, int64_t* sp_label,
                                     int64_t* seg_refined, uint32_t* masks_out, int32_t* counts_out, pbn_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (n_pick < 0 || n_fold < 1 || n_sp < 1) return PBN_ERR_ARG;
    if (!masks || !superpoint || !seg || !hist || !sp_label || !seg_refined || (n_pick > 0 && (!pick || !masks_out || !counts_out)))
        return PBN_ERR_ARG;
    const int words = pbn_post_words(n_fold);
    const int nb = cdiv(n_fold, TPB);
    PBN_TRY(fill_bytes(hist, 0, sizeof(int) * (size_t)n_sp * (n_pick + 1), stream));
    if (n_pick > 0) PBN_TRY(fill_bytes(masks_out, 0, sizeof(uint32_t) * (size_t)n_pick * words, stream));
    hipLaunchKernelGGL(k_point_labels, dim3(nb), dim3(TPB), 0, stream, masks, pick, n_pick, words, n_fold, (long long*)seg);
    hipLaunchKernelGGL(k_sp_hist, dim3(nb), dim3(TPB), 0, stream, (const long long*)seg, (const long long*)superpoint, n_fold,
                       n_sp, n_pick, hist);
    hipLaunchKernelGGL(k_sp_argmax, dim3(cdiv(n_sp, TPB)), dim3(TPB), 0, stream, hist, n_sp, n_pick, (long long*)sp_label);
    hipLaunchKernelGGL(k_relabel_points, dim3(nb), dim3(TPB), 0, stream, (const long long*)sp_label,
                       (const long long*)superpoint, n_fold, n_sp, n_pick, words, (long long*)seg_refined, masks_out);
    if (n_pick > 0) hipLaunchKernelGGL(k_row_popcount, dim3(n_pick), dim3(64), 0, stream, masks_out, words, counts_out);
    PBN_LAUNCH_CHECK();
    return PBN_OK;
}

extern "C" int pbn_bitmask_to_dense(const uint32_t* masks, const int32_t* rows, int n_rows, int n_fold, int32_t* dense,
                                    pbn_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (n_rows < 0 || n_fold < 1) return PBN_ERR_ARG;
    if (n_rows == 0) return PBN_OK;
    if (!masks || !dense) return PBN_ERR_ARG;
    hipLaunchKernelGGL(k_bits_to_dense, dim3(cdiv((long long)n_rows * n_fold, TPB)), dim3(TPB), 0, stream, masks, rows, n_rows,
                       pbn_post_words(n_fold), n_fold, dense);
    PBN_LAUNCH_CHECK();
    return PBN_OK;
}

extern "C" int pbn_post_max_proposals(void) { return POST_MAX_PROPOSALS; }

extern "C" int pbn_post_select(const float* clt_score, const int32_t* counts, int n_prop, float score_t, int npoint_t,
                               int32_t* rows, int32_t* n_rows, int32_t* status, pbn_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (n_prop < 1 || !clt_score || !counts || !rows || !n_rows || !status) return PBN_ERR_ARG;
    if (n_prop > POST_MAX_PROPOSALS) return PBN_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(k_post_select, dim3(1), dim3(TPB), 0, stream, clt_score, counts, n_prop, score_t, npoint_t, rows, n_rows,
                       status);
    PBN_LAUNCH_CHECK();
    return PBN_OK;
}

extern "C" int pbn_mask_iou_dev(const uint32_t* masks, const int32_t* rows, const int32_t* n_rows, int n_prop, int n_fold,
                                const int32_t* counts, float* iou, pbn_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (n_prop < 1 || n_fold < 1 || !masks || !rows || !n_rows || !counts || !iou) return PBN_ERR_ARG;
    if (n_prop > POST_MAX_PROPOSALS) return PBN_ERR_UNSUPPORTED;
    const long long pairs = (long long)n_prop * n_prop;
    hipLaunchKernelGGL(k_mask_iou_dev, dim3((unsigned)(pairs < 8192 ? pairs : 8192)), dim3(64), 0, stream, masks, rows, n_rows, n_prop,
                       pbn_post_words(n_fold), counts, iou);
    PBN_LAUNCH_CHECK();
    return PBN_OK;
}

extern "C" int pbn_post_nms(const float* clt_score, const int32_t* rows, const int32_t* n_rows, int n_prop, const float* iou,
                            float nms_t, int32_t* pick, int32_t* pick_rows, int32_t* n_pick, pbn_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (n_prop < 1 || !clt_score || !rows || !n_rows || !iou || !pick || !pick_rows || !n_pick) return PBN_ERR_ARG;
    if (n_prop > POST_MAX_PROPOSALS) return PBN_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(k_post_nms, dim3(1), dim3(TPB), 0, stream, clt_score, rows, n_rows, n_prop, iou, nms_t, pick, pick_rows,
                       n_pick);
    PBN_LAUNCH_CHECK();
    return PBN_OK;
}

extern "C" int pbn_superpoint_refine_dev(const uint32_t* masks, const int32_t* pick_rows, const int32_t* n_pick, int n_prop,
                                         int n_fold, const int64_t* superpoint, int n_sp_cap, int64_t* seg, int32_t* hist,
                                         int64_t* sp_label, int64_t* seg_refined, uint32_t* masks_out, int32_t* counts_out,
                                         int32_t* status, pbn_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (n_prop < 1 || n_fold < 1 || n_sp_cap < 1) return PBN_ERR_ARG;
    if (!masks || !pick_rows || !n_pick || !superpoint || !seg || !hist || !sp_label || !seg_refined || !masks_out ||
        !counts_out || !status)
        return PBN_ERR_ARG;
    if (n_prop > POST_MAX_PROPOSALS) return PBN_ERR_UNSUPPORTED;
    const int words = pbn_post_words(n_fold);
    const int nb = cdiv(n_fold, TPB);
    const long long clear_max = (long long)n_sp_cap * (n_prop + 1) > (long long)n_prop * words ? (long long)n_sp_cap * (n_prop + 1)
                                                                                                : (long long)n_prop * words;
    // + 1: clear_max / TPB + 1 blocks, one also for an empty table
    hipLaunchKernelGGL(k_refine_clear, dim3(stride_blocks(clear_max + 1)), dim3(TPB), 0, stream, n_pick, n_prop, n_sp_cap, words,
                       hist, masks_out);
    hipLaunchKernelGGL(k_point_labels_dev, dim3(nb), dim3(TPB), 0, stream, masks, pick_rows, n_pick, n_prop, words, n_fold,
                       (long long*)seg);
    hipLaunchKernelGGL(k_sp_hist_dev, dim3(nb), dim3(TPB), 0, stream, (const long long*)seg, (const long long*)superpoint, n_fold,
                       n_sp_cap, n_pick, n_prop, hist, status);
    hipLaunchKernelGGL(k_sp_argmax_dev, dim3(cdiv(n_sp_cap, TPB)), dim3(TPB), 0, stream, hist, n_sp_cap, n_pick, n_prop,
                       (long long*)sp_label);
    hipLaunchKernelGGL(k_relabel_points_dev, dim3(nb), dim3(TPB), 0, stream, (const long long*)sp_label,
                       (const long long*)superpoint, n_fold, n_sp_cap, n_pick, n_prop, words, (long long*)seg_refined, masks_out);
    hipLaunchKernelGGL(k_row_popcount_dev, dim3(n_prop), dim3(64), 0, stream, masks_out, words, n_pick, n_prop, counts_out);
    PBN_LAUNCH_CHECK();
    return PBN_OK;
}

extern "C" int pbn_post_compact(const int32_t* counts2, const int32_t* pick_rows, const int32_t* n_pick, int n_prop, int n_fold,
                                const float* clt_score, const int64_t* proposals_idx, int n_entries, const void* proposals_offset,
                                int offset_i64, const void* pred_sem, int sem_i64, int64_t n_sem, const int64_t* label_table,
                                int n_labels, const uint32_t* masks2, int32_t* keep, float* scores_out, int64_t* semantic_id_out,
                                int32_t* clusters, int32_t* n_keep, int32_t* status, pbn_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (n_prop < 1 || n_fold < 1 || n_entries < 0 || n_sem < 0 || n_labels < 1) return PBN_ERR_ARG;
    if (!counts2 || !pick_rows || !n_pick || !clt_score || !proposals_idx || !proposals_offset || !pred_sem || !label_table ||
        !masks2 || !keep || !scores_out || !semantic_id_out || !clusters || !n_keep || !status)
        return PBN_ERR_ARG;
    if (n_prop > POST_MAX_PROPOSALS) return PBN_ERR_UNSUPPORTED;
    if (((long long)n_prop * n_fold + TPB - 1) / TPB > 0x7fffffffLL) return PBN_ERR_RANGE;
    hipLaunchKernelGGL(k_post_compact, dim3(1), dim3(TPB), 0, stream, counts2, pick_rows, n_pick, n_prop, clt_score,
                       (const long long*)proposals_idx, n_entries, proposals_offset, offset_i64, pred_sem, sem_i64,
                       (long long)n_sem, (const long long*)label_table, n_labels, keep, scores_out, (long long*)semantic_id_out,
                       n_keep, status);
    hipLaunchKernelGGL(k_bits_to_dense_dev, dim3(cdiv((long long)n_prop * n_fold, TPB)), dim3(TPB), 0, stream, masks2, keep, n_keep,
                       n_prop, pbn_post_words(n_fold), n_fold, clusters);
    PBN_LAUNCH_CHECK();
    return PBN_OK;
}
