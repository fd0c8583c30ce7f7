// apassoc.hip -- the AP association of one validation scene (tools/eval.py:205-250, the tables behind
// evaluate.assign_instances_for_scan) without a host stop: ground-truth ids encoded and numbered on the device, the overlap
// table of the capacity-shaped clusters that pbn_post_compact leaves, and one compact record per scene appended to an epoch
// log that the host reads once.  Capacities come from the host, live counts (n_keep, n_gt) stay in device scalars; grids are
// sized by capacity or fixed and striding, and work past the live count leaves.  Integer atomics only: every result is
// bit-identical from run to run.
#include "pbn_common.h"
#include "assoc_dev.h"

namespace pbn {
namespace {

constexpr int TPB = POST_TPB;
constexpr int OVERLAP_CHUNK = 4096;                 // points per workgroup of k_instance_overlap_dev
constexpr int OVERLAP_LDS_BINS = 8192;

__device__ __forceinline__ int live_count(const int* dev, int cap) {
    const int n = dev ? *dev : cap;
    return n < 0 ? 0 : (n > cap ? cap : n);
}

__global__ __launch_bounds__(TPB) void k_fill_i32(int* __restrict__ p, int n, int value) {
    for (int i = blockIdx.x * TPB + threadIdx.x; i < n; i += gridDim.x * TPB) p[i] = value;
}

// ---- pbn_gt_encode_dev: get_val_gt.py:26-37 ------------------------------------------------------------------------------
// first[inst] = lowest point index of the instance (`instance_mask[0]`)
__global__ __launch_bounds__(TPB) void k_gt_first(const void* __restrict__ ins, int ins_i64, int n_pts, int n_inst_cap,
                                                 int* __restrict__ first, int* __restrict__ status) {
    for (int i = blockIdx.x * TPB + threadIdx.x; i < n_pts; i += gridDim.x * TPB) {
        const long long inst = load_index(ins, ins_i64, i);
        if (inst < 0) continue;
        if (inst >= n_inst_cap) { atomicOr(status, PBN_AP_STATUS_INSTANCE_CAP); continue; }
        atomicMin(&first[inst], i);
    }
}

// ids[i] = gt_code of (sem[first[inst]], inst), 0 without an instance
__global__ __launch_bounds__(TPB) void k_gt_code(const void* __restrict__ sem, int sem_i64, const void* __restrict__ ins,
                                                int ins_i64, int n_pts, const int* __restrict__ label_table, int n_labels,
                                                const int* __restrict__ first, int n_inst_cap, int* __restrict__ ids,
                                                int* __restrict__ status) {
    for (int i = blockIdx.x * TPB + threadIdx.x; i < n_pts; i += gridDim.x * TPB) {
        const long long inst = load_index(ins, ins_i64, i);
        int code = 0;
        if (inst >= 0 && inst < n_inst_cap) {
            const int f = first[inst];                     // <= i: this very point took part in the minimum
            const GtCode g = gt_code((f >= 0 && f < n_pts) ? load_index(sem, sem_i64, f) : 0, inst, label_table, n_labels);
            if (g.status) atomicOr(status, g.status);
            code = g.code;
        }
        ids[i] = code;
    }
}

// ---- pbn_gt_index_dev: np.unique(ids, return_inverse=True) through a direct table -------------------------------------
// table[id] += 1 per point (the id's vertex count)
__global__ __launch_bounds__(TPB) void k_gt_hist(const void* __restrict__ ids, int ids_i64, int n_pts, int id_cap,
                                                int* __restrict__ table, int* __restrict__ status) {
    for (int base = blockIdx.x * TPB; base < n_pts; base += gridDim.x * TPB) {     // uniform per block: whole waves ballot
        const int i = base + threadIdx.x;
        int bin = -1;
        if (i < n_pts) {
            const long long id = load_index(ids, ids_i64, i);
            if (id < 0 || id >= id_cap) atomicOr(status, PBN_AP_STATUS_ID_RANGE);
            else bin = (int)id;
        }
        wave_merged_add(table, bin);
    }
}

// gt_number_scan (assoc_dev.h) by one workgroup; an id past u_cap slots reports ID_COUNT
__global__ __launch_bounds__(TPB) void k_gt_scan(int* __restrict__ table, int id_cap, int* __restrict__ uid,
                                                int* __restrict__ gt_vert, int u_cap, int* __restrict__ n_gt,
                                                int* __restrict__ status) {
    __shared__ int s_wave[TPB / 64];
    bool over = false;
    const int live = gt_number_scan(table, id_cap, uid, gt_vert, u_cap, s_wave, &over);
    if (over) atomicOr(status, PBN_AP_STATUS_ID_COUNT);
    if (threadIdx.x == 0) *n_gt = live;
}

__global__ __launch_bounds__(TPB) void k_gt_lookup(const void* __restrict__ ids, int ids_i64, int n_pts, int id_cap,
                                                  const int* __restrict__ table, int* __restrict__ gt_index) {
    for (int i = blockIdx.x * TPB + threadIdx.x; i < n_pts; i += gridDim.x * TPB) {
        const long long id = load_index(ids, ids_i64, i);
        gt_index[i] = (id >= 0 && id < id_cap) ? table[id] : -1;
    }
}

// ---- pbn_instance_overlap_dev ------------------------------------------------------------------------------------------
// zero the live rectangle [n_keep, n_gt] of inter (row stride u_cap)
__global__ __launch_bounds__(TPB) void k_overlap_clear(const int* __restrict__ n_keep_dev, int p_cap,
                                                      const int* __restrict__ n_gt_dev, int u_cap, int* __restrict__ inter) {
    const int rows = live_count(n_keep_dev, p_cap), cols = live_count(n_gt_dev, u_cap);
    const long long n = (long long)rows * cols, step = (long long)gridDim.x * TPB;
    for (long long e = (long long)blockIdx.x * TPB + threadIdx.x; e < n; e += step) {
        const long long r = e / cols;
        inter[r * u_cap + (e - r * cols)] = 0;
    }
}

// inter[p][gt_index[i]] += 1 for every point i inside prediction p (mask value != 0): the association counts of
// tools/eval.py:230-245 (`count_nonzero(logical_and(gt_ids == id, pred_mask))` per (prediction, instance) pair, one pass
// over the scene per pair in the reference) as ONE pass per prediction.  A block owns OVERLAP_CHUNK consecutive points of
// one prediction; instances are runs of neighbouring vertices, so a wave first merges lanes that hit the same bin.
// Row gate p < n_keep and live bin count n_gt on the device (a null pointer: the capacity itself, the host-count form
// pbn_instance_overlap); output row stride u_cap.
// USE_LDS: a block's bins in LDS first (u_cap <= OVERLAP_LDS_BINS); without it straight to global atomics, and no LDS is held
template <bool USE_LDS>
__global__ __launch_bounds__(TPB) void k_instance_overlap_dev(const int* __restrict__ clusters, const int* __restrict__ n_keep_dev,
                                                             int p_cap, int n_pts, const int* __restrict__ gt_index,
                                                             const int* __restrict__ n_gt_dev, int u_cap,
                                                             int* __restrict__ inter) {
    __shared__ int s_hist[USE_LDS ? OVERLAP_LDS_BINS : 1];
    const int p = blockIdx.y;
    if (p >= live_count(n_keep_dev, p_cap)) return;         // uniform per block
    const int n_gt = live_count(n_gt_dev, u_cap);
    const int lo = blockIdx.x * OVERLAP_CHUNK;
    const int hi = min(n_pts, lo + OVERLAP_CHUNK);
    int* out = inter + (size_t)p * u_cap;
    if (USE_LDS) {
        for (int b = threadIdx.x; b < n_gt; b += TPB) s_hist[b] = 0;
        __syncthreads();
    }
    const int* row = clusters + (size_t)p * n_pts;
    for (int base = lo; base < hi; base += TPB) {           // uniform trip count: the ballots need whole waves
        const int i = base + threadIdx.x;
        int bin = -1;
        if (i < hi && row[i] != 0) {
            const int g = gt_index[i];
            if (g >= 0 && g < n_gt) bin = g;
        }
        if (USE_LDS) wave_merged_add(s_hist, bin);
        else wave_merged_add(out, bin);
    }
    if (USE_LDS) {
        __syncthreads();
        for (int b = threadIdx.x; b < n_gt; b += TPB) {
            const int c = s_hist[b];
            if (c) atomicAdd(&out[b], c);
        }
    }
}

// ---- pbn_ap_record_append ----------------------------------------------------------------------------------------------
// One thread: ap_record_reserve (assoc_dev.h) for this scene.  Consumes (reads and clears) the association status.
__global__ __launch_bounds__(64) void k_ap_record_reserve(int* __restrict__ state, int* __restrict__ log, int log_words,
                                                         int scene_tag, const int* __restrict__ n_keep_dev, int p_cap,
                                                         const int* __restrict__ n_gt_dev, int u_cap, int n_pts,
                                                         const int* __restrict__ post_status, int* __restrict__ assoc_status) {
    if (threadIdx.x != 0) return;
    const int status = (post_status ? *post_status : 0) | *assoc_status;
    *assoc_status = 0;
    ap_record_reserve(state, log, log_words, scene_tag, live_count(n_keep_dev, p_cap), live_count(n_gt_dev, u_cap), n_pts, status);
}

// body of the record at the published offset: uid | gt_vert | label_id | conf bits | inter rows compacted from stride u_cap
__global__ __launch_bounds__(TPB) void k_ap_record_write(const int* __restrict__ state, int* __restrict__ log,
                                                        const int* __restrict__ uid, const int* __restrict__ gt_vert,
                                                        const long long* __restrict__ semantic_id,
                                                        const float* __restrict__ conf, const int* __restrict__ inter,
                                                        int u_cap) {
    const int off = state[ST_OFFSET];
    if (off < 0) return;
    int* rec = log + off;
    const int nk = rec[2], ng = rec[3];
    if (nk == 0) return;
    const long long head = 2LL * ng + 2LL * nk, total = head + (long long)nk * ng;
    const long long step = (long long)gridDim.x * TPB;
    for (long long e = (long long)blockIdx.x * TPB + threadIdx.x; e < total; e += step) {
        int v;
        if (e < head) v = ap_record_head_word(e, nk, ng, rec, uid, gt_vert, semantic_id, conf);
        else {
            const long long r = e - head, q = r / ng;
            v = inter[q * u_cap + (r - q * ng)];
        }
        rec[AP_HDR + e] = v;
    }
}

}  // namespace
}  // namespace pbn

using namespace pbn;

extern "C" int pbn_gt_encode_dev(const void* sem, int sem_i64, const void* ins, int ins_i64, int n_pts,
                                 const int32_t* label_table, int n_labels, int32_t* first, int n_inst_cap, int32_t* ids,
                                 int32_t* status, pbn_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (n_pts < 0 || n_labels < 1 || n_inst_cap < 1) return PBN_ERR_ARG;
    if (!label_table || !first || !status) return PBN_ERR_ARG;
    if (n_pts == 0) return PBN_OK;
    if (!sem || !ins || !ids) return PBN_ERR_ARG;
    const int nb = stride_blocks(n_pts);
    hipLaunchKernelGGL(k_fill_i32, dim3(stride_blocks(n_inst_cap)), dim3(TPB), 0, stream, first, n_inst_cap, 0x7fffffff);
    hipLaunchKernelGGL(k_gt_first, dim3(nb), dim3(TPB), 0, stream, ins, ins_i64, n_pts, n_inst_cap, first, status);
    hipLaunchKernelGGL(k_gt_code, dim3(nb), dim3(TPB), 0, stream, sem, sem_i64, ins, ins_i64, n_pts, label_table, n_labels,
                       (const int*)first, n_inst_cap, ids, status);
    PBN_LAUNCH_CHECK();
    return PBN_OK;
}

extern "C" int pbn_gt_index_dev(const void* ids, int ids_i64, int n_pts, int32_t* table, int id_cap, int32_t* uid,
                                int32_t* gt_vert, int u_cap, int32_t* n_gt, int32_t* gt_index, int32_t* status,
                                pbn_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (n_pts < 0 || id_cap < 1 || u_cap < 1) return PBN_ERR_ARG;
    if (!table || !uid || !gt_vert || !n_gt || !status || (n_pts > 0 && (!ids || !gt_index))) return PBN_ERR_ARG;
    if (id_cap > GT_ID_CAP_MAX) return PBN_ERR_UNSUPPORTED;
    const int nb = stride_blocks(n_pts);
    hipLaunchKernelGGL(k_fill_i32, dim3(stride_blocks(id_cap)), dim3(TPB), 0, stream, table, id_cap, 0);
    if (n_pts > 0)
        hipLaunchKernelGGL(k_gt_hist, dim3(nb), dim3(TPB), 0, stream, ids, ids_i64, n_pts, id_cap, table, status);
    hipLaunchKernelGGL(k_gt_scan, dim3(1), dim3(TPB), 0, stream, table, id_cap, uid, gt_vert, u_cap, n_gt, status);
    if (n_pts > 0)
        hipLaunchKernelGGL(k_gt_lookup, dim3(nb), dim3(TPB), 0, stream, ids, ids_i64, n_pts, id_cap, (const int*)table, gt_index);
    PBN_LAUNCH_CHECK();
    return PBN_OK;
}

extern "C" int pbn_instance_overlap_dev(const int32_t* clusters, const int32_t* n_keep, int p_cap, int n_pts,
                                        const int32_t* gt_index, const int32_t* n_gt, int u_cap, int32_t* inter,
                                        pbn_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (p_cap < 0 || n_pts < 0 || u_cap < 1 || !n_gt) return PBN_ERR_ARG;
    if (p_cap == 0) return PBN_OK;
    if (!inter || (n_pts > 0 && (!clusters || !gt_index))) return PBN_ERR_ARG;
    if (p_cap > 65535) return PBN_ERR_UNSUPPORTED;          // one grid row per prediction
    if ((long long)p_cap * u_cap > 0x7fffffffLL) return PBN_ERR_RANGE;
    hipLaunchKernelGGL(k_overlap_clear, dim3(stride_blocks((long long)p_cap * u_cap)), dim3(TPB), 0, stream, n_keep, p_cap, n_gt,
                       u_cap, inter);
    if (n_pts > 0) {
        const dim3 grid(cdiv(n_pts, OVERLAP_CHUNK), p_cap);
        if (u_cap <= OVERLAP_LDS_BINS)
            hipLaunchKernelGGL(k_instance_overlap_dev<true>, grid, dim3(TPB), 0, stream, clusters, n_keep, p_cap, n_pts, gt_index,
                               n_gt, u_cap, inter);
        else
            hipLaunchKernelGGL(k_instance_overlap_dev<false>, grid, dim3(TPB), 0, stream, clusters, n_keep, p_cap, n_pts, gt_index,
                               n_gt, u_cap, inter);
    }
    PBN_LAUNCH_CHECK();
    return PBN_OK;
}

// the host-count form (the evaluator's table, tools/eval.py:230-245): every row and every bin live, inter[n_pred, n_gt] cleared whole
extern "C" int pbn_instance_overlap(const int32_t* masks, int n_pred, int n_pts, const int32_t* gt_index, int n_gt,
                                    int32_t* inter, pbn_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (n_pred < 0 || n_pts < 0 || n_gt < 1) return PBN_ERR_ARG;
    if (n_pred == 0) return PBN_OK;
    if (!inter) return PBN_ERR_ARG;
    PBN_TRY(fill_bytes(inter, 0, sizeof(int32_t) * (size_t)n_pred * n_gt, stream));
    if (n_pts == 0) return PBN_OK;
    if (!masks || !gt_index) return PBN_ERR_ARG;
    const dim3 grid(cdiv(n_pts, OVERLAP_CHUNK), n_pred);
    if (n_gt <= OVERLAP_LDS_BINS)
        hipLaunchKernelGGL(k_instance_overlap_dev<true>, grid, dim3(TPB), 0, stream, masks, (const int*)nullptr, n_pred, n_pts, gt_index,
                           (const int*)nullptr, n_gt, inter);
    else
        hipLaunchKernelGGL(k_instance_overlap_dev<false>, grid, dim3(TPB), 0, stream, masks, (const int*)nullptr, n_pred, n_pts, gt_index,
                           (const int*)nullptr, n_gt, inter);
    PBN_LAUNCH_CHECK();
    return PBN_OK;
}

extern "C" int pbn_ap_record_append(int32_t* state, int32_t* log, int64_t log_words, int scene_tag, const int32_t* n_keep,
                                    int p_cap, const int32_t* n_gt, int u_cap, int n_pts, const int32_t* post_status,
                                    int32_t* assoc_status, const int32_t* uid, const int32_t* gt_vert,
                                    const int64_t* semantic_id, const float* conf, const int32_t* inter, pbn_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (log_words < 0 || p_cap < 0 || u_cap < 1 || n_pts < 0) return PBN_ERR_ARG;
    if (!state || !n_gt || !assoc_status || !uid || !gt_vert || (log_words > 0 && !log)) return PBN_ERR_ARG;
    if (p_cap > 0 && (!semantic_id || !conf || !inter)) return PBN_ERR_ARG;
    if (log_words > 0x7fffffffLL || (long long)p_cap * u_cap > 0x7fffffffLL) return PBN_ERR_RANGE;
    hipLaunchKernelGGL(k_ap_record_reserve, dim3(1), dim3(64), 0, stream, state, log, (int)log_words, scene_tag, n_keep, p_cap,
                       n_gt, u_cap, n_pts, post_status, assoc_status);
    if (p_cap > 0) {
        const long long body = 2LL * u_cap + 2LL * p_cap + (long long)p_cap * u_cap;
        const int nb = stride_blocks(body) < 512 ? stride_blocks(body) : 512;
        hipLaunchKernelGGL(k_ap_record_write, dim3(nb), dim3(TPB), 0, stream, (const int*)state, log, uid, gt_vert,
                           (const long long*)semantic_id, conf, inter, u_cap);
    }
    PBN_LAUNCH_CHECK();
    return PBN_OK;
}
