// apassoc_batch.hip -- the AP association (apassoc.hip) for ALL scenes of one merged forward, on what the batched post-processing
// (post_batch.hip) leaves: one label per folded point instead of a dense [P, n] table.  After the superpoint vote the instances of
// a scene are disjoint, so the whole overlap table of a scene is ONE histogram over its points with the key
// (point_instance[i], gt_index[i]); the per-scene form walks the scene once per prediction.  The records go into the same epoch
// log, byte for byte what pbn_gt_[encode|index]_dev + pbn_instance_overlap_dev on the densified labels + pbn_ap_record_append
// write scene after scene.
//   * SIX launches whatever B is (EIGHT with the (sem, ins) form of the ground truth; the per-scene form takes 8 / 11 for ONE
//     scene): clear | [first | code] | histogram of the ids | numbering (one workgroup per scene) | reserve (one thread: the B
//     records' sizes, the log's state machine, the headers) | record bodies, overlap counters zeroed | overlap histogram.
//     With n_prop == 0 the last two are not needed and not launched: FOUR / SIX.
//   * no gt_index vector and no overlap table in the workspace: the overlap pass looks a point's id up in its scene's direct
//     table, and the counters are the inter[n_keep, n_gt] words of the record itself.  A record that did not fit has no counters
//     and its points are skipped;
//   * a workgroup walks OVERLAP_CHUNK consecutive folded points and keeps the counters of the scene of its first point in LDS when
//     n_keep * n_gt is at most OVERLAP_LDS_COUNTERS (pbn_ap_assoc_batch_lds_counters), flushing the non-zero ones once; lanes of
//     another scene (a chunk may straddle boundaries) and scenes above the bound add to the record directly, one add per distinct
//     counter of a wave;
//   * integer atomics only, so two runs give the same log bytes; nothing waits for the host, grids are sized by capacity.
#include "pbn_common.h"
#include "assoc_dev.h"

namespace pbn {
namespace {

constexpr int TPB = POST_TPB;
constexpr int OVERLAP_CHUNK = 2048;                 // folded points per workgroup of k_batch_overlap
constexpr int OVERLAP_LDS_COUNTERS = 8192;          // 32 KiB of counters per workgroup
constexpr int BODY_BLOCKS = 64;                     // blocks per scene of k_batch_body
// per-scene words of the workspace's small block: n_gt | association status | n_keep (clamped) | offset of the record (-1 = not written)
constexpr int SC_NGT = 0, SC_STATUS = 1, SC_NKEEP = 2, SC_OFFSET = 3, SC_WORDS = 4;

// tables cleared, `first` to "no point yet", the per-scene scalars to 0 / -1
__global__ __launch_bounds__(TPB) void k_batch_clear(int* __restrict__ table, long long n_table, int* __restrict__ first,
                                                    long long n_first, int* __restrict__ scene_words, int n_scenes) {
    const long long t = (long long)blockIdx.x * TPB + threadIdx.x, step = (long long)gridDim.x * TPB;
    for (long long e = t; e < n_table; e += step) table[e] = 0;
    for (long long e = t; e < n_first; e += step) first[e] = 0x7fffffff;
    if (t < (long long)n_scenes * SC_WORDS) scene_words[t] = (t % SC_WORDS) == SC_OFFSET ? -1 : 0;
}

// ---- ground-truth encoding per scene (get_val_gt.py:26-37, k_gt_first / k_gt_code of apassoc.hip with a scene axis) ----------
__global__ __launch_bounds__(TPB) void k_batch_gt_first(const void* __restrict__ ins, int ins_i64, pbn_tta_table U, int n_inst_cap,
                                                       int* __restrict__ first, int* __restrict__ scene_words) {
    const int n_total = start_of(U.point_start, U.n_scenes);
    for (int i = blockIdx.x * TPB + threadIdx.x; i < n_total; i += gridDim.x * TPB) {
        const long long inst = load_index(ins, ins_i64, i);
        if (inst < 0) continue;
        const int scene = scene_of_folded(U.point_start, U.n_scenes, i);
        if (inst >= n_inst_cap) { atomicOr(&scene_words[scene * SC_WORDS + SC_STATUS], PBN_AP_STATUS_INSTANCE_CAP); continue; }
        atomicMin(&first[(size_t)scene * n_inst_cap + inst], i - start_of(U.point_start, scene));
    }
}

__global__ __launch_bounds__(TPB) void k_batch_gt_code(const void* __restrict__ sem, int sem_i64, const void* __restrict__ ins,
                                                      int ins_i64, pbn_tta_table U, const int* __restrict__ label_table,
                                                      int n_labels, const int* __restrict__ first, int n_inst_cap,
                                                      int* __restrict__ ids, int* __restrict__ scene_words) {
    const int n_total = start_of(U.point_start, U.n_scenes);
    for (int i = blockIdx.x * TPB + threadIdx.x; i < n_total; i += gridDim.x * TPB) {
        const long long inst = load_index(ins, ins_i64, i);
        int code = 0;
        if (inst >= 0 && inst < n_inst_cap) {
            const int scene = scene_of_folded(U.point_start, U.n_scenes, i);
            const int p0 = start_of(U.point_start, scene), n_j = start_of(U.point_start, scene + 1) - p0;
            const int f = first[(size_t)scene * n_inst_cap + inst];          // <= i - p0: this very point took part in the minimum
            const GtCode g = gt_code((f >= 0 && f < n_j) ? load_index(sem, sem_i64, (long long)p0 + f) : 0, inst, label_table,
                                     n_labels);
            if (g.status) atomicOr(&scene_words[scene * SC_WORDS + SC_STATUS], g.status);
            code = g.code;
        }
        ids[i] = code;
    }
}

// ---- ground-truth numbering per scene: np.unique through one direct table per scene -------------------------------------
// table[scene][id] += 1 per point (the id's vertex count); B * id_cap <= 2^23, so the flat bin fits an int
__global__ __launch_bounds__(TPB) void k_batch_hist(const void* __restrict__ ids, int ids_i64, pbn_tta_table U, int id_cap,
                                                   int* __restrict__ table, int* __restrict__ scene_words) {
    const int n_total = start_of(U.point_start, U.n_scenes);
    for (int base = blockIdx.x * TPB; base < n_total; base += gridDim.x * TPB) {      // uniform per block: whole waves ballot
        const int i = base + threadIdx.x;
        int bin = -1;
        if (i < n_total) {
            const int scene = scene_of_folded(U.point_start, U.n_scenes, i);
            const long long id = load_index(ids, ids_i64, i);
            if (id < 0 || id >= id_cap) atomicOr(&scene_words[scene * SC_WORDS + SC_STATUS], PBN_AP_STATUS_ID_RANGE);
            else bin = scene * id_cap + (int)id;
        }
        wave_merged_add(table, bin);
    }
}

// k_gt_scan (apassoc.hip), one workgroup per scene: gt_number_scan over the scene's table; an id past u_cap slots reports ID_COUNT
__global__ __launch_bounds__(TPB) void k_batch_scan(int* __restrict__ table_all, int id_cap, int* __restrict__ uid_all,
                                                   int* __restrict__ gt_vert_all, int u_cap, int* __restrict__ scene_words) {
    __shared__ int s_wave[TPB / 64];
    const int scene = blockIdx.x;
    bool over = false;
    const int live = gt_number_scan(table_all + (size_t)scene * id_cap, id_cap, uid_all + (size_t)scene * u_cap,
                                    gt_vert_all + (size_t)scene * u_cap, u_cap, s_wave, &over);
    if (over) atomicOr(&scene_words[scene * SC_WORDS + SC_STATUS], PBN_AP_STATUS_ID_COUNT);
    if (threadIdx.x == 0) scene_words[scene * SC_WORDS + SC_NGT] = live;
}

// ---- the B records: k_ap_record_reserve (apassoc.hip) for scene 0 .. B - 1 in order, by one thread ------------------------
__global__ __launch_bounds__(64) void k_batch_reserve(int* __restrict__ state, int* __restrict__ log, int log_words,
                                                     pbn_ap_scene_tags tags, pbn_tta_table U,
                                                     const int* __restrict__ post_scalars, int n_prop,
                                                     int* __restrict__ scene_words) {
    if (threadIdx.x != 0) return;
    int kept_sum = 0;
#pragma unroll 1
    for (int j = 0; j < U.n_scenes; ++j) {
        int* sw = scene_words + j * SC_WORDS;
        // n_keep clamped as pbn_scene_summary does: the scenes' counts sum to at most P
        const int nk = post_scalars && n_prop > 0 ? max(0, min(post_scalars[j], n_prop - kept_sum)) : 0;
        kept_sum += nk;
        const int ng = sw[SC_NGT];
        const int status = (post_scalars ? post_scalars[U.n_scenes + j] : 0) | sw[SC_STATUS];
        sw[SC_NKEEP] = nk;
        sw[SC_OFFSET] = ap_record_reserve(state, log, log_words, tags.tag[j], nk, ng,
                                          start_of(U.point_start, j + 1) - start_of(U.point_start, j), status);
    }
}

// body of scene blockIdx.y's record: uid | gt_vert | label_id | conf bits, and the overlap counters zeroed
__global__ __launch_bounds__(TPB) void k_batch_body(int* __restrict__ log, const int* __restrict__ scene_words,
                                                   const int* __restrict__ uid_all, const int* __restrict__ gt_vert_all, int u_cap,
                                                   const long long* __restrict__ semantic_id, const float* __restrict__ conf,
                                                   int n_prop) {
    const int scene = blockIdx.y;
    const int* sw = scene_words + scene * SC_WORDS;
    const int off = sw[SC_OFFSET], nk = sw[SC_NKEEP], ng = sw[SC_NGT];
    if (off < 0 || nk == 0) return;
    int* rec = log + off;
    const int* uid = uid_all + (size_t)scene * u_cap;
    const int* gt_vert = gt_vert_all + (size_t)scene * u_cap;
    const long long* sid = semantic_id + (size_t)scene * n_prop;
    const float* cf = conf + (size_t)scene * n_prop;
    const long long head = 2LL * ng + 2LL * nk, total = head + (long long)nk * ng;
    const long long step = (long long)gridDim.x * TPB;
    for (long long e = (long long)blockIdx.x * TPB + threadIdx.x; e < total; e += step)
        rec[AP_HDR + e] = e < head ? ap_record_head_word(e, nk, ng, rec, uid, gt_vert, sid, cf) : 0;
}

// inter[label][slot of the point's id] += 1 straight into the records
__global__ __launch_bounds__(TPB) void k_batch_overlap(const int* __restrict__ point_instance, const void* __restrict__ ids,
                                                      int ids_i64, pbn_tta_table U, int id_cap, const int* __restrict__ table,
                                                      const int* __restrict__ scene_words, int* __restrict__ log) {
    __shared__ int s_cnt[OVERLAP_LDS_COUNTERS];
    const int n_total = start_of(U.point_start, U.n_scenes);
    const int lo = blockIdx.x * OVERLAP_CHUNK;
    const int hi = min(n_total, lo + OVERLAP_CHUNK);
    // the workgroup's own scene: that of its first point (uniform)
    const int scene0 = scene_of_folded(U.point_start, U.n_scenes, lo);
    const int off0 = scene_words[scene0 * SC_WORDS + SC_OFFSET];
    const int nk0 = scene_words[scene0 * SC_WORDS + SC_NKEEP], ng0 = scene_words[scene0 * SC_WORDS + SC_NGT];
    const long long cnt0 = off0 >= 0 ? (long long)nk0 * ng0 : 0;
    const bool lds = cnt0 > 0 && cnt0 <= OVERLAP_LDS_COUNTERS;
    const int lds_words = lds ? (int)cnt0 : 0;
    for (int e = threadIdx.x; e < lds_words; e += TPB) s_cnt[e] = 0;
    __syncthreads();
    for (int base = lo; base < hi; base += TPB) {              // uniform trip count: the ballots need whole waves
        const int i = base + threadIdx.x;
        int direct = -1;                                       // word of the log this lane adds to directly
        if (i < hi) {
            const int label = point_instance[i];
            const int scene = scene_of_folded(U.point_start, U.n_scenes, i);
            const int* sw = scene_words + scene * SC_WORDS;
            const int off = scene == scene0 ? off0 : sw[SC_OFFSET];
            const int nk = scene == scene0 ? nk0 : sw[SC_NKEEP];
            if (off >= 0 && label >= 0 && label < nk) {        // -100 and every other label outside [0, n_keep) count for nothing
                const long long id = load_index(ids, ids_i64, i);
                const int g = (id >= 0 && id < id_cap) ? table[(size_t)scene * id_cap + id] : -1;
                if (g >= 0) {
                    const int ng = scene == scene0 ? ng0 : sw[SC_NGT];
                    const int bin = label * ng + g;
                    if (lds && scene == scene0) atomicAdd(&s_cnt[bin], 1);
                    else direct = off + AP_HDR + 2 * ng + 2 * nk + bin;
                }
            }
        }
        wave_merged_add(log, direct);
    }
    __syncthreads();
    if (!lds) return;                                          // uniform
    int* out = log + off0 + AP_HDR + 2 * ng0 + 2 * nk0;
    for (int e = threadIdx.x; e < lds_words; e += TPB) {
        const int c = s_cnt[e];
        if (c) atomicAdd(&out[e], c);
    }
}

struct BatchCarve {
    int *table, *first, *ids, *uid, *gt_vert, *scene_words;
    size_t bytes;
    bool ok;
};

BatchCarve carve(void* ws, size_t ws_bytes, int n_points_total, int n_scenes, int u_cap, int id_cap, int n_inst_cap) {
    Carver c(ws, ws_bytes);
    BatchCarve r;
    r.table = c.take<int>((size_t)n_scenes * id_cap);
    r.first = c.take<int>((size_t)n_scenes * n_inst_cap);
    r.ids = c.take<int>(n_inst_cap > 0 ? (size_t)n_points_total : 0);
    r.uid = c.take<int>((size_t)n_scenes * u_cap);
    r.gt_vert = c.take<int>((size_t)n_scenes * u_cap);
    r.scene_words = c.take<int>((size_t)PBN_MAX_SCENES * SC_WORDS);
    r.bytes = align_up(c.off, 256);
    r.ok = c.ok;
    return r;
}

bool batch_sizes_ok(int n_points_total, int n_scenes, int u_cap, int id_cap, int n_inst_cap) {
    return n_points_total >= 0 && n_scenes >= 1 && n_scenes <= PBN_MAX_SCENES && u_cap >= 1 && id_cap >= 1 &&
           id_cap <= GT_ID_CAP_MAX && n_inst_cap >= 0;
}

}  // namespace
}  // namespace pbn

using namespace pbn;

extern "C" size_t pbn_ap_assoc_batch_workspace_bytes(int n_points_total, int n_scenes, int u_cap, int id_cap, int n_inst_cap) {
    if (!batch_sizes_ok(n_points_total, n_scenes, u_cap, id_cap, n_inst_cap)) return 0;
    return carve(nullptr, 0, n_points_total, n_scenes, u_cap, id_cap, n_inst_cap).bytes;
}

extern "C" int pbn_ap_assoc_batch_lds_counters(void) { return OVERLAP_LDS_COUNTERS; }

extern "C" int pbn_ap_assoc_batch(pbn_tta_table units, const int32_t* point_instance, const int32_t* post_scalars,
                                  const float* scores, const int64_t* semantic_id, int n_prop, const void* ids, int ids_i64,
                                  const void* sem, int sem_i64, const void* ins, int ins_i64, const int32_t* label_table,
                                  int n_labels, int u_cap, int id_cap, int n_inst_cap, pbn_ap_scene_tags tags, int32_t* state,
                                  int32_t* log, int64_t log_words, void* workspace, size_t workspace_bytes,
                                  pbn_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    const int B = units.n_scenes, copies = units.copies;
    if (B < 1 || B > PBN_MAX_SCENES || copies < 1 || (long long)B * copies > PBN_MAX_SCENES) return PBN_ERR_ARG;
    if (units.point_start[0] != 0 || units.sp_start[0] != 0) return PBN_ERR_ARG;
    for (int j = 0; j < B; ++j)
        if (units.point_start[j + 1] < units.point_start[j] || units.sp_start[j + 1] < units.sp_start[j]) return PBN_ERR_ARG;
    if (n_prop < 0 || u_cap < 1 || id_cap < 1 || log_words < 0) return PBN_ERR_ARG;
    const int n_total = units.point_start[B];
    const bool encode = ids == nullptr;
    if (encode && n_total > 0 && (!sem || !ins)) return PBN_ERR_ARG;          // neither form of the ground truth
    if (encode && (!label_table || n_labels < 1 || n_inst_cap < 1)) return PBN_ERR_ARG;
    if (!state || !workspace || (log_words > 0 && !log)) return PBN_ERR_ARG;
    if (n_prop > 0 && (!point_instance || !post_scalars || !scores || !semantic_id)) return PBN_ERR_ARG;
    if (n_prop > POST_MAX_PROPOSALS || id_cap > GT_ID_CAP_MAX) return PBN_ERR_UNSUPPORTED;
    if (log_words > 0x7fffffffLL) return PBN_ERR_RANGE;
    const int inst_cap = encode ? n_inst_cap : 0;
    const BatchCarve w = carve(workspace, workspace_bytes, n_total, B, u_cap, id_cap, inst_cap);
    if (!w.ok) return PBN_ERR_WORKSPACE;

    const long long n_table = (long long)B * id_cap, n_first = (long long)B * inst_cap;
    hipLaunchKernelGGL(k_batch_clear, dim3(stride_blocks(n_table > n_first ? n_table : n_first)), dim3(TPB), 0, stream, w.table,
                       n_table, w.first, n_first, w.scene_words, B);
    const void* id_src = ids;
    int id_i64 = ids_i64;
    if (n_total > 0) {
        const int nb = stride_blocks(n_total);
        if (encode) {
            hipLaunchKernelGGL(k_batch_gt_first, dim3(nb), dim3(TPB), 0, stream, ins, ins_i64, units, inst_cap, w.first,
                               w.scene_words);
            hipLaunchKernelGGL(k_batch_gt_code, dim3(nb), dim3(TPB), 0, stream, sem, sem_i64, ins, ins_i64, units, label_table,
                               n_labels, (const int*)w.first, inst_cap, w.ids, w.scene_words);
            id_src = w.ids;
            id_i64 = 0;
        }
        hipLaunchKernelGGL(k_batch_hist, dim3(nb), dim3(TPB), 0, stream, id_src, id_i64, units, id_cap, w.table, w.scene_words);
    }
    hipLaunchKernelGGL(k_batch_scan, dim3(B), dim3(TPB), 0, stream, w.table, id_cap, w.uid, w.gt_vert, u_cap, w.scene_words);
    hipLaunchKernelGGL(k_batch_reserve, dim3(1), dim3(64), 0, stream, state, log, (int)log_words, tags, units, post_scalars, n_prop,
                       w.scene_words);
    if (n_prop > 0) {
        hipLaunchKernelGGL(k_batch_body, dim3(BODY_BLOCKS, B), dim3(TPB), 0, stream, log, (const int*)w.scene_words,
                           (const int*)w.uid, (const int*)w.gt_vert, u_cap, (const long long*)semantic_id, scores, n_prop);
        if (n_total > 0)
            hipLaunchKernelGGL(k_batch_overlap, dim3(cdiv(n_total, OVERLAP_CHUNK)), dim3(TPB), 0, stream, point_instance, id_src,
                               id_i64, units, id_cap, (const int*)w.table, (const int*)w.scene_words, log);
    }
    PBN_LAUNCH_CHECK();
    return PBN_OK;
}
