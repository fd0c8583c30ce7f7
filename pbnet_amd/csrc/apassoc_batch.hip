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
#include "post_dev.h"

namespace pbn {
namespace {

constexpr int TPB = 256;
constexpr int STRIDE_BLOCKS = 2048;                 // cap of every striding grid
constexpr int GT_ID_CAP_MAX = 1 << 20;              // direct table per scene, as pbn_gt_index_dev
constexpr int SCAN_IDS = 4;                         // ids per thread and trip of k_batch_scan
constexpr int OVERLAP_CHUNK = 2048;                 // folded points per workgroup of k_batch_overlap
constexpr int OVERLAP_LDS_COUNTERS = 8192;          // 32 KiB of counters per workgroup
constexpr int BODY_BLOCKS = 64;                     // blocks per scene of k_batch_body
constexpr int HDR = PBN_AP_RECORD_HEADER;
constexpr int ST_USED = 0, ST_WANTED = 1, ST_RECORDS = 2, ST_OVERFLOW = 3, ST_OFFSET = 4;
// per-scene words of the workspace's small block: n_gt | association status | n_keep (clamped) | offset of the record (-1 = not written)
constexpr int SC_NGT = 0, SC_STATUS = 1, SC_NKEEP = 2, SC_OFFSET = 3, SC_WORDS = 4;

__device__ __forceinline__ long long load_label(const void* p, int i64, long long i) {
    return i64 ? ((const long long*)p)[i] : (long long)((const int*)p)[i];
}

// the scene that owns folded point `pt` (0 <= pt < point_start[B]): the last j with point_start[j] <= pt, so an empty scene is
// stepped over (summary.hip)
__device__ __forceinline__ int scene_of_folded(const pbn_tta_table& U, int pt) {
    int s = 0;
#pragma unroll
    for (int j = 1; j < PBN_MAX_SCENES; ++j) s = (j < U.n_scenes && pt >= U.point_start[j]) ? j : s;
    return s;
}

__device__ __forceinline__ int start_of(const pbn_tta_table& U, int j) {
    int v = U.point_start[0];
#pragma unroll
    for (int k = 1; k <= PBN_MAX_SCENES; ++k) v = k == j ? U.point_start[k] : v;
    return v;
}

// one add per distinct bin of a wave (apassoc.hip): every lane of the wave must call this; bin < 0 takes no part
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
    const int n_total = start_of(U, U.n_scenes);
    for (int i = blockIdx.x * TPB + threadIdx.x; i < n_total; i += gridDim.x * TPB) {
        const long long inst = load_label(ins, ins_i64, i);
        if (inst < 0) continue;
        const int scene = scene_of_folded(U, i);
        if (inst >= n_inst_cap) { atomicOr(&scene_words[scene * SC_WORDS + SC_STATUS], PBN_AP_STATUS_INSTANCE_CAP); continue; }
        atomicMin(&first[(size_t)scene * n_inst_cap + inst], i - start_of(U, scene));
    }
}

__global__ __launch_bounds__(TPB) void k_batch_gt_code(const void* __restrict__ sem, int sem_i64, const void* __restrict__ ins,
                                                      int ins_i64, pbn_tta_table U, const int* __restrict__ label_table,
                                                      int n_labels, const int* __restrict__ first, int n_inst_cap,
                                                      int* __restrict__ ids, int* __restrict__ scene_words) {
    const int n_total = start_of(U, U.n_scenes);
    for (int i = blockIdx.x * TPB + threadIdx.x; i < n_total; i += gridDim.x * TPB) {
        const long long inst = load_label(ins, ins_i64, i);
        int code = 0;
        if (inst >= 0 && inst < n_inst_cap) {
            const int scene = scene_of_folded(U, i);
            const int p0 = start_of(U, scene), n_j = start_of(U, scene + 1) - p0;
            const int f = first[(size_t)scene * n_inst_cap + inst];          // <= i - p0: this very point took part in the minimum
            long long s = (f >= 0 && f < n_j) ? load_label(sem, sem_i64, (long long)p0 + f) : 0;
            if (s == -100) s = 0;
            if (s < 0 || s >= n_labels) atomicOr(&scene_words[scene * SC_WORDS + SC_STATUS], PBN_AP_STATUS_SEMANTIC_RANGE);
            else code = label_table[s] * 1000 + (int)inst + 1;
        }
        ids[i] = code;
    }
}

// ---- ground-truth numbering per scene: np.unique through one direct table per scene -------------------------------------
// table[scene][id] += 1 per point (the id's vertex count); B * id_cap <= 2^23, so the flat bin fits an int
__global__ __launch_bounds__(TPB) void k_batch_hist(const void* __restrict__ ids, int ids_i64, pbn_tta_table U, int id_cap,
                                                   int* __restrict__ table, int* __restrict__ scene_words) {
    const int n_total = start_of(U, U.n_scenes);
    for (int base = blockIdx.x * TPB; base < n_total; base += gridDim.x * TPB) {      // uniform per block: whole waves ballot
        const int i = base + threadIdx.x;
        int bin = -1;
        if (i < n_total) {
            const int scene = scene_of_folded(U, i);
            const long long id = load_label(ids, ids_i64, i);
            if (id < 0 || id >= id_cap) atomicOr(&scene_words[scene * SC_WORDS + SC_STATUS], PBN_AP_STATUS_ID_RANGE);
            else bin = scene * id_cap + (int)id;
        }
        wave_merged_add(table, bin);
    }
}

// k_gt_scan (apassoc.hip), one workgroup per scene: the scene's table walked in ascending id order, the ids with a count get
// consecutive slots (uid, gt_vert) and table[id] becomes the slot; an id past u_cap slots gets -1 and reports ID_COUNT
__global__ __launch_bounds__(TPB) void k_batch_scan(int* __restrict__ table_all, int id_cap, int* __restrict__ uid_all,
                                                   int* __restrict__ gt_vert_all, int u_cap, int* __restrict__ scene_words) {
    __shared__ int s_wave[TPB / 64];
    const int scene = blockIdx.x;
    int* table = table_all + (size_t)scene * id_cap;
    int* uid = uid_all + (size_t)scene * u_cap;
    int* gt_vert = gt_vert_all + (size_t)scene * u_cap;
    const int lane = lane_id(), wave = (int)(threadIdx.x >> 6);
    int base = 0;
    bool over = false;
    for (int t0 = 0; t0 < id_cap; t0 += TPB * SCAN_IDS) {                          // uniform trip count
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
        for (int w = 0; w < TPB / 64; ++w) {
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
                over = true;
            }
            ++pos;
        }
        base += all;
    }
    if (over) atomicOr(&scene_words[scene * SC_WORDS + SC_STATUS], PBN_AP_STATUS_ID_COUNT);
    if (threadIdx.x == 0) scene_words[scene * SC_WORDS + SC_NGT] = base < u_cap ? base : u_cap;
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
        const long long words = nk == 0 ? HDR : (long long)HDR + 2LL * ng + 2LL * nk + (long long)nk * ng;
        const int status = (post_scalars ? post_scalars[U.n_scenes + j] : 0) | sw[SC_STATUS];
        sw[SC_NKEEP] = nk;
        const long long wanted = (long long)state[ST_WANTED] + words;
        state[ST_WANTED] = wanted > 0x7fffffffLL ? 0x7fffffff : (int)wanted;
        const int used = state[ST_USED];
        if (state[ST_OVERFLOW] || used < 0 || (long long)used + words > (long long)log_words) {
            state[ST_OVERFLOW] = 1;                         // sticky: nothing is written after the first record that did not fit
            state[ST_OFFSET] = -1;
            sw[SC_OFFSET] = -1;
            continue;
        }
        int* rec = log + used;
        rec[0] = PBN_AP_RECORD_MAGIC;
        rec[1] = tags.tag[j];
        rec[2] = nk;
        rec[3] = ng;
        rec[4] = start_of(U, j + 1) - start_of(U, j);
        rec[5] = status;
        rec[6] = (int)words;
        rec[7] = 0;
        state[ST_USED] = used + (int)words;
        state[ST_RECORDS] += 1;
        state[ST_OFFSET] = used;
        sw[SC_OFFSET] = used;
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
    const long long a = ng, b = 2LL * ng, c = b + nk, d = c + nk, total = d + (long long)nk * ng;
    const long long step = (long long)gridDim.x * TPB;
    for (long long e = (long long)blockIdx.x * TPB + threadIdx.x; e < total; e += step) {
        int v = 0;
        if (e < a) v = uid[e];
        else if (e < b) v = gt_vert[e - a];
        else if (e < c) {
            const long long s = sid[e - b];
            v = (int)s;
            if (s != (long long)v) atomicOr(&rec[5], PBN_AP_STATUS_LABEL_RANGE);
        } else if (e < d) v = __float_as_int(cf[e - c]);
        rec[HDR + e] = v;
    }
}

// inter[label][slot of the point's id] += 1 straight into the records
__global__ __launch_bounds__(TPB) void k_batch_overlap(const int* __restrict__ point_instance, const void* __restrict__ ids,
                                                      int ids_i64, pbn_tta_table U, int id_cap, const int* __restrict__ table,
                                                      const int* __restrict__ scene_words, int* __restrict__ log) {
    __shared__ int s_cnt[OVERLAP_LDS_COUNTERS];
    const int n_total = start_of(U, U.n_scenes);
    const int lo = blockIdx.x * OVERLAP_CHUNK;
    const int hi = min(n_total, lo + OVERLAP_CHUNK);
    // the workgroup's own scene: that of its first point (uniform)
    const int scene0 = scene_of_folded(U, lo);
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
            const int scene = scene_of_folded(U, i);
            const int* sw = scene_words + scene * SC_WORDS;
            const int off = scene == scene0 ? off0 : sw[SC_OFFSET];
            const int nk = scene == scene0 ? nk0 : sw[SC_NKEEP];
            if (off >= 0 && label >= 0 && label < nk) {        // -100 and every other label outside [0, n_keep) count for nothing
                const long long id = load_label(ids, ids_i64, i);
                const int g = (id >= 0 && id < id_cap) ? table[(size_t)scene * id_cap + id] : -1;
                if (g >= 0) {
                    const int ng = scene == scene0 ? ng0 : sw[SC_NGT];
                    const int bin = label * ng + g;
                    if (lds && scene == scene0) atomicAdd(&s_cnt[bin], 1);
                    else direct = off + HDR + 2 * ng + 2 * nk + bin;
                }
            }
        }
        wave_merged_add(log, direct);
    }
    __syncthreads();
    if (!lds) return;                                          // uniform
    int* out = log + off0 + HDR + 2 * ng0 + 2 * nk0;
    for (int e = threadIdx.x; e < lds_words; e += TPB) {
        const int c = s_cnt[e];
        if (c) atomicAdd(&out[e], c);
    }
}

inline int stride_blocks(long long n) {
    const long long b = (n + TPB - 1) / TPB;
    return (int)(b < 1 ? 1 : (b > STRIDE_BLOCKS ? STRIDE_BLOCKS : b));
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
