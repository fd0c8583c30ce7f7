// post_batch.hip -- the post-processing of post.hip's device-resident form for ALL scenes of one merged forward
// (pbnet_amd/serving.py): the same per-scene arithmetic with a scene axis and no dense [P, n] table.  pbn_post_batch has no TTA
// fold; pbn_post_batch_tta folds the `copies` copies of every scene onto one, and is the same thirteen launches: the scene table
// and every working table are over FOLDED points, and only three kernels see unfolded numbering (k_pb_scene_of, k_pb_set_bits,
// the first-member class lookup of k_pb_compact) -- through fold_of_point, of which copies = 1 is pbn_post_batch.
//   * the scene table (point ranges and vote-table ranges of the B <= PBN_MAX_SCENES scenes) is a launch argument, by value;
//   * a proposal belongs to the scene of its first member; its bitset is over point - point_start[scene], row pitch = words of
//     the largest scene;
//   * the per-scene lists (survivors, picks, renumbering) are rows of [B, P] tables, the live counts n_rows[B], n_pick[B],
//     n_keep[B] device scalars; the per-scene steps run one workgroup per scene (grid = B), the rest over capacities;
//   * the masks leave as one label per point (point_instance), so the rebuilt bitsets and the dense table are never made: the
//     size of a rebuilt cluster is counted from the refined labels (integer adds, which commute).
// Every result is the same on every run: the only atomics are integer OR / ADD.
#include <hip/hip_bf16.h>
#include <hip/hip_fp16.h>
#include "pbn_common.h"
#include "post_dev.h"

namespace pbn {
namespace {

constexpr int TPB = POST_TPB;
constexpr int NO_LABEL = -100;

struct SceneRef { int scene, point_base, sp_base, sp_cap; };

// the scene that owns merged point `pt` (-1: none): the last j with point_start[j] <= pt -- B + 1 comparisons
__device__ __forceinline__ SceneRef scene_of_point(const pbn_scene_table& T, long long pt) {
    SceneRef r{0, T.point_start[0], T.sp_start[0], T.sp_start[1] - T.sp_start[0]};
#pragma unroll
    for (int j = 1; j < PBN_MAX_SCENES; ++j)
        if (j < T.n_scenes && pt >= T.point_start[j]) r = SceneRef{j, T.point_start[j], T.sp_start[j], T.sp_start[j + 1] - T.sp_start[j]};
    if (pt < T.point_start[0] || pt >= start_of(T.point_start, T.n_scenes)) r.scene = -1;
    return r;
}

struct FoldRef { int scene, local; };

// merged UNFOLDED point `pt` -> (scene, folded scene-local point).  Scene j's `copies` copies lie one after the other in
// copies * point_start[j] .. copies * point_start[j + 1]; the fold is (pt - copies * point_start[j]) % n_j, taken with copies - 1
// conditional subtractions (no division).  scene -1: the point lies in no scene.  copies = 1: scene_of_point and pt - point_base.
__device__ __forceinline__ FoldRef fold_of_point(const pbn_scene_table& T, int copies, long long pt) {
    int scene = 0, base = T.point_start[0], n = T.point_start[1] - T.point_start[0];
#pragma unroll
    for (int j = 1; j < PBN_MAX_SCENES; ++j)
        if (j < T.n_scenes && pt >= (long long)copies * T.point_start[j]) {
            scene = j;
            base = T.point_start[j];
            n = T.point_start[j + 1] - T.point_start[j];
        }
    if (pt < (long long)copies * T.point_start[0] || pt >= (long long)copies * start_of(T.point_start, T.n_scenes))
        return FoldRef{-1, 0};
    int local = (int)(pt - (long long)copies * base);              // < copies * n_j <= the merged point count: an int
    for (int c = 1; c < copies; ++c) local -= local >= n ? n : 0;
    return FoldRef{scene, local};
}

// the scene whose vote slice holds table row `row` (0 <= row < sp_start[B]); slices of capacity 0 are stepped over
__device__ __forceinline__ int scene_of_vote_row(const pbn_scene_table& T, int row) {
    return scene_of_folded(T.sp_start, T.n_scenes, row);
}

// prop_scene[p] = scene of the first member, in unfolded numbering (-1: no first member, or it lies in no scene); score[p] = clt_score[p] as fp32
__global__ __launch_bounds__(TPB) void k_pb_scene_of(const long long* __restrict__ proposals_idx, int n_entries,
                                                    const void* __restrict__ offsets, int offsets_i64, int n_prop,
                                                    const void* __restrict__ clt_score, int score_dtype, pbn_scene_table T,
                                                    int copies, int* __restrict__ prop_scene, float* __restrict__ score) {
    const int p = blockIdx.x * TPB + threadIdx.x;
    if (p >= n_prop) return;
    const long long e0 = load_index(offsets, offsets_i64, p), e1 = load_index(offsets, offsets_i64, p + 1);
    int scene = -1;
    if (e0 >= 0 && e0 < e1 && e1 <= n_entries) scene = fold_of_point(T, copies, proposals_idx[2 * e0 + 1]).scene;
    prop_scene[p] = scene;
    score[p] = score_dtype == PBN_F32    ? ((const float*)clt_score)[p]
               : score_dtype == PBN_BF16 ? __bfloat162float(((const __hip_bfloat16*)clt_score)[p])
                                         : __half2float(((const __half*)clt_score)[p]);
}

// bit (folded scene-local point) of row proposal: a member in another copy of the proposal's scene folds onto the same bits
// (eval_map.py:67); a member outside its proposal's scene is dropped
__global__ __launch_bounds__(TPB) void k_pb_set_bits(const long long* __restrict__ proposals_idx, int n_entries, int n_prop,
                                                    const int* __restrict__ prop_scene, pbn_scene_table T, int copies, int pitch,
                                                    unsigned* __restrict__ masks) {
    const int e = blockIdx.x * TPB + threadIdx.x;
    if (e >= n_entries) return;
    const long long p = proposals_idx[2 * (size_t)e + 0];
    if (p < 0 || p >= n_prop) return;
    const int scene = prop_scene[p];
    const FoldRef r = fold_of_point(T, copies, proposals_idx[2 * (size_t)e + 1]);
    if (scene < 0 || r.scene != scene) return;
    atomicOr(&masks[(size_t)p * pitch + (r.local >> 5)], 1u << (r.local & 31));
}

// counts[p] = popcount of row p (one wave per row)
__global__ __launch_bounds__(64) void k_pb_popcount(const unsigned* __restrict__ masks, int pitch, int* __restrict__ counts) {
    const unsigned* row = masks + (size_t)blockIdx.x * pitch;
    int c = 0;
    for (int w = threadIdx.x; w < pitch; w += 64) c += __popc(row[w]);
    c = wave_reduce_add(c);
    if (threadIdx.x == 0) counts[blockIdx.x] = c;
}

// k_post_select per scene (workgroup = scene): rows[scene, :] = that scene's proposals with score > score_t (fp32) and
// count > npoint_t, ascending in the merged numbering, tail -1; n_rows[scene]; the scene's status word is cleared here
__global__ __launch_bounds__(TPB) void k_pb_select(const float* __restrict__ score, const int* __restrict__ counts,
                                                  const int* __restrict__ prop_scene, int n_prop, float score_t, int npoint_t,
                                                  int* __restrict__ rows, int* __restrict__ n_rows, int* __restrict__ status) {
    __shared__ int s_wave[TPB / 64];
    const int scene = blockIdx.x;
    int* out = rows + (size_t)scene * n_prop;
    int base = 0;
    for (int p0 = 0; p0 < n_prop; p0 += TPB) {     // uniform trip count: the scan needs whole blocks
        const int p = p0 + threadIdx.x;
        const bool flag = p < n_prop && prop_scene[p] == scene && score[p] > score_t && counts[p] > npoint_t;
        int total;
        const int pos = block_flag_scan(flag, s_wave, &total);
        if (flag) out[base + pos] = p;
        base += total;
    }
    for (int p = base + threadIdx.x; p < n_prop; p += TPB) out[p] = -1;
    if (threadIdx.x == 0) { n_rows[scene] = base; status[scene] = 0; }
}

// k_mask_iou_dev over the pairs WITHIN a scene: a fixed grid of one-wave workgroups strides over sum_j n_rows[j]^2 live pairs.
// Scene j's block of the [P, P] table starts at row sum(n_rows[:j]) (the scenes' survivors are disjoint, so the rows fit).
__global__ __launch_bounds__(64) void k_pb_iou(const unsigned* __restrict__ masks, const int* __restrict__ rows,
                                              const int* __restrict__ n_rows_dev, int n_scenes, int cap, int pitch,
                                              const int* __restrict__ counts, float* __restrict__ iou) {
    int nr[PBN_MAX_SCENES];
    int n_pairs = 0, n_sum = 0;
#pragma unroll
    for (int j = 0; j < PBN_MAX_SCENES; ++j) {
        nr[j] = j < n_scenes ? max(0, min(n_rows_dev[j], cap - n_sum)) : 0;
        n_sum += nr[j];
        n_pairs += nr[j] * nr[j];                  // sum n_j <= cap <= 4096: fits
    }
    for (int e = blockIdx.x; e < n_pairs; e += gridDim.x) {      // uniform per wave: one pair per wave and trip
        int scene = 0, n = 1, local = 0, row_base = 0, lo = 0, rb = 0;
#pragma unroll
        for (int j = 0; j < PBN_MAX_SCENES; ++j) {
            const int sq = nr[j] * nr[j];
            if (e >= lo && e < lo + sq) { scene = j; n = nr[j]; local = e - lo; row_base = rb; }
            lo += sq;
            rb += nr[j];
        }
        const int i = local / n, k = local - i * n;
        const int ri = rows[(size_t)scene * cap + i], rk = rows[(size_t)scene * cap + k];
        if (ri < 0 || ri >= cap || rk < 0 || rk >= cap) continue;
        const int c = mask_pair_intersection(masks + (size_t)ri * pitch, masks + (size_t)rk * pitch, pitch);
        if (threadIdx.x == 0) iou[(size_t)(row_base + i) * cap + k] = mask_pair_iou(c, counts[ri], counts[rk]);
    }
}

// k_post_nms per scene (workgroup = scene): nms_walk (post_dev.h) over the scene's own survivor list and its block of the IoU
// table.  pick_rows[scene, :] = the picked proposals in pick order, tail -1; n_pick[scene]
__global__ __launch_bounds__(TPB) void k_pb_nms(const float* __restrict__ score, const int* __restrict__ rows,
                                               const int* __restrict__ n_rows_dev, int cap, const float* __restrict__ iou,
                                               float nms_t, int* __restrict__ pick_rows, int* __restrict__ n_pick_dev) {
    __shared__ float s_score[POST_MAX_PROPOSALS];
    __shared__ unsigned short s_order[POST_MAX_PROPOSALS];
    __shared__ unsigned char s_supp[POST_MAX_PROPOSALS];
    const int scene = blockIdx.x;
    int row_base = 0;
    for (int j = 0; j < scene; ++j) row_base += max(0, min(n_rows_dev[j], cap - row_base));
    const int n = max(0, min(n_rows_dev[scene], cap - row_base));
    const int n_pick = nms_walk(s_score, s_order, s_supp, score, rows + (size_t)scene * cap, n, cap, iou + (size_t)row_base * cap,
                                nms_t, nullptr, pick_rows + (size_t)scene * cap);
    if (threadIdx.x == 0) n_pick_dev[scene] = n_pick;
}

// zero what the vote and the size count accumulate into: columns [0, n_pick[j]] of every row of scene j's vote slice, and counts2
__global__ __launch_bounds__(TPB) void k_pb_clear(const int* __restrict__ n_pick_dev, int cap, pbn_scene_table T,
                                                 int* __restrict__ votes, int* __restrict__ counts2) {
    const long long first = (long long)blockIdx.x * TPB + threadIdx.x, step = (long long)gridDim.x * TPB;
#pragma unroll
    for (int j = 0; j < PBN_MAX_SCENES; ++j) {
        if (j >= T.n_scenes) continue;
        const int cols = min(max(n_pick_dev[j], 0), cap) + 1;
        const long long n_hist = (long long)(T.sp_start[j + 1] - T.sp_start[j]) * cols;
        for (long long e = first; e < n_hist; e += step) {
            const long long sp = e / cols;
            votes[(size_t)(T.sp_start[j] + sp) * (cap + 1) + (e - sp * cols)] = 0;
        }
    }
    for (long long e = first; e < (long long)T.n_scenes * cap; e += step) counts2[e] = 0;
}

// k_point_labels_dev + k_sp_hist_dev per scene: seg[pt] = the LAST pick of the point's scene that contains it, else -100; in a
// scene with superpoints the label votes in row sp_start[scene] + id of the flat table (bucket n_pick = unlabelled).  An id >=
// the scene's capacity sets that scene's superpoint bit and writes nothing; a negative id takes no part.
__global__ __launch_bounds__(TPB) void k_pb_paint_vote(const unsigned* __restrict__ masks, const int* __restrict__ pick_rows,
                                                      const int* __restrict__ n_pick_dev, int cap, int pitch, int n_points,
                                                      pbn_scene_table T, const long long* __restrict__ superpoint,
                                                      int* __restrict__ seg, int* __restrict__ votes, int* __restrict__ status) {
    const int pt = blockIdx.x * TPB + threadIdx.x;
    if (pt >= n_points) return;
    const SceneRef r = scene_of_point(T, pt);
    if (r.scene < 0) { seg[pt] = NO_LABEL; return; }
    const int n_pick = min(max(n_pick_dev[r.scene], 0), cap);
    const int local = pt - r.point_base;
    const int* my_pick = pick_rows + (size_t)r.scene * cap;
    int lab = NO_LABEL;
    for (int c = n_pick - 1; c >= 0; --c) {
        const int row = my_pick[c];
        if (row >= 0 && row < cap && ((masks[(size_t)row * pitch + (local >> 5)] >> (local & 31)) & 1u)) { lab = c; break; }
    }
    seg[pt] = lab;
    if (r.sp_cap <= 0) return;
    const long long sp = superpoint[pt];
    if (sp >= r.sp_cap) { atomicOr(&status[r.scene], POST_STATUS_SUPERPOINT); return; }
    if (sp < 0) return;
    atomicAdd(&votes[(size_t)(r.sp_base + sp) * (cap + 1) + (lab < 0 ? n_pick : lab)], 1);
}

// k_sp_argmax_dev over the flat table: first arg-max bucket of the row among [0, n_pick of the row's scene], bucket n_pick -> -100
__global__ __launch_bounds__(TPB) void k_pb_sp_argmax(const int* __restrict__ votes, int n_sp_total, const int* __restrict__ n_pick_dev,
                                                     int cap, pbn_scene_table T, int* __restrict__ sp_label) {
    const int row = blockIdx.x * TPB + threadIdx.x;
    if (row >= n_sp_total) return;
    const int n_label = min(max(n_pick_dev[scene_of_vote_row(T, row)], 0), cap);
    const int* h = votes + (size_t)row * (cap + 1);
    int best = h[0], arg = 0;
    for (int l = 1; l <= n_label; ++l)
        if (h[l] > best) { best = h[l]; arg = l; }
    sp_label[row] = arg == n_label ? NO_LABEL : arg;
}

// seg_refined[pt] = label of the point's superpoint (a scene without superpoints: the painted label itself, i.e. every point
// its own superpoint); counts2[scene, label] = points that carry the label -- the size of the rebuilt cluster.  Neighbouring
// points mostly share a label, so a wave merges equal bins before it adds.
__global__ __launch_bounds__(TPB) void k_pb_relabel(const int* __restrict__ sp_label, const long long* __restrict__ superpoint,
                                                   const int* __restrict__ seg, const int* __restrict__ n_pick_dev, int cap,
                                                   int n_points, pbn_scene_table T, int* __restrict__ seg_refined,
                                                   int* __restrict__ counts2) {
    const long long pt = (long long)blockIdx.x * TPB + threadIdx.x;
    int bin = -1;
    if (pt < n_points) {
        const SceneRef r = scene_of_point(T, pt);
        int l = NO_LABEL;
        if (r.scene >= 0) {
            if (r.sp_cap > 0) {
                const long long sp = superpoint[pt];
                if (sp >= 0 && sp < r.sp_cap) l = sp_label[r.sp_base + sp];
            } else {
                l = seg[pt];
            }
            if (l >= 0 && l < min(max(n_pick_dev[r.scene], 0), cap)) bin = r.scene * cap + l;
            else l = NO_LABEL;
        }
        seg_refined[pt] = l;
    }
    wave_merged_add(counts2, bin);                 // uniform: every lane of the wave is here
}

// k_post_compact per scene (workgroup = scene): the picks that still own a point, in pick order, renumbered from 0
// (renumber[scene, pick] = new number or -1); per kept instance its score, the class of the proposal's first member through the
// label table and its point count; tails: score 0, class -1, count 0; n_keep[scene].  The first member is looked up UNFOLDED
// (eval_map.py:64 reads the class before the fold): pred_sem holds n_points = copies * (folded points) labels
__global__ __launch_bounds__(TPB) void k_pb_compact(const int* __restrict__ counts2, const int* __restrict__ pick_rows,
                                                   const int* __restrict__ n_pick_dev, int cap, const float* __restrict__ score,
                                                   const long long* __restrict__ proposals_idx, int n_entries,
                                                   const void* __restrict__ offsets, int offsets_i64,
                                                   const void* __restrict__ pred_sem, int sem_i64, int n_points,
                                                   const long long* __restrict__ label_table, int n_labels,
                                                   int* __restrict__ renumber, float* __restrict__ scores_out,
                                                   long long* __restrict__ sem_out, int* __restrict__ npoints_out,
                                                   int* __restrict__ n_keep_dev, int* __restrict__ status) {
    __shared__ int s_wave[TPB / 64];
    const int scene = blockIdx.x;
    const size_t at = (size_t)scene * cap;
    const int n_pick = min(max(n_pick_dev[scene], 0), cap);
    int base = 0;
    for (int c0 = 0; c0 < n_pick; c0 += TPB) {
        const int c = c0 + threadIdx.x;
        const bool flag = c < n_pick && counts2[at + c] > 0;
        int total;
        const int pos = block_flag_scan(flag, s_wave, &total);
        if (c < n_pick) renumber[at + c] = flag ? base + pos : -1;
        if (flag) {
            const int p = pick_rows[at + c];
            long long cls = -1;
            float sc = 0.f;
            if (p >= 0 && p < cap) {
                sc = score[p];
                cls = first_member_class(proposals_idx, n_entries, offsets, offsets_i64, p, pred_sem, sem_i64, n_points, label_table,
                                         n_labels);
            }
            if (cls < 0) atomicOr(&status[scene], POST_STATUS_CLASS);
            scores_out[at + base + pos] = sc;
            sem_out[at + base + pos] = cls;
            npoints_out[at + base + pos] = counts2[at + c];
        }
        base += total;
    }
    for (int k = base + threadIdx.x; k < cap; k += TPB) {
        scores_out[at + k] = 0.f;
        sem_out[at + k] = -1;
        npoints_out[at + k] = 0;
    }
    if (threadIdx.x == 0) n_keep_dev[scene] = base;
}

// point_instance[pt] = the kept-instance number of the point's refined label inside its scene, else -100
__global__ __launch_bounds__(TPB) void k_pb_point_instance(const int* __restrict__ seg_refined, const int* __restrict__ renumber,
                                                          int cap, int n_points, pbn_scene_table T,
                                                          int* __restrict__ point_instance) {
    const int pt = blockIdx.x * TPB + threadIdx.x;
    if (pt >= n_points) return;
    const int l = seg_refined[pt];
    const int scene = scene_of_point(T, pt).scene;
    int v = NO_LABEL;
    if (scene >= 0 && l >= 0 && l < cap) {
        const int k = renumber[(size_t)scene * cap + l];
        if (k >= 0) v = k;
    }
    point_instance[pt] = v;
}

// a merged forward without proposals: every point unlabelled, n_keep and status 0
__global__ __launch_bounds__(TPB) void k_pb_empty(int n_points, int n_scalars, int* __restrict__ point_instance,
                                                 int* __restrict__ scalars) {
    const int step = gridDim.x * TPB;
    for (int pt = blockIdx.x * TPB + threadIdx.x; pt < n_points; pt += step) point_instance[pt] = NO_LABEL;
    if (blockIdx.x == 0 && (int)threadIdx.x < n_scalars) scalars[threadIdx.x] = 0;
}

bool sizes_ok(int n_prop, int n_points_total, int n_scenes, int n_sp_total) {
    return n_prop >= 0 && n_prop <= POST_MAX_PROPOSALS && n_points_total >= 1 && n_scenes >= 1 && n_scenes <= PBN_MAX_SCENES &&
           n_sp_total >= 0;
}

void lay_out(int n_prop, int n_points_total, int n_scenes, int n_sp_total, pbn_post_batch_layout* L) {
    const size_t p = (size_t)n_prop, n = (size_t)n_points_total, b = (size_t)n_scenes;
    size_t off = 0;
    auto take = [&off](size_t bytes) { const size_t at = align_up(off, 256); off = at + bytes; return (int64_t)at; };
    L->masks = take(4 * p * (size_t)pbn_post_words(n_points_total));
    L->counts = take(4 * p);
    L->prop_scene = take(4 * p);
    L->score = take(4 * p);
    L->rows = take(4 * b * p);
    L->pick_rows = take(4 * b * p);
    L->n_rows = take(4 * PBN_MAX_SCENES);
    L->n_pick = take(4 * PBN_MAX_SCENES);
    L->iou = take(4 * p * p);
    L->votes = take(4 * (size_t)n_sp_total * (p + 1));
    L->sp_label = take(4 * (size_t)n_sp_total);
    L->seg = take(4 * n);
    L->seg_refined = take(4 * n);
    L->counts2 = take(4 * b * p);
    L->renumber = take(4 * b * p);
    L->total_bytes = (int64_t)align_up(off, 256);
}

}  // namespace
}  // namespace pbn

using namespace pbn;

extern "C" size_t pbn_post_batch_workspace_bytes(int n_prop, int n_points_total, int n_scenes, int n_sp_total,
                                                 pbn_post_batch_layout* layout) {
    if (!sizes_ok(n_prop, n_points_total, n_scenes, n_sp_total)) return 0;
    pbn_post_batch_layout L;
    lay_out(n_prop, n_points_total, n_scenes, n_sp_total, &L);
    if (layout) *layout = L;
    return (size_t)L.total_bytes;
}

namespace pbn {
namespace {

// Both entries.  `scenes` is over FOLDED points; the merged arrays the proposals and pred_sem index hold n_points_merged =
// copies * scenes.point_start[B] points (copies = 1: pbn_post_batch).
int post_batch_run(const int64_t* proposals_idx, int n_entries, const void* proposals_offset, int offset_i64, int n_prop,
                   const void* clt_score, int score_dtype, const void* pred_sem, int sem_i64, int n_points_merged,
                   const pbn_scene_table& scenes, int copies, const int64_t* superpoint, float score_t, int npoint_t, float nms_t,
                   const int64_t* label_table, int n_labels, int32_t* point_instance, float* scores, int64_t* semantic_id,
                   int32_t* npoints, int32_t* scalars, void* workspace, size_t workspace_bytes, pbn_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    const int B = scenes.n_scenes;
    if (n_prop < 0 || n_entries < 0 || n_points_merged < 1 || n_labels < 1 || B < 1 || B > PBN_MAX_SCENES) return PBN_ERR_ARG;
    if (copies < 1 || (long long)B * copies > PBN_MAX_SCENES) return PBN_ERR_ARG;
    if (n_prop > POST_MAX_PROPOSALS) return PBN_ERR_UNSUPPORTED;
    if (score_dtype != PBN_F32 && score_dtype != PBN_BF16 && score_dtype != PBN_F16) return PBN_ERR_ARG;
    if (scenes.point_start[0] != 0 || scenes.sp_start[0] != 0 || (long long)copies * scenes.point_start[B] != n_points_merged)
        return PBN_ERR_ARG;
    const int n_points_total = scenes.point_start[B];          // folded: what every table below is over
    int largest = 0;
    for (int j = 0; j < B; ++j) {
        if (scenes.point_start[j + 1] < scenes.point_start[j] || scenes.sp_start[j + 1] < scenes.sp_start[j]) return PBN_ERR_ARG;
        if (scenes.point_start[j + 1] - scenes.point_start[j] > largest) largest = scenes.point_start[j + 1] - scenes.point_start[j];
    }
    const int n_sp_total = scenes.sp_start[B];
    if (!point_instance || !scalars || (n_sp_total > 0 && !superpoint)) return PBN_ERR_ARG;
    const int nb_points = cdiv(n_points_total, TPB);
    if (n_prop == 0) {
        hipLaunchKernelGGL(k_pb_empty, dim3(stride_blocks(n_points_total)), dim3(TPB), 0, stream, n_points_total, 2 * B,
                           point_instance, scalars);
        PBN_LAUNCH_CHECK();
        return PBN_OK;
    }
    if (!proposals_idx || !proposals_offset || !clt_score || !pred_sem || !label_table || !scores || !semantic_id || !npoints ||
        !workspace)
        return PBN_ERR_ARG;
    pbn_post_batch_layout L;
    lay_out(n_prop, n_points_total, B, n_sp_total, &L);
    if ((size_t)L.total_bytes > workspace_bytes) return PBN_ERR_WORKSPACE;
    char* ws = (char*)workspace;
    unsigned* masks = (unsigned*)(ws + L.masks);
    int* counts = (int*)(ws + L.counts);
    int* prop_scene = (int*)(ws + L.prop_scene);
    float* score = (float*)(ws + L.score);
    int* rows = (int*)(ws + L.rows);
    int* pick_rows = (int*)(ws + L.pick_rows);
    int* n_rows = (int*)(ws + L.n_rows);
    int* n_pick = (int*)(ws + L.n_pick);
    float* iou = (float*)(ws + L.iou);
    int* votes = (int*)(ws + L.votes);
    int* sp_label = (int*)(ws + L.sp_label);
    int* seg = (int*)(ws + L.seg);
    int* seg_refined = (int*)(ws + L.seg_refined);
    int* counts2 = (int*)(ws + L.counts2);
    int* renumber = (int*)(ws + L.renumber);
    int* n_keep = scalars;
    int* status = scalars + B;
    const int pitch = pbn_post_words(largest);          // <= pbn_post_words(n_points_total), the pitch the workspace is sized by
    const long long* pidx = (const long long*)proposals_idx;

    PBN_TRY(fill_bytes(masks, 0, sizeof(uint32_t) * (size_t)n_prop * pitch, stream));
    hipLaunchKernelGGL(k_pb_scene_of, dim3(cdiv(n_prop, TPB)), dim3(TPB), 0, stream, pidx, n_entries, proposals_offset, offset_i64,
                       n_prop, clt_score, score_dtype, scenes, copies, prop_scene, score);
    if (n_entries > 0)
        hipLaunchKernelGGL(k_pb_set_bits, dim3(cdiv(n_entries, TPB)), dim3(TPB), 0, stream, pidx, n_entries, n_prop, prop_scene,
                           scenes, copies, pitch, masks);
    hipLaunchKernelGGL(k_pb_popcount, dim3(n_prop), dim3(64), 0, stream, masks, pitch, counts);
    hipLaunchKernelGGL(k_pb_select, dim3(B), dim3(TPB), 0, stream, score, counts, prop_scene, n_prop, score_t, npoint_t, rows,
                       n_rows, status);
    const long long pairs = (long long)n_prop * n_prop;
    hipLaunchKernelGGL(k_pb_iou, dim3((unsigned)(pairs < 8192 ? pairs : 8192)), dim3(64), 0, stream, masks, rows, n_rows, B, n_prop,
                       pitch, counts, iou);
    hipLaunchKernelGGL(k_pb_nms, dim3(B), dim3(TPB), 0, stream, score, rows, n_rows, n_prop, iou, nms_t, pick_rows, n_pick);
    const long long clear_max = (long long)n_sp_total * (n_prop + 1) > (long long)B * n_prop ? (long long)n_sp_total * (n_prop + 1)
                                                                                              : (long long)B * n_prop;
    // + 1: clear_max / TPB + 1 blocks, as pbn_superpoint_refine_dev sizes its clear
    hipLaunchKernelGGL(k_pb_clear, dim3(stride_blocks(clear_max + 1)), dim3(TPB), 0, stream, n_pick, n_prop, scenes, votes, counts2);
    hipLaunchKernelGGL(k_pb_paint_vote, dim3(nb_points), dim3(TPB), 0, stream, masks, pick_rows, n_pick, n_prop, pitch,
                       n_points_total, scenes, (const long long*)superpoint, seg, votes, status);
    if (n_sp_total > 0)
        hipLaunchKernelGGL(k_pb_sp_argmax, dim3(cdiv(n_sp_total, TPB)), dim3(TPB), 0, stream, votes, n_sp_total, n_pick, n_prop,
                           scenes, sp_label);
    hipLaunchKernelGGL(k_pb_relabel, dim3(nb_points), dim3(TPB), 0, stream, sp_label, (const long long*)superpoint, seg, n_pick,
                       n_prop, n_points_total, scenes, seg_refined, counts2);
    hipLaunchKernelGGL(k_pb_compact, dim3(B), dim3(TPB), 0, stream, counts2, pick_rows, n_pick, n_prop, score, pidx, n_entries,
                       proposals_offset, offset_i64, pred_sem, sem_i64, n_points_merged, (const long long*)label_table, n_labels,
                       renumber, scores, (long long*)semantic_id, npoints, n_keep, status);
    hipLaunchKernelGGL(k_pb_point_instance, dim3(nb_points), dim3(TPB), 0, stream, seg_refined, renumber, n_prop, n_points_total,
                       scenes, point_instance);
    PBN_LAUNCH_CHECK();
    return PBN_OK;
}

}  // namespace
}  // namespace pbn

extern "C" int pbn_post_batch(const int64_t* proposals_idx, int n_entries, const void* proposals_offset, int offset_i64, int n_prop,
                              const void* clt_score, int score_dtype, const void* pred_sem, int sem_i64, int n_points_total,
                              pbn_scene_table scenes, const int64_t* superpoint, float score_t, int npoint_t, float nms_t,
                              const int64_t* label_table, int n_labels, int32_t* point_instance, float* scores,
                              int64_t* semantic_id, int32_t* npoints, int32_t* scalars, void* workspace, size_t workspace_bytes,
                              pbn_stream_t stream) {
    return post_batch_run(proposals_idx, n_entries, proposals_offset, offset_i64, n_prop, clt_score, score_dtype, pred_sem, sem_i64,
                          n_points_total, scenes, 1, superpoint, score_t, npoint_t, nms_t, label_table, n_labels, point_instance,
                          scores, semantic_id, npoints, scalars, workspace, workspace_bytes, stream);
}

extern "C" int pbn_post_batch_tta(const int64_t* proposals_idx, int n_entries, const void* proposals_offset, int offset_i64,
                                  int n_prop, const void* clt_score, int score_dtype, const void* pred_sem, int sem_i64,
                                  int n_points_merged, pbn_tta_table units, const int64_t* superpoint, float score_t, int npoint_t,
                                  float nms_t, const int64_t* label_table, int n_labels, int32_t* point_instance, float* scores,
                                  int64_t* semantic_id, int32_t* npoints, int32_t* scalars, void* workspace,
                                  size_t workspace_bytes, pbn_stream_t stream) {
    if (units.n_scenes < 1 || units.n_scenes > PBN_MAX_SCENES) return PBN_ERR_ARG;
    pbn_scene_table folded;
    folded.n_scenes = units.n_scenes;
    for (int j = 0; j <= PBN_MAX_SCENES; ++j) {
        folded.point_start[j] = units.point_start[j];
        folded.sp_start[j] = units.sp_start[j];
    }
    return post_batch_run(proposals_idx, n_entries, proposals_offset, offset_i64, n_prop, clt_score, score_dtype, pred_sem, sem_i64,
                          n_points_merged, folded, units.copies, superpoint, score_t, npoint_t, nms_t, label_table, n_labels,
                          point_instance, scores, semantic_id, npoints, scalars, workspace, workspace_bytes, stream);
}
