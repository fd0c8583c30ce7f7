// summary.hip -- what a caller of the serving front still has to compute from a merged forward's post-processing
// (post_batch.hip), in one pass over the FOLDED points: the folded semantic label per point (the `copies` score rows of a point
// summed in float32, copy after copy, then the first maximum), and per kept instance the class its points vote for
// (eval_map.py:142-155: argmax(bincount(pred_sem[mask]))), the axis-aligned box and the centre.
//   * three launches: clear, fold + accumulate (one lane per folded point), finalise (one lane per (scene, instance) slot);
//   * the per-instance accumulators are rows of 14 + n_cls words (rounded up to even) indexed by the instance's position in the flat order of
//     all scenes' kept instances (sum n_keep <= P), so the workspace is P rows, not B x P;
//   * a workgroup keeps the rows of the scene of its first point in LDS when that scene has at most summary_lds_instances kept
//     instances and flushes them once; lanes of another scene (a workgroup may straddle a boundary) and scenes with more
//     instances add to the global rows directly;
//   * every atomic is an integer one (counts, order-preserving keys of the float32 bits, 16.16 fixed-point coordinate sums), so
//     the result does not depend on the order of arrival: two runs give the same bytes.
#include <hip/hip_bf16.h>
#include <hip/hip_fp16.h>
#include "pbn_common.h"
#include "post_dev.h"

namespace pbn {
namespace {

constexpr int TPB = POST_TPB;
constexpr int NO_LABEL = -100;
constexpr int SUMMARY_STATUS_CLASS = POST_STATUS_CLASS;     // the voted class is outside the label table
constexpr int SUMMARY_STATUS_COORD = 4;                     // a coordinate is NaN or |x| >= 32768: the point is left out of box and centre
constexpr int SUMMARY_STATUS_INSTANCE = 8;                  // a point_instance value >= n_keep, or negative and not -100

// One accumulator row, in 32-bit words (the same in LDS and in the workspace):
//   [0, 6)  three 64-bit sums of rint(x * 65536)      [6, 9) min keys      [9, 12) max keys      [12] points with valid coordinates
//   [13]    unused (keeps the class counts and the next row's sums 8-byte aligned)             [14, 14 + n_cls) points per class
constexpr int ACC_SUM = 0, ACC_MIN = 6, ACC_MAX = 9, ACC_VALID = 12, ACC_HIST = 14;
constexpr int ACC_LDS_WORDS = 4096;                         // 16 KiB of accumulator rows per workgroup
constexpr float COORD_LIMIT = 32768.0f, COORD_SCALE = 65536.0f;

__host__ __device__ constexpr int acc_stride(int n_cls) { return (ACC_HIST + n_cls + 1) & ~1; }
__host__ __device__ constexpr unsigned acc_init(int word) { return word >= ACC_MIN && word < ACC_MAX ? 0xffffffffu : 0u; }

template <typename T>
__device__ __forceinline__ float widen(T v) {
    if constexpr (sizeof(T) == 4) return v;
    else if constexpr (__is_same(T, __hip_bfloat16)) return __bfloat162float(v);
    else return __half2float(v);
}

struct Kept { int n, base; };

// scene j's kept instances and their first row in the flat order; the counts are clamped so that no row lies outside [0, P)
__device__ __forceinline__ Kept kept_of_scene(const int* __restrict__ post_scalars, int n_scenes, int n_prop, int j) {
    Kept r{0, 0};
    int sum = 0;
#pragma unroll
    for (int s = 0; s < PBN_MAX_SCENES; ++s) {
        const int n = s < n_scenes ? max(0, min(post_scalars[s], n_prop - sum)) : 0;
        if (s == j) r = Kept{n, sum};
        sum += n;
    }
    return r;
}

__global__ __launch_bounds__(TPB) void k_summary_clear(unsigned* __restrict__ acc, long long n_words, int stride,
                                                      int* __restrict__ status, int n_scenes) {
    const long long first = (long long)blockIdx.x * TPB + threadIdx.x, step = (long long)gridDim.x * TPB;
    for (long long e = first; e < n_words; e += step) acc[e] = acc_init((int)(e % stride));
    if (blockIdx.x == 0 && (int)threadIdx.x < n_scenes) status[threadIdx.x] = 0;
}

// add one point to an accumulator row (LDS or global: the same integer atomics)
__device__ __forceinline__ void acc_point(unsigned* row, int cls, bool with_xyz, bool valid, float x, float y, float z) {
    atomicAdd(&row[ACC_HIST + cls], 1u);
    if (!with_xyz || !valid) return;
    const float v[3] = {x, y, z};
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        atomicMin(&row[ACC_MIN + d], okey32(v[d]));
        atomicMax(&row[ACC_MAX + d], okey32(v[d]));
        // |x| < 2^15, so x * 2^16 is exact and below 2^31 in magnitude; rintf rounds ties to even
        const long long q = (long long)rintf(v[d] * COORD_SCALE);
        atomicAdd((unsigned long long*)&row[ACC_SUM + 2 * d], (unsigned long long)q);
    }
    atomicAdd(&row[ACC_VALID], 1u);
}

template <typename T>
__global__ __launch_bounds__(TPB) void k_summary_points(const T* __restrict__ score, int ld, int n_cls, pbn_tta_table U,
                                                       const int* __restrict__ point_instance,
                                                       const int* __restrict__ post_scalars, int n_prop,
                                                       const float* __restrict__ xyz, int lds_instances,
                                                       int* __restrict__ sem_fold, unsigned* __restrict__ acc,
                                                       int* __restrict__ status) {
    __shared__ __attribute__((aligned(8))) unsigned s_acc[ACC_LDS_WORDS];
    const int n_total = start_of(U.point_start, U.n_scenes);
    const int stride = acc_stride(n_cls);
    // the workgroup's own scene: that of its first point (uniform)
    const int scene0 = scene_of_folded(U.point_start, U.n_scenes, blockIdx.x * TPB);
    Kept kept0{0, 0};
    if (n_prop > 0) kept0 = kept_of_scene(post_scalars, U.n_scenes, n_prop, scene0);
    const bool lds = kept0.n > 0 && kept0.n <= lds_instances;
    const int lds_words = lds ? kept0.n * stride : 0;
    for (int e = threadIdx.x; e < lds_words; e += TPB) s_acc[e] = acc_init(e % stride);
    __syncthreads();

    const int pt = blockIdx.x * TPB + threadIdx.x;
    if (pt < n_total) {
        const int scene = scene_of_folded(U.point_start, U.n_scenes, pt);
        const int p0 = start_of(U.point_start, scene), n_j = start_of(U.point_start, scene + 1) - p0;
        const T* row = score + ((size_t)U.copies * p0 + (size_t)(pt - p0)) * ld;
        const size_t copy_step = (size_t)n_j * ld;
        float best = -__builtin_inff();
        int arg = 0;
        for (int k = 0; k < n_cls; ++k) {
            float s = widen(row[k]);
            for (int c = 1; c < U.copies; ++c) s = s + widen(row[c * copy_step + k]);     // one float32 addition per copy, in order
            if (s > best) { best = s; arg = k; }                                          // first maximum; a NaN never wins
        }
        sem_fold[pt] = arg;
        // every point's coordinates are checked, also those of a point that belongs to no instance
        float x = 0.f, y = 0.f, z = 0.f;
        bool valid = true;
        if (xyz) {
            x = xyz[3 * (size_t)pt + 0];
            y = xyz[3 * (size_t)pt + 1];
            z = xyz[3 * (size_t)pt + 2];
            valid = fabsf(x) < COORD_LIMIT && fabsf(y) < COORD_LIMIT && fabsf(z) < COORD_LIMIT;   // false for a NaN
            if (!valid) atomicOr(&status[scene], SUMMARY_STATUS_COORD);
        }
        const int inst = n_prop > 0 ? point_instance[pt] : NO_LABEL;
        if (inst != NO_LABEL) {
            const Kept kept = scene == scene0 ? kept0 : kept_of_scene(post_scalars, U.n_scenes, n_prop, scene);
            if (inst < 0 || inst >= kept.n) {
                atomicOr(&status[scene], SUMMARY_STATUS_INSTANCE);
            } else {
                unsigned* dst = (lds && scene == scene0) ? s_acc + (size_t)inst * stride
                                                         : acc + (size_t)(kept.base + inst) * stride;
                acc_point(dst, arg, xyz != nullptr, valid, x, y, z);
            }
        }
    }
    __syncthreads();
    // flush the workgroup's rows: only the words that took part
    unsigned* out = acc + (size_t)kept0.base * stride;
    for (int e = threadIdx.x; e < lds_words; e += TPB) {
        const int w = e % stride;
        const unsigned v = s_acc[e];
        if (w < ACC_MIN) {
            if ((w & 1) == 0) {
                const unsigned long long q = *(const unsigned long long*)&s_acc[e];
                if (q) atomicAdd((unsigned long long*)&out[e], q);
            }
        } else if (w < ACC_MAX) {
            if (v != 0xffffffffu) atomicMin(&out[e], v);
        } else if (w < ACC_VALID) {
            if (v) atomicMax(&out[e], v);
        } else if (v) {
            atomicAdd(&out[e], v);
        }
    }
}

// one lane per slot of the [B, P] tables: a kept instance gets its vote, box and centre, a tail slot -1 / 0 / zeros
__global__ __launch_bounds__(TPB) void k_summary_final(const unsigned* __restrict__ acc, int n_cls, int n_scenes, int n_prop,
                                                      const int* __restrict__ post_scalars,
                                                      const long long* __restrict__ label_table, int n_labels, int with_xyz,
                                                      long long* __restrict__ class_vote, int* __restrict__ class_points,
                                                      float* __restrict__ box, float* __restrict__ centroid,
                                                      int* __restrict__ status) {
    const int e = blockIdx.x * TPB + threadIdx.x;
    if (e >= n_scenes * n_prop) return;
    const int scene = e / n_prop, k = e - scene * n_prop;
    const Kept kept = kept_of_scene(post_scalars, n_scenes, n_prop, scene);
    float bx[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, ct[3] = {0.f, 0.f, 0.f};
    long long vote = -1;
    int points = 0;
    if (k < kept.n) {
        const unsigned* row = acc + (size_t)(kept.base + k) * acc_stride(n_cls);
        int arg = 0;
        unsigned most = row[ACC_HIST];
        for (int c = 1; c < n_cls; ++c) {
            const unsigned h = row[ACC_HIST + c];
            if (h > most) { most = h; arg = c; }       // ties: the lower class
        }
        points = (int)most;
        if (arg < n_labels) vote = label_table[arg];
        else atomicOr(&status[scene], SUMMARY_STATUS_CLASS);
        if (with_xyz) {
            const unsigned valid = row[ACC_VALID];
#pragma unroll
            for (int d = 0; d < 3; ++d) {
                if (valid) {
                    bx[d] = okey32_val(row[ACC_MIN + d]);
                    bx[3 + d] = okey32_val(row[ACC_MAX + d]);
                    const long long q = *(const long long*)&row[ACC_SUM + 2 * d];
                    ct[d] = (float)((double)q / (double)valid / 65536.0);
                } else {
                    bx[d] = bx[3 + d] = ct[d] = __builtin_nanf("");
                }
            }
        }
    }
    class_vote[e] = vote;
    class_points[e] = points;
    if (with_xyz) {
#pragma unroll
        for (int d = 0; d < 6; ++d) box[6 * (size_t)e + d] = bx[d];
#pragma unroll
        for (int d = 0; d < 3; ++d) centroid[3 * (size_t)e + d] = ct[d];
    }
}

bool summary_sizes_ok(int n_prop, int n_cls) {
    return n_prop >= 0 && n_prop <= POST_MAX_PROPOSALS && n_cls >= 1 && n_cls <= SEL_MAX_CLASSES;
}

template <typename T>
void launch_points(hipStream_t stream, int n_total, const void* score, int ld, int n_cls, const pbn_tta_table& U,
                   const int32_t* point_instance, const int32_t* post_scalars, int n_prop, const float* xyz, int32_t* sem_fold,
                   unsigned* acc, int32_t* status) {
    hipLaunchKernelGGL(k_summary_points<T>, dim3(cdiv(n_total, TPB)), dim3(TPB), 0, stream, (const T*)score, ld, n_cls, U,
                       point_instance, post_scalars, n_prop, xyz, ACC_LDS_WORDS / acc_stride(n_cls), sem_fold, acc, status);
}

}  // namespace
}  // namespace pbn

using namespace pbn;

extern "C" size_t pbn_scene_summary_workspace_bytes(int n_prop, int n_cls) {
    if (!summary_sizes_ok(n_prop, n_cls)) return 0;
    return align_up(sizeof(uint32_t) * (size_t)n_prop * acc_stride(n_cls), 256);
}

extern "C" int pbn_scene_summary_lds_instances(int n_cls) {
    if (n_cls < 1 || n_cls > SEL_MAX_CLASSES) return 0;
    return ACC_LDS_WORDS / acc_stride(n_cls);
}

extern "C" int pbn_scene_summary(const void* sem_score, int ld, int n_cls, int score_dtype, int n_points_merged,
                                 pbn_tta_table units, const int32_t* point_instance, const int32_t* post_scalars, int n_prop,
                                 const float* xyz, const int64_t* label_table, int n_labels, int32_t* sem_fold,
                                 int64_t* class_vote, int32_t* class_points, float* box, float* centroid, int32_t* status,
                                 void* workspace, size_t workspace_bytes, pbn_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    const int B = units.n_scenes, copies = units.copies;
    if (n_prop < 0 || n_points_merged < 1 || B < 1 || B > PBN_MAX_SCENES) return PBN_ERR_ARG;
    if (copies < 1 || (long long)B * copies > PBN_MAX_SCENES) return PBN_ERR_ARG;
    if (n_cls < 1 || n_cls > SEL_MAX_CLASSES || ld < n_cls) return PBN_ERR_ARG;
    if (score_dtype != PBN_F32 && score_dtype != PBN_BF16 && score_dtype != PBN_F16) return PBN_ERR_ARG;
    if (units.point_start[0] != 0 || units.sp_start[0] != 0 || (long long)copies * units.point_start[B] != n_points_merged)
        return PBN_ERR_ARG;
    for (int j = 0; j < B; ++j)
        if (units.point_start[j + 1] < units.point_start[j] || units.sp_start[j + 1] < units.sp_start[j]) return PBN_ERR_ARG;
    if (n_prop > POST_MAX_PROPOSALS) return PBN_ERR_UNSUPPORTED;
    if (!sem_score || !sem_fold || !status) return PBN_ERR_ARG;
    if (xyz && n_prop > 0 && (!box || !centroid)) return PBN_ERR_ARG;
    if (n_prop > 0) {
        if (!point_instance || !post_scalars || !label_table || n_labels < 1 || !class_vote || !class_points || !workspace ||
            ((uintptr_t)workspace & 7))
            return PBN_ERR_ARG;
        if (pbn_scene_summary_workspace_bytes(n_prop, n_cls) > workspace_bytes) return PBN_ERR_WORKSPACE;
    }
    const int n_total = units.point_start[B];
    const int stride = acc_stride(n_cls);
    unsigned* acc = (unsigned*)workspace;
    const long long n_words = (long long)n_prop * stride;
    hipLaunchKernelGGL(k_summary_clear, dim3((unsigned)(n_words / TPB + 1 < 1024 ? n_words / TPB + 1 : 1024)), dim3(TPB), 0, stream,
                       acc, n_words, stride, status, B);
    if (score_dtype == PBN_F32)
        launch_points<float>(stream, n_total, sem_score, ld, n_cls, units, point_instance, post_scalars, n_prop, xyz, sem_fold,
                             acc, status);
    else if (score_dtype == PBN_BF16)
        launch_points<__hip_bfloat16>(stream, n_total, sem_score, ld, n_cls, units, point_instance, post_scalars, n_prop, xyz,
                                      sem_fold, acc, status);
    else
        launch_points<__half>(stream, n_total, sem_score, ld, n_cls, units, point_instance, post_scalars, n_prop, xyz, sem_fold,
                              acc, status);
    if (n_prop > 0)
        hipLaunchKernelGGL(k_summary_final, dim3(cdiv((long long)B * n_prop, TPB)), dim3(TPB), 0, stream, acc, n_cls, B, n_prop,
                           post_scalars, (const long long*)label_table, n_labels, xyz != nullptr ? 1 : 0,
                           (long long*)class_vote, class_points, box, centroid, status);
    PBN_LAUNCH_CHECK();
    return PBN_OK;
}
