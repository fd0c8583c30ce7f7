// losses.hip -- the seven loss terms of model_fn (the reference's network/PBNet.py:366-416, diceLoss :463-468) and their
// gradients, each as one pass over its inputs: what pbnet_amd.network.PBNet.model_losses and autograd spell as a few hundred
// small torch launches.  Memory-bound; arithmetic per row in float32, sums in float64.
//
// Forward, three streaming kernels and a finaliser:
//   k_loss_points   one ROW per lane, grid-stride: the K logits of a row in registers (4 elements per load when the row
//                   address allows), max-subtracted logsumexp - score[label]; |pred - gt|_1 and the direction cosine of the
//                   offset row.  An ignored row (label -100, or a label outside [0, K), counted as bad) reads no logits, a
//                   row with ins_label -100 reads no offsets.
//   k_loss_mask     the shape of metrics.hip: groups of 4 rows per lane, 16-byte loads where the address allows, workgroup 0
//                   takes the unaligned head and tail.  Writes gt_mask back with -1 -> 0 (the reference's in-place quirk,
//                   see model_losses) and the weight byte (gt != -1) the backward needs, since gt_mask no longer tells.
//   k_loss_scores   one wave per proposal: max over its row of the IoU table, the fg / bg ramp, BCE against clt.
//   k_loss_finalize ONE workgroup adds the per-workgroup float64 partials in index order and writes terms / counts / state.
// No floating-point atomics (the library-wide rule of metrics.hip): every workgroup stores its partial sums, grids depend on
// the row counts only, so the same inputs give the same bits on every run and device.
//
// Backward, one kernel per pass: reads `state` and the device scalar grad_loss (no host synchronisation after the forward),
// recomputes the softmax, writes each gradient once in the dtype of its input.
#include "pbn_common.h"
#include "vec4_dev.h"

namespace pbn {
namespace {

constexpr int TPB = 256;                    // 4 waves
constexpr int WAVES = TPB / WAVE;
constexpr int GRID_CAP = 1024;              // partials one finaliser thread adds; 4 workgroups per CU on 256 CUs
constexpr int N_POINT = 6;                  // sum keep*nll, sum valid*l1, sum valid*cos, n_keep, n_valid, bad labels
constexpr int N_MASK = 5;                   // sum w*bce, sum w, sum t*p, sum t^2, sum p^2
constexpr float EPS = 1e-8f;

int grid_points(long long n) { const long long g = (n + TPB - 1) / TPB; return (int)(g < 1 ? 1 : (g > GRID_CAP ? GRID_CAP : g)); }
int grid_mask(long long n) { return grid_points(n / 4); }
int grid_scores(long long p) { return grid_points(p * WAVE); }      // a wave per proposal

struct Partials {                            // the workspace: [gp][N_POINT] | [gm][N_MASK] | [gs] doubles
    int gp, gm, gs;
    Partials(long long n_points, long long n_rows, long long n_prop)
        : gp(grid_points(n_points)), gm(n_rows < 0 ? 0 : grid_mask(n_rows)), gs(n_rows < 0 ? 0 : grid_scores(n_prop)) {}
    size_t bytes() const { return sizeof(double) * ((size_t)gp * N_POINT + (size_t)gm * N_MASK + (size_t)gs); }
};

__device__ __forceinline__ float load_any(const void* p, int dt, long long i) {
    if (dt == PBN_F32) return ((const float*)p)[i];
    if (dt == PBN_BF16) return Elem<PBN_BF16>::widen(((const unsigned short*)p)[i]);
    return Elem<PBN_F16>::widen(((const unsigned short*)p)[i]);
}
__device__ __forceinline__ void store_any(void* p, int dt, long long i, float v) {
    if (dt == PBN_F32) ((float*)p)[i] = v;
    else if (dt == PBN_BF16) ((unsigned short*)p)[i] = Elem<PBN_BF16>::narrow(v);
    else ((unsigned short*)p)[i] = Elem<PBN_F16>::narrow(v);
}

// torch.nn.BCELoss: both logs clamped at -100
__device__ __forceinline__ float bce(float p, float t) {
    return -(t * fmaxf(logf(p), -100.f) + (1.f - t) * fmaxf(logf(1.f - p), -100.f));
}
__device__ __forceinline__ float bce_grad(float p, float t) { return (p - t) / fmaxf(p * (1.f - p), 1e-12f); }

// the workgroup's sums of NV per-lane values -> out[0:NV]: wave butterflies, then the waves in order
template <int NV>
__device__ __forceinline__ void block_sums(double (&a)[NV], double* __restrict__ out) {
    __shared__ double part[WAVES][NV];
    const int tid = (int)threadIdx.x;
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        double v = a[k];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
        if (lane_id() == 0) part[tid >> 6][k] = v;
    }
    __syncthreads();
    if (tid < NV) {
        double s = 0.0;
        for (int w = 0; w < WAVES; ++w) s += part[w][tid];
        out[tid] = s;
    }
}

// the K logits of one row, widened; v[c] = -inf for c >= K
template <int DT, int KMAX>
__device__ __forceinline__ void load_row(const typename Elem<DT>::T* __restrict__ p, int K, bool vec, float (&v)[KMAX]) {
    typedef typename Elem<DT>::T T;
#pragma unroll
    for (int g = 0; g < KMAX / 4; ++g) {
        if (4 * g + 4 <= K) {
            T q[4];
            load4(p + 4 * g, vec, q);
#pragma unroll
            for (int j = 0; j < 4; ++j) v[4 * g + j] = Elem<DT>::widen(q[j]);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) v[4 * g + j] = 4 * g + j < K ? Elem<DT>::widen(p[4 * g + j]) : -INFINITY;
        }
    }
}

// max, sum exp(v - max) and the label's logit of a row held in registers (no dynamic register index)
template <int KMAX>
__device__ __forceinline__ void row_softmax(const float (&v)[KMAX], int label, float& m, float& s, float& vl) {
    m = v[0];
#pragma unroll
    for (int c = 1; c < KMAX; ++c) m = fmaxf(m, v[c]);
    s = 0.f;
    vl = 0.f;
#pragma unroll
    for (int c = 0; c < KMAX; ++c) {
        s += expf(v[c] - m);
        vl = c == label ? v[c] : vl;
    }
}

struct OffsetRow { float pred[3], gt[3]; };
__device__ __forceinline__ OffsetRow load_offset_row(const void* off, int off_dt, const float* __restrict__ info,
                                                     const float* __restrict__ xyz, long long i) {
    OffsetRow r;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        r.pred[d] = load_any(off, off_dt, 3 * i + d);
        r.gt[d] = info[9 * i + d] - xyz[3 * i + d];
    }
    return r;
}

template <int DT, int KMAX>
__global__ __launch_bounds__(TPB) void k_loss_points(const typename Elem<DT>::T* __restrict__ sem, int ld, int vec,
                                                    const long long* __restrict__ label, const void* __restrict__ off,
                                                    int off_dt, const float* __restrict__ info, const float* __restrict__ xyz,
                                                    const long long* __restrict__ ins, long long n, int K,
                                                    double* __restrict__ part) {
    double a[N_POINT] = {0, 0, 0, 0, 0, 0};
    for (long long i = (long long)blockIdx.x * TPB + threadIdx.x; i < n; i += (long long)gridDim.x * TPB) {
        const long long lab = label[i];
        const bool keep = lab >= 0 && lab < K;
        if (keep) {
            float v[KMAX], m, s, vl;
            load_row<DT, KMAX>(sem + i * ld, K, vec != 0, v);
            row_softmax<KMAX>(v, (int)lab, m, s, vl);
            a[0] += (double)(logf(s) + m - vl);
            a[3] += 1.0;
        } else if (lab != -100) {
            a[5] += 1.0;                                   // neither ignored nor a class: never used as an index
        }
        if (ins[i] != -100) {
            const OffsetRow r = load_offset_row(off, off_dt, info, xyz, i);
            float l1 = 0.f, gg = 0.f, pp = 0.f, gp = 0.f;
#pragma unroll
            for (int d = 0; d < 3; ++d) {
                l1 += fabsf(r.pred[d] - r.gt[d]);
                gg += r.gt[d] * r.gt[d];
                pp += r.pred[d] * r.pred[d];
                gp += r.gt[d] * r.pred[d];
            }
            a[1] += (double)l1;
            a[2] += (double)(gp / ((sqrtf(gg) + EPS) * (sqrtf(pp) + EPS)));
            a[4] += 1.0;
        }
    }
    block_sums<N_POINT>(a, part + (size_t)blockIdx.x * N_POINT);
}

template <int DT>
__global__ __launch_bounds__(TPB) void k_loss_mask(const typename Elem<DT>::T* __restrict__ pred, long long* __restrict__ gt,
                                                  unsigned char* __restrict__ weight, long long n, int head, int vec_p,
                                                  int vec_g, double* __restrict__ part) {
    typedef typename Elem<DT>::T T;
    const int tid = (int)threadIdx.x;
    double a[N_MASK] = {0, 0, 0, 0, 0};

    auto row = [&](long long i, T raw, long long g) {
        const float p = Elem<DT>::widen(raw);
        const bool w = g != -1;
        const float t = (float)(g > 0 ? g : 0);
        if (!w) gt[i] = 0;
        weight[i] = w ? 1 : 0;
        if (w) { a[0] += (double)bce(p, t); a[1] += 1.0; }
        a[2] += (double)(t * p);
        a[3] += (double)(t * t);
        a[4] += (double)(p * p);
    };

    const long long groups = (n - head) >> 2;
    for (long long g = (long long)blockIdx.x * TPB + tid; g < groups; g += (long long)gridDim.x * TPB) {
        const long long i = head + 4 * g;
        T pv[4];
        long long gv[4];
        load4(pred + i, vec_p != 0, pv);
        load4(gt + i, vec_g != 0, gv);
#pragma unroll
        for (int j = 0; j < 4; ++j) row(i + j, pv[j], gv[j]);
    }
    if (blockIdx.x == 0) {                                 // the unaligned head and the tail, one row per lane (< 8)
        const long long tail0 = head + 4 * groups;
        if (tid < head + (int)(n - tail0)) {
            const long long i = tid < head ? tid : tail0 + (tid - head);
            row(i, pred[i], gt[i]);
        }
    }
    block_sums<N_MASK>(a, part + (size_t)blockIdx.x * N_MASK);
}

// the ramp of get_segmented_scores as torch's `scores * k + b` evaluates it: a rounded multiply, then a rounded add, never one
// FMA (HIP's __fmul_rn / __fadd_rn are the plain operators and contract like them; the pragma is what holds)
__device__ __forceinline__ float ramp(float v, float k, float b) {
#pragma clang fp contract(off)
    const float prod = v * k;
    return prod + b;
}

// gt_scores[p] = get_segmented_scores(max_i iou[p, i])
__global__ __launch_bounds__(TPB) void k_loss_scores(const float* __restrict__ iou, int n_inst, const void* __restrict__ clt,
                                                    int clt_dt, long long n_prop, float fg, float bg, float ramp_k,
                                                    float ramp_b, float* __restrict__ gt_scores, double* __restrict__ part) {
    const int lane = lane_id();
    double a[1] = {0};
    for (long long p = (long long)blockIdx.x * WAVES + (threadIdx.x >> 6); p < n_prop; p += (long long)gridDim.x * WAVES) {
        float m = -INFINITY;
        for (int i = lane; i < n_inst; i += WAVE) m = fmaxf(m, iou[p * n_inst + i]);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
        if (lane == 0) {
            const float s = m > fg ? 1.f : (m < bg ? 0.f : ramp(m, ramp_k, ramp_b));
            gt_scores[p] = s;
            a[0] += (double)bce(load_any(clt, clt_dt, p), s);
        }
    }
    block_sums<1>(a, part + blockIdx.x);
}

// terms f32[8] = semantic, offset_norm, offset_dir, mask, dice, score, loss, 0; counts i64[4] = n_valid, sum w, n_keep, bad
// labels; state f64[8] = n_keep, n_valid + 1e-6, R, 2A + 1, U = B + C + 1 + 1e-8, P, 0, 0.  n_rows < 0: the point terms only.
// Empty means are 0 / 0 = NaN, as torch's.  Two NaN cases differ from torch and cannot arise from pbn_get_iou's table or from
// sigmoid scores: a NaN in the IoU table is dropped by the row maximum (fmaxf; torch's max propagates it), and a NaN pred_mask
// on an IGNORED row is skipped by the BCE sum (torch's weight * NaN is NaN); it still reaches the dice sums.
__global__ __launch_bounds__(TPB) void k_loss_finalize(const double* __restrict__ part, int gp, int gm, int gs,
                                                      long long n_rows, long long n_prop, float* __restrict__ terms,
                                                      long long* __restrict__ counts, double* __restrict__ state) {
    __shared__ double sum[N_POINT + N_MASK + 1];
    const int tid = (int)threadIdx.x;
    if (tid < N_POINT + N_MASK + 1) {
        const double* col;
        int n, stride;
        if (tid < N_POINT) { col = part + tid; n = gp; stride = N_POINT; }
        else if (tid < N_POINT + N_MASK) { col = part + (size_t)gp * N_POINT + (tid - N_POINT); n = gm; stride = N_MASK; }
        else { col = part + (size_t)gp * N_POINT + (size_t)gm * N_MASK; n = gs; stride = 1; }
        double s = 0.0;
        for (int i = 0; i < n; ++i) s += col[(size_t)i * stride];
        sum[tid] = s;
    }
    __syncthreads();
    if (tid != 0) return;
    const double n_keep = sum[3], denom = sum[4] + 1e-6;
    const double semantic = sum[0] / n_keep, off_norm = sum[1] / denom, off_dir = -sum[2] / denom;
    double loss = semantic + off_norm + off_dir, mask = 0.0, dice = 0.0, score = 0.0, inter = 0.0, uni = 0.0;
    if (n_rows >= 0) {
        inter = 2.0 * sum[N_POINT + 2] + 1.0;
        uni = sum[N_POINT + 3] + sum[N_POINT + 4] + 1.0 + 1e-8;
        mask = sum[N_POINT + 0] / (double)n_rows;
        dice = 1.0 - inter / uni;
        score = sum[N_POINT + N_MASK] / (double)n_prop;
        loss += mask + dice + score;
    }
    terms[0] = (float)semantic; terms[1] = (float)off_norm; terms[2] = (float)off_dir; terms[3] = (float)mask;
    terms[4] = (float)dice; terms[5] = (float)score; terms[6] = (float)loss; terms[7] = 0.f;
    counts[0] = (long long)sum[4]; counts[1] = (long long)sum[N_POINT + 1]; counts[2] = (long long)n_keep;
    counts[3] = (long long)sum[5];
    state[0] = n_keep; state[1] = denom; state[2] = (double)(n_rows < 0 ? 0 : n_rows); state[3] = inter; state[4] = uni;
    state[5] = (double)n_prop; state[6] = 0.0; state[7] = 0.0;
}

// g_sem[i, c] = keep_i (softmax_c - [c == label]) / n_keep;  g_off[i] = valid_i / (n_valid + 1e-6) (sign(pred - gt) -
// [g^/(n + eps) - (g^ . pred) pred / (n (n + eps)^2)]) with g^ = gt / (|gt| + eps), n = |pred| (the norm's gradient at 0 is 0)
template <int DT, int KMAX>
__global__ __launch_bounds__(TPB) void k_loss_points_bwd(const typename Elem<DT>::T* __restrict__ sem, int ld, int vec,
                                                        const long long* __restrict__ label, const void* __restrict__ off,
                                                        int off_dt, const float* __restrict__ info,
                                                        const float* __restrict__ xyz, const long long* __restrict__ ins,
                                                        long long n, int K, const double* __restrict__ state,
                                                        const float* __restrict__ grad_loss,
                                                        typename Elem<DT>::T* __restrict__ g_sem, int g_vec,
                                                        void* __restrict__ g_off) {
    typedef typename Elem<DT>::T T;
    const float gl = *grad_loss;
    const float k_sem = (float)((double)gl / state[0]), k_off = (float)((double)gl / state[1]);
    for (long long i = (long long)blockIdx.x * TPB + threadIdx.x; i < n; i += (long long)gridDim.x * TPB) {
        const long long lab = label[i];
        const bool keep = lab >= 0 && lab < K;
        float v[KMAX], m = 0.f, s = 1.f, vl;
        if (keep) {
            load_row<DT, KMAX>(sem + i * ld, K, vec != 0, v);
            row_softmax<KMAX>(v, (int)lab, m, s, vl);
        }
        const float inv = keep ? k_sem / s : 0.f;
        T* out = g_sem + i * K;
#pragma unroll
        for (int g = 0; g < KMAX / 4; ++g) {
            if (4 * g >= K) break;
            T q[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int c = 4 * g + j;
                q[j] = Elem<DT>::narrow(keep ? expf(v[c] - m) * inv - (c == (int)lab ? k_sem : 0.f) : 0.f);
            }
            if (4 * g + 4 <= K) {
                store4(out + 4 * g, g_vec != 0, q);
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (4 * g + j < K) out[4 * g + j] = q[j];
            }
        }
        float go[3] = {0.f, 0.f, 0.f};
        if (ins[i] != -100) {
            const OffsetRow r = load_offset_row(off, off_dt, info, xyz, i);
            float gg = 0.f, pp = 0.f, gp = 0.f;
#pragma unroll
            for (int d = 0; d < 3; ++d) {
                gg += r.gt[d] * r.gt[d];
                pp += r.pred[d] * r.pred[d];
            }
            const float gn = sqrtf(gg) + EPS, nrm = sqrtf(pp), ne = nrm + EPS;
#pragma unroll
            for (int d = 0; d < 3; ++d) gp += (r.gt[d] / gn) * r.pred[d];
            const float back = nrm > 0.f ? gp / (nrm * ne * ne) : 0.f;
#pragma unroll
            for (int d = 0; d < 3; ++d) {
                const float diff = r.pred[d] - r.gt[d];
                const float sgn = diff > 0.f ? 1.f : (diff < 0.f ? -1.f : 0.f);
                go[d] = k_off * (sgn - ((r.gt[d] / gn) / ne - back * r.pred[d]));
            }
        }
#pragma unroll
        for (int d = 0; d < 3; ++d) store_any(g_off, off_dt, 3 * i + d, go[d]);
    }
}

// g_mask[r] = w (p - t) / max(p (1 - p), 1e-12) / R - 2 t / U + (2A + 1) 2 p / U^2; gt is the forward's rewritten mask
template <int DT>
__global__ __launch_bounds__(TPB) void k_loss_mask_bwd(const typename Elem<DT>::T* __restrict__ pred,
                                                      const long long* __restrict__ gt,
                                                      const unsigned char* __restrict__ weight, long long n, int head,
                                                      int vec_p, int vec_g, int vec_o, const double* __restrict__ state,
                                                      const float* __restrict__ grad_loss,
                                                      typename Elem<DT>::T* __restrict__ g_mask) {
    typedef typename Elem<DT>::T T;
    const int tid = (int)threadIdx.x;
    const float gl = *grad_loss;
    const float k_bce = (float)((double)gl / state[2]), k_t = (float)(2.0 * gl / state[4]),
                k_p = (float)(2.0 * gl * state[3] / (state[4] * state[4]));

    auto row = [&](long long i, T raw, long long g) -> T {
        const float p = Elem<DT>::widen(raw), t = (float)g;
        const float b = weight[i] ? bce_grad(p, t) * k_bce : 0.f;
        return Elem<DT>::narrow(b - k_t * t + k_p * p);
    };

    const long long groups = (n - head) >> 2;
    for (long long g = (long long)blockIdx.x * TPB + tid; g < groups; g += (long long)gridDim.x * TPB) {
        const long long i = head + 4 * g;
        T pv[4], ov[4];
        long long gv[4];
        load4(pred + i, vec_p != 0, pv);
        load4(gt + i, vec_g != 0, gv);
#pragma unroll
        for (int j = 0; j < 4; ++j) ov[j] = row(i + j, pv[j], gv[j]);
        store4(g_mask + i, vec_o != 0, ov);
    }
    if (blockIdx.x == 0) {
        const long long tail0 = head + 4 * groups;
        if (tid < head + (int)(n - tail0)) {
            const long long i = tid < head ? tid : tail0 + (tid - head);
            g_mask[i] = row(i, pred[i], gt[i]);
        }
    }
}

// g_clt[p] = (c - s) / max(c (1 - c), 1e-12) / P
__global__ __launch_bounds__(TPB) void k_loss_scores_bwd(const void* __restrict__ clt, int clt_dt,
                                                        const float* __restrict__ gt_scores, long long n_prop,
                                                        const double* __restrict__ state, const float* __restrict__ grad_loss,
                                                        void* __restrict__ g_clt) {
    const float k = (float)((double)*grad_loss / state[5]);
    for (long long p = (long long)blockIdx.x * TPB + threadIdx.x; p < n_prop; p += (long long)gridDim.x * TPB)
        store_any(g_clt, clt_dt, p, bce_grad(load_any(clt, clt_dt, p), gt_scores[p]) * k);
}

bool known(int dt) { return dt == PBN_F32 || dt == PBN_BF16 || dt == PBN_F16; }
int elem_size(int dt) { return dt == PBN_F32 ? 4 : 2; }

// what both entries check before any launch
int check_args(const void* sem, int sem_dt, int sem_ld, const void* label, const void* off, int off_dt, const void* info,
               const void* xyz, const void* ins, int64_t n_points, int n_class, const void* pred_mask, int mask_dt,
               const void* gt_mask, const void* weight, int64_t n_rows, const void* clt, int clt_dt, const void* gt_scores,
               int64_t n_prop) {
    if (n_points < 0 || n_prop < 0 || n_class < 2 || n_class > 64 || sem_ld < n_class) return PBN_ERR_ARG;
    if (!known(sem_dt) || !known(off_dt)) return PBN_ERR_UNSUPPORTED;
    if (n_points > 0 && (!sem || !label || !off || !info || !xyz || !ins)) return PBN_ERR_ARG;
    if ((uintptr_t)sem % elem_size(sem_dt) || (uintptr_t)off % elem_size(off_dt) || (uintptr_t)info % 4 || (uintptr_t)xyz % 4 ||
        (uintptr_t)label % 8 || (uintptr_t)ins % 8)
        return PBN_ERR_ARG;
    if (n_rows < 0) return PBN_OK;
    if (!known(mask_dt) || !known(clt_dt)) return PBN_ERR_UNSUPPORTED;
    if (n_rows > 0 && (!pred_mask || !gt_mask || !weight)) return PBN_ERR_ARG;
    if (n_prop > 0 && (!clt || !gt_scores)) return PBN_ERR_ARG;
    if ((uintptr_t)pred_mask % elem_size(mask_dt) || (uintptr_t)gt_mask % 8 || (uintptr_t)clt % elem_size(clt_dt) ||
        (uintptr_t)gt_scores % 4)
        return PBN_ERR_ARG;
    return PBN_OK;
}

// rows load (store) as 4-element vectors when the base and every row start are multiples of the vector size
int row_vec(const void* p, int ld, int dt) { return (uintptr_t)p % (4 * elem_size(dt)) == 0 && ld % 4 == 0; }

// one pass's arguments; backward: part is null and the four trailing fields are set
struct PointPass {
    const void* sem; int sem_dt, ld; const int64_t* label; const void* off; int off_dt; const float* info; const float* xyz;
    const int64_t* ins; int64_t n; int K, grid; double* part;
    const double* state; const float* grad_loss; void* g_sem; void* g_off;
};
struct MaskPass {
    const void* pred; int dt; int64_t* gt; uint8_t* weight; int64_t n; int grid; double* part;
    const double* state; const float* grad_loss; void* g_mask;
};

template <int DT, int KMAX>
void launch_points_k(const PointPass& a, hipStream_t stream) {
    typedef typename Elem<DT>::T T;
    const int vec = row_vec(a.sem, a.ld, DT);
    if (a.part)
        hipLaunchKernelGGL((k_loss_points<DT, KMAX>), dim3(a.grid), dim3(TPB), 0, stream, (const T*)a.sem, a.ld, vec,
                           (const long long*)a.label, a.off, a.off_dt, a.info, a.xyz, (const long long*)a.ins, (long long)a.n,
                           a.K, a.part);
    else
        hipLaunchKernelGGL((k_loss_points_bwd<DT, KMAX>), dim3(a.grid), dim3(TPB), 0, stream, (const T*)a.sem, a.ld, vec,
                           (const long long*)a.label, a.off, a.off_dt, a.info, a.xyz, (const long long*)a.ins, (long long)a.n,
                           a.K, a.state, a.grad_loss, (T*)a.g_sem, row_vec(a.g_sem, a.K, DT), a.g_off);
}
template <int DT>
void launch_points_dt(const PointPass& a, hipStream_t stream) {
    if (a.K <= 16) launch_points_k<DT, 16>(a, stream);
    else if (a.K <= 32) launch_points_k<DT, 32>(a, stream);
    else launch_points_k<DT, 64>(a, stream);
}
int launch_points(const PointPass& a, hipStream_t stream) {
    if (a.sem_dt == PBN_F32) launch_points_dt<PBN_F32>(a, stream);
    else if (a.sem_dt == PBN_BF16) launch_points_dt<PBN_BF16>(a, stream);
    else launch_points_dt<PBN_F16>(a, stream);
    PBN_LAUNCH_CHECK();
    return PBN_OK;
}

template <int DT>
void launch_mask_dt(const MaskPass& a, hipStream_t stream) {
    typedef typename Elem<DT>::T T;
    int vec_p = 0, vec_g = 0;
    int head = pick_head((uintptr_t)a.pred, (int)sizeof(T), (uintptr_t)a.gt, 8, &vec_p, &vec_g);
    if (head > a.n) head = (int)a.n;
    if (a.part) {
        hipLaunchKernelGGL((k_loss_mask<DT>), dim3(a.grid), dim3(TPB), 0, stream, (const T*)a.pred, (long long*)a.gt, a.weight,
                           (long long)a.n, head, vec_p, vec_g, a.part);
    } else {
        const int vec_o = ((uintptr_t)a.g_mask + (size_t)head * sizeof(T)) % (4 * sizeof(T)) == 0;
        hipLaunchKernelGGL((k_loss_mask_bwd<DT>), dim3(a.grid), dim3(TPB), 0, stream, (const T*)a.pred, (const long long*)a.gt,
                           a.weight, (long long)a.n, head, vec_p, vec_g, vec_o, a.state, a.grad_loss, (T*)a.g_mask);
    }
}
int launch_mask(const MaskPass& a, hipStream_t stream) {
    if (a.dt == PBN_F32) launch_mask_dt<PBN_F32>(a, stream);
    else if (a.dt == PBN_BF16) launch_mask_dt<PBN_BF16>(a, stream);
    else launch_mask_dt<PBN_F16>(a, stream);
    PBN_LAUNCH_CHECK();
    return PBN_OK;
}

}  // namespace
}  // namespace pbn

using namespace pbn;

extern "C" size_t pbn_losses_workspace_bytes(int64_t n_points, int64_t n_rows, int64_t n_prop) {
    if (n_points < 0 || n_prop < 0) return 0;
    return align_up(Partials(n_points, n_rows, n_prop).bytes(), 256);
}

extern "C" int pbn_losses_forward(const void* sem_score, int sem_dtype, int sem_ld, const int64_t* sem_label,
                                  const void* offset_pred, int offset_dtype, const float* inst_info, const float* xyz,
                                  const int64_t* ins_label, int64_t n_points, int n_class, const void* pred_mask,
                                  int mask_dtype, int64_t* gt_mask, uint8_t* mask_weight, int64_t n_rows, const float* iou,
                                  int n_inst, const void* clt_scores, int clt_dtype, int64_t n_prop, double fg_thresh,
                                  double bg_thresh, float* gt_scores, float* terms, int64_t* counts, double* state,
                                  void* workspace, size_t workspace_bytes, pbn_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    const int rc = check_args(sem_score, sem_dtype, sem_ld, sem_label, offset_pred, offset_dtype, inst_info, xyz, ins_label,
                              n_points, n_class, pred_mask, mask_dtype, gt_mask, mask_weight, n_rows, clt_scores, clt_dtype,
                              gt_scores, n_prop);
    if (rc != PBN_OK) return rc;
    if (!terms || !counts || !state || !workspace) return PBN_ERR_ARG;
    if (n_rows >= 0 && n_prop > 0 && (!iou || n_inst < 1 || (uintptr_t)iou % 4)) return PBN_ERR_ARG;
    if ((uintptr_t)workspace % 16) return PBN_ERR_ARG;
    const Partials P(n_points, n_rows, n_prop);
    if (workspace_bytes < P.bytes()) return PBN_ERR_WORKSPACE;
    double* part_points = (double*)workspace;
    double* part_mask = part_points + (size_t)P.gp * N_POINT;
    double* part_scores = part_mask + (size_t)P.gm * N_MASK;

    int r = launch_points({sem_score, sem_dtype, sem_ld, sem_label, offset_pred, offset_dtype, inst_info, xyz, ins_label, n_points,
                           n_class, P.gp, part_points, nullptr, nullptr, nullptr, nullptr}, stream);
    if (r != PBN_OK) return r;
    if (n_rows >= 0) {
        r = launch_mask({pred_mask, mask_dtype, gt_mask, mask_weight, n_rows, P.gm, part_mask, nullptr, nullptr, nullptr}, stream);
        if (r != PBN_OK) return r;
        // k = 1 / (fg - bg), b = bg / (bg - fg) in double, then float32: the scalars torch multiplies and adds
        hipLaunchKernelGGL(k_loss_scores, dim3(P.gs), dim3(TPB), 0, stream, iou, n_inst, clt_scores, clt_dtype, (long long)n_prop,
                           (float)fg_thresh, (float)bg_thresh, (float)(1.0 / (fg_thresh - bg_thresh)),
                           (float)(bg_thresh / (bg_thresh - fg_thresh)), gt_scores, part_scores);
        PBN_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(k_loss_finalize, dim3(1), dim3(TPB), 0, stream, (const double*)workspace, P.gp, P.gm, P.gs,
                       (long long)n_rows, (long long)n_prop, terms, (long long*)counts, state);
    PBN_LAUNCH_CHECK();
    return PBN_OK;
}

extern "C" int pbn_losses_backward(const void* sem_score, int sem_dtype, int sem_ld, const int64_t* sem_label,
                                   const void* offset_pred, int offset_dtype, const float* inst_info, const float* xyz,
                                   const int64_t* ins_label, int64_t n_points, int n_class, const void* pred_mask,
                                   int mask_dtype, const int64_t* gt_mask, const uint8_t* mask_weight, int64_t n_rows,
                                   const void* clt_scores, int clt_dtype, const float* gt_scores, int64_t n_prop,
                                   const double* state, const float* grad_loss, void* g_sem, void* g_offset, void* g_mask,
                                   void* g_clt, pbn_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    const int rc = check_args(sem_score, sem_dtype, sem_ld, sem_label, offset_pred, offset_dtype, inst_info, xyz, ins_label,
                              n_points, n_class, pred_mask, mask_dtype, gt_mask, mask_weight, n_rows, clt_scores, clt_dtype,
                              gt_scores, n_prop);
    if (rc != PBN_OK) return rc;
    if (!state || !grad_loss || (n_points > 0 && (!g_sem || !g_offset))) return PBN_ERR_ARG;
    if ((uintptr_t)g_sem % elem_size(sem_dtype) || (uintptr_t)g_offset % elem_size(offset_dtype)) return PBN_ERR_ARG;
    if (n_rows >= 0) {
        if ((n_rows > 0 && !g_mask) || (n_prop > 0 && !g_clt)) return PBN_ERR_ARG;
        if ((uintptr_t)g_mask % elem_size(mask_dtype) || (uintptr_t)g_clt % elem_size(clt_dtype)) return PBN_ERR_ARG;
    }
    const Partials P(n_points, n_rows, n_prop);
    int r = PBN_OK;
    if (n_points > 0)
        r = launch_points({sem_score, sem_dtype, sem_ld, sem_label, offset_pred, offset_dtype, inst_info, xyz, ins_label, n_points,
                           n_class, P.gp, nullptr, state, grad_loss, g_sem, g_offset}, stream);
    if (r != PBN_OK) return r;
    if (n_rows > 0)
        r = launch_mask({pred_mask, mask_dtype, (int64_t*)gt_mask, (uint8_t*)mask_weight, n_rows, P.gm, nullptr, state, grad_loss,
                         g_mask}, stream);
    if (r != PBN_OK) return r;
    if (n_rows >= 0 && n_prop > 0) {
        hipLaunchKernelGGL(k_loss_scores_bwd, dim3(grid_points(n_prop)), dim3(TPB), 0, stream, clt_scores, clt_dtype, gt_scores,
                           (long long)n_prop, state, grad_loss, g_clt);
        PBN_LAUNCH_CHECK();
    }
    return PBN_OK;
}
