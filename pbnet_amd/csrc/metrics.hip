// metrics.hip -- the counts behind a validation epoch: semantic intersection / output / target histograms (and the K x K
// confusion table) of /root/reference/tools/mIOU.py:18-31, and the mask-branch agreement counts of
// /root/reference/train.py:152-168.  Integers only: every counter is a sum of ones, 32-bit in LDS, 64-bit in global memory,
// so a result does not depend on the order the workgroups arrive in (no floating-point atomics anywhere in the library).
//
// Shape of both kernels: grid-stride over GROUPS of 4 consecutive points, one group per lane and iteration, each array read
// with 16-byte loads (8 bytes for a 16-bit mask score) when the group's address allows and with scalar loads otherwise; the
// host picks the 0-3 leading points (`head`) that make the most bytes vector-loadable, workgroup 0 takes those and the 0-3
// trailing points one per lane.  A launch covers at most CHUNK points on at most GRID_CAP workgroups, so one workgroup
// never sees more than 2^26 + 8 points and a 32-bit counter cannot wrap.
//
// tools/mIOU.py bins with histc(bins=K, min=0, max=K-1): the integer v lands in bin floor(v * K / (K - 1)), which is v for
// 0 <= v < K - 1 (v / (K - 1) < 1) and the clamped last bin for v = K - 1, and nowhere for v outside [0, K - 1]: the
// identity on [0, K).  K = 1 would make min == max, where histc takes its range from the data instead: refused.
#include "pbn_common.h"
#include "vec4_dev.h"

namespace pbn {
namespace {

constexpr int TPB = 256;                    // 4 waves
constexpr int WAVES = TPB / WAVE;
constexpr int GRID_CAP = 1024;              // 4 workgroups per CU on 256 CUs; bounds the global adds of one launch
constexpr int MIN_ITERS = 4;                // a workgroup is worth starting for 4 * 1024 points
constexpr long long CHUNK = 1LL << 36;      // points per launch (a multiple of 4)
constexpr int MASK_DIRECT_MAX = 65536;      // rows one workgroup reduces alone (no zero fill, plain stores)

// LDS: `copies` private histograms of C = 3K (+ K*K) counters: intersection | output | target | confusion[target][pred].
template <typename TP, typename TT>
__global__ __launch_bounds__(TPB) void k_sem_confusion(const TP* __restrict__ pred, const TT* __restrict__ target, long long n,
                                                      int head, int vec_p, int vec_t, int K, long long ignore, int copies,
                                                      int has_conf, unsigned long long* __restrict__ acc3k,
                                                      unsigned long long* __restrict__ conf_kk) {
    extern __shared__ __attribute__((aligned(16))) unsigned hist[];
    const int tid = (int)threadIdx.x;
    const int C = 3 * K + (has_conf ? K * K : 0);
    for (int i = tid; i < copies * C; i += TPB) hist[i] = 0u;
    __syncthreads();
    unsigned* h = hist + (copies > 1 ? (tid >> 6) * C : 0);

    auto count = [&](long long p, long long t) {
        const bool t_in = t >= 0 && t < K;
        if (t_in) atomicAdd(&h[2 * K + (int)t], 1u);
        const bool live = t != ignore;
        const long long q = live ? p : ignore;            // mIOU.py:24 `output[target == ignore_index] = ignore_index`
        if (q >= 0 && q < K) {
            atomicAdd(&h[K + (int)q], 1u);
            if (q == t) atomicAdd(&h[(int)q], 1u);
            if (has_conf && live && t_in) atomicAdd(&h[3 * K + (int)t * K + (int)q], 1u);
        }
    };

    const long long groups = (n - head) >> 2;
    for (long long g = (long long)blockIdx.x * TPB + tid; g < groups; g += (long long)gridDim.x * TPB) {
        const long long i = head + 4 * g;
        TP pv[4];
        TT tv[4];
        load4(pred + i, vec_p != 0, pv);
        load4(target + i, vec_t != 0, tv);
#pragma unroll
        for (int j = 0; j < 4; ++j) count((long long)pv[j], (long long)tv[j]);
    }
    if (blockIdx.x == 0) {                                 // the unaligned head and the tail, one point per lane (< 8)
        const long long tail0 = head + 4 * groups;
        if (tid < head + (int)(n - tail0)) {
            const long long i = tid < head ? tid : tail0 + (tid - head);
            count((long long)pred[i], (long long)target[i]);
        }
    }
    __syncthreads();
    for (int c = tid; c < C; c += TPB) {
        unsigned long long s = 0;
        for (int w = 0; w < copies; ++w) s += hist[w * C + c];
        if (s != 0) atomicAdd(c < 3 * K ? &acc3k[c] : &conf_kk[c - 3 * K], s);
    }
}

// row8 = rows seen, agree, n_pos, pos_pred1, n_neg, neg_pred1, n_nan, 0.  direct: ONE workgroup, plain stores; otherwise
// the row was zeroed before the launch and every workgroup adds its non-zero sums.
template <int DT, typename TG>
__global__ __launch_bounds__(TPB) void k_mask_accuracy(const typename Elem<DT>::T* __restrict__ pred,
                                                      const TG* __restrict__ gt, long long n, int head, int vec_p, int vec_g,
                                                      float threshold, int direct, unsigned long long* __restrict__ row8) {
    typedef typename Elem<DT>::T TP;
    __shared__ int part[WAVES][8];
    const int tid = (int)threadIdx.x;
    int c[7] = {0, 0, 0, 0, 0, 0, 0};

    auto count = [&](TP raw, long long g) {
        const float v = Elem<DT>::widen(raw);
        const bool nan = v != v;
        const bool one = v >= threshold;                   // train.py:155 `>=`: exactly the threshold is 1
        const bool pos = g == 1, neg = g == 0;
        c[0] += 1;
        c[1] += (!nan && (one ? pos : neg)) ? 1 : 0;
        c[2] += pos ? 1 : 0;
        c[3] += (pos && one) ? 1 : 0;
        c[4] += neg ? 1 : 0;
        c[5] += (neg && one) ? 1 : 0;
        c[6] += nan ? 1 : 0;
    };

    const long long groups = (n - head) >> 2;
    for (long long g = (long long)blockIdx.x * TPB + tid; g < groups; g += (long long)gridDim.x * TPB) {
        const long long i = head + 4 * g;
        TP pv[4];
        TG gv[4];
        load4(pred + i, vec_p != 0, pv);
        load4(gt + i, vec_g != 0, gv);
#pragma unroll
        for (int j = 0; j < 4; ++j) count(pv[j], (long long)gv[j]);
    }
    if (blockIdx.x == 0) {
        const long long tail0 = head + 4 * groups;
        if (tid < head + (int)(n - tail0)) {
            const long long i = tid < head ? tid : tail0 + (tid - head);
            count(pred[i], (long long)gt[i]);
        }
    }
#pragma unroll
    for (int k = 0; k < 7; ++k) {
        const int s = wave_reduce_add(c[k]);
        if (lane_id() == 0) part[tid >> 6][k] = s;
    }
    __syncthreads();
    if (tid < 8) {
        unsigned long long s = 0;
        if (tid < 7)
            for (int w = 0; w < WAVES; ++w) s += (unsigned long long)part[w][tid];
        if (direct) row8[tid] = s;
        else if (s != 0) atomicAdd(&row8[tid], s);
    }
}

int grid_for(long long n) {
    const long long want = (n / 4 + (long long)TPB * MIN_ITERS - 1) / ((long long)TPB * MIN_ITERS);
    return (int)(want < 1 ? 1 : (want > GRID_CAP ? GRID_CAP : want));
}

template <typename TP, typename TT>
int launch_sem(const void* pred, const void* target, int64_t n, int K, int ignore_index, int64_t* acc3k, int64_t* conf_kk,
               hipStream_t stream) {
    const int C = 3 * K + (conf_kk ? K * K : 0);
    const int copies = K <= 32 ? WAVES : 1;                // K = 64 with the table: 17 KB for one copy, 69 KB for four
    for (int64_t o = 0; o < n; o += CHUNK) {
        const TP* p = (const TP*)pred + o;
        const TT* t = (const TT*)target + o;
        const long long m = n - o < CHUNK ? n - o : CHUNK;
        int vec_p = 0, vec_t = 0;
        int head = pick_head((uintptr_t)p, (int)sizeof(TP), (uintptr_t)t, (int)sizeof(TT), &vec_p, &vec_t);
        if (head > m) head = (int)m;
        hipLaunchKernelGGL((k_sem_confusion<TP, TT>), dim3(grid_for(m)), dim3(TPB), sizeof(unsigned) * copies * C, stream, p, t,
                           m, head, vec_p, vec_t, K, (long long)ignore_index, copies, conf_kk ? 1 : 0,
                           (unsigned long long*)acc3k, (unsigned long long*)conf_kk);
        PBN_LAUNCH_CHECK();
    }
    return PBN_OK;
}

template <int DT, typename TG>
int launch_mask(const void* pred, const void* gt, int64_t n, float threshold, int64_t* row8, hipStream_t stream) {
    typedef typename Elem<DT>::T TP;
    const int direct = n <= MASK_DIRECT_MAX;
    if (!direct) {
        const int rc = fill_bytes(row8, 0, 8 * sizeof(int64_t), stream);
        if (rc != PBN_OK) return rc;
    }
    for (int64_t o = 0; o < n || o == 0; o += CHUNK) {     // n == 0 still writes the (all-zero) row
        const TP* p = (const TP*)pred + o;
        const TG* g = (const TG*)gt + o;
        const long long m = n - o < CHUNK ? n - o : CHUNK;
        int vec_p = 0, vec_g = 0;
        int head = pick_head((uintptr_t)p, (int)sizeof(TP), (uintptr_t)g, (int)sizeof(TG), &vec_p, &vec_g);
        if (head > m) head = (int)m;
        hipLaunchKernelGGL((k_mask_accuracy<DT, TG>), dim3(direct ? 1 : grid_for(m)), dim3(TPB), 0, stream, p, g, m, head,
                           vec_p, vec_g, threshold, direct, (unsigned long long*)row8);
        PBN_LAUNCH_CHECK();
    }
    return PBN_OK;
}

}  // namespace
}  // namespace pbn

using namespace pbn;

extern "C" int pbn_sem_confusion(const void* pred, int pred_i64, const void* target, int target_i64, int64_t n, int n_class,
                                 int ignore_index, int64_t* acc3k, int64_t* conf_kk, pbn_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (n < 0 || !acc3k || n_class < 2 || n_class > 64) return PBN_ERR_ARG;
    if ((pred_i64 != 0 && pred_i64 != 1) || (target_i64 != 0 && target_i64 != 1)) return PBN_ERR_ARG;
    if (n == 0) return PBN_OK;
    if (!pred || !target) return PBN_ERR_ARG;
    if ((uintptr_t)pred % (pred_i64 ? 8 : 4) || (uintptr_t)target % (target_i64 ? 8 : 4)) return PBN_ERR_ARG;
    if (pred_i64)
        return target_i64 ? launch_sem<long long, long long>(pred, target, n, n_class, ignore_index, acc3k, conf_kk, stream)
                          : launch_sem<long long, int>(pred, target, n, n_class, ignore_index, acc3k, conf_kk, stream);
    return target_i64 ? launch_sem<int, long long>(pred, target, n, n_class, ignore_index, acc3k, conf_kk, stream)
                      : launch_sem<int, int>(pred, target, n, n_class, ignore_index, acc3k, conf_kk, stream);
}

extern "C" int pbn_mask_accuracy(const void* pred_mask, int dtype, const void* gt_mask, int gt_i64, int64_t n, float threshold,
                                 int64_t* row8, pbn_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (n < 0 || !row8 || (gt_i64 != 0 && gt_i64 != 1)) return PBN_ERR_ARG;
    if (dtype != PBN_F32 && dtype != PBN_BF16 && dtype != PBN_F16) return PBN_ERR_ARG;
    if (n > 0 && (!pred_mask || !gt_mask)) return PBN_ERR_ARG;
    if ((uintptr_t)pred_mask % (dtype == PBN_F32 ? 4 : 2) || (uintptr_t)gt_mask % (gt_i64 ? 8 : 4)) return PBN_ERR_ARG;
    switch (dtype * 2 + gt_i64) {
        case PBN_F32 * 2 + 0: return launch_mask<PBN_F32, int>(pred_mask, gt_mask, n, threshold, row8, stream);
        case PBN_F32 * 2 + 1: return launch_mask<PBN_F32, long long>(pred_mask, gt_mask, n, threshold, row8, stream);
        case PBN_BF16 * 2 + 0: return launch_mask<PBN_BF16, int>(pred_mask, gt_mask, n, threshold, row8, stream);
        case PBN_BF16 * 2 + 1: return launch_mask<PBN_BF16, long long>(pred_mask, gt_mask, n, threshold, row8, stream);
        case PBN_F16 * 2 + 0: return launch_mask<PBN_F16, int>(pred_mask, gt_mask, n, threshold, row8, stream);
        default: return launch_mask<PBN_F16, long long>(pred_mask, gt_mask, n, threshold, row8, stream);
    }
}
