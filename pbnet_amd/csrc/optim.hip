// optim.hip -- the optimizer step of the training loop (train.py:350-357: Adam, SGD with momentum, AdamW) as ONE launch over
// every tensor that shares a step count, and the running loss meters of train_epoch (tools/log.py:16-30 AverageMeter).
//
// Multi-tensor shape: the host cuts every tensor into chunks of at most PBN_OPTIM_CHUNK elements and uploads one record per
// chunk (pbn_optim_chunk_rec).  A workgroup takes whole chunks, grid-stride over the table; inside a chunk one thread owns one
// group of four consecutive elements per iteration (one element on the dword path), reads parameter, gradient and state once
// and writes parameter and state once: no atomics, no reduction, a result does not depend on the grid.  A chunk whose four
// addresses are all 16-byte aligned (the host decides and records it) moves as 16-byte vectors with a 0-3 element tail;
// gradients are views into flat buffers at arbitrary element offsets, so the other chunks move dword by dword.
//
// Arithmetic contract (tests/optim_ref.py restates it in numpy float32): every operation below is one float32 operation
// rounded once, in the written order.  Built with -ffp-contract=off (no FMA), no fast-math; '/' and sqrtf are correctly
// rounded (hipcc's default for HIP, -fhip-fp32-correctly-rounded-divide-sqrt) and denormals are kept.  The scalars are
// formed by the host in float64 and rounded to float32 once; they arrive as kernel arguments.
#include "pbn_common.h"
#include "vec4_dev.h"

#pragma clang fp contract(off)

namespace pbn {
namespace {

constexpr int TPB = 256;                    // 4 waves
constexpr int GRID_CAP = 2048;              // 8 workgroups per CU on 256 CUs; the rest of the table is grid-strided
static_assert(PBN_OPTIM_CHUNK % (4 * TPB) == 0, "a chunk is a whole number of 16-byte passes of one workgroup");

struct AdamRule {
    float lr, beta1, one_minus_beta1, beta2, one_minus_beta2, eps, weight_decay, step_size, bc2_sqrt;
    int decoupled;
    // s0 = exp_avg, s1 = exp_avg_sq
    __device__ __forceinline__ void operator()(float& p, float g, float& m, float& v) const {
        if (weight_decay != 0.0f) {
            if (decoupled) {
                const float shrink = lr * weight_decay;
                p = p * (1.0f - shrink);
            } else {
                const float wp = weight_decay * p;
                g = g + wp;
            }
        }
        const float dm = g - m;
        const float sm = dm * one_minus_beta1;
        m = m + sm;
        const float vb = v * beta2;
        const float gg = g * g;
        const float sg = gg * one_minus_beta2;
        v = vb + sg;
        const float r = sqrtf(v);
        const float q = r / bc2_sqrt;
        const float d = q + eps;
        const float u = m / d;
        const float su = step_size * u;
        p = p - su;
    }
};

struct SgdRule {
    float lr, momentum, weight_decay;
    int first;
    // s0 = momentum_buffer; s1 unused
    __device__ __forceinline__ void operator()(float& p, float g, float& buf, float&) const {
        if (weight_decay != 0.0f) {
            const float wp = weight_decay * p;
            g = g + wp;
        }
        if (first) {
            buf = g;
        } else {
            const float bm = buf * momentum;
            buf = bm + g;
        }
        const float sb = lr * buf;
        p = p - sb;
    }
};

template <typename Rule, bool TWO_STATES>
__global__ __launch_bounds__(TPB) void k_optim_step(const pbn_optim_chunk_rec* __restrict__ table, int n_chunks, Rule rule) {
    const int tid = (int)threadIdx.x;
    for (int c = (int)blockIdx.x; c < n_chunks; c += (int)gridDim.x) {
        const pbn_optim_chunk_rec rec = table[c];
        float* __restrict__ p = (float*)rec.param;
        const float* __restrict__ g = (const float*)rec.grad;
        float* __restrict__ s0 = (float*)rec.state0;
        float* __restrict__ s1 = (float*)rec.state1;
        const int n = rec.n < PBN_OPTIM_CHUNK ? rec.n : PBN_OPTIM_CHUNK;    // a record can never reach past its chunk
        if (rec.vec) {
            const int groups = n >> 2;
            for (int q = tid; q < groups; q += TPB) {
                const int i = 4 * q;
                float pv[4], gv[4], av[4], bv[4] = {0.0f, 0.0f, 0.0f, 0.0f};
                load4(p + i, true, pv);
                load4(g + i, true, gv);
                load4(s0 + i, true, av);
                if (TWO_STATES) load4(s1 + i, true, bv);
#pragma unroll
                for (int j = 0; j < 4; ++j) rule(pv[j], gv[j], av[j], bv[j]);
                store4(p + i, true, pv);
                store4(s0 + i, true, av);
                if (TWO_STATES) store4(s1 + i, true, bv);
            }
            const int i = 4 * groups + tid;                                   // the 0-3 trailing elements
            if (tid < 4 && i < n) {
                float pv = p[i], av = s0[i], bv = TWO_STATES ? s1[i] : 0.0f;
                rule(pv, g[i], av, bv);
                p[i] = pv;
                s0[i] = av;
                if (TWO_STATES) s1[i] = bv;
            }
        } else {
            for (int i = tid; i < n; i += TPB) {
                float pv = p[i], av = s0[i], bv = TWO_STATES ? s1[i] : 0.0f;
                rule(pv, g[i], av, bv);
                p[i] = pv;
                s0[i] = av;
                if (TWO_STATES) s1[i] = bv;
            }
        }
    }
}

// terms f32[k], weights f64[k]; acc f64[3k] = last value | sum of value * weight | sum of weight (AverageMeter's val, sum,
// count).  One workgroup of one wave, lane j owns term j: a fixed order, no atomics.
__global__ __launch_bounds__(WAVE) void k_loss_meter_update(const float* __restrict__ terms, const double* __restrict__ weights,
                                                           double* __restrict__ acc, int k) {
    for (int j = (int)threadIdx.x; j < k; j += WAVE) {
        const double v = (double)terms[j], w = weights[j];
        const double vw = v * w;
        acc[j] = v;
        acc[k + j] = acc[k + j] + vw;
        acc[2 * k + j] = acc[2 * k + j] + w;
    }
}

template <typename Rule, bool TWO_STATES>
int launch_step(const void* table, int n_chunks, const Rule& rule, hipStream_t stream) {
    const int grid = n_chunks < GRID_CAP ? n_chunks : GRID_CAP;
    hipLaunchKernelGGL((k_optim_step<Rule, TWO_STATES>), dim3(grid), dim3(TPB), 0, stream, (const pbn_optim_chunk_rec*)table,
                       n_chunks, rule);
    PBN_LAUNCH_CHECK();
    return PBN_OK;
}

bool is_finite_f(float x) { return x == x && x - x == 0.0f; }

}  // namespace
}  // namespace pbn

using namespace pbn;

extern "C" int pbn_optim_chunk(void) { return PBN_OPTIM_CHUNK; }

extern "C" int pbn_optim_adam(const void* table, int n_chunks, float lr, float beta1, float one_minus_beta1, float beta2,
                              float one_minus_beta2, float eps, float weight_decay, float step_size, float bc2_sqrt,
                              int decoupled, pbn_stream_t stream) {
    if (n_chunks < 0 || (decoupled != 0 && decoupled != 1)) return PBN_ERR_ARG;
    if (!is_finite_f(lr) || !is_finite_f(step_size) || !is_finite_f(weight_decay) || !(bc2_sqrt > 0.0f) || !(eps >= 0.0f)) return PBN_ERR_ARG;
    if (n_chunks == 0) return PBN_OK;
    if (!table || (uintptr_t)table % 8) return PBN_ERR_ARG;
    const AdamRule rule{lr, beta1, one_minus_beta1, beta2, one_minus_beta2, eps, weight_decay, step_size, bc2_sqrt, decoupled};
    return launch_step<AdamRule, true>(table, n_chunks, rule, (hipStream_t)stream);
}

extern "C" int pbn_optim_sgd(const void* table, int n_chunks, float lr, float momentum, float weight_decay, int first,
                             pbn_stream_t stream) {
    if (n_chunks < 0 || (first != 0 && first != 1)) return PBN_ERR_ARG;
    if (!is_finite_f(lr) || !is_finite_f(momentum) || !is_finite_f(weight_decay)) return PBN_ERR_ARG;
    if (n_chunks == 0) return PBN_OK;
    if (!table || (uintptr_t)table % 8) return PBN_ERR_ARG;
    const SgdRule rule{lr, momentum, weight_decay, first};
    return launch_step<SgdRule, false>(table, n_chunks, rule, (hipStream_t)stream);
}

extern "C" int pbn_loss_meter_update(const float* terms, const double* weights, double* acc, int k, pbn_stream_t stream) {
    if (k < 0 || k > 1024) return PBN_ERR_ARG;
    if (k == 0) return PBN_OK;
    if (!terms || !weights || !acc) return PBN_ERR_ARG;
    if ((uintptr_t)terms % 4 || (uintptr_t)weights % 8 || (uintptr_t)acc % 8) return PBN_ERR_ARG;
    hipLaunchKernelGGL(k_loss_meter_update, dim3(1), dim3(WAVE), 0, (hipStream_t)stream, terms, weights, acc, k);
    PBN_LAUNCH_CHECK();
    return PBN_OK;
}
