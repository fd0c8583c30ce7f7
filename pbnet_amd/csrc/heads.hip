// heads.hip -- the two-layer heads of PBNet (the reference's network/PBNet.py:43-82, eval mode) evaluated at gathered rows:
// out = act(W2 . prelu(bn(W1 . x)) + b2) per row, one launch per head (pbn_mlp_rows).
#include "pbn_common.h"

namespace pbn {
namespace {

constexpr int TPB = 256;

// One thread per output row; the row is read through up to two index levels (row = idx_b[idx_a[i]]), so "gather the
// voxel features to the points" and "undo the Z-order" cost nothing extra.  All arithmetic in fp32, weights are uniform
// (scalar loads), one rounding at the end.
// RowIO<T>: E elements of a 16-byte vector as floats
template <typename T> struct RowIO;
template <> struct RowIO<float> {
    static constexpr int E = 4;
    static __device__ __forceinline__ void unpack(const uint4& v, float* f) {
        f[0] = __uint_as_float(v.x); f[1] = __uint_as_float(v.y); f[2] = __uint_as_float(v.z); f[3] = __uint_as_float(v.w);
    }
};
template <> struct RowIO<__hip_bfloat16> {
    static constexpr int E = 8;
    static __device__ __forceinline__ void unpack(const uint4& v, float* f) {
        const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int i = 0; i < 4; ++i) { f[2 * i] = __uint_as_float(w[i] << 16); f[2 * i + 1] = __uint_as_float(w[i] & 0xffff0000u); }
    }
};
template <> struct RowIO<__half> {
    static constexpr int E = 8;
    static __device__ __forceinline__ void unpack(const uint4& v, float* f) {
        const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float2 t = __half22float2(__builtin_bit_cast(__half2, w[i]));
            f[2 * i] = t.x; f[2 * i + 1] = t.y;
        }
    }
};

template <typename T, int C, int H>
__global__ __launch_bounds__(TPB) void k_mlp_rows(const T* __restrict__ in, int ld_in, const long long* __restrict__ idx_a,
                                                 const long long* __restrict__ idx_b, int n_cap,
                                                 const int* __restrict__ n_dev, long long in_rows,
                                                 const float* __restrict__ w1, const float* __restrict__ scale,
                                                 const float* __restrict__ shift, const float* __restrict__ slope,
                                                 const float* __restrict__ w2, const float* __restrict__ b2, int n_out,
                                                 int sigmoid, T* __restrict__ out, int ld_out) {
    constexpr int E = RowIO<T>::E;
    const int n = n_dev ? min(*n_dev, n_cap) : n_cap;
    const int i = blockIdx.x * TPB + threadIdx.x;
    if (i >= n) return;
    long long row = idx_a ? idx_a[i] : i;
    if (idx_b && row >= 0) row = idx_b[row];
    float x[C];
    // a resolved row outside the slab (capacity-planned mode: a level overflowed its capacity and the index tables name
    // rows that were never computed) reads as zeros instead of memory past the slab; the overflow itself is flagged elsewhere
    const bool inside = row >= 0 && (in_rows < 0 || row < in_rows);
    const uint4* src = reinterpret_cast<const uint4*>(in + (size_t)(inside ? row : 0) * ld_in);
#pragma unroll
    for (int v = 0; v < C / E; ++v) {
        RowIO<T>::unpack(inside ? src[v] : make_uint4(0u, 0u, 0u, 0u), x + v * E);
    }
    float h[H];
#pragma unroll
    for (int k = 0; k < H; ++k) {
        float a = 0.f;
#pragma unroll
        for (int c = 0; c < C; ++c) a = fmaf(w1[k * C + c], x[c], a);
        a = fmaf(a, scale[k], shift[k]);
        h[k] = a >= 0.f ? a : a * slope[k];
    }
    for (int o = 0; o < n_out; ++o) {
        float a = b2 ? b2[o] : 0.f;
#pragma unroll
        for (int k = 0; k < H; ++k) a = fmaf(w2[o * H + k], h[k], a);
        if (sigmoid) a = 1.0f / (1.0f + expf(-a));
        st_f32(out + (size_t)i * ld_out + o, a);
    }
}

// The same heads on the matrix cores (round 4).  k_mlp_rows is latency-bound per wave: every thread streams the 1 024 + H n_out
// weights through scalar loads for 1 700 dependent FMAs (38 us for 161 k rows of a 32 -> 32 -> 32 head whose arithmetic is 3 us
// of the vector ALUs).  Here a wave takes 16 rows per round on v_mfma_f32_16x16x4_f32 (exact fp32: an fmaf chain), both layers
// TRANSPOSED so that no operand ever changes lanes:
//   layer 1:  D1[h][row] = sum_c W1[h][c] x[row][c]      A = W1 (lane (kq, h) holds w1[h][8 kq + kb] for step kb),
//                                                        B = x^T (lane (kq, row) holds the 8 channels 8 kq .. 8 kq + 7 of its row:
//                                                        ONE 16-byte load for 16-bit slabs); D1: lane (q, row) = hidden 4 q + i
//   layer 2:  D2[o][row] = sum_h W2[o][h] hid[row][h]    B = the D1 registers as they are (step (t, i): hidden 16 t + 4 kq + i),
//                                                        A = W2 indexed accordingly; D2: lane (q, row) = outputs 4 q + i of its row
// Weights, BatchNorm constants and slopes live in registers for the wave's whole loop over row blocks.  Summation order differs from
// k_mlp_rows (channels 0, 8, 16, 24, 1, 9, ...): fp32 results agree to rounding (tests: 1e-5).
typedef float mlp_f32x4 __attribute__((ext_vector_type(4)));
template <typename T, int H, int U>
__global__ __launch_bounds__(TPB) void k_mlp_rows_mfma(const T* __restrict__ in, int ld_in, const long long* __restrict__ idx_a,
                                                      const long long* __restrict__ idx_b, int n_cap,
                                                      const int* __restrict__ n_dev, long long in_rows,
                                                      const float* __restrict__ w1, const float* __restrict__ scale,
                                                      const float* __restrict__ shift, const float* __restrict__ slope,
                                                      const float* __restrict__ w2, const float* __restrict__ b2, int n_out,
                                                      int sigmoid, T* __restrict__ out, int ld_out) {
    constexpr int C = 32, HT = H / 16;
    const int n = n_dev ? min(*n_dev, n_cap) : n_cap;
    const int lane = threadIdx.x & 63, kq = lane >> 4, r = lane & 15;
    const int wave = (int)((blockIdx.x * TPB + threadIdx.x) >> 6), n_waves = (int)((gridDim.x * TPB) >> 6);
    // ---- per-wave constants ----
    float a1[HT][8];                 // layer-1 A operands: w1[16 t + r][8 kq + kb]
#pragma unroll
    for (int t = 0; t < HT; ++t)
#pragma unroll
        for (int kb = 0; kb < 8; ++kb) a1[t][kb] = w1[(16 * t + r) * C + 8 * kq + kb];
    float sc[HT][4], sh[HT][4], sl[HT][4];      // of hidden 16 t + 4 kq + i (this lane's D1 registers)
#pragma unroll
    for (int t = 0; t < HT; ++t)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int hh = 16 * t + 4 * kq + i;
            sc[t][i] = scale[hh]; sh[t][i] = shift[hh]; sl[t][i] = slope[hh];
        }
    float a2[U][HT][4];              // layer-2 A operands: w2[16 u + r][16 t + 4 kq + i]
    float bias[U][4];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int o = 16 * u + r;
#pragma unroll
        for (int t = 0; t < HT; ++t)
#pragma unroll
            for (int i = 0; i < 4; ++i) a2[u][t][i] = o < n_out ? w2[o * H + 16 * t + 4 * kq + i] : 0.0f;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int oo = 16 * u + 4 * kq + i;
            bias[u][i] = (b2 && oo < n_out) ? b2[oo] : 0.0f;
        }
    }
    for (int blk = wave; blk * 16 < n; blk += n_waves) {
        const int i_row = blk * 16 + r;
        long long row = -1;
        if (i_row < n) {
            row = idx_a ? idx_a[i_row] : i_row;
            if (idx_b && row >= 0) row = idx_b[row];
        }
        const bool inside = row >= 0 && (in_rows < 0 || row < in_rows);
        float x[8];
        {
            const unsigned char* src = reinterpret_cast<const unsigned char*>(in + (size_t)(inside ? row : 0) * ld_in) + (size_t)kq * 8 * sizeof(T);
            if constexpr (sizeof(T) == 4) {
                const uint4 v0 = inside ? reinterpret_cast<const uint4*>(src)[0] : make_uint4(0u, 0u, 0u, 0u);
                const uint4 v1 = inside ? reinterpret_cast<const uint4*>(src)[1] : make_uint4(0u, 0u, 0u, 0u);
                RowIO<T>::unpack(v0, x);
                RowIO<T>::unpack(v1, x + 4);
            } else {
                RowIO<T>::unpack(inside ? reinterpret_cast<const uint4*>(src)[0] : make_uint4(0u, 0u, 0u, 0u), x);
            }
        }
        mlp_f32x4 d1[HT];
#pragma unroll
        for (int t = 0; t < HT; ++t) {
            d1[t] = mlp_f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int kb = 0; kb < 8; ++kb) d1[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1[t][kb], x[kb], d1[t], 0, 0, 0);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float v = fmaf(d1[t][i], sc[t][i], sh[t][i]);
                d1[t][i] = v >= 0.f ? v : v * sl[t][i];
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            mlp_f32x4 d2 = mlp_f32x4{bias[u][0], bias[u][1], bias[u][2], bias[u][3]};
#pragma unroll
            for (int t = 0; t < HT; ++t)
#pragma unroll
                for (int i = 0; i < 4; ++i) d2 = __builtin_amdgcn_mfma_f32_16x16x4f32(a2[u][t][i], d1[t][i], d2, 0, 0, 0);
            if (i_row < n) {
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int oo = 16 * u + 4 * kq + i;
                    if (oo < n_out) {
                        float v = d2[i];
                        if (sigmoid) v = 1.0f / (1.0f + expf(-v));
                        st_f32(out + (size_t)i_row * ld_out + oo, v);
                    }
                }
            }
        }
    }
}

}  // namespace
}  // namespace pbn

using namespace pbn;

extern "C" int pbn_mlp_rows(const void* in, int ld_in, int in_rows, int channels, const int64_t* idx_a, const int64_t* idx_b,
                            int n, const int32_t* n_dev, const float* w1, const float* scale, const float* shift,
                            const float* slope, int hidden, const float* w2, const float* b2, int n_out, int sigmoid,
                            void* out, int ld_out, int dtype, pbn_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (n < 0 || n_out < 1 || ld_out < n_out || ld_in < channels) return PBN_ERR_ARG;
    if (channels != 32 || (hidden != 16 && hidden != 32)) return PBN_ERR_UNSUPPORTED;
    if (n == 0) return PBN_OK;
    if (!in || !w1 || !scale || !shift || !slope || !w2 || !out) return PBN_ERR_ARG;
    const int esz = dtype == PBN_F32 ? 4 : 2;
    if ((ld_in * esz) % 16 || ((uintptr_t)in & 15)) return PBN_ERR_ARG;
    // matrix-core form (default; PBN_MLP_FORM=0: the scalar kernel, kept as the cross-check): 16 rows per wave and round
    static const int form_env = getenv("PBN_MLP_FORM") ? atoi(getenv("PBN_MLP_FORM")) : 1;
    const bool mfma = form_env != 0 && n_out <= 32;
    long long wgs = cdiv(n, TPB);
    if (mfma) {
        // ~4 row blocks per wave: the ~60 register-resident weight words of a wave pay off (scripts/probe_heads.py, HIP-graph replay,
        // 161 517 gathered rows, bf16: 32->32->32 35.3 -> 24.4 us, 32->16->20 16.8 -> 12.7, the 3- and 1-output heads 8.6 either way;
        // one block per wave: no gain at all).  PBN_MLP_BLOCKS: row blocks per wave (measurement)
        static const int bpw_env = getenv("PBN_MLP_BLOCKS") ? atoi(getenv("PBN_MLP_BLOCKS")) : 4;
        wgs = cdiv(cdiv(n, 16), (TPB / 64) * (bpw_env > 0 ? bpw_env : 1));
        if (wgs > 8192) wgs = 8192;
        if (wgs < 1) wgs = 1;
    }
    const bool known = dispatch_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        auto launch = [&](auto kernel) {
            hipLaunchKernelGGL(kernel, dim3((unsigned)wgs), dim3(TPB), 0, stream, (const T*)in, ld_in, (const long long*)idx_a,
                               (const long long*)idx_b, n, n_dev, (long long)in_rows, w1, scale, shift, slope, w2, b2, n_out,
                               sigmoid, (T*)out, ld_out);
        };
        if (!mfma) {
            if (hidden == 16) launch(k_mlp_rows<T, 32, 16>);
            else launch(k_mlp_rows<T, 32, 32>);
        } else if (hidden == 16) {
            if (n_out <= 16) launch(k_mlp_rows_mfma<T, 16, 1>);
            else launch(k_mlp_rows_mfma<T, 16, 2>);
        } else {
            if (n_out <= 16) launch(k_mlp_rows_mfma<T, 32, 1>);
            else launch(k_mlp_rows_mfma<T, 32, 2>);
        }
    });
    if (!known) return PBN_ERR_ARG;
    PBN_LAUNCH_CHECK();
    return PBN_OK;
}
