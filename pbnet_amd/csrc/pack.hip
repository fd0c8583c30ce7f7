// pack.hip -- weight packing: fp32 master [K, A, B] -> MFMA-fragment order (include/pbnet_hip.h, pbn_spconv_forward).
#include "pbn_common.h"

namespace pbn {
namespace {

constexpr int TPB = 256;

// element (k, ci, co) of the convolution = src[flip ? K-1-k : k][ci][co], or [..][co][ci] when `transpose` (the dgrad
// weights of a forward kernel).  One thread per packed element; E = elements per 16-byte vector.
template <typename T>
__device__ __forceinline__ void pack_weight_element(const float* __restrict__ src, int K, int A, int B, int flip, int transpose,
                                                    int cin, int cout, int cin_p, int cout_p, long long e, T* __restrict__ out) {
    constexpr int E = 16 / (int)sizeof(T);
    const int ntt = cout_p / 16;
    const int j = (int)(e % E);
    const int lane = (int)((e / E) % 64);
    const int tt = (int)((e / (E * 64)) % ntt);
    const int st = (int)(e / ((long long)E * 64 * ntt));
    const int g = lane >> 4, c = lane & 15;
    const int r = st * 4 * E + g * E + j;           // row of the flattened (offset, channel) axis
    const int k = r / cin_p, ci = r - k * cin_p;
    const int co = tt * 16 + c;
    float v = 0.f;
    if (k < K && ci < cin && co < cout) {
        const int ks = flip ? K - 1 - k : k;
        v = transpose ? src[((size_t)ks * A + co) * B + ci] : src[((size_t)ks * A + ci) * B + co];
    }
    st_f32(out + e, v);
}

template <typename T>
__global__ __launch_bounds__(TPB) void k_pack_weight(const float* __restrict__ src, int K, int A, int B, int flip,
                                                    int transpose, int cin, int cout, int cin_p, int cout_p, int n_steps,
                                                    T* __restrict__ out) {
    constexpr int E = 16 / (int)sizeof(T);
    const long long e = (long long)blockIdx.x * TPB + threadIdx.x;
    const long long total = (long long)n_steps * (cout_p / 16) * 64 * E;
    if (e >= total) return;
    pack_weight_element<T>(src, K, A, B, flip, transpose, cin, cout, cin_p, cout_p, e, out);
}

// every layer's weights (both the forward and the input-gradient form) in ONE launch: blockIdx.y = job of a device table
template <typename T>
__global__ __launch_bounds__(TPB) void k_pack_weights_batch(const pbn_pack_job* __restrict__ jobs) {
    constexpr int E = 16 / (int)sizeof(T);
    const pbn_pack_job jb = jobs[blockIdx.y];
    const long long total = (long long)jb.n_steps * (jb.cout_p / 16) * 64 * E;
    for (long long e = (long long)blockIdx.x * TPB + threadIdx.x; e < total; e += (long long)gridDim.x * TPB)
        pack_weight_element<T>(jb.src, jb.n_offsets, jb.dim_a, jb.dim_b, jb.flip, jb.transpose, jb.cin, jb.cout, jb.cin_p,
                               jb.cout_p, e, (T*)jb.out);
}

}  // namespace
}  // namespace pbn

using namespace pbn;

extern "C" int pbn_pack_weight(const float* src, int n_offsets, int dim_a, int dim_b, int flip, int transpose, int dtype,
                               int vecs_per_offset, int n_steps, int cout_padded, void* out, pbn_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!src || !out || n_offsets < 1 || dim_a < 1 || dim_b < 1 || vecs_per_offset < 1 || n_steps < 1 || cout_padded < 16 ||
        (cout_padded & 15))
        return PBN_ERR_ARG;
    const int esz = dtype == PBN_F32 ? 4 : 2;
    const int e = 16 / esz;
    const int cin = transpose ? dim_b : dim_a, cout = transpose ? dim_a : dim_b;
    const int cin_p = vecs_per_offset * e;
    if (cin_p < cin || cout_padded < cout || (long long)n_steps * 4 * e < (long long)n_offsets * cin_p) return PBN_ERR_ARG;
    const long long total = (long long)n_steps * (cout_padded / 16) * 64 * e;
    if (!dispatch_dtype(dtype, [&](auto t) {
            using T = decltype(t);
            hipLaunchKernelGGL(k_pack_weight<T>, dim3(cdiv(total, TPB)), dim3(TPB), 0, stream, src, n_offsets, dim_a, dim_b, flip,
                               transpose, cin, cout, cin_p, cout_padded, n_steps, (T*)out);
        }))
        return PBN_ERR_ARG;
    PBN_LAUNCH_CHECK();
    return PBN_OK;
}

extern "C" int pbn_pack_weights_batch(const pbn_pack_job* jobs_dev, int n_jobs, int max_vectors, int dtype, pbn_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (n_jobs < 0 || max_vectors < 0) return PBN_ERR_ARG;
    if (n_jobs == 0 || max_vectors == 0) return PBN_OK;
    if (!jobs_dev || n_jobs > 65535) return PBN_ERR_ARG;
    const int e = dtype == PBN_F32 ? 4 : 8;
    long long bx = cdiv((long long)max_vectors * e, TPB);
    if (bx > 512) bx = 512;
    const dim3 grid((unsigned)bx, (unsigned)n_jobs);
    if (!dispatch_dtype(dtype, [&](auto t) {
            hipLaunchKernelGGL(k_pack_weights_batch<decltype(t)>, grid, dim3(TPB), 0, stream, jobs_dev);
        }))
        return PBN_ERR_ARG;
    PBN_LAUNCH_CHECK();
    return PBN_OK;
}
