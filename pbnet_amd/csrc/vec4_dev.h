// vec4_dev.h -- the memory shape of the library's streaming kernels (metrics.hip, losses.hip): four consecutive elements per
// lane, read or written with one aligned vector access (16 bytes; 8 for a 16-bit type) when the address allows and with four
// scalar accesses otherwise, and the PBN_F32 / PBN_BF16 / PBN_F16 storage types with their float32 conversions.
#pragma once
#include <hip/hip_fp16.h>

#include "pbn_common.h"

namespace pbn {

// four consecutive elements: one or two aligned vector loads, or four scalar loads
__device__ __forceinline__ void load4(const int* p, bool vec, int (&v)[4]) {
    if (vec) {
        const int4 q = *reinterpret_cast<const int4*>(p);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = p[j];
    }
}
__device__ __forceinline__ void load4(const long long* p, bool vec, long long (&v)[4]) {
    if (vec) {
        const longlong2 a = *reinterpret_cast<const longlong2*>(p), b = *reinterpret_cast<const longlong2*>(p + 2);
        v[0] = a.x; v[1] = a.y; v[2] = b.x; v[3] = b.y;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = p[j];
    }
}
__device__ __forceinline__ void load4(const float* p, bool vec, float (&v)[4]) {
    if (vec) {
        const float4 q = *reinterpret_cast<const float4*>(p);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = p[j];
    }
}
__device__ __forceinline__ void load4(const unsigned short* p, bool vec, unsigned short (&v)[4]) {
    if (vec) {
        const ushort4 q = *reinterpret_cast<const ushort4*>(p);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = p[j];
    }
}
__device__ __forceinline__ void store4(float* p, bool vec, const float (&v)[4]) {
    if (vec) {
        *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) p[j] = v[j];
    }
}
__device__ __forceinline__ void store4(unsigned short* p, bool vec, const unsigned short (&v)[4]) {
    if (vec) {
        *reinterpret_cast<ushort4*>(p) = make_ushort4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) p[j] = v[j];
    }
}

// storage type of a pbn_dtype; widen is exact, narrow rounds to nearest even once
template <int DT>
struct Elem;
template <>
struct Elem<PBN_F32> {
    typedef float T;
    static __device__ __forceinline__ float widen(float v) { return v; }
    static __device__ __forceinline__ float narrow(float v) { return v; }
};
template <>
struct Elem<PBN_BF16> {
    typedef unsigned short T;
    static __device__ __forceinline__ float widen(unsigned short v) { return __uint_as_float((unsigned)v << 16); }
    static __device__ __forceinline__ unsigned short narrow(float v) {
        const unsigned u = __float_as_uint(v);
        if (v != v) return (unsigned short)((u >> 16) | 0x40u);
        return (unsigned short)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
    }
};
template <>
struct Elem<PBN_F16> {
    typedef unsigned short T;
    static __device__ __forceinline__ float widen(unsigned short v) { return __half2float(__ushort_as_half(v)); }
    static __device__ __forceinline__ unsigned short narrow(float v) { return __half_as_ushort(__float2half_rn(v)); }
};

// The 0-3 leading points after which the most bytes per group come from aligned vector loads.  A group of array X loads as
// vectors when its address is a multiple of min(16, 4 * element size).
static inline int pick_head(uintptr_t a, int es_a, uintptr_t b, int es_b, int* vec_a, int* vec_b) {
    const int al_a = 4 * es_a < 16 ? 4 * es_a : 16, al_b = 4 * es_b < 16 ? 4 * es_b : 16;
    int best = 0, best_score = -1;
    for (int h = 0; h < 4; ++h) {
        const int va = (a + (uintptr_t)h * es_a) % al_a == 0, vb = (b + (uintptr_t)h * es_b) % al_b == 0;
        const int score = va * es_a + vb * es_b;
        if (score > best_score) { best = h; best_score = score; *vec_a = va; *vec_b = vb; }
    }
    return best;
}

}  // namespace pbn
