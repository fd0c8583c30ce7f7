// pbn_common.h -- shared helpers for the gfx950 kernels of libpbnet_hip.so (wave64, CDNA4 only).
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <hip/hip_fp16.h>
#include <stdint.h>
#include "../../include/pbnet_hip.h"

namespace pbn {

constexpr int WAVE = 64;
// classes a semantic head may have: bounds the LDS tables of k_sem_argmax_table / k_select_points (front.hip) and the score
// registers of k_summary_points (summary.hip)
constexpr int SEL_MAX_CLASSES = 32;

extern thread_local int g_last_hip_error;

#define PBN_HIP_CHECK(expr)                                  \
    do {                                                     \
        hipError_t _e = (expr);                              \
        if (_e != hipSuccess) {                              \
            pbn::g_last_hip_error = (int)_e;                 \
            return PBN_ERR_HIP;                              \
        }                                                    \
    } while (0)

#define PBN_LAUNCH_CHECK() PBN_HIP_CHECK(hipGetLastError())

// returns the status of a failing call of this library (fill_bytes, scan_exclusive_i32, ...)
#define PBN_TRY(expr)                                        \
    do {                                                     \
        const int _rc = (expr);                              \
        if (_rc != PBN_OK) return _rc;                       \
    } while (0)

// calls f with a value of the element type of `dtype` (a generic lambda: `using T = decltype(t)`); false = unknown dtype
template <typename F>
static inline bool dispatch_dtype(int dtype, F&& f) {
    if (dtype == PBN_F32) f(float{});
    else if (dtype == PBN_BF16) f(__hip_bfloat16{});
    else if (dtype == PBN_F16) f(__half{});
    else return false;
    return true;
}

template <typename T> __device__ __forceinline__ float to_f32(T v);
template <> __device__ __forceinline__ float to_f32<float>(float v) { return v; }
template <> __device__ __forceinline__ float to_f32<__hip_bfloat16>(__hip_bfloat16 v) { return __bfloat162float(v); }
template <> __device__ __forceinline__ float to_f32<__half>(__half v) { return __half2float(v); }
// *p = v, rounded once (to nearest even) to T
template <typename T> __device__ __forceinline__ void st_f32(T* p, float v);
template <> __device__ __forceinline__ void st_f32<float>(float* p, float v) { *p = v; }
template <> __device__ __forceinline__ void st_f32<__hip_bfloat16>(__hip_bfloat16* p, float v) { *p = __float2bfloat16(v); }
template <> __device__ __forceinline__ void st_f32<__half>(__half* p, float v) { *p = __float2half(v); }

static inline int cdiv(long long a, long long b) { return (int)((a + b - 1) / b); }
static inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

// Bump allocator over a caller-provided workspace (256-byte aligned carves).
struct Carver {
    char* base;
    size_t off;
    size_t cap;
    bool ok;
    Carver(void* p, size_t bytes) : base((char*)p), off(0), cap(bytes), ok(true) {}
    template <typename T>
    T* take(size_t n) {
        size_t start = align_up(off, 256);
        size_t end = start + n * sizeof(T);
        if (base != nullptr && end > cap) ok = false;
        off = end;
        return base ? (T*)(base + start) : (T*)nullptr;
    }
};

__device__ __forceinline__ int lane_id() { return (int)(threadIdx.x & 63); }

__device__ __forceinline__ int wave_reduce_add(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// element i of an int32 or int64 vector
__device__ __forceinline__ long long load_index(const void* p, int is_i64, long long i) {
    return is_i64 ? ((const long long*)p)[i] : (long long)((const int*)p)[i];
}

// order-preserving key of a float32 (augment.hip's okey for 32 bits): a < b  <=>  okey32(a) < okey32(b) as unsigned, so
// integer atomicMin / atomicMax give a float minimum / maximum; NaN has no place in the order
__device__ __forceinline__ unsigned okey32(float v) {
    const unsigned b = __float_as_uint(v);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float okey32_val(unsigned k) {
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

// 64-bit finalizer (splitmix64): all 64 bits (upright.hip's generator), and its low word -> table slot
__device__ __forceinline__ uint64_t mix64(uint64_t k) {
    k ^= k >> 30;
    k *= 0xbf58476d1ce4e5b9ULL;
    k ^= k >> 27;
    k *= 0x94d049bb133111ebULL;
    k ^= k >> 31;
    return k;
}
__device__ __forceinline__ uint32_t hash64(uint64_t k) { return (uint32_t)mix64(k); }

// ---- device-wide exclusive scan (int32), three launches; tmp must hold scan_tmp_ints(n) = cdiv(n, SCAN_TILE) + 2 ints:
// one sum per tile, then sums[nb] = the total (k_scan_sums writes it), then one spare -------------------------------------
constexpr int SCAN_THREADS = 256;
constexpr int SCAN_ITEMS = 8;
constexpr int SCAN_TILE = SCAN_THREADS * SCAN_ITEMS;  // 2048 elements per block

static inline size_t scan_tmp_ints(long long n) { return (size_t)cdiv(n, SCAN_TILE) + 2; }

// out[i] = sum_{j<i} in[j] for i in [0,n); if total != nullptr, *total = sum of all.  in may alias out.
int scan_exclusive_i32(const int* in, int* out, int n, int* tmp, int* total, hipStream_t stream);
// the same in ONE launch (chained scan over the workgroups); state: scan_chained_state_words(n) 64-bit words zeroed by the caller.
// A workgroup that gives up waiting for its predecessors ORs SCAN_CHAIN_SPIN into *status (status may be null).  The callers
// are grouping's scans (cluster.hip), so the bit lives in grouping's status word next to its own bits 1, 2 and 4; it is not
// scan_dev.h's SCAN_WALK_CAP, which has the same value in the scan-decode stages' word.
constexpr int SCAN_CHAIN_SPIN = 16;
size_t scan_chained_state_words(long long n);
int scan_exclusive_i32_chained(const int* in, int* out, int n, unsigned long long* state_zeroed, int* total, int* status,
                               hipStream_t stream);

// coords.hip: every cube map of a pyramid in one launch (see the definition)
struct MapJobs {
    const int* coords[6]; const int* n_dev[6]; const unsigned long long* keys[6]; const int* vals[6]; int* nbr[6];
    unsigned mask[6]; int ksize[6], stride[6];
    int n_jobs, n_max, x_fastest;
};
int kernel_maps_multi(const MapJobs& jobs, long long total_max, hipStream_t stream);

// Several byte fills in ONE kernel launch (a stage's zero / 0xff / 0x7f groups), any alignment and size; replaces
// hipMemsetAsync on every path that may be captured in a HIP graph (see common.hip for why).
struct FillRange { void* p; size_t bytes; unsigned char value; };
int fill_ranges(const FillRange* ranges, int n, hipStream_t stream);
static inline int fill_bytes(void* p, unsigned char value, size_t bytes, hipStream_t stream) {
    const FillRange r{p, bytes, value};
    return fill_ranges(&r, 1, stream);
}

// coords.hip internals shared with executor.hip (see the definitions for the `clear` contract)
int coords_unique_impl(const int32_t* coords, const int32_t* n_dev, int n_max, uint64_t* table_keys, int32_t* table_vals,
                       int capacity, int32_t* unique_index, int32_t* inverse, int32_t* unique_coords, int32_t* n_unique,
                       void* workspace, size_t workspace_bytes, int32_t* status, bool clear, hipStream_t stream);
int coords_stride_impl(const int32_t* fine_coords, const int32_t* n_fine_dev, int n_fine_max, int stride_out,
                       uint64_t* table_keys, int32_t* table_vals, int capacity, int32_t* coarse_coords,
                       int32_t* parent_row, int32_t* child_k, int32_t* nbr_down, int32_t* nbr_up, int32_t* n_coarse,
                       void* workspace, size_t workspace_bytes, int32_t* status, bool clear, hipStream_t stream);

int coords_insert_identity(const int32_t* coords, const int32_t* n_dev, int n_max, uint64_t* keys, int32_t* vals,
                           int capacity, int32_t* out_coords, int32_t* n_out, int32_t* status, hipStream_t stream);
int coords_morton_iota(const int32_t* coords, const int32_t* n_dev, int n_max, uint64_t* keys, int32_t* iota,
                       hipStream_t stream);
int coords_apply_perm(const int32_t* ucoords, const int32_t* perm32, const int32_t* uidx32, const int32_t* inv32, int n_max,
                      int32_t* sorted_coords, int64_t* perm64, int64_t* inv_perm64, int64_t* uidx64, int64_t* inv64,
                      hipStream_t stream);
// executor.hip: the levels above level 0 and every map, given a finished level 0 (coords, table, count)
int coords_build_upper(int n, int want_k5, int x_fastest, void* arena, const pbn_coords_layout* L, hipStream_t stream);
int coords_number_first(const int32_t* slot_of_row, const int32_t* table_vals, const int32_t* n_dev, int n_max, int32_t* scan_tmp,
                        int32_t* newid, int32_t* first_row, int32_t* n_out, const int32_t* status, hipStream_t stream);
// pyramid.hip: the sorted, hash-free lineage of pbn_coords_prepare (scratch lives in the arena's sort_temp block)
size_t pyramid_scratch_bytes(int n);
int coords_prepare_sorted(const int32_t* coords, const int32_t* n_dev, int n, int want_k5, int x_fastest, void* arena,
                          const pbn_prepare_layout* P, hipStream_t stream);
// cloud.hip: k_cloud_box for thin.hip -- box[0..2] / box[3..5] = minimum / maximum per axis as order-preserving u32 keys
// (the caller fills them with 0xff / 0 first), status |= SCAN_NONFINITE when a coordinate is NaN or infinite; n > 0
int cloud_box(const float* xyz, int n, unsigned* box, int32_t* status, hipStream_t stream);
// prepare.hip: device radix sort of (key, value) pairs; temp from sort_pairs_temp_bytes(n)
size_t sort_pairs_temp_bytes(int n);
int sort_pairs_u64_i32(const uint64_t* keys_in, uint64_t* keys_out, const int32_t* vals_in, int32_t* vals_out, int n,
                       void* temp, size_t temp_bytes, hipStream_t stream);

}  // namespace pbn
