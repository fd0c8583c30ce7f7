// front.hip -- the glue between the big kernels of the inference front (PBNet.forward, the reference's network/PBNet.py:113-280),
// fused: every entry point replaces a run of small tensor ops (index / cat / where / floor / arange ...) of the reference by ONE
// launch with the same integer results and the same fp32 arithmetic.  Nothing here is arithmetic-heavy; the point is
// launch count (host and device) on the inference path, where the stages between U-Nets are latency bound.
// A device count (n_dev, ...) makes the size beside it a capacity; NULL = the size is exact.
#include "pbn_common.h"

namespace pbn {
namespace {

constexpr int TPB = 256;

// largest e in [0, n) with start[e] <= r  (start ascending, start[0] = 0, start[n] = total > r)
__device__ __forceinline__ int upper_entry(const int* __restrict__ start, int n, int r) {
    int lo = 0, hi = n;  // invariant: start[lo] <= r < start[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (start[mid] <= r) lo = mid; else hi = mid;
    }
    return lo;
}

// ---- local-scene rows (PBNet.py:182-247) ---------------------------------------------------------------------------
// One thread per (row, 32-bit word of the output feature row).  Word w of a row of ESZ-byte elements:
//   elements [0, C)      : point_feat[p, :]
//   element  C           : sem_score[p, sem_pred[p]]      (PBNet.py:162-163: softmax score of the point's own class)
//   element  C + 1       : entry weight                   (PBNet.py:194,230)
//   elements [C+2, ld)   : 0
template <int ESZ>
__global__ __launch_bounds__(TPB) void k_local_scene_rows(
    const int* __restrict__ ent_row_start, const int* __restrict__ ent_member_start, const int* __restrict__ ent_scene,
    const float* __restrict__ ent_weight, int n_ent_cap, int n_rows_cap, const int* __restrict__ n_ent_dev,
    const int* __restrict__ n_rows_dev, const int* __restrict__ member_idx,
    const long long* __restrict__ ins_ind, const float* __restrict__ xyz, float inv_voxel,
    const unsigned char* __restrict__ point_feat, int ld_feat, int channels, const unsigned char* __restrict__ sem_score,
    int ld_sem, const long long* __restrict__ sem_pred, int dtype, long long* __restrict__ point_idx,
    long long* __restrict__ row_scene, int* __restrict__ coords, unsigned* __restrict__ feat_out, int words_per_row) {
    const int n_ent = n_ent_dev ? min(*n_ent_dev, n_ent_cap) : n_ent_cap;
    const int n_rows = n_rows_dev ? min(*n_rows_dev, n_rows_cap) : n_rows_cap;
    const long long e = (long long)blockIdx.x * TPB + threadIdx.x;
    if (e >= (long long)n_rows * words_per_row) return;
    const int r = (int)(e / words_per_row), w = (int)(e - (long long)r * words_per_row);
    const int ent = upper_entry(ent_row_start, n_ent, r);
    const int local = member_idx[ent_member_start[ent] + (r - ent_row_start[ent])];
    const long long p = ins_ind[local];
    if (w == 0) {
        point_idx[r] = p;
        row_scene[r] = ent_scene[ent];
        // the reference divides a device tensor by a host scalar: that is a multiplication by the fp32 reciprocal
        const float x = xyz[3 * p + 0] * inv_voxel, y = xyz[3 * p + 1] * inv_voxel, z = xyz[3 * p + 2] * inv_voxel;
        reinterpret_cast<int4*>(coords)[r] = make_int4(ent_scene[ent], (int)floorf(x), (int)floorf(y), (int)floorf(z));
    }
    constexpr int EPW = 4 / ESZ;  // elements per word
    unsigned out = 0;
#pragma unroll
    for (int k = 0; k < EPW; ++k) {
        const int c = w * EPW + k;
        unsigned bits = 0;
        if (c < channels) {
            if (ESZ == 4) bits = *reinterpret_cast<const unsigned*>(point_feat + ((size_t)p * ld_feat + c) * 4);
            else bits = *reinterpret_cast<const unsigned short*>(point_feat + ((size_t)p * ld_feat + c) * 2);
        } else if (c == channels) {
            const size_t o = (size_t)p * ld_sem + (sem_pred ? (size_t)sem_pred[p] : 0);
            if (ESZ == 4) bits = *reinterpret_cast<const unsigned*>(sem_score + o * 4);
            else bits = *reinterpret_cast<const unsigned short*>(sem_score + o * 2);
        } else if (c == channels + 1) {
            const float wt = ent_weight[ent];
            if (ESZ == 4) bits = __float_as_uint(wt);
            else if (dtype == PBN_BF16) bits = __builtin_bit_cast(unsigned short, __float2bfloat16(wt));
            else bits = __builtin_bit_cast(unsigned short, __float2half(wt));
        }
        out |= bits << (8 * ESZ * k);
    }
    feat_out[e] = out;
}

// ---- out[i, :C] = in[idx2[idx[i]], :C], out[i, C:ld_out] = 0  (32-bit words) ----------------------------------------
__global__ __launch_bounds__(TPB) void k_gather_pad_rows(const unsigned* __restrict__ in, int ld_in_w, int row_w,
                                                        const long long* __restrict__ idx,
                                                        const long long* __restrict__ idx2, int n_cap,
                                                        const int* __restrict__ n_dev, unsigned* __restrict__ out,
                                                        int ld_out_w) {
    const int n = n_dev ? min(*n_dev, n_cap) : n_cap;
    const long long e = (long long)blockIdx.x * TPB + threadIdx.x;
    if (e >= (long long)n * ld_out_w) return;
    const int i = (int)(e / ld_out_w), w = (int)(e - (long long)i * ld_out_w);
    unsigned v = 0;
    if (w < row_w) {
        long long r = idx ? idx[i] : i;
        if (idx2) r = idx2[r];
        v = in[(size_t)r * ld_in_w + w];
    }
    out[e] = v;
}

// ---- semantic argmax + own-class softmax score + [class, batch] population table (PBNet.py:134,151-163) -------------
// Block = SEL_BLOCK consecutive points.  Besides the global table it leaves the per-block class histogram that
// k_select_points turns into stable output positions.
constexpr int SEL_BLOCK = 1024;                   // SEL_MAX_CLASSES: pbn_common.h

template <typename T>
__global__ __launch_bounds__(TPB) void k_sem_argmax_table(const T* __restrict__ score, int ld, int n_cls,
                                                         const int* __restrict__ batch, int nb, int n,
                                                         long long* __restrict__ sem_pred, T* __restrict__ sem_prob,
                                                         int* __restrict__ table, int* __restrict__ block_hist) {
    __shared__ int s_tab[SEL_MAX_CLASSES * PBN_MAX_SCENES];
    __shared__ int s_cls[SEL_MAX_CLASSES];
    for (int e = threadIdx.x; e < n_cls * nb; e += TPB) s_tab[e] = 0;
    if (threadIdx.x < n_cls) s_cls[threadIdx.x] = 0;
    __syncthreads();
    const int base = blockIdx.x * SEL_BLOCK;
    for (int k = 0; k < SEL_BLOCK / TPB; ++k) {
        const int i = base + k * TPB + threadIdx.x;
        if (i >= n) break;
        const T* s = score + (size_t)i * ld;
        float best = -__builtin_inff();
        int arg = 0;
        for (int c = 0; c < n_cls; ++c) {
            const float v = to_f32<T>(s[c]);
            if (v > best) { best = v; arg = c; }       // first maximum wins
        }
        float sum = 0.f;
        for (int c = 0; c < n_cls; ++c) {
            const float v = to_f32<T>(s[c]);
            sum += expf(v - best);
        }
        sem_pred[i] = arg;
        if (sem_prob) st_f32(sem_prob + i, 1.0f / sum);
        atomicAdd(&s_cls[arg], 1);
        const int b = batch ? batch[i] : 0;
        if (b >= 0 && b < nb) atomicAdd(&s_tab[arg * nb + b], 1);
    }
    __syncthreads();
    for (int e = threadIdx.x; e < n_cls * nb; e += TPB)
        if (s_tab[e]) atomicAdd(&table[e], s_tab[e]);
    if (threadIdx.x < n_cls) block_hist[blockIdx.x * n_cls + threadIdx.x] = s_cls[threadIdx.x];
}

// ---- stable class-major selection of the points of the kept classes + their grouping inputs (PBNet.py:151-170) -------
// Output position of point i of class c = class_base[c] + #(points j < i of class c): blocks in front come from the
// per-block histograms, waves in front from a per-wave histogram, lanes in front from ballots.  Deterministic.
template <typename T>
__global__ __launch_bounds__(TPB) void k_select_points(const long long* __restrict__ sem_pred, int n, int n_cls,
                                                      const int* __restrict__ class_base,
                                                      const int* __restrict__ block_hist, const float* __restrict__ xyz,
                                                      const T* __restrict__ offset, int ld_off,
                                                      long long* __restrict__ ins_ind, float* __restrict__ ins_orig,
                                                      float* __restrict__ ins_off, int* __restrict__ ins_sem) {
    __shared__ int s_base[SEL_MAX_CLASSES];
    __shared__ int s_wave[4][SEL_MAX_CLASSES];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (threadIdx.x < n_cls) {
        int t = class_base[threadIdx.x];
        if (t >= 0)
            for (int b = 0; b < (int)blockIdx.x; ++b) t += block_hist[b * n_cls + threadIdx.x];
        else
            t = -(1 << 30);                           // dropped class: stays negative whatever is added to it
        s_base[threadIdx.x] = t;
    }
    for (int e = threadIdx.x; e < 4 * SEL_MAX_CLASSES; e += TPB) (&s_wave[0][0])[e] = 0;
    __syncthreads();
    const int wbase = blockIdx.x * SEL_BLOCK + wave * (SEL_BLOCK / 4);
    int cls[SEL_BLOCK / 256];
#pragma unroll
    for (int k = 0; k < SEL_BLOCK / 256; ++k) {
        const int i = wbase + k * 64 + lane;
        cls[k] = i < n ? (int)sem_pred[i] : -1;
        if (cls[k] >= 0) atomicAdd(&s_wave[wave][cls[k]], 1);
    }
    __syncthreads();
    // running position per class for this wave (lane c owns class c)
    int run = 0;
    if (lane < n_cls) {
        run = s_base[lane];
        for (int w = 0; w < wave; ++w) run += s_wave[w][lane];
    }
#pragma unroll
    for (int k = 0; k < SEL_BLOCK / 256; ++k) {
        const int i = wbase + k * 64 + lane;
        const int c = cls[k];
        int pos = -1;
        unsigned long long todo = __ballot(c >= 0);
        while (todo) {
            const int leader = __ffsll((long long)todo) - 1;
            const int lc = __shfl(c, leader, 64);
            const unsigned long long m = __ballot(c == lc);
            const int start = __shfl(run, lc, 64);
            if (c == lc) pos = start >= 0 ? start + __popcll(m & ((1ULL << lane) - 1ULL)) : -1;
            if (lane == lc) run += (run >= 0) ? __popcll(m) : 0;
            todo &= ~m;
        }
        if (pos >= 0) {
            const float x = xyz[3 * (size_t)i + 0], y = xyz[3 * (size_t)i + 1], z = xyz[3 * (size_t)i + 2];
            const T* o = offset + (size_t)i * ld_off;
            const float ox = to_f32<T>(o[0]), oy = to_f32<T>(o[1]), oz = to_f32<T>(o[2]);
            ins_ind[pos] = i;
            ins_orig[3 * (size_t)pos + 0] = x; ins_orig[3 * (size_t)pos + 1] = y; ins_orig[3 * (size_t)pos + 2] = z;
            ins_off[3 * (size_t)pos + 0] = x + ox; ins_off[3 * (size_t)pos + 1] = y + oy; ins_off[3 * (size_t)pos + 2] = z + oz;
            ins_sem[pos] = c;
        }
    }
}

// ---- proposals (PBNet.py:317-347 + 240-252): rows whose mask score passes the threshold, order preserved ------------
// pass 1: kept rows per block of SEL_BLOCK rows and per local scene (wave-aggregated atomics: rows are grouped by scene)
template <typename T>
__global__ __launch_bounds__(TPB) void k_mask_count(const T* __restrict__ score, int ld, float thd,
                                                   const long long* __restrict__ row_scene, int n_cap,
                                                   const int* __restrict__ n_dev, int n_scenes,
                                                   int* __restrict__ per_scene, int* __restrict__ block_cnt) {
    const int n = n_dev ? min(*n_dev, n_cap) : n_cap;
    __shared__ int s_cnt;
    if (threadIdx.x == 0) s_cnt = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int base = blockIdx.x * SEL_BLOCK;
    int mine = 0;
    for (int k = 0; k < SEL_BLOCK / TPB; ++k) {
        const int i = base + k * TPB + threadIdx.x;
        const bool keep = i < n && to_f32<T>(score[(size_t)i * ld]) > thd;
        const int sc = keep ? (int)row_scene[i] : -1;
        unsigned long long todo = __ballot(keep);
        mine += keep ? 1 : 0;
        while (todo) {
            const int leader = __ffsll((long long)todo) - 1;
            const int ls = __shfl(sc, leader, 64);
            const unsigned long long m = __ballot(sc == ls);
            if (lane == leader && ls >= 0 && ls < n_scenes) atomicAdd(&per_scene[ls], __popcll(m));
            todo &= ~m;
        }
    }
    mine = wave_reduce_add(mine);
    if (lane == 0 && mine) atomicAdd(&s_cnt, mine);
    __syncthreads();
    if (threadIdx.x == 0) block_cnt[blockIdx.x] = s_cnt;
}

// pass 2: compaction.  Thread t of a block owns SEL_BLOCK/TPB CONSECUTIVE rows, so positions follow the row order.
template <typename T>
__global__ __launch_bounds__(TPB) void k_proposal_rows(const T* __restrict__ score, int ld, float thd,
                                                      const long long* __restrict__ row_scene,
                                                      const long long* __restrict__ point_idx, int n_cap,
                                                      const int* __restrict__ n_dev,
                                                      const int* __restrict__ dense_of, const int* __restrict__ block_cnt,
                                                      const float* __restrict__ xyz, float scale, float inv_voxel,
                                                      const uint4* __restrict__ point_feat, int ld_feat_vec, int vpr,
                                                      long long* __restrict__ prop_idx, T* __restrict__ prop_ms,
                                                      int* __restrict__ coords, uint4* __restrict__ feat) {
    constexpr int PER = SEL_BLOCK / TPB;
    const int n = n_dev ? min(*n_dev, n_cap) : n_cap;
    __shared__ int wtot[TPB / 64];
    __shared__ int s_base;
    int part = 0;
    for (int b = threadIdx.x; b < (int)blockIdx.x; b += TPB) part += block_cnt[b];
    part = wave_reduce_add(part);
    if ((threadIdx.x & 63) == 0) wtot[threadIdx.x >> 6] = part;
    __syncthreads();
    if (threadIdx.x == 0) s_base = wtot[0] + wtot[1] + wtot[2] + wtot[3];
    __syncthreads();
    const int block_base = s_base;
    const int r0 = blockIdx.x * SEL_BLOCK + threadIdx.x * PER;
    bool keep[PER];
    int cnt = 0;
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        const int i = r0 + k;
        keep[k] = i < n && to_f32<T>(score[(size_t)i * ld]) > thd;
        cnt += keep[k] ? 1 : 0;
    }
    // exclusive prefix of cnt over the block
    int incl = cnt;
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(incl, o, 64);
        if (lane >= o) incl += t;
    }
    __syncthreads();
    if (lane == 63) wtot[threadIdx.x >> 6] = incl;
    __syncthreads();
    int woff = 0;
    for (int w = 0; w < (int)(threadIdx.x >> 6); ++w) woff += wtot[w];
    int pos = block_base + woff + incl - cnt;
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        if (!keep[k]) continue;
        const int i = r0 + k;
        const long long p = point_idx[i];
        const int dense = dense_of[(int)row_scene[i]];
        prop_idx[2 * (size_t)pos + 0] = dense;
        prop_idx[2 * (size_t)pos + 1] = p;
        prop_ms[pos] = score[(size_t)i * ld];
        if (coords) {
            // (xyz * scale) / voxel with device-tensor-by-host-scalar semantics: two fp32 multiplications
            const float x = (xyz[3 * p + 0] * scale) * inv_voxel, y = (xyz[3 * p + 1] * scale) * inv_voxel,
                        z = (xyz[3 * p + 2] * scale) * inv_voxel;
            reinterpret_cast<int4*>(coords)[pos] = make_int4(dense, (int)floorf(x), (int)floorf(y), (int)floorf(z));
        }
        if (feat)
            for (int v = 0; v < vpr; ++v) feat[(size_t)pos * vpr + v] = point_feat[(size_t)p * ld_feat_vec + v];
        ++pos;
    }
}

}  // namespace
}  // namespace pbn

using namespace pbn;

extern "C" int pbn_local_scene_rows(const int32_t* ent_row_start, const int32_t* ent_member_start, const int32_t* ent_scene,
                                    const float* ent_weight, int n_ent, int n_rows, const int32_t* n_ent_dev,
                                    const int32_t* n_rows_dev, const int32_t* member_idx, const int64_t* ins_ind,
                                    const float* xyz, float inv_voxel, const void* point_feat, int ld_feat, int channels,
                                    const void* sem_score, int ld_sem, const int64_t* sem_pred, int dtype, int64_t* point_idx,
                                    int64_t* row_scene, int32_t* coords, void* feat_out, int ld_out, pbn_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!n_ent_dev != !n_rows_dev) return PBN_ERR_ARG;
    if (n_ent < 0 || n_rows < 0 || channels < 0 || ld_out < channels + 2 || ld_feat < channels) return PBN_ERR_ARG;
    if (n_rows == 0) return PBN_OK;
    if (n_ent == 0 || !ent_row_start || !ent_member_start || !ent_scene || !ent_weight || !member_idx || !ins_ind || !xyz ||
        !point_feat || !sem_score || !point_idx || !row_scene || !coords || !feat_out)
        return PBN_ERR_ARG;
    const int esz = dtype == PBN_F32 ? 4 : 2;
    if ((ld_out * esz) % 4 || ((uintptr_t)feat_out & 3) || ((uintptr_t)coords & 15)) return PBN_ERR_ARG;
    const int wpr = ld_out * esz / 4;
    const long long total = (long long)n_rows * wpr;
    hipLaunchKernelGGL((esz == 4 ? k_local_scene_rows<4> : k_local_scene_rows<2>), dim3(cdiv(total, TPB)), dim3(TPB), 0, stream,
                       ent_row_start, ent_member_start, ent_scene, ent_weight, n_ent, n_rows, n_ent_dev, n_rows_dev, member_idx,
                       (const long long*)ins_ind, xyz, inv_voxel, (const unsigned char*)point_feat, ld_feat, channels,
                       (const unsigned char*)sem_score, ld_sem, (const long long*)sem_pred, dtype, (long long*)point_idx,
                       (long long*)row_scene, coords, (unsigned*)feat_out, wpr);
    PBN_LAUNCH_CHECK();
    return PBN_OK;
}

extern "C" int pbn_gather_pad_rows(const void* in, int ld_in_bytes, int row_bytes, const int64_t* idx, const int64_t* idx2, int n,
                                   const int32_t* n_dev, void* out, int ld_out_bytes, pbn_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (n < 0 || row_bytes <= 0 || (row_bytes & 3) || (ld_in_bytes & 3) || (ld_out_bytes & 3) || ld_out_bytes < row_bytes ||
        ld_in_bytes < row_bytes)
        return PBN_ERR_ARG;
    if (n == 0) return PBN_OK;
    if (!in || !out || (((uintptr_t)in | (uintptr_t)out) & 3)) return PBN_ERR_ARG;
    const long long total = (long long)n * (ld_out_bytes / 4);
    hipLaunchKernelGGL(k_gather_pad_rows, dim3(cdiv(total, TPB)), dim3(TPB), 0, stream, (const unsigned*)in, ld_in_bytes / 4,
                       row_bytes / 4, (const long long*)idx, (const long long*)idx2, n, n_dev, (unsigned*)out,
                       ld_out_bytes / 4);
    PBN_LAUNCH_CHECK();
    return PBN_OK;
}

extern "C" int pbn_select_blocks(int n) { return n > 0 ? cdiv(n, SEL_BLOCK) : 0; }

extern "C" int pbn_sem_argmax_table(const void* score, int ld, int n_cls, const int32_t* batch, int nb, int n, int dtype,
                                    int64_t* sem_pred, void* sem_prob, int32_t* table, int32_t* block_hist,
                                    pbn_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (n < 0 || n_cls < 1 || n_cls > SEL_MAX_CLASSES || nb < 1 || nb > PBN_MAX_SCENES || ld < n_cls || !table) return PBN_ERR_ARG;
    PBN_TRY(fill_bytes(table, 0, sizeof(int) * (size_t)n_cls * nb, stream));
    if (n == 0) return PBN_OK;
    if (!score || !sem_pred || !block_hist) return PBN_ERR_ARG;
    if (!dispatch_dtype(dtype, [&](auto t) {
            using T = decltype(t);
            hipLaunchKernelGGL(k_sem_argmax_table<T>, dim3(cdiv(n, SEL_BLOCK)), dim3(TPB), 0, stream, (const T*)score, ld, n_cls,
                               batch, nb, n, (long long*)sem_pred, (T*)sem_prob, table, block_hist);
        }))
        return PBN_ERR_ARG;
    PBN_LAUNCH_CHECK();
    return PBN_OK;
}

extern "C" int pbn_select_points(const int64_t* sem_pred, int n, int n_cls, const int32_t* class_base,
                                 const int32_t* block_hist, const float* xyz, const void* offset, int ld_off, int dtype,
                                 int64_t* ins_ind, float* ins_orig, float* ins_off, int32_t* ins_sem,
                                 pbn_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (n < 0 || n_cls < 1 || n_cls > SEL_MAX_CLASSES || ld_off < 3) return PBN_ERR_ARG;
    if (n == 0) return PBN_OK;
    if (!sem_pred || !class_base || !block_hist || !xyz || !offset || !ins_ind || !ins_orig || !ins_off || !ins_sem)
        return PBN_ERR_ARG;
    if (!dispatch_dtype(dtype, [&](auto t) {
            using T = decltype(t);
            hipLaunchKernelGGL(k_select_points<T>, dim3(cdiv(n, SEL_BLOCK)), dim3(TPB), 0, stream, (const long long*)sem_pred, n,
                               n_cls, class_base, block_hist, xyz, (const T*)offset, ld_off, (long long*)ins_ind, ins_orig,
                               ins_off, ins_sem);
        }))
        return PBN_ERR_ARG;
    PBN_LAUNCH_CHECK();
    return PBN_OK;
}

extern "C" int pbn_mask_count(const void* mask_score, int ld, float thd, const int64_t* row_scene, int n, const int32_t* n_dev,
                              int n_scenes, int dtype, int32_t* per_scene, int32_t* block_cnt, pbn_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (n < 0 || n_scenes < 0 || ld < 1) return PBN_ERR_ARG;
    if (n_scenes > 0) {
        if (!per_scene) return PBN_ERR_ARG;
        PBN_TRY(fill_bytes(per_scene, 0, sizeof(int) * (size_t)n_scenes, stream));
    }
    if (n == 0) return PBN_OK;
    if (!mask_score || !row_scene || !block_cnt) return PBN_ERR_ARG;
    if (!dispatch_dtype(dtype, [&](auto t) {
            using T = decltype(t);
            hipLaunchKernelGGL(k_mask_count<T>, dim3(cdiv(n, SEL_BLOCK)), dim3(TPB), 0, stream, (const T*)mask_score, ld, thd,
                               (const long long*)row_scene, n, n_dev, n_scenes, per_scene, block_cnt);
        }))
        return PBN_ERR_ARG;
    PBN_LAUNCH_CHECK();
    return PBN_OK;
}

extern "C" int pbn_proposal_rows(const void* mask_score, int ld, float thd, const int64_t* row_scene, const int64_t* point_idx,
                                 int n, const int32_t* n_dev, const int32_t* dense_of, const int32_t* block_cnt,
                                 const float* xyz, float scale, float inv_voxel, const void* point_feat, int ld_feat,
                                 int channels, int dtype, int64_t* proposals_idx, void* proposals_ms, int32_t* coords,
                                 void* feat_out, pbn_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (n < 0 || ld < 1) return PBN_ERR_ARG;
    if (n == 0) return PBN_OK;
    if (!mask_score || !row_scene || !point_idx || !dense_of || !block_cnt || !proposals_idx || !proposals_ms)
        return PBN_ERR_ARG;
    const int esz = dtype == PBN_F32 ? 4 : 2;
    int vpr = 0;
    if (feat_out) {
        if (!point_feat || channels < 1 || (channels * esz) % 16 || (ld_feat * esz) % 16 ||
            (((uintptr_t)point_feat | (uintptr_t)feat_out) & 15))
            return PBN_ERR_ARG;
        vpr = channels * esz / 16;
    }
    if (coords && (!xyz || ((uintptr_t)coords & 15))) return PBN_ERR_ARG;
    if (!dispatch_dtype(dtype, [&](auto t) {
            using T = decltype(t);
            hipLaunchKernelGGL(k_proposal_rows<T>, dim3(cdiv(n, SEL_BLOCK)), dim3(TPB), 0, stream, (const T*)mask_score, ld, thd,
                               (const long long*)row_scene, (const long long*)point_idx, n, n_dev, dense_of, block_cnt, xyz,
                               scale, inv_voxel, (const uint4*)point_feat, feat_out ? ld_feat * esz / 16 : 0, vpr,
                               (long long*)proposals_idx, (T*)proposals_ms, coords, (uint4*)feat_out);
        }))
        return PBN_ERR_ARG;
    PBN_LAUNCH_CHECK();
    return PBN_OK;
}
