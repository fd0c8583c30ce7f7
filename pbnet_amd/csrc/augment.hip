// augment.hip -- batch construction of the reference's trainMerge / valMerge
// (datasets/scannetv2/dataset_preprocess.py:82-305, :308-385) on the device: affine + extent, elastic distortion, the crop
// loop, compaction, instance relabelling and instance statistics.  Compiled with -ffp-contract=off: every float64 expression
// below is evaluated in the reference's order without fused multiply-adds.
//
// Layout: the points of a batch are one row range; a "unit" is one dataAugment call (a primary scene, its mix-up partner or a
// validation copy), a "scene" is the units that are concatenated into one batch entry (primary + partner).  Rows of a unit and
// of a scene are contiguous, offsets int32[n+1].  Per-segment minima / maxima are exact in any order: they are reduced as
// order-preserving 64-bit keys with integer atomics.  No floating-point atomics anywhere in this file.
#include "pbn_common.h"

namespace {

using namespace pbn;

constexpr int AUG_THREADS = 256;
constexpr int AUG_ITEMS = 8;
constexpr int AUG_CHUNK = AUG_THREADS * AUG_ITEMS;     // compaction chunk (rows)
constexpr int CROP_TRIES = 5;
constexpr int CROP_LEVELS = 17;
constexpr int CROP_TRIPLES = CROP_TRIES * CROP_LEVELS;
constexpr int NO_INST = -100;

// state words of one scene's crop loop
enum { ST_DONE = 0, ST_NEXT = 1, ST_USED = 2, ST_LAST_START = 3, ST_LAST_K = 4, ST_SUCCESS = 5, ST_ERROR = 6, ST_TRIES = 7 };

__device__ __forceinline__ unsigned long long okey(double v) {
    unsigned long long b = (unsigned long long)__double_as_longlong(v);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ULL);
}
__device__ __forceinline__ double okey_val(unsigned long long k) {
    unsigned long long b = (k >> 63) ? (k & 0x7fffffffffffffffULL) : ~k;
    return __longlong_as_double((long long)b);
}

// keys[seg][0:3] = min keys, [3:6] = max keys
__global__ void k_keys_init(unsigned long long* keys, int n_seg) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_seg * 6) keys[i] = (i % 6) < 3 ? ~0ULL : 0ULL;
}

__global__ void k_keys_final(const unsigned long long* keys, int n_seg, double* ext) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_seg * 6) ext[i] = okey_val(keys[i]);
}

// block-wide min / max of 3 columns, then one atomic per value per block
__device__ __forceinline__ void block_extent(double mn[3], double mx[3], unsigned long long* keys) {
    __shared__ unsigned long long s[6][AUG_THREADS / WAVE];
    unsigned long long k[6];
#pragma unroll
    for (int d = 0; d < 3; ++d) { k[d] = okey(mn[d]); k[3 + d] = okey(mx[d]); }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
        for (int d = 0; d < 6; ++d) {
            unsigned long long v = __shfl_xor(k[d], o, 64);
            k[d] = d < 3 ? (v < k[d] ? v : k[d]) : (v > k[d] ? v : k[d]);
        }
    }
    int w = threadIdx.x / WAVE;
    if (lane_id() == 0)
        for (int d = 0; d < 6; ++d) s[d][w] = k[d];
    __syncthreads();
    if (threadIdx.x < 6) {
        int d = threadIdx.x;
        unsigned long long v = s[d][0];
        for (int j = 1; j < AUG_THREADS / WAVE; ++j) v = d < 3 ? (s[d][j] < v ? s[d][j] : v) : (s[d][j] > v ? s[d][j] : v);
        if (d < 3) atomicMin(&keys[d], v); else atomicMax(&keys[d], v);
    }
}

// ---- affine ------------------------------------------------------------------------------------------------------
// float32 minimum of the units that subtract it first (trainMerge:229 `xyz - xyz.min(0)` on the .npy float32 array)
__global__ void k_min_f32(const float* __restrict__ xyz, const int* __restrict__ uoff, const int* __restrict__ pre_min,
                          unsigned long long* keys) {
    int u = blockIdx.y;
    if (!pre_min[u]) return;
    double mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int r = uoff[u] + blockIdx.x * blockDim.x + threadIdx.x; r < uoff[u + 1]; r += gridDim.x * blockDim.x)
        for (int d = 0; d < 3; ++d) { double v = (double)xyz[3 * (size_t)r + d]; mn[d] = fmin(mn[d], v); mx[d] = fmax(mx[d], v); }
    block_extent(mn, mx, keys + 6 * u);
}

// y = x @ m in float64 (x first reduced by its float32 minimum where asked), extent of y
__global__ void k_affine(const float* __restrict__ xyz, const int* __restrict__ uoff, const int* __restrict__ pre_min,
                         const double* __restrict__ pre_ext, const double* __restrict__ mats, double* __restrict__ out,
                         unsigned long long* keys) {
    int u = blockIdx.y;
    const double* m = mats + 9 * u;
    float m0[3] = {0.f, 0.f, 0.f};
    if (pre_min[u])
        for (int d = 0; d < 3; ++d) m0[d] = (float)pre_ext[6 * u + d];
    double mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int r = uoff[u] + blockIdx.x * blockDim.x + threadIdx.x; r < uoff[u + 1]; r += gridDim.x * blockDim.x) {
        double x[3];
        for (int d = 0; d < 3; ++d) {
            float v = xyz[3 * (size_t)r + d];
            if (pre_min[u]) v = v - m0[d];
            x[d] = (double)v;
        }
        for (int j = 0; j < 3; ++j) {
            double y = x[0] * m[j] + x[1] * m[3 + j] + x[2] * m[6 + j];
            out[3 * (size_t)r + j] = y;
            mn[j] = fmin(mn[j], y);
            mx[j] = fmax(mx[j], y);
        }
    }
    block_extent(mn, mx, keys + 6 * u);
}

// y = (y - min) [* scale], extent of the result
__global__ void k_sub_scale(double* __restrict__ xyz, const int* __restrict__ uoff, const double* __restrict__ ext,
                            const double* __restrict__ scale, const int* __restrict__ has_scale, unsigned long long* keys) {
    int u = blockIdx.y;
    double mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int r = uoff[u] + blockIdx.x * blockDim.x + threadIdx.x; r < uoff[u + 1]; r += gridDim.x * blockDim.x)
        for (int d = 0; d < 3; ++d) {
            double y = xyz[3 * (size_t)r + d] - ext[6 * u + d];
            if (has_scale[u]) y = y * scale[u];
            xyz[3 * (size_t)r + d] = y;
            mn[d] = fmin(mn[d], y);
            mx[d] = fmax(mx[d], y);
        }
    block_extent(mn, mx, keys + 6 * u);
}

__global__ void k_sub_min(double* __restrict__ xyz, const int* __restrict__ uoff, const int* __restrict__ flags,
                          const double* __restrict__ ext) {
    int u = blockIdx.y;
    if (!flags[u]) return;
    for (int r = uoff[u] + blockIdx.x * blockDim.x + threadIdx.x; r < uoff[u + 1]; r += gridDim.x * blockDim.x)
        for (int d = 0; d < 3; ++d) xyz[3 * (size_t)r + d] = xyz[3 * (size_t)r + d] - ext[6 * u + d];
}

// ---- elastic -----------------------------------------------------------------------------------------------------
// one pass of scipy.ndimage.convolve(n, ones(3 along `axis`)/3 as float32, mode='constant', cval=0): float64 accumulation
// in the footprint's order (i-1, i, i+1), cast to float32.  desc[j] = (unit, b0, b1, b2, first float of its 3 grids).
__global__ void k_blur(const float* __restrict__ in, float* __restrict__ out, const int* __restrict__ desc, int n_el,
                       int total, int axis) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    int j = 0;
    while (j + 1 < n_el && desc[5 * (j + 1) + 4] <= i) ++j;
    const int* dj = desc + 5 * j;
    int b[3] = {dj[1], dj[2], dj[3]};
    int cells = b[0] * b[1] * b[2];
    int local = (i - dj[4]) % cells;
    int base = i - local;
    int c[3] = {local / (b[1] * b[2]), (local / b[2]) % b[1], local % b[2]};
    int stride = axis == 0 ? b[1] * b[2] : (axis == 1 ? b[2] : 1);
    const double w = (double)(1.0f / 3.0f);
    double t = 0.0;
    for (int o = -1; o <= 1; ++o) {
        int q = c[axis] + o;
        double v = (q >= 0 && q < b[axis]) ? (double)in[base + local + o * stride] : 0.0;
        t = t + w * v;
    }
    out[i] = (float)t;
}

// RegularGridInterpolator(linear, bounds_error=0, fill_value=0) on the axes linspace(-(b-1)g, (b-1)g, b) (exact integers):
// cell i = (number of axis values <= x) - 1 clipped to [0, b-2], corners in itertools.product order
__device__ __forceinline__ double rgi(const float* __restrict__ grid, const int b[3], int gran, const double x[3]) {
    int idx[3];
    double nd[3];
    for (int d = 0; d < 3; ++d) {
        double a0 = (double)(-(b[d] - 1) * gran), a1 = (double)((b[d] - 1) * gran);
        if (!(x[d] >= a0 && x[d] <= a1)) return 0.0;              // out of bounds (or NaN): fill_value
        int lo = 0, hi = b[d];                                    // count of axis values <= x by bisection
        while (lo < hi) {
            int mid = (lo + hi) >> 1;
            if ((double)(-(b[d] - 1) * gran + 2 * gran * mid) <= x[d]) lo = mid + 1; else hi = mid;
        }
        int i = lo - 1;
        i = i < 0 ? 0 : (i > b[d] - 2 ? b[d] - 2 : i);
        idx[d] = i;
        double g0 = (double)(-(b[d] - 1) * gran + 2 * gran * i), g1 = (double)(-(b[d] - 1) * gran + 2 * gran * (i + 1));
        nd[d] = (x[d] - g0) / (g1 - g0);
    }
    double value = 0.0;
    for (int h = 0; h < 8; ++h) {
        double weight = 1.0;
        int flat = 0;
        for (int d = 0; d < 3; ++d) {
            int up = (h >> (2 - d)) & 1;
            weight = weight * (up ? nd[d] : 1.0 - nd[d]);
            flat = flat * b[d] + idx[d] + up;
        }
        value = value + (double)grid[flat] * weight;
    }
    return value;
}

__global__ void k_elastic(double* __restrict__ xyz, const int* __restrict__ uoff, const int* __restrict__ desc,
                          const float* __restrict__ noise, int gran, double mag, unsigned long long* keys) {
    const int* dj = desc + 5 * blockIdx.y;
    int u = dj[0];
    int b[3] = {dj[1], dj[2], dj[3]};
    int cells = b[0] * b[1] * b[2];
    const float* g = noise + dj[4];
    double mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int r = uoff[u] + blockIdx.x * blockDim.x + threadIdx.x; r < uoff[u + 1]; r += gridDim.x * blockDim.x) {
        double x[3] = {xyz[3 * (size_t)r], xyz[3 * (size_t)r + 1], xyz[3 * (size_t)r + 2]};
        for (int d = 0; d < 3; ++d) {
            double y = x[d] + rgi(g + d * cells, b, gran, x) * mag;
            xyz[3 * (size_t)r + d] = y;
            mn[d] = fmin(mn[d], y);
            mx[d] = fmax(mx[d], y);
        }
    }
    block_extent(mn, mx, keys + 6 * u);
}

// ---- crop --------------------------------------------------------------------------------------------------------
// crop(): offset = clip(full_scale - room_range + 0.001, None, 0) * rand(3); valid = min(x+o) >= 0 and all(x+o < full_scale)
__device__ __forceinline__ void crop_offset(const double* ext, const double* level, const double* t, double o[3]) {
    for (int d = 0; d < 3; ++d) {
        double rr = ext[3 + d] - ext[d];
        double c = level[d] - rr + 0.001;
        c = c > 0.0 ? 0.0 : c;
        o[d] = c * t[d];
    }
}
__device__ __forceinline__ bool crop_valid(const double x[3], const double o[3], const double* level) {
    double a = x[0] + o[0], b = x[1] + o[1], c = x[2] + o[2];
    double m = fmin(fmin(a, b), c);
    return m >= 0.0 && a < level[0] && b < level[1] && c < level[2];
}

// the 17 candidate iterations of try `t` of every scene still cropping: counts[t][scene][k]
__global__ void k_crop_count(const double* __restrict__ xyz, const int* __restrict__ soff, const int* __restrict__ mode,
                             const double* __restrict__ trip, const double* __restrict__ levels,
                             const double* __restrict__ ext, const int* __restrict__ state, int t, int n_scenes,
                             int* __restrict__ counts) {
    int s = blockIdx.y;
    const int* st = state + 8 * s;
    if (mode[s] != 0 || st[ST_DONE]) return;
    int start = st[ST_NEXT];
    double o[CROP_LEVELS][3];
    for (int k = 0; k < CROP_LEVELS; ++k) {
        int q = start + k < CROP_TRIPLES ? start + k : CROP_TRIPLES - 1;
        crop_offset(ext + 6 * s, levels + 3 * k, trip + 3 * ((size_t)s * CROP_TRIPLES + q), o[k]);
    }
    int c[CROP_LEVELS];
    for (int k = 0; k < CROP_LEVELS; ++k) c[k] = 0;
    for (int r = soff[s] + blockIdx.x * blockDim.x + threadIdx.x; r < soff[s + 1]; r += gridDim.x * blockDim.x) {
        double x[3] = {xyz[3 * (size_t)r], xyz[3 * (size_t)r + 1], xyz[3 * (size_t)r + 2]};
        for (int k = 0; k < CROP_LEVELS; ++k) c[k] += crop_valid(x, o[k], levels + 3 * k) ? 1 : 0;
    }
    for (int k = 0; k < CROP_LEVELS; ++k) {
        int v = wave_reduce_add(c[k]);
        if (lane_id() == 0 && v) atomicAdd(&counts[((size_t)t * n_scenes + s) * CROP_LEVELS + k], v);
    }
}

// the `while valid.sum() > max_crop_p` loop of try t: stops at the first candidate with at most max_crop_p points
__global__ void k_crop_pick(const int* __restrict__ mode, const int* __restrict__ n_trip, const int* __restrict__ counts,
                            int* __restrict__ state, int t, int n_scenes, int max_crop_p, int min_crop_p) {
    int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n_scenes) return;
    int* st = state + 8 * s;
    if (mode[s] != 0 || st[ST_DONE]) return;
    const int* c = counts + ((size_t)t * n_scenes + s) * CROP_LEVELS;
    int k = 0;
    while (k < CROP_LEVELS && c[k] > max_crop_p) ++k;
    if (k == CROP_LEVELS) { st[ST_ERROR] = 1; st[ST_DONE] = 1; return; }
    int start = st[ST_NEXT];
    st[ST_LAST_START] = start;
    st[ST_LAST_K] = k;
    st[ST_USED] = start + k + 1;
    if (start + k >= n_trip[s]) { st[ST_ERROR] = 2; st[ST_DONE] = 1; return; }
    st[ST_TRIES] = t + 1;
    if (c[k] >= min_crop_p) { st[ST_SUCCESS] = 1; st[ST_DONE] = 1; return; }
    st[ST_NEXT] = start + k + 1;
    if (t + 1 == CROP_TRIES) st[ST_DONE] = 1;
}

struct CropView {
    bool all;            // keep every point un-offset
    bool offset;         // the last try succeeded: x + o
    double o[3];
    const double* level;
};
__device__ __forceinline__ CropView crop_view(int s, const int* mode, const double* trip, const double* levels,
                                              const int* state, const double* ext_pre) {
    CropView v;
    const int* st = state + 8 * s;
    v.all = mode[s] != 0;
    v.offset = false;
    v.o[0] = v.o[1] = v.o[2] = 0.0;
    v.level = levels;
    if (!v.all) {
        int k = st[ST_LAST_K], q = st[ST_LAST_START] + k;
        q = q < CROP_TRIPLES ? q : CROP_TRIPLES - 1;
        v.level = levels + 3 * k;
        crop_offset(ext_pre + 6 * s, v.level, trip + 3 * ((size_t)s * CROP_TRIPLES + q), v.o);
        v.offset = st[ST_SUCCESS] != 0;
    }
    return v;
}

// extent of the scene after the crop's offset (all points: the reference's min is taken before the mask selects rows)
__global__ void k_crop_extent(const double* __restrict__ xyz, const int* __restrict__ soff, const int* __restrict__ mode,
                              const double* __restrict__ trip, const double* __restrict__ levels,
                              const int* __restrict__ state, const double* __restrict__ ext_pre, unsigned long long* keys) {
    int s = blockIdx.y;
    CropView v = crop_view(s, mode, trip, levels, state, ext_pre);
    double mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int r = soff[s] + blockIdx.x * blockDim.x + threadIdx.x; r < soff[s + 1]; r += gridDim.x * blockDim.x)
        for (int d = 0; d < 3; ++d) {
            double y = xyz[3 * (size_t)r + d];
            if (v.offset) y = y + v.o[d];
            mn[d] = fmin(mn[d], y);
            mx[d] = fmax(mx[d], y);
        }
    block_extent(mn, mx, keys + 6 * s);
}

// ---- compaction + relabel ----------------------------------------------------------------------------------------
__device__ __forceinline__ int seg_of(const int* off, int n, int r) {
    int lo = 0, hi = n - 1;                                   // last segment whose start <= r
    while (lo < hi) {
        int mid = (lo + hi + 1) >> 1;
        if (off[mid] <= r) lo = mid; else hi = mid - 1;
    }
    return lo;
}

struct CompactArgs {
    const double* xyz; const float* rgb; const float* nl; const long long* sem; const int* ins;
    const double* shift; const int* ins_shift; const int* uoff; int n_units; int per_scene;
    const int* soff; int n_scenes; const int* mode; const double* trip; const double* levels; const int* state;
    const double* ext_pre; const double* ext_post; const int* loff; int* lmap; int* present; int* maxlab; int* scene_n;
    int* scan; double* xyz_o; float* feat_o; long long* sem_o; int* lab_o; int* sinfo; int n_rows;
};

__device__ __forceinline__ bool row_mask(const CompactArgs& a, int r, int s, CropView& v) {
    if (v.all) return true;
    double x[3] = {a.xyz[3 * (size_t)r], a.xyz[3 * (size_t)r + 1], a.xyz[3 * (size_t)r + 2]};
    return crop_valid(x, v.o, v.level);
}
__device__ __forceinline__ int row_label(const CompactArgs& a, int r) {
    int u = seg_of(a.uoff, a.n_units, r);
    int l = a.ins[r];
    return l != NO_INST ? l + a.ins_shift[u] : l;
}

__device__ __forceinline__ void flush_scene(const CompactArgs& a, int s, int cnt, int mx) {
    if (s < 0) return;
    if (cnt) atomicAdd(&a.scene_n[s], cnt);
    if (mx != INT32_MIN) atomicMax(&a.maxlab[s], mx);
}

// per chunk: rows kept; per scene: rows kept, maximum instance label, presence of each label >= 0
__global__ void k_mask_count(CompactArgs a) {
    __shared__ int s_cnt[AUG_THREADS / WAVE];
    int base = blockIdx.x * AUG_CHUNK + threadIdx.x * AUG_ITEMS;
    int cnt = 0, run = 0, run_max = INT32_MIN;
    int s_prev = -1;
    CropView v;
    for (int k = 0; k < AUG_ITEMS; ++k) {
        int r = base + k;
        if (r >= a.n_rows) break;
        int s = seg_of(a.soff, a.n_scenes, r);
        if (s != s_prev) {
            flush_scene(a, s_prev, run, run_max);
            run = 0;
            run_max = INT32_MIN;
            v = crop_view(s, a.mode, a.trip, a.levels, a.state, a.ext_pre);
            s_prev = s;
        }
        if (!row_mask(a, r, s, v)) continue;
        ++cnt;
        ++run;
        int l = row_label(a, r);
        run_max = l > run_max ? l : run_max;
        if (l >= 0) a.present[a.loff[s] + l] = 1;
    }
    // one atomic per wave when the wave's rows lie in one scene (the common case), per thread otherwise
    int s0 = __shfl(s_prev, 0, 64);
    bool uniform = __all(s_prev == s0 || s_prev < 0);
    if (uniform) {
        int wr = wave_reduce_add(run);
        int wm = run_max;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { int t = __shfl_xor(wm, o, 64); wm = t > wm ? t : wm; }
        if (lane_id() == 0) flush_scene(a, s0, wr, wm);
    } else {
        flush_scene(a, s_prev, run, run_max);
    }
    int w = wave_reduce_add(cnt);
    if (lane_id() == 0) s_cnt[threadIdx.x / WAVE] = w;
    __syncthreads();
    if (threadIdx.x == 0) {
        int t = 0;
        for (int j = 0; j < AUG_THREADS / WAVE; ++j) t += s_cnt[j];
        a.scan[blockIdx.x] = t;
    }
}

// exclusive scan of the chunk counts (one workgroup, sequential tiles) -> scan[0..n_chunks]
__global__ void k_chunk_scan(int* scan, int n_chunks) {
    __shared__ int s[AUG_THREADS];
    __shared__ int carry;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    for (int base = 0; base < n_chunks; base += AUG_THREADS) {
        int i = base + threadIdx.x;
        int v = i < n_chunks ? scan[i] : 0;
        s[threadIdx.x] = v;
        __syncthreads();
        for (int o = 1; o < AUG_THREADS; o <<= 1) {
            int add = threadIdx.x >= o ? s[threadIdx.x - o] : 0;
            __syncthreads();
            s[threadIdx.x] += add;
            __syncthreads();
        }
        int incl = s[threadIdx.x];
        if (i < n_chunks) scan[i] = carry + incl - v;
        __syncthreads();
        if (threadIdx.x == AUG_THREADS - 1) carry += incl;
        __syncthreads();
    }
    if (threadIdx.x == 0) scan[n_chunks] = carry;
}

// getCroppedInstLabel / getInstLabel: `while j < max(): if j absent: labels == max() -> j; j += 1`, simulated on the
// presence table of one scene by one wave (lanes fill the identity map, lane 0 walks the loop).  sinfo[s] = (points kept,
// instance_num = max() + 1 after relabelling, first output row, 0).
__global__ void k_relabel(CompactArgs a) {
    int s = blockIdx.x;
    int lo = a.loff[s], cap = a.loff[s + 1] - lo;
    int* map = a.lmap + lo;
    int* pres = a.present + lo;
    for (int l = threadIdx.x; l < cap; l += blockDim.x) map[l] = l;
    __syncthreads();
    if (threadIdx.x != 0) return;
    int mx = a.maxlab[s];
    int n = a.scene_n[s];
    int inst = 0;
    if (n > 0) {
        int cur = mx;
        for (int j = 0; j < cur; ++j) {
            if (!pres[j]) {
                map[cur] = j;
                pres[j] = 1;
                pres[cur] = 0;
                while (cur > 0 && !pres[cur]) --cur;
            }
        }
        inst = cur + 1;
    }
    int start = 0;
    for (int q = 0; q < s; ++q) start += a.scene_n[q];
    a.sinfo[4 * s + 0] = n;
    a.sinfo[4 * s + 1] = inst;
    a.sinfo[4 * s + 2] = start;
    a.sinfo[4 * s + 3] = 0;
}

// kept rows in input order: xyz - min (float64), feat = f32(rgb + shift) | nl, sem, relabelled instance
__global__ void k_scatter(CompactArgs a) {
    __shared__ int s_pre[AUG_THREADS];
    int base = blockIdx.x * AUG_CHUNK + threadIdx.x * AUG_ITEMS;
    unsigned keep = 0;
    int s_prev = -1;
    CropView v;
    for (int k = 0; k < AUG_ITEMS; ++k) {
        int r = base + k;
        if (r >= a.n_rows) break;
        int s = seg_of(a.soff, a.n_scenes, r);
        if (s != s_prev) { v = crop_view(s, a.mode, a.trip, a.levels, a.state, a.ext_pre); s_prev = s; }
        if (row_mask(a, r, s, v)) keep |= 1u << k;
    }
    int cnt = __popc(keep);
    s_pre[threadIdx.x] = cnt;
    __syncthreads();
    for (int o = 1; o < AUG_THREADS; o <<= 1) {
        int add = threadIdx.x >= o ? s_pre[threadIdx.x - o] : 0;
        __syncthreads();
        s_pre[threadIdx.x] += add;
        __syncthreads();
    }
    int pos = a.scan[blockIdx.x] + s_pre[threadIdx.x] - cnt;
    s_prev = -1;
    for (int k = 0; k < AUG_ITEMS; ++k) {
        if (!(keep >> k & 1u)) continue;
        int r = base + k;
        int s = seg_of(a.soff, a.n_scenes, r);
        if (s != s_prev) { v = crop_view(s, a.mode, a.trip, a.levels, a.state, a.ext_pre); s_prev = s; }
        int u = seg_of(a.uoff, a.n_units, r);
        for (int d = 0; d < 3; ++d) {
            double y = a.xyz[3 * (size_t)r + d];
            if (v.offset) y = y + v.o[d];
            a.xyz_o[3 * (size_t)pos + d] = y - a.ext_post[6 * s + d];
            a.feat_o[6 * (size_t)pos + d] = (float)((double)a.rgb[3 * (size_t)r + d] + a.shift[3 * u + d]);
            a.feat_o[6 * (size_t)pos + 3 + d] = a.nl[3 * (size_t)r + d];
        }
        a.sem_o[pos] = a.sem[r];
        int l = row_label(a, r);
        a.lab_o[pos] = l >= 0 ? a.lmap[a.loff[s] + l] : l;
        ++pos;
    }
}

__global__ void k_fill_i32(int* p, int n, int v) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = v;
}

// ---- instances ---------------------------------------------------------------------------------------------------
// getInstanceInfo, one workgroup per instance of the batch: each thread walks a fixed row subset of its scene, then a fixed
// tree combines the threads -- the float64 sums come out the same on every run.
__global__ void k_inst_stats(const double* __restrict__ xyz, const int* __restrict__ lab, const int* __restrict__ ostart,
                             int n_scenes, const int* __restrict__ ipos, int* __restrict__ pointnum, float* __restrict__ stats) {
    __shared__ double s_sum[3][AUG_THREADS], s_min[3][AUG_THREADS], s_max[3][AUG_THREADS];
    __shared__ int s_n[AUG_THREADS];
    int g = blockIdx.x;
    int s = seg_of(ipos, n_scenes, g);
    int i = g - ipos[s];
    double sum[3] = {0.0, 0.0, 0.0}, mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
    int n = 0;
    for (int r = ostart[s] + threadIdx.x; r < ostart[s + 1]; r += AUG_THREADS) {
        if (lab[r] != i) continue;
        ++n;
        for (int d = 0; d < 3; ++d) {
            double x = xyz[3 * (size_t)r + d];
            sum[d] = sum[d] + x;
            mn[d] = fmin(mn[d], x);
            mx[d] = fmax(mx[d], x);
        }
    }
    for (int d = 0; d < 3; ++d) { s_sum[d][threadIdx.x] = sum[d]; s_min[d][threadIdx.x] = mn[d]; s_max[d][threadIdx.x] = mx[d]; }
    s_n[threadIdx.x] = n;
    __syncthreads();
    for (int o = AUG_THREADS / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) {
            int t = threadIdx.x;
            for (int d = 0; d < 3; ++d) {
                s_sum[d][t] = s_sum[d][t] + s_sum[d][t + o];
                s_min[d][t] = fmin(s_min[d][t], s_min[d][t + o]);
                s_max[d][t] = fmax(s_max[d][t], s_max[d][t + o]);
            }
            s_n[t] += s_n[t + o];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        int cnt = s_n[0];
        pointnum[g] = cnt;
        for (int d = 0; d < 3; ++d) {
            stats[9 * (size_t)g + d] = (float)(s_sum[d][0] / (double)cnt);
            stats[9 * (size_t)g + 3 + d] = (float)s_min[d][0];
            stats[9 * (size_t)g + 6 + d] = (float)s_max[d][0];
        }
    }
}

// inst_info rows (-100 outside [0, instance_num)) and `ins` with the batch's running instance offset
__global__ void k_inst_rows(const int* __restrict__ lab, const int* __restrict__ ostart, int n_scenes,
                            const int* __restrict__ ipos, const int* __restrict__ inst_off, const float* __restrict__ stats,
                            float* __restrict__ info, long long* __restrict__ ins) {
    int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= ostart[n_scenes]) return;
    int s = seg_of(ostart, n_scenes, r);
    int l = lab[r];
    int n_inst = ipos[s + 1] - ipos[s];
    bool in = l >= 0 && l < n_inst;
    for (int c = 0; c < 9; ++c) info[9 * (size_t)r + c] = in ? stats[9 * (size_t)(ipos[s] + l) + c] : -100.0f;
    ins[r] = l != NO_INST ? (long long)l + inst_off[s] : (long long)NO_INST;
}

// ME.utils.sparse_quantize: floor(xyz / voxel) of the float64 coordinates, batch index first; xyz_original in float32
__global__ void k_quantize(const double* __restrict__ xyz, const int* __restrict__ ostart, int n_scenes, double voxel,
                           int* __restrict__ c4, float* __restrict__ xyz32) {
    int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= ostart[n_scenes]) return;
    int s = seg_of(ostart, n_scenes, r);
    c4[4 * (size_t)r] = s;
    for (int d = 0; d < 3; ++d) {
        double x = xyz[3 * (size_t)r + d];
        c4[4 * (size_t)r + 1 + d] = (int)floor(x / voxel);
        xyz32[3 * (size_t)r + d] = (float)x;
    }
}

int seg_blocks(long long rows_per_seg) {
    int b = cdiv(rows_per_seg > 0 ? rows_per_seg : 1, AUG_THREADS * 4);
    return b < 1 ? 1 : (b > 256 ? 256 : b);
}

}  // namespace

extern "C" {

int pbn_aug_chunks(int n_rows) { return n_rows <= 0 ? 1 : cdiv(n_rows, AUG_CHUNK); }

size_t pbn_aug_workspace_bytes(int n_segments) { return (size_t)(n_segments > 0 ? n_segments : 1) * 6 * sizeof(uint64_t); }

int pbn_aug_affine(const float* xyz, const int32_t* unit_off, int n_units, int max_unit_rows, const int32_t* pre_min,
                   const double* mats, const double* scale, const int32_t* has_scale, double* out, double* ext,
                   void* workspace, pbn_stream_t stream_) {
    if (n_units <= 0 || max_unit_rows < 0 || !xyz || !unit_off || !pre_min || !mats || !scale || !has_scale || !out || !ext ||
        !workspace)
        return PBN_ERR_ARG;
    hipStream_t stream = (hipStream_t)stream_;
    unsigned long long* keys = (unsigned long long*)workspace;
    dim3 grid(seg_blocks(max_unit_rows), n_units);
    int kb = cdiv(6 * n_units, 256);
    k_keys_init<<<kb, 256, 0, stream>>>(keys, n_units);
    k_min_f32<<<grid, AUG_THREADS, 0, stream>>>(xyz, unit_off, pre_min, keys);
    k_keys_final<<<kb, 256, 0, stream>>>(keys, n_units, ext);
    k_keys_init<<<kb, 256, 0, stream>>>(keys, n_units);
    k_affine<<<grid, AUG_THREADS, 0, stream>>>(xyz, unit_off, pre_min, ext, mats, out, keys);
    k_keys_final<<<kb, 256, 0, stream>>>(keys, n_units, ext);
    k_keys_init<<<kb, 256, 0, stream>>>(keys, n_units);
    k_sub_scale<<<grid, AUG_THREADS, 0, stream>>>(out, unit_off, ext, scale, has_scale, keys);
    k_keys_final<<<kb, 256, 0, stream>>>(keys, n_units, ext);
    PBN_LAUNCH_CHECK();
    return PBN_OK;
}

int pbn_aug_elastic(double* xyz, const int32_t* unit_off, int n_units, int max_unit_rows, const int32_t* desc,
                    int n_el, int total_cells, float* noise, float* tmp, int gran, double mag, double* ext, void* workspace,
                    pbn_stream_t stream_) {
    if (n_units <= 0 || n_el <= 0 || total_cells <= 0 || gran <= 0 || !xyz || !unit_off || !desc || !noise || !tmp || !ext ||
        !workspace)
        return PBN_ERR_ARG;
    hipStream_t stream = (hipStream_t)stream_;
    unsigned long long* keys = (unsigned long long*)workspace;
    int cb = cdiv(total_cells, 256);
    float* a = noise;
    float* b = tmp;
    for (int p = 0; p < 6; ++p) {                 // blur0, blur1, blur2, blur0, blur1, blur2
        k_blur<<<cb, 256, 0, stream>>>(a, b, desc, n_el, total_cells, p % 3);
        float* t = a; a = b; b = t;
    }
    int kb = cdiv(6 * n_units, 256);
    k_keys_init<<<kb, 256, 0, stream>>>(keys, n_units);
    k_elastic<<<dim3(seg_blocks(max_unit_rows), n_el), AUG_THREADS, 0, stream>>>(xyz, unit_off, desc, a, gran, mag, keys);
    k_keys_final<<<kb, 256, 0, stream>>>(keys, n_units, ext);     // units without elastic keep +inf / -inf (unused)
    PBN_LAUNCH_CHECK();
    return PBN_OK;
}

int pbn_aug_sub_min(double* xyz, const int32_t* unit_off, int n_units, int max_unit_rows, const int32_t* flags,
                    const double* ext, pbn_stream_t stream_) {
    if (n_units <= 0 || !xyz || !unit_off || !flags || !ext) return PBN_ERR_ARG;
    hipStream_t stream = (hipStream_t)stream_;
    k_sub_min<<<dim3(seg_blocks(max_unit_rows), n_units), AUG_THREADS, 0, stream>>>(xyz, unit_off, flags, ext);
    PBN_LAUNCH_CHECK();
    return PBN_OK;
}

int pbn_aug_crop(const double* xyz, const int32_t* scene_off, int n_scenes, int max_scene_rows, const int32_t* mode,
                 const double* triples, const int32_t* n_triples, const double* levels, int max_crop_p, int min_crop_p,
                 int32_t* counts, int32_t* state, double* ext_pre, double* ext_post, void* workspace, pbn_stream_t stream_) {
    if (n_scenes <= 0 || !xyz || !scene_off || !mode || !triples || !n_triples || !levels || !counts || !state || !ext_pre ||
        !ext_post || !workspace)
        return PBN_ERR_ARG;
    hipStream_t stream = (hipStream_t)stream_;
    unsigned long long* keys = (unsigned long long*)workspace;
    PBN_HIP_CHECK(hipMemsetAsync(counts, 0, sizeof(int32_t) * CROP_TRIES * n_scenes * CROP_LEVELS, stream));
    PBN_HIP_CHECK(hipMemsetAsync(state, 0, sizeof(int32_t) * 8 * n_scenes, stream));
    dim3 grid(seg_blocks(max_scene_rows), n_scenes);
    int kb = cdiv(6 * n_scenes, 256);
    k_keys_init<<<kb, 256, 0, stream>>>(keys, n_scenes);
    k_crop_extent<<<grid, AUG_THREADS, 0, stream>>>(xyz, scene_off, mode, triples, levels, state, ext_pre, keys);  // mode!=0 or
    k_keys_final<<<kb, 256, 0, stream>>>(keys, n_scenes, ext_pre);   // no try yet: plain extent (room_range)
    for (int t = 0; t < CROP_TRIES; ++t) {
        k_crop_count<<<grid, AUG_THREADS, 0, stream>>>(xyz, scene_off, mode, triples, levels, ext_pre, state, t, n_scenes,
                                                       counts);
        k_crop_pick<<<cdiv(n_scenes, 64), 64, 0, stream>>>(mode, n_triples, counts, state, t, n_scenes, max_crop_p,
                                                                min_crop_p);
    }
    k_keys_init<<<kb, 256, 0, stream>>>(keys, n_scenes);
    k_crop_extent<<<grid, AUG_THREADS, 0, stream>>>(xyz, scene_off, mode, triples, levels, state, ext_pre, keys);
    k_keys_final<<<kb, 256, 0, stream>>>(keys, n_scenes, ext_post);
    PBN_LAUNCH_CHECK();
    return PBN_OK;
}

int pbn_aug_compact(const double* xyz, const float* rgb, const float* nl, const int64_t* sem, const int32_t* ins,
                    const double* shift, const int32_t* ins_shift, const int32_t* unit_off, int n_units,
                    const int32_t* scene_off, int n_scenes, const int32_t* mode, const double* triples, const double* levels,
                    const int32_t* state, const double* ext_pre, const double* ext_post, const int32_t* label_off,
                    int32_t* label_map, int32_t* present, int32_t* scene_i32, int32_t* scan, double* xyz_out,
                    float* feat_out, int64_t* sem_out, int32_t* label_out, int32_t* scene_info, int n_rows, int n_labels,
                    pbn_stream_t stream_) {
    if (n_units <= 0 || n_scenes <= 0 || n_rows < 0 || n_labels <= 0 || !xyz || !rgb || !nl || !sem || !ins || !shift || !ins_shift ||
        !unit_off || !scene_off || !mode || !triples || !levels || !state || !ext_pre || !ext_post || !label_off ||
        !label_map || !present || !scene_i32 || !scan || !xyz_out || !feat_out || !sem_out || !label_out || !scene_info)
        return PBN_ERR_ARG;
    hipStream_t stream = (hipStream_t)stream_;
    CompactArgs a;
    a.xyz = xyz; a.rgb = rgb; a.nl = nl; a.sem = (const long long*)sem; a.ins = ins; a.shift = shift; a.ins_shift = ins_shift;
    a.uoff = unit_off; a.n_units = n_units; a.per_scene = 0; a.soff = scene_off; a.n_scenes = n_scenes; a.mode = mode;
    a.trip = triples; a.levels = levels; a.state = state; a.ext_pre = ext_pre; a.ext_post = ext_post; a.loff = label_off;
    a.lmap = label_map; a.present = present; a.maxlab = scene_i32; a.scene_n = scene_i32 + n_scenes; a.scan = scan;
    a.xyz_o = xyz_out; a.feat_o = feat_out; a.sem_o = (long long*)sem_out; a.lab_o = label_out; a.sinfo = scene_info;
    a.n_rows = n_rows;
    int n_chunks = pbn_aug_chunks(n_rows);
    // label_map / present: n_labels = label_off[n_scenes] ints each; scene_i32: 2 * n_scenes
    PBN_HIP_CHECK(hipMemsetAsync(present, 0, sizeof(int32_t) * n_labels, stream));
    k_fill_i32<<<cdiv(n_scenes, 64), 64, 0, stream>>>(scene_i32, n_scenes, INT32_MIN);
    PBN_HIP_CHECK(hipMemsetAsync(scene_i32 + n_scenes, 0, sizeof(int32_t) * n_scenes, stream));
    k_fill_i32<<<n_chunks, AUG_THREADS, 0, stream>>>(scan, n_chunks + 1, 0);
    k_mask_count<<<n_chunks, AUG_THREADS, 0, stream>>>(a);
    k_chunk_scan<<<1, AUG_THREADS, 0, stream>>>(scan, n_chunks);
    k_relabel<<<n_scenes, WAVE, 0, stream>>>(a);
    k_scatter<<<n_chunks, AUG_THREADS, 0, stream>>>(a);
    PBN_LAUNCH_CHECK();
    return PBN_OK;
}

int pbn_aug_instances(const double* xyz, const int32_t* label, const int32_t* out_start, int n_scenes,
                      const int32_t* inst_start, const int32_t* inst_off, int n_inst, int n_rows, int32_t* pointnum,
                      float* stats, float* inst_info, int64_t* ins, pbn_stream_t stream_) {
    if (n_scenes <= 0 || n_inst < 0 || n_rows < 0 || !xyz || !label || !out_start || !inst_start || !inst_off || !pointnum ||
        !stats || !inst_info || !ins)
        return PBN_ERR_ARG;
    hipStream_t stream = (hipStream_t)stream_;
    if (n_inst > 0)
        k_inst_stats<<<n_inst, AUG_THREADS, 0, stream>>>(xyz, label, out_start, n_scenes, inst_start, pointnum, stats);
    if (n_rows > 0)
        k_inst_rows<<<cdiv(n_rows, 256), 256, 0, stream>>>(label, out_start, n_scenes, inst_start, inst_off, stats,
                                                                  inst_info, (long long*)ins);
    PBN_LAUNCH_CHECK();
    return PBN_OK;
}

int pbn_aug_quantize(const double* xyz, const int32_t* out_start, int n_scenes, int n_rows, double voxel_size,
                     int32_t* coords, float* xyz_f32, pbn_stream_t stream_) {
    if (n_scenes <= 0 || n_rows < 0 || !(voxel_size > 0.0) || !xyz || !out_start || !coords || !xyz_f32) return PBN_ERR_ARG;
    hipStream_t stream = (hipStream_t)stream_;
    if (n_rows > 0)
        k_quantize<<<cdiv(n_rows, 256), 256, 0, stream>>>(xyz, out_start, n_scenes, voxel_size, coords, xyz_f32);
    PBN_LAUNCH_CHECK();
    return PBN_OK;
}

}  // extern "C"
