// cloud.hip -- a scan without a mesh: the exact k nearest neighbours of every point and PCA normals over them, the two
// inputs lib/segmentator's segment_point leaves to its caller ("the edges can actually be obtained from knn graph").
//
//   box     minimum / maximum per axis as order-preserving u32 keys with integer atomics (augment.hip's idiom), and the
//           check for non-finite coordinates (status bit 1; nothing after it is trusted and the search does not run);
//   grid    one thread: the cell size h (the caller's, or from the box and n / k), enlarged until every axis has at most
//           1024 cells (a cell key (cz, cy, cx) is 30 bits) and the grid has at most t_cap cells; it lives on the device
//           (CloudGrid), nothing is read back;
//   keys    cell key per point + the digit histograms of radix_sort_u32; the stable sort by key with values 0..n-1 is the
//           order (cell key, index);
//   table   from the SORTED keys: thread i opens its cell where key[i-1] differs and closes it where key[i+1] differs, so
//           table[cell] = (first, last + 1) and untouched cells stay (0, 0) = empty; the same kernel gathers the points
//           into sorted order as float4 (x, y, z, index bits);
//   search  one lane per query IN SORTED ORDER (neighbouring lanes walk the same cells and the same candidates), Chebyshev
//           shells of cells around the query's cell, the best k as 64-bit keys (d2 bits << 32 | j) kept sorted in LDS,
//           column layout s_best[rank * 256 + lane]: a wave's access to one rank is 64 consecutive 8-byte words,
//           conflict-free; k = 32 is 64 KiB per workgroup.  No per-lane array, no scratch.
//
// Cell starts: a dense table, not a binary search.  A shell of radius 1 is 27 cells: 27 reads of 8 bytes against 27
// searches of ~17 dependent reads each over the unique keys.  Its size is bounded on the host (t_cap = 4 n clamped to
// [4096, 2^20] cells, 8 bytes each) and the grid kernel enlarges h until the grid fits, so the table never depends on the
// data's extent.  h is a matter of speed only: the result below does not depend on it.
//
// Arithmetic contract (-ffp-contract=off, as mesh.hip): d2(i, j) = ((dx*dx + dy*dy) + dz*dz), dx = x[j] - x[i], every
// operation rounded to float32.  Row i = the k points j != i with the smallest (bits of d2, j), ascending; a short row ends
// in idx = -1, d2 = +inf.  d2 is a sum of squares of finite numbers: never NaN, never -0, so its bits order as its value.
//
// Termination and exactness.  Per axis t(p) = (double(p) - min) * inv (two rounded double operations) and
// cell(p) = floor(t(p)) clamped to [0, dim - 1].  Both are monotone in p.  After the shells 0..r the scanned block is the
// cells [c - r, c + r] of the query's cell c on every axis (clipped).  A point NOT yet scanned lies beyond one of the
// block's faces that is not the grid's outer wall, say the upper face of axis a: cell(p) >= c + r + 1, hence
// t(p) >= c + r + 1 (the clamp only lowers a cell).  With T the exact value of t's expression, |t - T| <= 2^-41 (two
// roundings of 2^-53 relative on a value of at most 1024: h >= extent / 1023), so
//     (p - q) * inv  =  T(p) - T(q)  >=  (c + r + 1) - t(q) - 2^-40,
// and the subtraction that computes the right side errs by at most 2^-43.  D = ((c + r + 1) - t(q) - 2^-38) / inv, scaled
// by (1 - 2^-40) against the division's rounding and floored at 0, is therefore a lower bound of the real p - q; the lower
// face gives t(q) - (c - r) in the same way.  float32 rounding is monotone: fl(p - q) >= fl(D), fl(dx * dx) >=
// fl(fl(D) * fl(D)), and adding the two other non-negative squares never lowers a rounded sum.  So every unscanned point
// has a COMPUTED d2 >= bound2 = fl(fl(D) * fl(D)), D the smallest over the block's inner faces.  A query stops when its
// k-th d2 is STRICTLY below bound2 (strictly: an unscanned point at the same d2 with a smaller index would belong in the
// row; an unfilled row has k-th d2 = +inf and never passes), or when the block covers the grid, which happens at
// r <= 1023 whatever the data: the loop cannot spin.  Neither condition mentions h beyond the bound's value.  The loop is
// shell_walk below, the only one in this file: the search and both fixed-radius kernels differ in what they do with a
// point (visit) and in when they have enough (enough, r2), never in which cells they scan or in the bound.
//
// Normals: one lane per point, float64, no atomics.  S = the point, then its valid neighbours in rank order; mean, then
// the six covariance sums, in that order; the eigenvector of the smallest eigenvalue by a FIXED number of cyclic Jacobi
// sweeps (no data-dependent loop); flipped towards the viewpoint; rounded to float32.  |S| < 3 gives the zero vector.
// pbn_cloud_normals_views runs the same kernel with a viewpoint per point (views[view_of[i]], the sensor position that saw
// it; an index outside the views flips nothing); pbn_cloud_normals is the case of one view and no view_of.
//
// Fixed radius (pbn_cloud_radius_count / pbn_cloud_radius_raw_index): the same grid front (cloud_front below, which
// pbn_cloud_knn runs too) with a cell a hair above the radius, and shell_walk with a radius in place of a k-th neighbour.
// rf = the caller's float32 radius, r2 = fl(rf * rf), j is a neighbour of i when j != i and d2(i, j) <= r2.  By the
// argument above every unscanned point has a computed d2 >= bound2, so shell_walk stops a query when bound2 is STRICTLY
// above r2 (an unscanned point exactly at r2 is a neighbour), when the block covers the grid, or when it has what it came for:
//   count   count[i] = min(neighbours, cap), in a register; the lane stops at cap;
//   route   for a dropped point the kept point with the smallest (d2 bits, j) within r2, one 64-bit key in registers; it
//           also stops once its best d2 is strictly below bound2, as a search for k = 1 would.  Kept lanes write their own
//           rank at once.  keep is read in SORTED order (k_radius_sorted_keep gathers it once through the order), so a
//           candidate's flag lies next to its neighbours' like the candidate itself.
// Neither has LDS, a per-lane array or an atomic.
#include <cmath>

#include "scan_dev.h"

namespace pbn {
namespace {

constexpr int CLOUD_AXIS_CELLS = 1024;
constexpr int CLOUD_EVENTS = 5;                   // around: box + grid | keys + sort | table | search
constexpr u64 CLOUD_PAD_KEY = ((u64)0x7f800000u << 32) | 0xffffffffu;   // d2 = +inf, idx = -1: after every real candidate
constexpr double BOUND_SLACK = 1.0 / 274877906944.0;          // 2^-38 (see the header)
constexpr double BOUND_SCALE = 1.0 - 1.0 / 1099511627776.0;   // 1 - 2^-40

struct CloudGrid {
    double mn[3];
    double inv;       // 1 / h; 0 when the grid is a single cell
    int dim[3];
    int pad;
};

// the ONE expression behind both the cell assignment and the stopping bound
__device__ __forceinline__ double cloud_t(double p, double mn, double inv) { return (p - mn) * inv; }
__device__ __forceinline__ int cloud_cell(double t, int dim) {            // NaN -> 0
    return t >= 0.0 ? (t < (double)dim ? (int)t : dim - 1) : 0;
}

// ---- box ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TPB) void k_cloud_box(const float* __restrict__ xyz, int n, unsigned* __restrict__ box,
                                                   int* __restrict__ status) {
    unsigned lo0 = 0xffffffffu, lo1 = 0xffffffffu, lo2 = 0xffffffffu, hi0 = 0u, hi1 = 0u, hi2 = 0u;
    int bad = 0;
    for (int i = blockIdx.x * TPB + threadIdx.x; i < n; i += gridDim.x * TPB) {
        const float x = xyz[3 * (size_t)i], y = xyz[3 * (size_t)i + 1], z = xyz[3 * (size_t)i + 2];
        bad |= (int)((__float_as_uint(x) & 0x7f800000u) == 0x7f800000u) | (int)((__float_as_uint(y) & 0x7f800000u) == 0x7f800000u) |
               (int)((__float_as_uint(z) & 0x7f800000u) == 0x7f800000u);
        const unsigned kx = okey32(x), ky = okey32(y), kz = okey32(z);
        lo0 = min(lo0, kx); lo1 = min(lo1, ky); lo2 = min(lo2, kz);
        hi0 = max(hi0, kx); hi1 = max(hi1, ky); hi2 = max(hi2, kz);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        lo0 = min(lo0, (unsigned)__shfl_xor((int)lo0, o, 64)); lo1 = min(lo1, (unsigned)__shfl_xor((int)lo1, o, 64));
        lo2 = min(lo2, (unsigned)__shfl_xor((int)lo2, o, 64)); hi0 = max(hi0, (unsigned)__shfl_xor((int)hi0, o, 64));
        hi1 = max(hi1, (unsigned)__shfl_xor((int)hi1, o, 64)); hi2 = max(hi2, (unsigned)__shfl_xor((int)hi2, o, 64));
        bad |= __shfl_xor(bad, o, 64);
    }
    if (lane_id() == 0) {
        atomicMin(&box[0], lo0); atomicMin(&box[1], lo1); atomicMin(&box[2], lo2);
        atomicMax(&box[3], hi0); atomicMax(&box[4], hi1); atomicMax(&box[5], hi2);
        if (bad) atomicOr(status, SCAN_NONFINITE);
    }
}

// ---- grid --------------------------------------------------------------------------------------------------------------
// One thread.  Points on a scan lie on surfaces, so the automatic h aims at k / 2 points per cell of a SURFACE of the box's
// area (a shell of radius 1 then holds ~4.5 k candidates and the k-th neighbour lies ~0.8 h away, inside the first bound);
// a box without area (a line) is divided along its length; a single location gets one cell.
__global__ void k_cloud_grid(const unsigned* __restrict__ box, const int* __restrict__ status, int n, int k, float cell,
                             int t_cap, CloudGrid* __restrict__ g) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    double mn[3], mx[3], ext[3];
    for (int a = 0; a < 3; ++a) {
        mn[a] = (double)okey32_val(box[a]);
        mx[a] = (double)okey32_val(box[3 + a]);
        ext[a] = mx[a] - mn[a];
    }
    int dim[3] = {1, 1, 1};
    double inv = 0.0;
    const bool sane = *status == 0 && ext[0] >= 0.0 && ext[1] >= 0.0 && ext[2] >= 0.0;
    if (sane) {
        const double area = 2.0 * (ext[0] * ext[1] + ext[1] * ext[2] + ext[0] * ext[2]);
        const double len = ext[0] + ext[1] + ext[2];
        const double longest = fmax(ext[0], fmax(ext[1], ext[2]));
        double h = cell > 0.0f ? (double)cell : area > 0.0 ? sqrt(area * (double)k / (2.0 * (double)n))
                                              : len > 0.0 ? len * (double)k / (double)n : 1.0;
        if (!(h > 0.0) || !__builtin_isfinite(h)) h = 1.0;
        const double h_min = longest / 1023.0 * (1.0 + 1.0e-9);            // t <= 1023 on every axis
        if (h < h_min) h = h_min;
        bool fits = false;
        for (int it = 0; it < 64 && !fits; ++it) {                          // 1.25^32 > 1023: all axes reach one cell
            inv = 1.0 / h;
            if (!__builtin_isfinite(inv)) break;
            long long cells = 1;
            for (int a = 0; a < 3; ++a) {
                dim[a] = cloud_cell(cloud_t(mx[a], mn[a], inv), CLOUD_AXIS_CELLS) + 1;   // the cell of the largest coordinate
                cells *= dim[a];
            }
            fits = cells <= (long long)t_cap;
            h *= 1.25;
        }
        if (!fits) { dim[0] = dim[1] = dim[2] = 1; inv = 0.0; }
    }
    for (int a = 0; a < 3; ++a) { g->mn[a] = sane ? mn[a] : 0.0; g->dim[a] = dim[a]; }
    g->inv = inv;
    g->pad = 0;
}

// ---- keys --------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TPB) void k_cloud_keys(const float* __restrict__ xyz, int n, const CloudGrid* __restrict__ g,
                                                    u64* __restrict__ keys, int* __restrict__ vals,
                                                    unsigned* __restrict__ ghist) {
    __shared__ unsigned s_hist[RADIX_U32_PASSES][RADIX];
    hist_clear(s_hist);
    __syncthreads();
    const double m0 = g->mn[0], m1 = g->mn[1], m2 = g->mn[2], inv = g->inv;
    const int d0 = g->dim[0], d1 = g->dim[1], d2 = g->dim[2];
    for (int i = blockIdx.x * TPB + threadIdx.x; i < n; i += gridDim.x * TPB) {
        const int cx = cloud_cell(cloud_t((double)xyz[3 * (size_t)i], m0, inv), d0);
        const int cy = cloud_cell(cloud_t((double)xyz[3 * (size_t)i + 1], m1, inv), d1);
        const int cz = cloud_cell(cloud_t((double)xyz[3 * (size_t)i + 2], m2, inv), d2);
        const unsigned key = ((unsigned)cz << 20) | ((unsigned)cy << 10) | (unsigned)cx;
        keys[i] = (u64)key;
        vals[i] = i;
        hist_add(s_hist, key);
    }
    __syncthreads();
    hist_flush(s_hist, ghist);
}

// ---- table -------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int cloud_linear(unsigned key, int d0, int d1) {
    return ((int)(key >> 20) * d1 + (int)((key >> 10) & 1023u)) * d0 + (int)(key & 1023u);
}

__global__ __launch_bounds__(TPB) void k_cloud_table(const u64* __restrict__ keys, const int* __restrict__ order, int n,
                                                     const float* __restrict__ xyz, const CloudGrid* __restrict__ g,
                                                     int t_cap, int* __restrict__ table, float4* __restrict__ pts) {
    const int d0 = g->dim[0], d1 = g->dim[1];
    for (int i = blockIdx.x * TPB + threadIdx.x; i < n; i += gridDim.x * TPB) {
        const unsigned key = (unsigned)keys[i];
        const int lin = cloud_linear(key, d0, d1);
        if ((unsigned)lin < (unsigned)t_cap) {                               // always, by the grid kernel's bound
            if (i == 0 || (unsigned)keys[i - 1] != key) table[2 * (size_t)lin] = i;
            if (i == n - 1 || (unsigned)keys[i + 1] != key) table[2 * (size_t)lin + 1] = i + 1;
        }
        int j = order[i];
        if ((unsigned)j >= (unsigned)n) j = 0;                               // only after a failed sort (flagged): stay in bounds
        pts[i] = make_float4(xyz[3 * (size_t)j], xyz[3 * (size_t)j + 1], xyz[3 * (size_t)j + 2], __int_as_float(j));
    }
}

// ---- search ------------------------------------------------------------------------------------------------------------
// lower bound of the real coordinate gap to one inner face (see the header): gap = face - t(q) or t(q) - face, in cells
__device__ __forceinline__ float face_bound2(double gap, double inv) {
    double d = (gap - BOUND_SLACK) / inv * BOUND_SCALE;
    if (!(d > 0.0)) d = 0.0;
    const float f = (float)d;
    return f * f;
}

// Cell and t() of a query, as the walks below hold them.
struct CloudQuery {
    int cx, cy, cz, d0, d1, d2;
    double tx, ty, tz, inv;
};

__device__ __forceinline__ CloudQuery cloud_query(const float4 q, unsigned key, const CloudGrid* __restrict__ g) {
    CloudQuery c;
    c.cx = (int)(key & 1023u); c.cy = (int)((key >> 10) & 1023u); c.cz = (int)(key >> 20);
    c.d0 = g->dim[0]; c.d1 = g->dim[1]; c.d2 = g->dim[2];
    c.inv = g->inv;
    c.tx = cloud_t((double)q.x, g->mn[0], c.inv); c.ty = cloud_t((double)q.y, g->mn[1], c.inv);
    c.tz = cloud_t((double)q.z, g->mn[2], c.inv);
    return c;
}

// bound2 of the block of shells 0..r (see the header): the smallest over its faces inside the grid; false when it has none
__device__ __forceinline__ bool block_bound2(const CloudQuery& c, int r, float& bound2) {
    bound2 = __uint_as_float(0x7f800000u);
    bool inner = false;                                                      // does the block have a face inside the grid?
    if (c.cx - r > 0) { inner = true; bound2 = fminf(bound2, face_bound2(c.tx - (double)(c.cx - r), c.inv)); }
    if (c.cy - r > 0) { inner = true; bound2 = fminf(bound2, face_bound2(c.ty - (double)(c.cy - r), c.inv)); }
    if (c.cz - r > 0) { inner = true; bound2 = fminf(bound2, face_bound2(c.tz - (double)(c.cz - r), c.inv)); }
    if (c.cx + r < c.d0 - 1) { inner = true; bound2 = fminf(bound2, face_bound2((double)(c.cx + r + 1) - c.tx, c.inv)); }
    if (c.cy + r < c.d1 - 1) { inner = true; bound2 = fminf(bound2, face_bound2((double)(c.cy + r + 1) - c.ty, c.inv)); }
    if (c.cz + r < c.d2 - 1) { inner = true; bound2 = fminf(bound2, face_bound2((double)(c.cz + r + 1) - c.tz, c.inv)); }
    return inner;
}

// The file's ONE walk over the Chebyshev shells of cells around a query's cell (the header's "Termination and exactness").
// visit(i, pts[i]) sees every point of the scanned cells, the query included, and returns false once the lane needs no
// more; after each shell the walk ends when the block covers the grid, when bound2 > r2 (a search passes r2 = +inf:
// never), or when enough(bound2) says so.
template <typename Visit, typename Enough>
__device__ __forceinline__ void shell_walk(const float4* __restrict__ pts, const int2* __restrict__ table,
                                            const CloudQuery& c, float r2, Visit visit, Enough enough) {
    const int cx = c.cx, cy = c.cy, cz = c.cz;
    bool more = true;
    for (int r = 0; r < CLOUD_AXIS_CELLS; ++r) {
        const int xlo = max(cx - r, 0), xhi = min(cx + r, c.d0 - 1);
        const int ylo = max(cy - r, 0), yhi = min(cy + r, c.d1 - 1);
        const int zlo = max(cz - r, 0), zhi = min(cz + r, c.d2 - 1);
        for (int z = zlo; z <= zhi && more; ++z) {
            for (int y = ylo; y <= yhi && more; ++y) {
                // a row on the shell's y / z faces is scanned whole, an inner row only at its two ends
                const bool full = (z - cz == r) || (cz - z == r) || (y - cy == r) || (cy - y == r);
                int x = full ? xlo : (cx - r >= 0 ? cx - r : cx + r);
                while (x <= xhi && more) {
                    const int2 se = table[(size_t)(z * c.d1 + y) * c.d0 + x];
                    for (int i = se.x; i < se.y && more; ++i) more = visit(i, pts[i]);
                    x = full ? x + 1 : (x < cx + r ? cx + r : xhi + 1);
                }
            }
        }
        float bound2;
        if (!more || !block_bound2(c, r, bound2) || bound2 > r2 || enough(bound2)) break;
    }
}

__global__ __launch_bounds__(TPB) void k_cloud_search(const float4* __restrict__ pts, const u64* __restrict__ keys,
                                                      const int2* __restrict__ table, const CloudGrid* __restrict__ g,
                                                      const int* __restrict__ status, int n, int k,
                                                      int* __restrict__ idx, float* __restrict__ d2_out) {
    extern __shared__ __attribute__((aligned(16))) u64 s_best[];            // [k][TPB], lane-minor
    if (*status != 0) return;                                                // non-finite input or a failed sort: no row is written
    const int tid = threadIdx.x;
    const int t = blockIdx.x * TPB + tid;
    if (t >= n) return;                                                      // no barrier below: every lane owns its column
    u64* __restrict__ best = s_best + tid;
    for (int r = 0; r < k; ++r) best[r * TPB] = CLOUD_PAD_KEY;
    u64 worst = CLOUD_PAD_KEY;

    const float4 q = pts[t];
    const int qi = __float_as_int(q.w);
    shell_walk(pts, table, cloud_query(q, (unsigned)keys[t], g), __uint_as_float(0x7f800000u),   // r2 = +inf: no radius
               [&](int, const float4 c) {
                   const int j = __float_as_int(c.w);
                   if (j == qi) return true;                                 // self goes by index, not by distance
                   const float dx = c.x - q.x, dy = c.y - q.y, dz = c.z - q.z;
                   const float dd = (dx * dx + dy * dy) + dz * dz;
                   const u64 ck = ((u64)__float_as_uint(dd) << 32) | (unsigned)j;
                   if (ck < worst) {
                       int p = k - 1;
                       while (p > 0) {                                       // at most k - 1 steps
                           const u64 prev = best[(p - 1) * TPB];
                           if (prev <= ck) break;
                           best[p * TPB] = prev;
                           --p;
                       }
                       best[p * TPB] = ck;
                       worst = best[(k - 1) * TPB];
                   }
                   return true;                                              // a search never has enough before a shell ends
               },
               [&](float bound2) { return __uint_as_float((unsigned)(worst >> 32)) < bound2; });
    for (int r = 0; r < k; ++r) {
        const u64 b = best[r * TPB];
        idx[(size_t)qi * k + r] = (int)(unsigned)b;
        d2_out[(size_t)qi * k + r] = __uint_as_float((unsigned)(b >> 32));
    }
}

// ---- fixed radius ------------------------------------------------------------------------------------------------------
// One lane per query in sorted order; count[query] = min(points j != query with d2 <= r2, cap).
__global__ __launch_bounds__(TPB) void k_radius_count(const float4* __restrict__ pts, const u64* __restrict__ keys,
                                                      const int2* __restrict__ table, const CloudGrid* __restrict__ g,
                                                      const int* __restrict__ status, int n, float r2, int cap,
                                                      int* __restrict__ count) {
    if (*status != 0) return;                                                // non-finite input or a failed sort: no row is written
    const int t = blockIdx.x * TPB + threadIdx.x;
    if (t >= n) return;
    const float4 q = pts[t];
    const int qi = __float_as_int(q.w);
    int cnt = 0;
    shell_walk(pts, table, cloud_query(q, (unsigned)keys[t], g), r2,
                [&](int, const float4 c) {
                    const float dx = c.x - q.x, dy = c.y - q.y, dz = c.z - q.z;
                    const float dd = (dx * dx + dy * dy) + dz * dz;
                    cnt += (int)(__float_as_int(c.w) != qi && dd <= r2);     // self goes by index, not by distance
                    return cnt < cap;
                },
                [](float) { return false; });
    count[qi] = cnt;
}

// keep in sorted order for the walk, and as the 0 / 1 ints the scan takes
__global__ __launch_bounds__(TPB) void k_radius_sorted_keep(const float4* __restrict__ pts, const unsigned char* __restrict__ keep,
                                                            const int* __restrict__ status, int n,
                                                            unsigned char* __restrict__ skeep, int* __restrict__ flag) {
    if (*status != 0) return;                                                // pts is not trusted
    for (int i = blockIdx.x * TPB + threadIdx.x; i < n; i += gridDim.x * TPB) {
        skeep[i] = keep[__float_as_int(pts[i].w)] ? 1 : 0;
        flag[i] = keep[i] ? 1 : 0;
    }
}

// One lane per point in sorted order; route[point] = its rank when kept, else the rank of the kept point with the smallest
// (d2 bits, index) among those with d2 <= r2, else -1.  rank[] is the exclusive scan of keep in the caller's order.
__global__ __launch_bounds__(TPB) void k_radius_route(const float4* __restrict__ pts, const u64* __restrict__ keys,
                                                      const int2* __restrict__ table, const CloudGrid* __restrict__ g,
                                                      const int* __restrict__ status, int n, float r2,
                                                      const unsigned char* __restrict__ skeep, const int* __restrict__ rank,
                                                      int* __restrict__ route) {
    if (*status != 0) return;
    const int t = blockIdx.x * TPB + threadIdx.x;
    if (t >= n) return;
    const float4 q = pts[t];
    const int qi = __float_as_int(q.w);
    if (skeep[t]) { route[qi] = rank[qi]; return; }
    u64 best = CLOUD_PAD_KEY;
    shell_walk(pts, table, cloud_query(q, (unsigned)keys[t], g), r2,
                [&](int i, const float4 c) {
                    const float dx = c.x - q.x, dy = c.y - q.y, dz = c.z - q.z;
                    const float dd = (dx * dx + dy * dy) + dz * dz;
                    const u64 ck = ((u64)__float_as_uint(dd) << 32) | (unsigned)__float_as_int(c.w);
                    if (skeep[i] && dd <= r2 && ck < best) best = ck;        // the query itself is dropped: never a candidate
                    return true;
                },
                [&](float bound2) { return __uint_as_float((unsigned)(best >> 32)) < bound2; });
    route[qi] = best == CLOUD_PAD_KEY ? -1 : rank[(int)(unsigned)best];
}

__global__ __launch_bounds__(TPB) void k_radius_gather(const int* __restrict__ inverse, int n_raw, const int* __restrict__ route,
                                                       int n, const int* __restrict__ status, int* __restrict__ out) {
    if (*status != 0) return;                                                // no row is written
    for (int i = blockIdx.x * TPB + threadIdx.x; i < n_raw; i += gridDim.x * TPB) {
        const int t = inverse[i];
        out[i] = (unsigned)t < (unsigned)n ? route[t] : -1;
    }
}

// ---- normals -----------------------------------------------------------------------------------------------------------
// The unit eigenvector of point i's neighbourhood covariance, before any flip; false (nothing written) with |S| < 3.
__device__ __forceinline__ bool cloud_pca(const float* __restrict__ xyz, int n, const int* __restrict__ idx, int k, int i,
                                          double& px, double& py, double& pz, double& nx, double& ny, double& nz) {
    px = (double)xyz[3 * (size_t)i]; py = (double)xyz[3 * (size_t)i + 1]; pz = (double)xyz[3 * (size_t)i + 2];
    double sx = px, sy = py, sz = pz;
    int m = 1;
    for (int r = 0; r < k; ++r) {
        const int j = idx[(size_t)i * k + r];
        if ((unsigned)j >= (unsigned)n) continue;                            // -1 (or anything out of range) is no neighbour
        sx = sx + (double)xyz[3 * (size_t)j]; sy = sy + (double)xyz[3 * (size_t)j + 1]; sz = sz + (double)xyz[3 * (size_t)j + 2];
        ++m;
    }
    if (m < 3) return false;
    const double mx = sx / (double)m, my = sy / (double)m, mz = sz / (double)m;
    double dx = px - mx, dy = py - my, dz = pz - mz;
    double a00 = dx * dx, a01 = dx * dy, a02 = dx * dz, a11 = dy * dy, a12 = dy * dz, a22 = dz * dz;
    for (int r = 0; r < k; ++r) {
        const int j = idx[(size_t)i * k + r];
        if ((unsigned)j >= (unsigned)n) continue;
        dx = (double)xyz[3 * (size_t)j] - mx; dy = (double)xyz[3 * (size_t)j + 1] - my; dz = (double)xyz[3 * (size_t)j + 2] - mz;
        a00 = a00 + dx * dx; a01 = a01 + dx * dy; a02 = a02 + dx * dz;
        a11 = a11 + dy * dy; a12 = a12 + dy * dz; a22 = a22 + dz * dz;
    }
    jacobi_smallest(a00, a01, a02, a11, a12, a22, nx, ny, nz);         // scan_dev.h
    return true;
}

// float64 throughout: 4 waves per SIMD leave the 128 VGPRs the rotations want (no scratch).  With view_of (non-null) point
// i looks at views[view_of[i]], and at nothing (no flip) when that index lies outside [0, n_views); without it every point
// looks at views[0].
__global__ __launch_bounds__(TPB) __attribute__((amdgpu_waves_per_eu(1, 4))) void k_cloud_normals(const float* __restrict__ xyz, int n, const int* __restrict__ idx,
                                                       int k, const float* __restrict__ views, int n_views,
                                                       const int* __restrict__ view_of, float* __restrict__ nl) {
    for (int i = blockIdx.x * TPB + threadIdx.x; i < n; i += gridDim.x * TPB) {
        double px, py, pz, nx, ny, nz;
        if (!cloud_pca(xyz, n, idx, k, i, px, py, pz, nx, ny, nz)) {
            nl[3 * (size_t)i] = 0.0f; nl[3 * (size_t)i + 1] = 0.0f; nl[3 * (size_t)i + 2] = 0.0f;
            continue;
        }
        const int w = view_of ? view_of[i] : 0;
        if ((unsigned)w < (unsigned)n_views) {
            const float* __restrict__ vp = views + 3 * (size_t)w;
            const double dot = (nx * ((double)vp[0] - px) + ny * ((double)vp[1] - py)) + nz * ((double)vp[2] - pz);
            if (dot < 0.0) { nx = -nx; ny = -ny; nz = -nz; }
        }
        nl[3 * (size_t)i] = (float)nx; nl[3 * (size_t)i + 1] = (float)ny; nl[3 * (size_t)i + 2] = (float)nz;
    }
}

// ---- workspace -------------------------------------------------------------------------------------------------------
struct CloudWs {
    unsigned* box; CloudGrid* grid; SortBufs sort; float4* pts; int* table; int t_cap;
};

int table_cap(int n) {
    const long long want = 4LL * n;
    return (int)(want < 4096 ? 4096 : want > (1 << 20) ? (1 << 20) : want);
}

CloudWs carve(Carver& cv, int n) {
    CloudWs w{};
    const size_t N = (size_t)(n > 0 ? n : 1);
    w.box = cv.take<unsigned>(64);
    w.grid = cv.take<CloudGrid>(1);
    w.sort = sort_carve(cv, N, 1);
    w.pts = cv.take<float4>(N);
    w.t_cap = table_cap(n);
    w.table = cv.take<int>(2 * (size_t)w.t_cap);
    return w;
}

size_t ws_bytes(int n) {
    Carver cv(nullptr, 0);
    carve(cv, n);
    return cv.off + 256;
}

bool bad_sizes(int n, int k) { return n < 0 || n > SCAN_MAX_POINTS || k < 1 || k > SCAN_MAX_K; }

// The grid front of every search in this file: status zeroed, then box -> grid -> keys -> sort -> table, after which
// w.pts, w.sort.keys_b, w.table and w.grid describe the cloud.  `k` only feeds the automatic cell size (cell <= 0).
// ev (optional): ev[0..3] are recorded around box + grid | keys + sort | table; ev[4..n_events) are the caller's, and with
// n == 0 (status zeroed, nothing else launched) they are recorded here too.
int cloud_front(const float* xyz, int n, int k, float cell, int32_t* status, const CloudWs& w, hipStream_t st, hipEvent_t* ev,
                int n_events) {
    const FillRange fr[] = {{status, sizeof(int32_t), 0}, {w.box, 3 * sizeof(unsigned), 0xff},
                            {w.box + 3, 3 * sizeof(unsigned), 0}, sort_hist_fill(w.sort, 0),
                            {w.table, 2 * (size_t)w.t_cap * sizeof(int), 0}};
    int rc = fill_ranges(fr, n > 0 ? 5 : 1, st);
    if (rc != PBN_OK) return rc;
    if (ev) PBN_HIP_CHECK(hipEventRecord(ev[0], st));
    if (n == 0) {
        if (ev) for (int i = 1; i < n_events; ++i) PBN_HIP_CHECK(hipEventRecord(ev[i], st));
        return PBN_OK;
    }
    hipLaunchKernelGGL(k_cloud_box, dim3(grid_for(n)), dim3(TPB), 0, st, xyz, n, w.box, status);
    hipLaunchKernelGGL(k_cloud_grid, dim3(1), dim3(64), 0, st, w.box, status, n, k, cell, w.t_cap, w.grid);
    if (ev) PBN_HIP_CHECK(hipEventRecord(ev[1], st));
    hipLaunchKernelGGL(k_cloud_keys, dim3(grid_for(n)), dim3(TPB), 0, st, xyz, n, w.grid, w.sort.keys_a, w.sort.vals_a,
                       w.sort.ghist[0]);
    PBN_LAUNCH_CHECK();
    rc = sort_run(w.sort, 0, n, status, st);
    if (rc != PBN_OK) return rc;
    if (ev) PBN_HIP_CHECK(hipEventRecord(ev[2], st));
    hipLaunchKernelGGL(k_cloud_table, dim3(grid_for(n)), dim3(TPB), 0, st, w.sort.keys_b, w.sort.vals_b, n, xyz, w.grid, w.t_cap,
                       w.table, w.pts);
    if (ev) PBN_HIP_CHECK(hipEventRecord(ev[3], st));
    return PBN_OK;
}

// ev (optional): CLOUD_EVENTS events
int cloud_knn(const float* xyz, int n, int k, float cell, int32_t* idx, float* d2, int32_t* status, void* workspace,
              size_t workspace_bytes, hipStream_t st, hipEvent_t* ev) {
    Carver cv(workspace, workspace_bytes);
    const CloudWs w = carve(cv, n);
    if (!cv.ok) return PBN_ERR_WORKSPACE;
    const int rc = cloud_front(xyz, n, k, cell, status, w, st, ev, CLOUD_EVENTS);
    if (rc != PBN_OK || n == 0) return rc;
    const size_t lds = (size_t)k * TPB * sizeof(u64);
    static const bool lds_attr = (hipFuncSetAttribute((const void*)k_cloud_search, hipFuncAttributeMaxDynamicSharedMemorySize,
                                                      (int)(SCAN_MAX_K * TPB * sizeof(u64))) == hipSuccess);
    if (!lds_attr) return PBN_ERR_HIP;
    hipLaunchKernelGGL(k_cloud_search, dim3((unsigned)cdiv(n, TPB)), dim3(TPB), lds, st, w.pts, w.sort.keys_b,
                       reinterpret_cast<const int2*>(w.table), w.grid, status, n, k, idx, d2);
    if (ev) PBN_HIP_CHECK(hipEventRecord(ev[4], st));
    PBN_LAUNCH_CHECK();
    return PBN_OK;
}

int knn_args(const float* xyz, int n, int k, const int32_t* idx, const float* d2, const int32_t* status, const void* workspace,
             size_t workspace_bytes) {
    if (bad_sizes(n, k)) return PBN_ERR_ARG;
    if ((n && (!xyz || !idx || !d2)) || !status || !workspace) return PBN_ERR_ARG;
    if (workspace_bytes < ws_bytes(n)) return PBN_ERR_WORKSPACE;
    return PBN_OK;
}

// ---- fixed radius: host ------------------------------------------------------------------------------------------------
constexpr int RADIUS_EVENTS = 5;                  // around: box + grid | keys + sort | table | count
constexpr float RADIUS_CELL_SCALE = 1.0f + 1.0f / 1024.0f;   // the automatic cell: a hair above the radius

struct RadiusWs {
    CloudWs cloud; unsigned char* skeep; int* flag; int* rank; int* scan_tmp; int* route;     // the five: the routing alone
};

RadiusWs radius_carve(Carver& cv, int n, bool routing) {
    RadiusWs w{};
    w.cloud = carve(cv, n);
    if (!routing) return w;
    const size_t N = (size_t)(n > 0 ? n : 1);
    w.skeep = cv.take<unsigned char>(N);
    w.flag = cv.take<int>(N); w.rank = cv.take<int>(N);
    w.scan_tmp = cv.take<int>(scan_tmp_ints((long long)N));
    w.route = cv.take<int>(N);
    return w;
}

size_t radius_ws_bytes(int n, bool routing) {
    Carver cv(nullptr, 0);
    radius_carve(cv, n, routing);
    return cv.off + 256;
}

bool bad_points(int n) { return n < 0 || n > SCAN_MAX_POINTS; }
bool bad_radius(float radius) { return !(radius > 0.0f) || !std::isfinite(radius); }
// the cell handed to k_cloud_grid, which enlarges it until the grid fits: never the result, only the speed
float radius_cell(float radius, float cell) { return cell > 0.0f ? cell : radius * RADIUS_CELL_SCALE; }

// ev (optional): RADIUS_EVENTS events
int radius_count(const float* xyz, int n, float radius, int cap, float cell, int32_t* count, int32_t* status, void* workspace,
                 size_t workspace_bytes, hipStream_t st, hipEvent_t* ev) {
    Carver cv(workspace, workspace_bytes);
    const CloudWs w = radius_carve(cv, n, false).cloud;
    if (!cv.ok) return PBN_ERR_WORKSPACE;
    const int rc = cloud_front(xyz, n, 1, radius_cell(radius, cell), status, w, st, ev, RADIUS_EVENTS);
    if (rc != PBN_OK || n == 0) return rc;
    hipLaunchKernelGGL(k_radius_count, dim3((unsigned)cdiv(n, TPB)), dim3(TPB), 0, st, w.pts, w.sort.keys_b,
                       reinterpret_cast<const int2*>(w.table), w.grid, status, n, radius * radius, cap, count);
    if (ev) PBN_HIP_CHECK(hipEventRecord(ev[4], st));
    PBN_LAUNCH_CHECK();
    return PBN_OK;
}

int radius_count_args(const float* xyz, int n, float radius, int cap, const int32_t* count, const int32_t* status,
                      const void* workspace, size_t workspace_bytes) {
    if (bad_points(n) || bad_radius(radius) || cap < 1) return PBN_ERR_ARG;
    if ((n && (!xyz || !count)) || !status || !workspace) return PBN_ERR_ARG;
    if (workspace_bytes < radius_ws_bytes(n, false)) return PBN_ERR_WORKSPACE;
    return PBN_OK;
}

}  // namespace

int cloud_box(const float* xyz, int n, unsigned* box, int32_t* status, hipStream_t st) {
    hipLaunchKernelGGL(k_cloud_box, dim3(grid_for(n)), dim3(TPB), 0, st, xyz, n, box, status);
    PBN_LAUNCH_CHECK();
    return PBN_OK;
}

}  // namespace pbn

using namespace pbn;

extern "C" int pbn_cloud_max_k(void) { return SCAN_MAX_K; }

extern "C" size_t pbn_cloud_workspace_bytes(int n_points, int k) {
    if (bad_sizes(n_points, k)) return 0;
    return ws_bytes(n_points);
}

extern "C" int pbn_cloud_knn(const float* xyz, int n_points, int k, float cell, int32_t* idx, float* d2, int32_t* status,
                             void* workspace, size_t workspace_bytes, pbn_stream_t stream) {
    const int rc = knn_args(xyz, n_points, k, idx, d2, status, workspace, workspace_bytes);
    if (rc != PBN_OK) return rc;
    return cloud_knn(xyz, n_points, k, cell, idx, d2, status, workspace, workspace_bytes, (hipStream_t)stream, nullptr);
}

extern "C" int pbn_cloud_knn_timed(const float* xyz, int n_points, int k, float cell, int32_t* idx, float* d2, int32_t* status,
                                   void* workspace, size_t workspace_bytes, pbn_stream_t stream, float* times_ms) {
    const int rc = knn_args(xyz, n_points, k, idx, d2, status, workspace, workspace_bytes);
    if (rc != PBN_OK) return rc;
    if (!times_ms) return PBN_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    return timed_stages<CLOUD_EVENTS>(st, times_ms, [&](hipEvent_t* ev) {
        return cloud_knn(xyz, n_points, k, cell, idx, d2, status, workspace, workspace_bytes, st, ev);
    });
}

extern "C" int pbn_cloud_normals(const float* xyz, int n_points, const int32_t* idx, int k, const float* viewpoint, float* nl,
                                 pbn_stream_t stream) {
    if (bad_sizes(n_points, k)) return PBN_ERR_ARG;
    if ((n_points && (!xyz || !idx || !nl)) || !viewpoint) return PBN_ERR_ARG;
    if (n_points == 0) return PBN_OK;
    hipLaunchKernelGGL(k_cloud_normals, dim3(grid_for(n_points)), dim3(TPB), 0, (hipStream_t)stream, xyz, n_points, idx, k,
                       viewpoint, 1, (const int*)nullptr, nl);
    PBN_LAUNCH_CHECK();
    return PBN_OK;
}

extern "C" int pbn_cloud_normals_views(const float* xyz, int n_points, const int32_t* idx, int k, const float* views, int n_views,
                                       const int32_t* view_of, float* nl, pbn_stream_t stream) {
    if (bad_sizes(n_points, k) || n_views < 0) return PBN_ERR_ARG;
    if ((n_points && (!xyz || !idx || !nl || !view_of)) || (n_views && !views)) return PBN_ERR_ARG;
    if (n_points == 0) return PBN_OK;
    hipLaunchKernelGGL(k_cloud_normals, dim3(grid_for(n_points)), dim3(TPB), 0, (hipStream_t)stream, xyz, n_points, idx, k,
                       views, n_views, view_of, nl);
    PBN_LAUNCH_CHECK();
    return PBN_OK;
}

extern "C" size_t pbn_cloud_radius_workspace_bytes(int n_points) {
    if (bad_points(n_points)) return 0;
    return radius_ws_bytes(n_points, false);
}

extern "C" int pbn_cloud_radius_count(const float* xyz, int n_points, float radius, int cap, float cell, int32_t* count,
                                      int32_t* status, void* workspace, size_t workspace_bytes, pbn_stream_t stream) {
    const int rc = radius_count_args(xyz, n_points, radius, cap, count, status, workspace, workspace_bytes);
    if (rc != PBN_OK) return rc;
    return radius_count(xyz, n_points, radius, cap, cell, count, status, workspace, workspace_bytes, (hipStream_t)stream, nullptr);
}

extern "C" int pbn_cloud_radius_count_timed(const float* xyz, int n_points, float radius, int cap, float cell, int32_t* count,
                                            int32_t* status, void* workspace, size_t workspace_bytes, pbn_stream_t stream,
                                            float* times_ms) {
    const int rc = radius_count_args(xyz, n_points, radius, cap, count, status, workspace, workspace_bytes);
    if (rc != PBN_OK) return rc;
    if (!times_ms) return PBN_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    return timed_stages<RADIUS_EVENTS>(st, times_ms, [&](hipEvent_t* ev) {
        return radius_count(xyz, n_points, radius, cap, cell, count, status, workspace, workspace_bytes, st, ev);
    });
}

extern "C" size_t pbn_cloud_radius_raw_index_workspace_bytes(int n_points, int n_raw) {
    if (bad_points(n_points) || bad_points(n_raw)) return 0;
    return radius_ws_bytes(n_points, true);
}

extern "C" int pbn_cloud_radius_raw_index(const float* xyz, int n_points, const uint8_t* keep, float radius, float cell,
                                          const int32_t* inverse, int n_raw, int32_t* raw_index, int32_t* status,
                                          void* workspace, size_t workspace_bytes, pbn_stream_t stream) {
    const int n = n_points;
    if (bad_points(n) || bad_points(n_raw) || bad_radius(radius)) return PBN_ERR_ARG;
    if ((n && (!xyz || !keep)) || (n_raw && (!inverse || !raw_index)) || !status || !workspace) return PBN_ERR_ARG;
    if (workspace_bytes < radius_ws_bytes(n, true)) return PBN_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    Carver cv(workspace, workspace_bytes);
    const RadiusWs w = radius_carve(cv, n, true);
    if (!cv.ok) return PBN_ERR_WORKSPACE;
    if (n_raw == 0 || n == 0) {                                              // nothing to route, or nobody to route to
        const FillRange fr[] = {{status, sizeof(int32_t), 0}, {raw_index, (size_t)n_raw * sizeof(int32_t), 0xff}};
        return fill_ranges(fr, n_raw > 0 ? 2 : 1, st);
    }
    int rc = cloud_front(xyz, n, 1, radius_cell(radius, cell), status, w.cloud, st, nullptr, 0);
    if (rc != PBN_OK) return rc;
    const int2* table = reinterpret_cast<const int2*>(w.cloud.table);
    hipLaunchKernelGGL(k_radius_sorted_keep, dim3(grid_for(n)), dim3(TPB), 0, st, w.cloud.pts, keep, status, n, w.skeep, w.flag);
    PBN_LAUNCH_CHECK();
    rc = scan_exclusive_i32(w.flag, w.rank, n, w.scan_tmp, nullptr, st);
    if (rc != PBN_OK) return rc;
    hipLaunchKernelGGL(k_radius_route, dim3((unsigned)cdiv(n, TPB)), dim3(TPB), 0, st, w.cloud.pts, w.cloud.sort.keys_b, table,
                       w.cloud.grid, status, n, radius * radius, w.skeep, w.rank, w.route);
    hipLaunchKernelGGL(k_radius_gather, dim3(grid_for(n_raw)), dim3(TPB), 0, st, inverse, n_raw, w.route, n, status, raw_index);
    PBN_LAUNCH_CHECK();
    return PBN_OK;
}
