// orient.hip -- consistent normal orientation of a cloud over its kNN graph (Hoppe et al. 1992; PCL / Open3D's
// orient_normals_consistent_tangent_plane): the signs are propagated along the minimum spanning forest of the graph under
// the weight 1 - |n_i . n_j|, found by Boruvka rounds over a union-find that carries each point's parity to its root.
//
// Contract: include/pbnet_hip.h ("Normal orientation"); tests/orient_ref.py restates it with a sequential Kruskal.  Edge
// keys (order_key(w) << 32 | slot) are distinct, so the forest is unique and so is every output, whatever finds it.
//
//   codes     per slot e = i * k + r: code[e] = j, ~j when the dot is negative, or ORIENT_NONE when the slot is no edge;
//             wkey[e] = order_key(w_e).  The slot's first lane (r = 0) writes comp[i] = i and sgn[i] = 0, or 2 = null.
//   min       per slot whose ends lie in different components: atomicMin of the 64-bit key on best[comp[i]] AND on
//             best[comp[j]] (an edge offered only to its source's side lets two components pick the twin slots of one
//             pair, or miss their minimum).  Lanes of a wave that follow each other with the same comp[i] -- the k slots of a
//             point, later whole waves -- reduce with shuffles first and only the run's first lane goes to memory; every
//             atomic is preceded by a read of the word and skipped when the key cannot win.
//   hook      a root c with a chosen edge links to the component o at its other end with parity sgn[a] ^ f ^ sgn[b], unless
//             o chose the same slot and c < o.  The link is ONE 64-bit word (o << 1 | parity) in an array of its own:
//             comp / sgn are read by other hooking threads in the same launch and do not move.
//   jump      every root that hooked doubles its pointer in place, link[c] = link[link[c]] with the parities XOR-ed, until
//             its target is a root.  A word is written by its owner only and read whole, so whatever mix of old and new
//             words a thread sees names an ancestor with the right parity: no thread waits for another, each iteration
//             moves at least one hop (capped at n, SCAN_WALK_CAP), and threads running together finish a chain of length L
//             in about log2 L iterations.
//   apply     every point takes ONE step, comp[i] = link[comp[i]], and best[] is reset.  link[] is never reset: a word is
//             read only through a current root, and a root has never hooked.
//   tail      per tree the counts of both parities and the lowest index by integer atomics on the root's words (one
//             atomic per wave where a wave lies in one tree), then the majority rule, nl_out, flipped, tree, stats.
//
// The host launches ceil(log2(max(n, 2))) rounds: a component with an outgoing edge hooks or is hooked onto, so their
// number at least halves.  active[t] is raised by round t - 1's hook; a round whose word is 0 returns at once, so nothing
// is read back inside the loop.
#include <cmath>

#include "scan_dev.h"

namespace pbn {
namespace {

constexpr int ORIENT_EVENTS = 4;                  // around: edge codes | rounds | tail
constexpr int ORIENT_NONE = (int)0x80000000u;     // no j is 2^31 - 1, so ~j never reaches it
constexpr u64 ORIENT_EMPTY = ~0ull;               // best[]: no offer; link[]: a root
constexpr unsigned char ORIENT_NULL = 2;          // sgn[] of a null point
constexpr int ORIENT_MAX_ROUNDS = 32;

// mesh.hip's order_key: NaN last, -0 ties with +0
__device__ __forceinline__ unsigned order_key(float w) {
    if (w != w) return 0xffffffffu;
    unsigned b = __float_as_uint(w);
    if (w == 0.0f) b = 0u;
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

__device__ __forceinline__ bool null_normal(float x, float y, float z) {
    const bool finite = (__float_as_uint(x) & 0x7f800000u) != 0x7f800000u && (__float_as_uint(y) & 0x7f800000u) != 0x7f800000u &&
                        (__float_as_uint(z) & 0x7f800000u) != 0x7f800000u;
    return !finite || (x == 0.0f && y == 0.0f && z == 0.0f);
}

__device__ __forceinline__ u64 peek(const u64* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void poke(u64* p, u64 v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// ---- edge codes --------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TPB) void k_orient_codes(const float* __restrict__ nl, int n, const int* __restrict__ idx, int k,
                                                      long long n_slots, int* __restrict__ code, unsigned* __restrict__ wkey,
                                                      int* __restrict__ comp, unsigned char* __restrict__ sgn) {
    for (long long e = (long long)blockIdx.x * TPB + threadIdx.x; e < n_slots; e += (long long)gridDim.x * TPB) {
        const int i = (int)(e / k);
        const float xi = nl[3 * (size_t)i], yi = nl[3 * (size_t)i + 1], zi = nl[3 * (size_t)i + 2];
        const bool null_i = null_normal(xi, yi, zi);
        if (e == (long long)i * k) {
            comp[i] = i;
            sgn[i] = null_i ? ORIENT_NULL : 0;
        }
        const int j = idx[e];
        int c = ORIENT_NONE;
        unsigned wk = 0u;
        if (!null_i && (unsigned)j < (unsigned)n && j != i) {
            const float xj = nl[3 * (size_t)j], yj = nl[3 * (size_t)j + 1], zj = nl[3 * (size_t)j + 2];
            if (!null_normal(xj, yj, zj)) {
                const float d = (xi * xj + yi * yj) + zi * zj;
                wk = order_key(1.0f - fabsf(d));
                c = d < 0.0f ? ~j : j;
            }
        }
        code[e] = c;
        wkey[e] = wk;
    }
}

// ---- round: minimum outgoing edge per component --------------------------------------------------------------------
__device__ __forceinline__ void offer(u64* __restrict__ best, int c, u64 key) {
#ifndef PBN_ORIENT_NO_PEEK
    if (key >= peek(&best[c])) return;                                       // the word only falls: a stale read skips no winner
#endif
    atomicMin(&best[c], key);
}

__global__ __launch_bounds__(TPB) void k_orient_min(const int* __restrict__ code, const unsigned* __restrict__ wkey, int k,
                                                    long long n_slots, const int* __restrict__ comp,
                                                    const int* __restrict__ active, u64* __restrict__ best) {
    if (*active == 0) return;
    const long long padded = (n_slots + WAVE - 1) / WAVE * WAVE;             // whole waves reach the shuffles
    for (long long e = (long long)blockIdx.x * TPB + threadIdx.x; e < padded; e += (long long)gridDim.x * TPB) {
        u64 key = ORIENT_EMPTY;
        int ci = -1, cj = -1;
        if (e < n_slots) {
            ci = comp[(int)(e / k)];
            const int c = code[e];
            if (c != ORIENT_NONE) {
                cj = comp[c < 0 ? ~c : c];
                if (cj != ci) key = ((u64)wkey[e] << 32) | (u64)e;
            }
        }
        if (key != ORIENT_EMPTY) offer(best, cj, key);
#ifndef PBN_ORIENT_NO_WAVE_MIN
        // the minimum over the run of lanes from this one on that share ci; its first lane holds the whole run's
        const int lane = lane_id();
        const int prev = __shfl_up(ci, 1, 64);
#pragma unroll
        for (int o = 1; o < WAVE; o <<= 1) {
            const int oc = __shfl_down(ci, o, 64);
            const unsigned lo = (unsigned)__shfl_down((int)(unsigned)key, o, 64);
            const unsigned hi = (unsigned)__shfl_down((int)(unsigned)(key >> 32), o, 64);
            const u64 ok = ((u64)hi << 32) | lo;
            if (lane + o < WAVE && oc == ci && ok < key) key = ok;
        }
        if (key != ORIENT_EMPTY && (lane == 0 || prev != ci)) offer(best, ci, key);
#else
        if (key != ORIENT_EMPTY) offer(best, ci, key);
#endif
    }
}

// ---- round: hook -----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TPB) void k_orient_hook(const int* __restrict__ code, int k, int n, const int* __restrict__ comp,
                                                     const unsigned char* __restrict__ sgn, const u64* __restrict__ best,
                                                     u64* __restrict__ link, int* __restrict__ active) {
    if (active[0] == 0) return;
    int hooked = 0;
    for (long long c0 = (long long)blockIdx.x * TPB + threadIdx.x; c0 < n; c0 += (long long)gridDim.x * TPB) {
        const int c = (int)c0;
        const u64 key = best[c];                                             // written only through roots
        if (key == ORIENT_EMPTY) continue;
        const long long e = (long long)(key & 0xffffffffull);
        const int a = (int)(e / k);
        const int cd = code[e];
        const int b = cd < 0 ? ~cd : cd;
        const int f = cd < 0 ? 1 : 0;
        const int ca = comp[a], cb = comp[b];
        const int o = ca == c ? cb : ca;                                     // the edge was offered to both of its sides
        if (best[o] == key && c < o) continue;                               // a mutual choice: the lower root stays
        link[c] = ((u64)(unsigned)o << 1) | (u64)((sgn[a] ^ f ^ sgn[b]) & 1);
        hooked = 1;
    }
    if (__any(hooked) && lane_id() == 0) atomicOr(&active[1], 1);
}

// ---- round: compress -------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TPB) void k_orient_jump(int n, const int* __restrict__ comp, const int* __restrict__ active,
                                                     u64* __restrict__ link, int* __restrict__ status) {
    if (active[1] == 0) return;                                              // this round hooked nothing
    for (long long c0 = (long long)blockIdx.x * TPB + threadIdx.x; c0 < n; c0 += (long long)gridDim.x * TPB) {
        const int c = (int)c0;
        if (comp[c] != c) continue;                                          // only a root of this round can have hooked
        u64 mine = peek(&link[c]);
        if (mine == ORIENT_EMPTY) continue;
        int steps = 0;
        for (;;) {
            const u64 next = peek(&link[(int)(mine >> 1)]);
            if (next == ORIENT_EMPTY) break;
            mine = (next & ~1ull) | ((mine ^ next) & 1ull);
            poke(&link[c], mine);
            if (++steps >= n) { atomicOr(status, SCAN_WALK_CAP); break; }   // a forest's chain has fewer than n hops
        }
    }
}

__global__ __launch_bounds__(TPB) void k_orient_apply(int n, const int* __restrict__ active, const u64* __restrict__ link,
                                                      int* __restrict__ comp, unsigned char* __restrict__ sgn,
                                                      u64* __restrict__ best) {
    if (active[1] == 0) return;                                              // nothing was offered either: best is clean
    for (long long i0 = (long long)blockIdx.x * TPB + threadIdx.x; i0 < n; i0 += (long long)gridDim.x * TPB) {
        const int i = (int)i0;
        best[i] = ORIENT_EMPTY;
        const u64 l = link[comp[i]];
        if (l == ORIENT_EMPTY) continue;
        comp[i] = (int)(l >> 1);
        sgn[i] = (unsigned char)(sgn[i] ^ (unsigned char)(l & 1));           // a null point is its own root: never here
    }
}

// ---- tail --------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TPB) void k_orient_count(int n, const int* __restrict__ comp, const unsigned char* __restrict__ sgn,
                                                      int* __restrict__ members, int* __restrict__ ones,
                                                      unsigned* __restrict__ lowest) {
    const long long padded = ((long long)n + WAVE - 1) / WAVE * WAVE;         // whole waves reach the ballots
    for (long long i0 = (long long)blockIdx.x * TPB + threadIdx.x; i0 < padded; i0 += (long long)gridDim.x * TPB) {
        const int i = (int)i0;
        const bool live = i < n && sgn[i] != ORIENT_NULL;
        const int r = live ? comp[i] : -1;
        const int s = live ? (int)sgn[i] : 0;
        const u64 mask = __ballot(live);
        if (mask == 0) continue;
        const int first = __ffsll((long long)mask) - 1;
        const int r0 = __shfl(r, first, 64);
        if (__all(!live || r == r0)) {                                       // the wave lies in one tree: one lane speaks
            const int cnt = __popcll(mask), cnt1 = __popcll(__ballot(live && s));
            const int low = __shfl(i, first, 64);                            // lanes ascend with i
            if (lane_id() == first) {
                atomicAdd(&members[r0], cnt);
                if (cnt1) atomicAdd(&ones[r0], cnt1);
                atomicMin(&lowest[r0], (unsigned)low);
            }
        } else if (live) {
            atomicAdd(&members[r], 1);
            if (s) atomicAdd(&ones[r], 1);
            atomicMin(&lowest[r], (unsigned)i);
        }
    }
}

__global__ __launch_bounds__(TPB) void k_orient_write(const float* __restrict__ nl, int n, const int* __restrict__ comp,
                                                      const unsigned char* __restrict__ sgn, const int* __restrict__ members,
                                                      const int* __restrict__ ones, const unsigned* __restrict__ lowest,
                                                      const int* __restrict__ active, int n_rounds, float* __restrict__ nl_out,
                                                      unsigned char* __restrict__ flipped, int* __restrict__ tree,
                                                      int* __restrict__ stats, int* __restrict__ status) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        int worked = 0;
        for (int t = 1; t <= n_rounds; ++t) worked += active[t] != 0;
        status[1] = worked;                                                  // rounds that hooked something
    }
    const long long padded = ((long long)n + WAVE - 1) / WAVE * WAVE;
    for (long long i0 = (long long)blockIdx.x * TPB + threadIdx.x; i0 < padded; i0 += (long long)gridDim.x * TPB) {
        const int i = (int)i0;
        bool is_null = false, flip = false, head = false;
        if (i < n) {
            const unsigned char s = sgn[i];
            is_null = s == ORIENT_NULL;
            int low = i;
            if (!is_null) {
                const int r = comp[i];
                const int n1 = ones[r], n0 = members[r] - n1;
                low = (int)lowest[r];
                // keep the majority's sign; on a tie the tree's lowest point keeps its own
                const int invert = n1 > n0 || (n1 == n0 && (sgn[low] & 1));
                flip = ((s & 1) ^ invert) != 0;
                head = low == i;
            }
            const unsigned m = flip ? 0x80000000u : 0u;
#pragma unroll
            for (int a = 0; a < 3; ++a)
                nl_out[3 * (size_t)i + a] = __uint_as_float(__float_as_uint(nl[3 * (size_t)i + a]) ^ m);
            flipped[i] = flip ? 1 : 0;
            tree[i] = low;
        }
        const int n_heads = __popcll(__ballot(head)), n_flip = __popcll(__ballot(flip)), n_null = __popcll(__ballot(is_null));
        if (lane_id() == 0) {
            if (n_heads) atomicAdd(&stats[0], n_heads);
            if (n_flip) atomicAdd(&stats[1], n_flip);
            if (n_null) atomicAdd(&stats[2], n_null);
        }
    }
}

// ---- host --------------------------------------------------------------------------------------------------------------
struct OrientWs {
    int* code; unsigned* wkey; int* comp; unsigned char* sgn; u64* best; u64* link; int* members; int* ones; unsigned* lowest;
    int* active;
};

OrientWs orient_carve(Carver& cv, int n, int k) {
    OrientWs w{};
    const size_t N = (size_t)(n > 0 ? n : 1), E = N * (size_t)k;
    w.code = cv.take<int>(E); w.wkey = cv.take<unsigned>(E);
    w.comp = cv.take<int>(N); w.sgn = cv.take<unsigned char>(N);
    w.best = cv.take<u64>(N); w.link = cv.take<u64>(N);
    w.members = cv.take<int>(N); w.ones = cv.take<int>(N); w.lowest = cv.take<unsigned>(N);
    w.active = cv.take<int>(ORIENT_MAX_ROUNDS + 2);
    return w;
}

size_t orient_ws_bytes(int n, int k) {
    Carver cv(nullptr, 0);
    orient_carve(cv, n, k);
    return cv.off + 256;
}

bool orient_bad_sizes(int n, int k) {
    return n < 0 || k < 1 || k > SCAN_MAX_K || (long long)n * k > 0x7fffffffLL;
}

int orient_rounds(int n) {                                                   // ceil(log2(max(n, 2)))
    int r = 1;
    while (r < 31 && (1LL << r) < (long long)n) ++r;
    return r;
}

// ev (optional): ORIENT_EVENTS events
int orient_run(const float* nl, int n, const int32_t* idx, int k, float* nl_out, uint8_t* flipped, int32_t* tree, int32_t* stats,
               int32_t* status, void* workspace, size_t workspace_bytes, hipStream_t st, hipEvent_t* ev) {
    Carver cv(workspace, workspace_bytes);
    const OrientWs w = orient_carve(cv, n, k);
    if (!cv.ok) return PBN_ERR_WORKSPACE;
    const size_t N = (size_t)n;
    const FillRange fr[] = {{status, 2 * sizeof(int32_t), 0}, {stats, 4 * sizeof(int32_t), 0},
                            {w.active, sizeof(int), 1}, {w.active + 1, (ORIENT_MAX_ROUNDS + 1) * sizeof(int), 0},
                            {w.best, N * sizeof(u64), 0xff}, {w.link, N * sizeof(u64), 0xff},
                            {w.members, N * sizeof(int), 0}, {w.ones, N * sizeof(int), 0},
                            {w.lowest, N * sizeof(unsigned), 0xff}};
    int rc = fill_ranges(fr, n > 0 ? 9 : 2, st);
    if (rc != PBN_OK) return rc;
    if (ev) PBN_HIP_CHECK(hipEventRecord(ev[0], st));
    if (n == 0) {
        if (ev) for (int i = 1; i < ORIENT_EVENTS; ++i) PBN_HIP_CHECK(hipEventRecord(ev[i], st));
        return PBN_OK;
    }
    const long long n_slots = (long long)n * k;
    const int g_slots = grid_for(n_slots, 4096), g_points = grid_for(n, 2048);
    hipLaunchKernelGGL(k_orient_codes, dim3(g_slots), dim3(TPB), 0, st, nl, n, idx, k, n_slots, w.code, w.wkey, w.comp, w.sgn);
    PBN_LAUNCH_CHECK();
    if (ev) PBN_HIP_CHECK(hipEventRecord(ev[1], st));
    const int rounds = orient_rounds(n);
    for (int t = 0; t < rounds; ++t) {
        int* act = w.active + t;                                             // act[0]: this round runs; act[1]: it hooked
        hipLaunchKernelGGL(k_orient_min, dim3(g_slots), dim3(TPB), 0, st, w.code, w.wkey, k, n_slots, w.comp, act, w.best);
        hipLaunchKernelGGL(k_orient_hook, dim3(g_points), dim3(TPB), 0, st, w.code, k, n, w.comp, w.sgn, w.best, w.link, act);
        hipLaunchKernelGGL(k_orient_jump, dim3(g_points), dim3(TPB), 0, st, n, w.comp, act, w.link, status);
        hipLaunchKernelGGL(k_orient_apply, dim3(g_points), dim3(TPB), 0, st, n, act, w.link, w.comp, w.sgn, w.best);
    }
    PBN_LAUNCH_CHECK();
    if (ev) PBN_HIP_CHECK(hipEventRecord(ev[2], st));
    hipLaunchKernelGGL(k_orient_count, dim3(g_points), dim3(TPB), 0, st, n, w.comp, w.sgn, w.members, w.ones, w.lowest);
    hipLaunchKernelGGL(k_orient_write, dim3(g_points), dim3(TPB), 0, st, nl, n, w.comp, w.sgn, w.members, w.ones, w.lowest,
                       w.active, rounds, nl_out, flipped, tree, stats, status);
    PBN_LAUNCH_CHECK();
    if (ev) PBN_HIP_CHECK(hipEventRecord(ev[3], st));
    return PBN_OK;
}

int orient_args(const float* nl, int n, const int32_t* idx, int k, const float* nl_out, const uint8_t* flipped,
                const int32_t* tree, const int32_t* stats, const int32_t* status, const void* workspace, size_t workspace_bytes) {
    if (orient_bad_sizes(n, k)) return PBN_ERR_ARG;
    if ((n && (!nl || !idx || !nl_out || !flipped || !tree)) || !stats || !status || !workspace) return PBN_ERR_ARG;
    if (workspace_bytes < orient_ws_bytes(n, k)) return PBN_ERR_WORKSPACE;
    return PBN_OK;
}

}  // namespace
}  // namespace pbn

using namespace pbn;

extern "C" size_t pbn_cloud_orient_workspace_bytes(int n_points, int k) {
    if (orient_bad_sizes(n_points, k)) return 0;
    return orient_ws_bytes(n_points, k);
}

extern "C" int pbn_cloud_orient(const float* nl, int n_points, const int32_t* idx, int k, float* nl_out, uint8_t* flipped,
                                int32_t* tree, int32_t* stats, int32_t* status, void* workspace, size_t workspace_bytes,
                                pbn_stream_t stream) {
    const int rc = orient_args(nl, n_points, idx, k, nl_out, flipped, tree, stats, status, workspace, workspace_bytes);
    if (rc != PBN_OK) return rc;
    return orient_run(nl, n_points, idx, k, nl_out, flipped, tree, stats, status, workspace, workspace_bytes, (hipStream_t)stream,
                      nullptr);
}

extern "C" int pbn_cloud_orient_timed(const float* nl, int n_points, const int32_t* idx, int k, float* nl_out, uint8_t* flipped,
                                      int32_t* tree, int32_t* stats, int32_t* status, void* workspace, size_t workspace_bytes,
                                      pbn_stream_t stream, float* times_ms) {
    const int rc = orient_args(nl, n_points, idx, k, nl_out, flipped, tree, stats, status, workspace, workspace_bytes);
    if (rc != PBN_OK) return rc;
    if (!times_ms) return PBN_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    return timed_stages<ORIENT_EVENTS>(st, times_ms, [&](hipEvent_t* ev) {
        return orient_run(nl, n_points, idx, k, nl_out, flipped, tree, stats, status, workspace, workspace_bytes, st, ev);
    });
}
