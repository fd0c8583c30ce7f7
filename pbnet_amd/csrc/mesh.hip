// mesh.hip -- decode of a raw mesh on the device: the vertex normals of datasets/scannetv2/decode_scannet.py:76-96
// (face_normal + vertex_normal) and the superpoints of lib/segmentator (csrc/segmentator.cpp, Felzenszwalb graph
// segmentation of the mesh, plus main.py:17's torch.unique relabel).
//
//   incidence  faces -> int32 (indices checked against [0, V)), occurrences counted per vertex, scanned, filled, and each
//              vertex's short list sorted by (face, slot): the face order of both references, with no float atomics;
//   normals    per face the cross product as numpy / segmentator.cpp compute it (each product rounded, then subtracted);
//              per vertex (a) numpy's sum of nf * area over the DISTINCT incident faces (nv[face[i]] += nf[i] adds once per
//              face), normalised, and (b) segmentator.cpp:195-198's running lerp, once per occurrence;
//   weights    3F edges (i1,i2), (i1,i3), (i3,i2) per face (segmentator.cpp:186-192), or the caller's edges
//              (segment_point), w as segmentator.cpp:204-229 computes it, NaN kept;
//   sort       sort.hip's LSD radix sort on (order-preserving u32 of w, edge index): a total, stable order, NaN last;
//   sweep      segment_graph + the small-segment join in host C++ over ONE read-back of the sorted (a, b, w), with the
//              reference's universe (union by rank, sizes, one-step path compression), so roots -- not only partitions --
//              come out as the reference's for the same edge order;
//   relabel    sup[v] = rank of root(v) among the roots (= torch.unique(index, return_inverse=True)[1]).
//
// Arithmetic contract: float32, operation by operation in the references' order; built with -ffp-contract=off (no FMA),
// no fast-math.  sqrtf and '/' are correctly rounded here: hipcc's default for HIP is
// -fhip-fp32-correctly-rounded-divide-sqrt, and the gfx950 disassembly of this file was checked for it -- every float
// division is the v_div_scale / v_div_fmas / v_div_fixup_f32 sequence (no bare v_rcp_f32), and every sqrtf is the scaled
// v_sqrt_f32 with the two-sided residual correction that LLVM emits for a correctly rounded llvm.sqrt.f32.  The
// tests compare nl bit for bit against numpy (tests/test_mesh_gpu.py).
#include <chrono>
#include <cmath>
#include <vector>

#include "scan_dev.h"

namespace pbn {
namespace {

constexpr int MESH_BAD_INDEX = 1;                 // status bit: an index outside [0, V); shares the word with SCAN_SORT_SPIN
constexpr int MESH_GRID = 4096;                   // cap of the striding grids (k_edge_weights keeps grid_for's 1024)

enum { MODE_NORMALS = 0, MODE_SEGMENT = 1, MODE_POINT = 2 };

__device__ __forceinline__ float3 ld3(const float* __restrict__ p, int i) {
    return make_float3(p[3 * (size_t)i], p[3 * (size_t)i + 1], p[3 * (size_t)i + 2]);
}
__device__ __forceinline__ void st3(float* __restrict__ p, int i, float3 v) {
    p[3 * (size_t)i] = v.x; p[3 * (size_t)i + 1] = v.y; p[3 * (size_t)i + 2] = v.z;
}

// ---- incidence ---------------------------------------------------------------------------------------------------------
// idx -> int32 (-1 where out of range, flagged); mesh mode also counts each occurrence on its vertex
__global__ __launch_bounds__(TPB) void k_mesh_index(const void* __restrict__ idx, int i64, long long n_idx, int n_vertices,
                                                    int* __restrict__ idx32, int* __restrict__ cnt, int* __restrict__ status) {
    for (long long i = blockIdx.x * (long long)TPB + threadIdx.x; i < n_idx; i += (long long)gridDim.x * TPB) {
        const long long v = load_index(idx, i64, i);
        if (v < 0 || v >= n_vertices) {
            atomicOr(status, MESH_BAD_INDEX);
            idx32[i] = -1;
        } else {
            idx32[i] = (int)v;
            if (cnt) atomicAdd(&cnt[v], 1);
        }
    }
}

// entry 3f + slot at off[v] + (arrival order); sorted per vertex by k_vertex
__global__ __launch_bounds__(TPB) void k_mesh_fill(const int* __restrict__ f32, long long n_idx, const int* __restrict__ off,
                                                   int* __restrict__ cur, int* __restrict__ inc) {
    for (long long i = blockIdx.x * (long long)TPB + threadIdx.x; i < n_idx; i += (long long)gridDim.x * TPB) {
        const int v = f32[i];
        if (v < 0) continue;
        inc[off[v] + atomicAdd(&cur[v], 1)] = (int)i;
    }
}

// ---- normals -----------------------------------------------------------------------------------------------------------
// nfa = numpy's nf * area (decode_scannet.py:77-88); snf = segmentator.cpp:135-143's normalised cross product
__global__ __launch_bounds__(TPB) void k_face_normals(const float* __restrict__ xyz, const int* __restrict__ f32, int n_faces,
                                                      float* __restrict__ nfa, float* __restrict__ snf) {
    for (int f = blockIdx.x * TPB + threadIdx.x; f < n_faces; f += gridDim.x * TPB) {
        const int i0 = f32[3 * (size_t)f], i1 = f32[3 * (size_t)f + 1], i2 = f32[3 * (size_t)f + 2];
        if (i0 < 0 || i1 < 0 || i2 < 0) {       // flagged: the call fails; nothing is read out of range
            st3(nfa, f, make_float3(0.f, 0.f, 0.f));
            if (snf) st3(snf, f, make_float3(0.f, 0.f, 0.f));
            continue;
        }
        const float3 p0 = ld3(xyz, i0), p1 = ld3(xyz, i1), p2 = ld3(xyz, i2);
        const float ax = p1.x - p0.x, ay = p1.y - p0.y, az = p1.z - p0.z;     // v01 (segmentator: p2 - p1)
        const float bx = p2.x - p0.x, by = p2.y - p0.y, bz = p2.z - p0.z;     // v02 (segmentator: p3 - p1)
        // np.cross: cp0 = a1*b2 - a2*b1, cp1 = a2*b0 - a0*b2, cp2 = a0*b1 - a1*b0 (products rounded, then subtracted);
        // segmentator.cpp:137 writes the same expressions
        const float cx = ay * bz - az * by, cy = az * bx - ax * bz, cz = ax * by - ay * bx;
        const float ss = (cx * cx + cy * cy) + cz * cz;                      // np.sum(vec ** 2, axis=1): ((x2 + y2) + z2)
        const float len = sqrtf(ss) + 1.0e-8f;
        const float area = len * 0.5f;
        st3(nfa, f, make_float3((cx / len) * area, (cy / len) * area, (cz / len) * area));
        if (snf) {
            const float n = sqrtf(ss);                                       // c.x*c.x + c.y*c.y + c.z*c.z, same order
            st3(snf, f, make_float3(cx / n, cy / n, cz / n));
        }
    }
}

// per vertex: sort its incidence list, then (a) numpy's normal -> nl, (b) the segmentator's lerp -> sn
__global__ __launch_bounds__(TPB) void k_vertex_normals(const int* __restrict__ off, int* __restrict__ inc, int n_vertices,
                                                        const float* __restrict__ nfa, const float* __restrict__ snf,
                                                        float* __restrict__ nl, float* __restrict__ sn) {
    for (int v = blockIdx.x * TPB + threadIdx.x; v < n_vertices; v += gridDim.x * TPB) {
        const int lo = off[v], hi = off[v + 1];
        for (int i = lo + 1; i < hi; ++i) {                                  // insertion sort: a handful of entries
            const int e = inc[i];
            int j = i - 1;
            while (j >= lo && inc[j] > e) { inc[j + 1] = inc[j]; --j; }
            inc[j + 1] = e;
        }
        if (nl) {
            float sx = 0.0f, sy = 0.0f, sz = 0.0f;
            int prev = -1;
            for (int i = lo; i < hi; ++i) {
                const int f = inc[i] / 3;
                if (f == prev) continue;                                     // a face naming v twice adds once
                prev = f;
                const float3 a = ld3(nfa, f);
                sx = sx + a.x; sy = sy + a.y; sz = sz + a.z;
            }
            const float len = sqrtf((sx * sx + sy * sy) + sz * sz) + 1.0e-8f;
            st3(nl, v, make_float3(sx / len, sy / len, sz / len));
        }
        if (sn) {
            float nx = 0.0f, ny = 0.0f, nz = 0.0f;
            int count = 0;
            for (int i = lo; i < hi;) {
                const int f = inc[i] / 3;
                int k = i;
                const float t = 1.0f / ((float)count + 1.0f);                 // counts[i] grows after the face's three lerps
                const float u = 1.0f - t;
                const float3 b = ld3(snf, f);
                for (; k < hi && inc[k] / 3 == f; ++k) {                     // one lerp per occurrence
                    nx = t * b.x + u * nx; ny = t * b.y + u * ny; nz = t * b.z + u * nz;
                }
                count += k - i;
                i = k;
            }
            st3(sn, v, make_float3(nx, ny, nz));
        }
    }
}

// ---- weights -----------------------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned order_key(float w) {
    if (w != w) return 0xffffffffu;                                          // NaN: last
    unsigned b = __float_as_uint(w);
    if (w == 0.0f) b = 0u;                                                   // -0 ties with +0, as std::sort sees it
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

__device__ __forceinline__ void edge_ends(const int* __restrict__ idx32, int mode, int e, int& a, int& b) {
    if (mode == MODE_POINT) {
        a = idx32[2 * (size_t)e]; b = idx32[2 * (size_t)e + 1];
    } else {
        const int f = e / 3, k = e - 3 * f;
        const int i1 = idx32[3 * (size_t)f], i2 = idx32[3 * (size_t)f + 1], i3 = idx32[3 * (size_t)f + 2];
        a = k == 2 ? i3 : i1;
        b = k == 0 ? i2 : k == 1 ? i3 : i2;
    }
}

__global__ __launch_bounds__(TPB) void k_edge_weights(const float* __restrict__ xyz, const float* __restrict__ nrm,
                                                      const int* __restrict__ idx32, int mode, int n_edges,
                                                      float* __restrict__ w_out, u64* __restrict__ keys,
                                                      int* __restrict__ vals, unsigned* __restrict__ ghist) {
    __shared__ unsigned s_hist[RADIX_U32_PASSES][RADIX];
    hist_clear(s_hist);
    __syncthreads();
    for (int e = blockIdx.x * TPB + threadIdx.x; e < n_edges; e += gridDim.x * TPB) {
        int a, b;
        edge_ends(idx32, mode, e, a, b);
        float ww = __uint_as_float(0x7fc00000u);
        if (a >= 0 && b >= 0) {
            const float3 n1 = ld3(nrm, a), n2 = ld3(nrm, b), p1 = ld3(xyz, a), p2 = ld3(xyz, b);
            float dx = p2.x - p1.x, dy = p2.y - p1.y, dz = p2.z - p1.z;
            const float dd = sqrtf((dx * dx + dy * dy) + dz * dz);
            dx = dx / dd; dy = dy / dd; dz = dz / dd;
            const float dot = (n1.x * n2.x + n1.y * n2.y) + n1.z * n2.z;
            const float dot2 = (n2.x * dx + n2.y * dy) + n2.z * dz;
            ww = 1.0f - dot;
            if (dot2 > 0) ww = ww * ww;                                      // NaN dot2 (dd = 0): not squared
        }
        w_out[e] = ww;
        const unsigned key = order_key(ww);
        keys[e] = (u64)key;
        vals[e] = e;
        hist_add(s_hist, key);
    }
    __syncthreads();
    hist_flush(s_hist, ghist);
}

// sorted edge i -> (a, b, w) in the read-back block (int32 a[E], int32 b[E], float w[E])
__global__ __launch_bounds__(TPB) void k_edge_gather(const int* __restrict__ order, const int* __restrict__ idx32, int mode,
                                                     int n_edges, const float* __restrict__ w, int* __restrict__ out) {
    for (int i = blockIdx.x * TPB + threadIdx.x; i < n_edges; i += gridDim.x * TPB) {
        int e = order[i];
        if ((unsigned)e >= (unsigned)n_edges) e = 0;                         // only after a failed sort (flagged): stay in bounds
        int a, b;
        edge_ends(idx32, mode, e, a, b);
        out[i] = a;
        out[(size_t)n_edges + i] = b;
        reinterpret_cast<float*>(out)[2 * (size_t)n_edges + i] = w[e];
    }
}

// ---- relabel -----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TPB) void k_root_flags(const int* __restrict__ root, int n, int* __restrict__ flag) {
    for (int v = blockIdx.x * TPB + threadIdx.x; v < n; v += gridDim.x * TPB) flag[v] = root[v] == v ? 1 : 0;
}
__global__ __launch_bounds__(TPB) void k_root_rank(const int* __restrict__ root, const int* __restrict__ rank, int n,
                                                   int64_t* __restrict__ sup) {
    for (int v = blockIdx.x * TPB + threadIdx.x; v < n; v += gridDim.x * TPB) sup[v] = (int64_t)rank[root[v]];
}

// ---- host: the reference's disjoint-set forest and sweep (segmentator.cpp:21-107, 234-243) ---------------------------
struct Universe {
    struct Elt { int rank, p, size; };
    std::vector<Elt> elts;
    explicit Universe(int n) : elts((size_t)n) {
        for (int i = 0; i < n; ++i) elts[(size_t)i] = Elt{0, i, 1};
    }
    int find(int x) {
        int y = x;
        while (y != elts[(size_t)y].p) y = elts[(size_t)y].p;
        elts[(size_t)x].p = y;
        return y;
    }
    void join(int x, int y) {
        if (elts[(size_t)x].rank > elts[(size_t)y].rank) {
            elts[(size_t)y].p = x;
            elts[(size_t)x].size += elts[(size_t)y].size;
        } else {
            elts[(size_t)x].p = y;
            elts[(size_t)y].size += elts[(size_t)x].size;
            if (elts[(size_t)x].rank == elts[(size_t)y].rank) elts[(size_t)y].rank++;
        }
    }
    int size(int x) const { return elts[(size_t)x].size; }
};

void sweep(int n_vertices, int n_edges, const int* ea, const int* eb, const float* ew, float c, int min_size, int* root) {
    Universe u(n_vertices);
    std::vector<float> threshold((size_t)n_vertices, c);
    for (int i = 0; i < n_edges; ++i) {
        int a = u.find(ea[i]);
        const int b = u.find(eb[i]);
        if (a != b && ew[i] <= threshold[(size_t)a] && ew[i] <= threshold[(size_t)b]) {
            u.join(a, b);
            a = u.find(a);
            threshold[(size_t)a] = ew[i] + (c / u.size(a));
        }
    }
    for (int j = 0; j < n_edges; ++j) {
        const int a = u.find(ea[j]);
        const int b = u.find(eb[j]);
        if (a != b && (u.size(a) < min_size || u.size(b) < min_size)) u.join(a, b);
    }
    for (int q = 0; q < n_vertices; ++q) root[q] = u.find(q);
}

// ---- workspace -------------------------------------------------------------------------------------------------------
struct MeshWs {
    int* status; int* idx32; int* cnt; int* cur; int* off; int* scan_tmp; int* inc; float* nfa; float* snf; float* sn;
    float* w; SortBufs sort; int* readback; int* root; int* rank;
};

// n_elems: faces (mesh modes) or edges (MODE_POINT)
MeshWs carve(Carver& cv, int mode, int n_vertices, int n_elems) {
    MeshWs w{};
    const size_t V = (size_t)(n_vertices > 0 ? n_vertices : 1);
    const size_t F = mode == MODE_POINT ? 0 : (size_t)n_elems;
    const size_t E = mode == MODE_POINT ? (size_t)n_elems : 3 * (size_t)n_elems;
    const size_t n_idx = mode == MODE_POINT ? 2 * E : 3 * F;
    w.status = cv.take<int>(64);
    w.idx32 = cv.take<int>(n_idx ? n_idx : 1);
    if (mode != MODE_POINT) {
        w.cnt = cv.take<int>(V);
        w.cur = cv.take<int>(V);
        w.off = cv.take<int>(V + 1);
        w.inc = cv.take<int>(3 * F + 1);
        w.nfa = cv.take<float>(3 * F + 1);
        if (mode == MODE_SEGMENT) {
            w.snf = cv.take<float>(3 * F + 1);
            w.sn = cv.take<float>(3 * V);
        }
    }
    w.scan_tmp = cv.take<int>(scan_tmp_ints((long long)V + 1));
    if (mode != MODE_NORMALS) {
        const size_t EE = E ? E : 1;
        w.w = cv.take<float>(EE);
        w.sort = sort_carve(cv, EE, 1);
        w.readback = cv.take<int>(3 * EE);
        w.root = cv.take<int>(V);
        w.rank = cv.take<int>(V + 1);
    }
    return w;
}

size_t ws_bytes(int mode, int n_vertices, int n_elems) {
    Carver cv(nullptr, 0);
    carve(cv, mode, n_vertices, n_elems);
    return cv.off + 256;
}

bool bad_sizes(int mode, int n_vertices, int n_elems) {
    if (n_vertices < 0 || n_elems < 0) return true;
    return mode == MODE_POINT ? n_elems > (1 << 30) - 1 : n_elems > ((1 << 30) - 1) / 3;
}

// incidence + normals of a mesh (modes NORMALS / SEGMENT); status / idx32 / lists ready on return (async)
int mesh_normals(const MeshWs& w, const float* xyz, int V, const void* faces, int i64, int F, float* nl, hipStream_t st,
                 hipEvent_t* ev) {
    const long long n_idx = 3LL * F;
    const FillRange fr[] = {{w.status, 64 * sizeof(int), 0}, {w.cnt, (size_t)(V > 0 ? V : 1) * sizeof(int), 0},
                            {w.cur, (size_t)(V > 0 ? V : 1) * sizeof(int), 0}};
    int rc = fill_ranges(fr, 3, st);
    if (rc != PBN_OK) return rc;
    if (n_idx) hipLaunchKernelGGL(k_mesh_index, dim3(grid_for(n_idx, MESH_GRID)), dim3(TPB), 0, st, faces, i64, n_idx, V, w.idx32, w.cnt,
                                  w.status);
    rc = scan_exclusive_i32(w.cnt, w.off, V, w.scan_tmp, w.off + V, st);
    if (rc != PBN_OK) return rc;
    if (n_idx) hipLaunchKernelGGL(k_mesh_fill, dim3(grid_for(n_idx, MESH_GRID)), dim3(TPB), 0, st, w.idx32, n_idx, w.off, w.cur, w.inc);
    if (ev) PBN_HIP_CHECK(hipEventRecord(ev[1], st));
    if (F) hipLaunchKernelGGL(k_face_normals, dim3(grid_for(F, MESH_GRID)), dim3(TPB), 0, st, xyz, w.idx32, F, w.nfa, w.snf);
    if (V) hipLaunchKernelGGL(k_vertex_normals, dim3(grid_for(V, MESH_GRID)), dim3(TPB), 0, st, w.off, w.inc, V, w.nfa, w.snf, nl, w.sn);
    if (ev) PBN_HIP_CHECK(hipEventRecord(ev[2], st));
    PBN_LAUNCH_CHECK();
    return PBN_OK;
}

// weights, sort, read-back, host sweep, relabel (modes SEGMENT / POINT); synchronises the stream
int mesh_segment(const MeshWs& w, int mode, const float* xyz, const float* nrm, int V, int E, float c, int min_size,
                 int64_t* sup, hipStream_t st, hipEvent_t* ev, float* times_ms) {
    if (E) {
        const FillRange fr = sort_hist_fill(w.sort, 0);
        const int frc = fill_ranges(&fr, 1, st);
        if (frc != PBN_OK) return frc;
        hipLaunchKernelGGL(k_edge_weights, dim3(grid_for(E)), dim3(TPB), 0, st, xyz, nrm, w.idx32, mode, E, w.w, w.sort.keys_a,
                           w.sort.vals_a, w.sort.ghist[0]);
        PBN_LAUNCH_CHECK();
    }
    if (ev) PBN_HIP_CHECK(hipEventRecord(ev[3], st));
    int rc = sort_run(w.sort, 0, E, w.status, st);
    if (rc != PBN_OK) return rc;
    if (ev) PBN_HIP_CHECK(hipEventRecord(ev[4], st));
    if (E) hipLaunchKernelGGL(k_edge_gather, dim3(grid_for(E, MESH_GRID)), dim3(TPB), 0, st, w.sort.vals_b, w.idx32, mode, E, w.w,
                              w.readback);
    PBN_LAUNCH_CHECK();
    std::vector<int> host(3 * (size_t)E + 1);
    int status = 0;
    PBN_HIP_CHECK(hipMemcpyAsync(&status, w.status, sizeof(int), hipMemcpyDeviceToHost, st));
    if (E) PBN_HIP_CHECK(hipMemcpyAsync(host.data(), w.readback, 3 * (size_t)E * sizeof(int), hipMemcpyDeviceToHost, st));
    if (ev) PBN_HIP_CHECK(hipEventRecord(ev[5], st));
    PBN_HIP_CHECK(hipStreamSynchronize(st));
    if (status & MESH_BAD_INDEX) return PBN_ERR_RANGE;
    if (status & SCAN_SORT_SPIN) return PBN_ERR_HIP;
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<int> root((size_t)(V > 0 ? V : 1));
    sweep(V, E, host.data(), host.data() + E, reinterpret_cast<const float*>(host.data() + 2 * (size_t)E), c, min_size,
          root.data());
    const auto t1 = std::chrono::steady_clock::now();
    if (ev) PBN_HIP_CHECK(hipEventRecord(ev[6], st));
    if (V) {
        PBN_HIP_CHECK(hipMemcpyAsync(w.root, root.data(), (size_t)V * sizeof(int), hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(k_root_flags, dim3(grid_for(V, MESH_GRID)), dim3(TPB), 0, st, w.root, V, w.rank);
        rc = scan_exclusive_i32(w.rank, w.rank, V, w.scan_tmp, nullptr, st);
        if (rc != PBN_OK) return rc;
        hipLaunchKernelGGL(k_root_rank, dim3(grid_for(V, MESH_GRID)), dim3(TPB), 0, st, w.root, w.rank, V, sup);
        PBN_LAUNCH_CHECK();
    }
    if (ev) PBN_HIP_CHECK(hipEventRecord(ev[7], st));
    PBN_HIP_CHECK(hipStreamSynchronize(st));       // the host copy of the roots must outlive the upload
    if (ev && times_ms) {
        for (int i = 0; i < 7; ++i) {
            if (i == 5) continue;
            float ms = 0.f;
            PBN_HIP_CHECK(hipEventElapsedTime(&ms, ev[i], ev[i + 1]));
            times_ms[i] = ms;
        }
        times_ms[5] = std::chrono::duration<float, std::milli>(t1 - t0).count();
    }
    return PBN_OK;
}

}  // namespace
}  // namespace pbn

using namespace pbn;

extern "C" size_t pbn_mesh_workspace_bytes(int mode, int n_vertices, int n_elems) {
    if (mode < MODE_NORMALS || mode > MODE_POINT || bad_sizes(mode, n_vertices, n_elems)) return 0;
    return ws_bytes(mode, n_vertices, n_elems);
}

extern "C" int pbn_mesh_vertex_normals(const float* xyz, int n_vertices, const void* faces, int faces_i64, int n_faces,
                                       float* nl, int32_t* status, void* workspace, size_t workspace_bytes, pbn_stream_t stream) {
    if (bad_sizes(MODE_NORMALS, n_vertices, n_faces)) return PBN_ERR_ARG;
    if ((n_vertices && (!xyz || !nl)) || (n_faces && !faces) || !status || !workspace) return PBN_ERR_ARG;
    if (workspace_bytes < ws_bytes(MODE_NORMALS, n_vertices, n_faces)) return PBN_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    Carver cv(workspace, workspace_bytes);
    const MeshWs w = carve(cv, MODE_NORMALS, n_vertices, n_faces);
    if (!cv.ok) return PBN_ERR_WORKSPACE;
    const int rc = mesh_normals(w, xyz, n_vertices, faces, faces_i64, n_faces, nl, st, nullptr);
    if (rc != PBN_OK) return rc;
    PBN_HIP_CHECK(hipMemcpyAsync(status, w.status, sizeof(int32_t), hipMemcpyDeviceToDevice, st));
    return PBN_OK;
}

extern "C" int pbn_mesh_segment(const float* xyz, int n_vertices, const void* faces, int faces_i64, int n_faces, float k_thresh,
                                int seg_min_verts, int64_t* sup, float* nl, void* workspace, size_t workspace_bytes,
                                float* times_ms, pbn_stream_t stream) {
    if (bad_sizes(MODE_SEGMENT, n_vertices, n_faces)) return PBN_ERR_ARG;
    if ((n_vertices && (!xyz || !sup)) || (n_faces && !faces) || !workspace) return PBN_ERR_ARG;
    if (workspace_bytes < ws_bytes(MODE_SEGMENT, n_vertices, n_faces)) return PBN_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    Carver cv(workspace, workspace_bytes);
    const MeshWs w = carve(cv, MODE_SEGMENT, n_vertices, n_faces);
    if (!cv.ok) return PBN_ERR_WORKSPACE;
    StageEvents<8> evs;
    if (times_ms) {
        PBN_HIP_CHECK(evs.make());
        PBN_HIP_CHECK(hipEventRecord(evs.ev[0], st));
    }
    hipEvent_t* ev = times_ms ? evs.ev : nullptr;
    const int rc = mesh_normals(w, xyz, n_vertices, faces, faces_i64, n_faces, nl, st, ev);
    if (rc != PBN_OK) return rc;
    return mesh_segment(w, MODE_SEGMENT, xyz, w.sn, n_vertices, 3 * n_faces, k_thresh, seg_min_verts, sup, st, ev, times_ms);
}

extern "C" int pbn_mesh_segment_point(const float* xyz, const float* normals, int n_points, const void* edges, int edges_i64,
                                      int n_edges, float k_thresh, int seg_min_verts, int64_t* sup, void* workspace,
                                      size_t workspace_bytes, pbn_stream_t stream) {
    if (bad_sizes(MODE_POINT, n_points, n_edges)) return PBN_ERR_ARG;
    if ((n_points && (!xyz || !normals || !sup)) || (n_edges && !edges) || !workspace) return PBN_ERR_ARG;
    if (workspace_bytes < ws_bytes(MODE_POINT, n_points, n_edges)) return PBN_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    Carver cv(workspace, workspace_bytes);
    const MeshWs w = carve(cv, MODE_POINT, n_points, n_edges);
    if (!cv.ok) return PBN_ERR_WORKSPACE;
    const int rc = fill_bytes(w.status, 0, 64 * sizeof(int), st);
    if (rc != PBN_OK) return rc;
    const long long n_idx = 2LL * n_edges;
    if (n_idx) hipLaunchKernelGGL(k_mesh_index, dim3(grid_for(n_idx, MESH_GRID)), dim3(TPB), 0, st, edges, edges_i64, n_idx, n_points,
                                  w.idx32, (int*)nullptr, w.status);
    PBN_LAUNCH_CHECK();
    return mesh_segment(w, MODE_POINT, xyz, normals, n_points, n_edges, k_thresh, seg_min_verts, sup, st, nullptr, nullptr);
}
