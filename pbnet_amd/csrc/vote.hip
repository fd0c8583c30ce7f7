// vote.hip -- an annotated raw scan's labels voted down to the kept points: per kept row the most frequent
// (semantic, instance) pair among the raw points routed to it (thin.hip's inverse / raw index), then the surviving
// instance ids renumbered densely.  Integers only: exact, and two runs give the same bytes.  tests/vote_ref.py restates
// it in numpy.
//
// Codes.  s = sem < 0 ? n_classes : sem; q = ins < 0 ? 2^21 - 1 : ins (q = 0 for every point without `ins`): any negative
// label is "unannotated", a label like any other that orders LAST.  Vote key = s << 21 | q, 31 bits.  sem >= n_classes
// raises status bit 1, ins >= 2^21 - 1 bit 2, a row outside [-1, m) bit 4 (the outputs are then unspecified, never out
// of bounds: the offending code is clamped, the offending point votes nowhere).
//
// Order (row, key, index) by two stable radix_sort_u32 calls, least significant first: by vote key with row + 1 as the
// value, then by row + 1 with the vote key as the value.  Each sort carries the OTHER word as its value, so no per-point
// key array is kept and the second sort's pairs are a coalesced swap of the first's output, not a gather.  row + 1 == 0
// are the non-voters: the leading run.  Heads of the (row, key) runs are flagged, scan_exclusive_i32 numbers them, each
// run's start position is written densely.  Pick: one lane per run; the lane whose run is the first of its row walks the
// row's runs and keeps the longest under strict > -- keys ascend, so the first maximum is the lowest key.  The walk is as
// long as the number of distinct pairs in the row (a wave waits for its longest).  No atomics besides the status word
// and the digit histograms.
//
// Compaction.  The winners' instance ids are marked in a table over the id range by plain stores of 1, the table is
// scanned, out_ins is renumbered in place and old_id[new] = old is written: ascending old-id order.  result[0] = status,
// result[1] = I', one read-back.
#include "scan_dev.h"

namespace pbn {
namespace {

typedef long long i64;
constexpr int VOTE_MAX_CLASSES = 1023;
constexpr int VOTE_INS_BITS = 21;
constexpr int VOTE_INS_NONE = (1 << VOTE_INS_BITS) - 1;      // the code of an unannotated instance; ids are 0 .. 2^21 - 2
constexpr int VOTE_IDS = 1 << VOTE_INS_BITS;       // entries of the id table (the last one is never marked)
constexpr int VOTE_SEM_RANGE = 1, VOTE_INS_RANGE = 2, VOTE_ROW_RANGE = 4;      // status bits; the word is shared with SCAN_SORT_SPIN
constexpr i64 VOTE_NONE = -100;                    // the reference's ignore label

// Rows nobody votes for keep this: -100, -100, 0, 0.
__global__ __launch_bounds__(TPB) void k_vote_fill(int m, i64* __restrict__ out_sem, i64* __restrict__ out_ins,
                                                   int* __restrict__ votes, int* __restrict__ members) {
    for (int t = blockIdx.x * TPB + threadIdx.x; t < m; t += gridDim.x * TPB) {
        out_sem[t] = VOTE_NONE; out_ins[t] = VOTE_NONE; votes[t] = 0; members[t] = 0;
    }
}

// The first sort's pairs (vote key, row + 1) with the key's digit histograms, and the range checks.  Pairs are written
// whatever the status, so the sorts always see keys that match their histograms.  keys == nullptr: the checks alone.
__global__ __launch_bounds__(TPB) void k_vote_keys(const int* __restrict__ rows, const int* __restrict__ sem,
                                                   const int* __restrict__ ins, int n, int m, int n_classes,
                                                   int* __restrict__ status, u64* __restrict__ keys, int* __restrict__ vals,
                                                   unsigned* __restrict__ ghist) {
    __shared__ unsigned s_hist[RADIX_U32_PASSES][RADIX];
    hist_clear(s_hist);
    __syncthreads();
    int bad = 0;
    for (int i = blockIdx.x * TPB + threadIdx.x; i < n; i += gridDim.x * TPB) {
        int s = sem[i], q = ins ? ins[i] : 0, r = rows[i];
        if (s >= n_classes) bad |= VOTE_SEM_RANGE;
        if (s < 0 || s >= n_classes) s = n_classes;
        if (q >= VOTE_INS_NONE) bad |= VOTE_INS_RANGE;
        if (q < 0 || q >= VOTE_INS_NONE) q = VOTE_INS_NONE;
        if (r < -1 || r >= m) { bad |= VOTE_ROW_RANGE; r = -1; }
        if (keys) {
            const unsigned key = ((unsigned)s << VOTE_INS_BITS) | (unsigned)q;
            keys[i] = (u64)key;
            vals[i] = r + 1;
            hist_add(s_hist, key);
        }
    }
    if (bad) atomicOr(status, bad);
    __syncthreads();
    if (keys) hist_flush(s_hist, ghist);
}

// The second sort's pairs: (row + 1, vote key) in the order of the first sort, with the rows' digit histograms.
__global__ __launch_bounds__(TPB) void k_vote_rows(const u64* __restrict__ skey, const int* __restrict__ srow, int n,
                                                   u64* __restrict__ keys, int* __restrict__ vals, unsigned* __restrict__ ghist) {
    __shared__ unsigned s_hist[RADIX_U32_PASSES][RADIX];
    hist_clear(s_hist);
    __syncthreads();
    for (int s = blockIdx.x * TPB + threadIdx.x; s < n; s += gridDim.x * TPB) {
        const unsigned rp = (unsigned)srow[s];
        keys[s] = (u64)rp;
        vals[s] = (int)(unsigned)skey[s];
        hist_add(s_hist, rp);
    }
    __syncthreads();
    hist_flush(s_hist, ghist);
}

// rowp1 / key: the pairs in (row, key, index) order.  A voter's position is a head when its row or its key changes.
__global__ __launch_bounds__(TPB) void k_vote_heads(const u64* __restrict__ rowp1, const int* __restrict__ key, int n,
                                                    int* __restrict__ head) {
    for (int s = blockIdx.x * TPB + threadIdx.x; s < n; s += gridDim.x * TPB) {
        const u64 rp = rowp1[s];
        head[s] = (rp != 0ull && (s == 0 || rowp1[s - 1] != rp || key[s - 1] != key[s])) ? 1 : 0;
    }
}

// before[s] = heads in front of s = the number of the run that starts at a head
__global__ __launch_bounds__(TPB) void k_vote_starts(const int* __restrict__ head, const int* __restrict__ before, int n,
                                                     int* __restrict__ start) {
    for (int s = blockIdx.x * TPB + threadIdx.x; s < n; s += gridDim.x * TPB)
        if (head[s]) start[before[s]] = s;
}

// One lane per run; the lane on the first run of a row owns the row and walks its runs.
__global__ __launch_bounds__(TPB) void k_vote_pick(const u64* __restrict__ rowp1, const int* __restrict__ key, int n, int m,
                                                   int n_classes, const int* __restrict__ start, const int* __restrict__ n_runs,
                                                   i64* __restrict__ out_sem, i64* __restrict__ out_ins, int* __restrict__ votes,
                                                   int* __restrict__ members) {
    const int R = min(*n_runs, n);
    for (int r = blockIdx.x * TPB + threadIdx.x; r < R; r += gridDim.x * TPB) {
        const int s0 = start[r];
        const u64 rp = rowp1[s0];
        if (r > 0 && rowp1[start[r - 1]] == rp) continue;                    // not the first run of its row
        const int row = (int)rp - 1;
        if ((unsigned)row >= (unsigned)m) continue;                          // only after a failed sort (flagged)
        int best = 0, best_key = 0, total = 0, t = r, s = s0;
        do {
            const int e = t + 1 < R ? start[t + 1] : n;
            const int len = e - s;
            if (len > best) { best = len; best_key = key[s]; }
            total += len;
            ++t;
            s = e;
        } while (t < R && rowp1[s] == rp);
        const int cs = (int)((unsigned)best_key >> VOTE_INS_BITS), cq = best_key & VOTE_INS_NONE;
        out_sem[row] = cs >= n_classes ? VOTE_NONE : (i64)cs;
        out_ins[row] = cq == VOTE_INS_NONE ? VOTE_NONE : (i64)cq;
        votes[row] = best;
        members[row] = total;
    }
}

__global__ __launch_bounds__(TPB) void k_vote_mark(const i64* __restrict__ out_ins, int m, int* __restrict__ table) {
    for (int t = blockIdx.x * TPB + threadIdx.x; t < m; t += gridDim.x * TPB) {
        const i64 q = out_ins[t];
        if (q >= 0 && q < VOTE_INS_NONE) table[q] = 1;
    }
}

// newid = the exclusive scan of the table: the rows' ids renumbered, and old_id[new] = old for every marked id
__global__ __launch_bounds__(TPB) void k_vote_renumber(i64* __restrict__ out_ins, int m, const int* __restrict__ table,
                                                       const int* __restrict__ newid, int cap, i64* __restrict__ old_id) {
    const int lanes = gridDim.x * TPB, lane = blockIdx.x * TPB + threadIdx.x;
    for (int t = lane; t < m; t += lanes) {
        const i64 q = out_ins[t];
        if (q >= 0 && q < VOTE_INS_NONE) out_ins[t] = (i64)newid[q];
    }
    for (int id = lane; id < VOTE_IDS; id += lanes)
        if (table[id] && newid[id] < cap) old_id[newid[id]] = (i64)id;      // cap: at most m ids can have won a row
}

struct VoteWs {
    SortBufs sort;                                  // sort 0: by vote key, sort 1: by row + 1
    int* head; int* before; int* start; int* scan_tmp; int* table; int* newid; int* n_runs;
};

VoteWs vote_carve(Carver& cv, int n) {
    VoteWs w{};
    const size_t N = (size_t)(n > 0 ? n : 1);
    w.sort = sort_carve(cv, N, 2);
    w.head = cv.take<int>(N); w.before = cv.take<int>(N); w.start = cv.take<int>(N);
    w.scan_tmp = cv.take<int>(scan_tmp_ints((long long)(N > (size_t)VOTE_IDS ? N : (size_t)VOTE_IDS)));
    w.table = cv.take<int>(VOTE_IDS); w.newid = cv.take<int>(VOTE_IDS);
    w.n_runs = cv.take<int>(1);
    return w;
}

size_t vote_ws_bytes(int n) {
    Carver cv(nullptr, 0);
    vote_carve(cv, n);
    return cv.off + 256;
}

constexpr int VOTE_EVENTS = 7;      // around: zeroing + fill + keys | key sort | row pairs + row sort | heads + scan + starts | pick | compaction

int vote_args(const int32_t* rows, const int32_t* sem, int n_raw, int m, int n_classes, const int64_t* out_sem,
              const int64_t* out_ins, const int32_t* votes, const int32_t* members, const int32_t* result, const void* workspace,
              size_t workspace_bytes) {
    if (n_raw < 0 || n_raw > SCAN_MAX_POINTS || m < 0 || m > SCAN_MAX_POINTS || n_classes < 1 || n_classes > VOTE_MAX_CLASSES)
        return PBN_ERR_ARG;
    if ((n_raw && (!rows || !sem)) || (m && (!out_sem || !out_ins || !votes || !members)) || !result || !workspace)
        return PBN_ERR_ARG;
    if (workspace_bytes < vote_ws_bytes(n_raw)) return PBN_ERR_WORKSPACE;
    return PBN_OK;
}

int vote_labels(const int32_t* rows, const int32_t* sem, const int32_t* ins, int n, int m, int n_classes, i64* out_sem,
                i64* out_ins, int32_t* votes, int32_t* members, int32_t* result, i64* old_id, void* workspace,
                size_t workspace_bytes, hipStream_t st, hipEvent_t* ev) {
    Carver cv(workspace, workspace_bytes);
    const VoteWs w = vote_carve(cv, n);
    if (!cv.ok) return PBN_ERR_WORKSPACE;
    const bool sorts = n > 0 && m > 0, compact = sorts && old_id != nullptr;
    const FillRange fr[] = {{result, 2 * sizeof(int32_t), 0}, sort_hist_fill(w.sort, 0), sort_hist_fill(w.sort, 1),
                            {w.n_runs, sizeof(int), 0}, {w.table, (size_t)VOTE_IDS * sizeof(int), 0}};
    int at = 0;                                                              // the next event
    if (ev) PBN_HIP_CHECK(hipEventRecord(ev[at++], st));                     // the zeroing of the id table is timed too
    int rc = fill_ranges(fr, compact ? 5 : sorts ? 4 : 1, st);
    if (rc != PBN_OK) return rc;
    if (m > 0) {
        hipLaunchKernelGGL(k_vote_fill, dim3(grid_for(m)), dim3(TPB), 0, st, m, out_sem, out_ins, votes, members);
        PBN_LAUNCH_CHECK();
    }
    const dim3 grid(grid_for(n)), block(TPB);
    if (n > 0) {                                                             // m == 0: the range checks alone
        hipLaunchKernelGGL(k_vote_keys, grid, block, 0, st, rows, sem, ins, n, m, n_classes, result,
                           sorts ? w.sort.keys_a : (u64*)nullptr, w.sort.vals_a, w.sort.ghist[0]);
        PBN_LAUNCH_CHECK();
    }
    if (ev) PBN_HIP_CHECK(hipEventRecord(ev[at++], st));
    if (sorts) {
        rc = sort_run(w.sort, 0, n, result, st);
        if (rc != PBN_OK) return rc;
        if (ev) PBN_HIP_CHECK(hipEventRecord(ev[at++], st));
        hipLaunchKernelGGL(k_vote_rows, grid, block, 0, st, w.sort.keys_b, w.sort.vals_b, n, w.sort.keys_a, w.sort.vals_a,
                           w.sort.ghist[1]);
        PBN_LAUNCH_CHECK();
        rc = sort_run(w.sort, 1, n, result, st);
        if (rc != PBN_OK) return rc;
        if (ev) PBN_HIP_CHECK(hipEventRecord(ev[at++], st));
        hipLaunchKernelGGL(k_vote_heads, grid, block, 0, st, w.sort.keys_b, w.sort.vals_b, n, w.head);
        PBN_LAUNCH_CHECK();
        rc = scan_exclusive_i32(w.head, w.before, n, w.scan_tmp, w.n_runs, st);
        if (rc != PBN_OK) return rc;
        hipLaunchKernelGGL(k_vote_starts, grid, block, 0, st, w.head, w.before, n, w.start);
        PBN_LAUNCH_CHECK();
        if (ev) PBN_HIP_CHECK(hipEventRecord(ev[at++], st));
        hipLaunchKernelGGL(k_vote_pick, grid, block, 0, st, w.sort.keys_b, w.sort.vals_b, n, m, n_classes, w.start, w.n_runs,
                           out_sem, out_ins, votes, members);
        PBN_LAUNCH_CHECK();
        if (ev) PBN_HIP_CHECK(hipEventRecord(ev[at++], st));
    }
    if (compact) {
        hipLaunchKernelGGL(k_vote_mark, dim3(grid_for(m)), block, 0, st, out_ins, m, w.table);
        PBN_LAUNCH_CHECK();
        rc = scan_exclusive_i32(w.table, w.newid, VOTE_IDS, w.scan_tmp, result + 1, st);
        if (rc != PBN_OK) return rc;
        hipLaunchKernelGGL(k_vote_renumber, dim3(grid_for(VOTE_IDS)), block, 0, st, out_ins, m, w.table, w.newid, m, old_id);
        PBN_LAUNCH_CHECK();
    }
    if (ev) while (at < VOTE_EVENTS) PBN_HIP_CHECK(hipEventRecord(ev[at++], st));
    return PBN_OK;
}

}  // namespace
}  // namespace pbn

using namespace pbn;

extern "C" size_t pbn_cloud_vote_workspace_bytes(int n_raw, int m) {
    if (n_raw < 0 || n_raw > SCAN_MAX_POINTS || m < 0 || m > SCAN_MAX_POINTS) return 0;
    return vote_ws_bytes(n_raw);
}

extern "C" int pbn_cloud_vote_labels(const int32_t* rows, const int32_t* sem, const int32_t* ins, int n_raw, int m, int n_classes,
                                     int64_t* out_sem, int64_t* out_ins, int32_t* votes, int32_t* members, int32_t* result,
                                     int64_t* old_id, void* workspace, size_t workspace_bytes, pbn_stream_t stream) {
    const int rc = vote_args(rows, sem, n_raw, m, n_classes, out_sem, out_ins, votes, members, result, workspace, workspace_bytes);
    if (rc != PBN_OK) return rc;
    return vote_labels(rows, sem, ins, n_raw, m, n_classes, (i64*)out_sem, (i64*)out_ins, votes, members, result, (i64*)old_id,
                       workspace, workspace_bytes, (hipStream_t)stream, nullptr);
}

extern "C" int pbn_cloud_vote_labels_timed(const int32_t* rows, const int32_t* sem, const int32_t* ins, int n_raw, int m,
                                           int n_classes, int64_t* out_sem, int64_t* out_ins, int32_t* votes, int32_t* members,
                                           int32_t* result, int64_t* old_id, void* workspace, size_t workspace_bytes,
                                           pbn_stream_t stream, float* times_ms) {
    const int rc = vote_args(rows, sem, n_raw, m, n_classes, out_sem, out_ins, votes, members, result, workspace, workspace_bytes);
    if (rc != PBN_OK) return rc;
    if (!times_ms) return PBN_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    return timed_stages<VOTE_EVENTS>(st, times_ms, [&](hipEvent_t* ev) {
        return vote_labels(rows, sem, ins, n_raw, m, n_classes, (i64*)out_sem, (i64*)out_ins, votes, members, result, (i64*)old_id,
                           workspace, workspace_bytes, st, ev);
    });
}
