// apeval.hip -- the AP table of an epoch on the device: tools/eval.py:27-190 (`evaluate_matches`, the host form is
// evaluate.evaluate_matches) run on the association logs where they lie (assoc_dev.h: the record layout).  Three steps per log
// (pbn_ap_table_add_log): a directory of the log's records by one wave, one row of derived counts per prediction, and the greedy
// matching by one wave per (record, overlap), which emits (cell, score, true) entries into one table; then per epoch
// (pbn_ap_table_finish) the entries are segmented by cell and one workgroup per cell sorts its segment and integrates the
// precision/recall curve in float64.  Capacities come from the host, every count stays on the device, the number of launches is
// fixed, only integer atomics are used and the sort key is total, so two runs give the same output bytes.  Compiled with
// -ffp-contract=off: the float64 quotients and comparisons below are the contract.
#include "pbn_common.h"
#include "assoc_dev.h"

namespace pbn {
namespace {

constexpr int TPB = POST_TPB;
constexpr int AP_LDS_ENTRIES = 4096;                // segment size up to which a cell is sorted and integrated in LDS
constexpr int AP_MAX_KEEP = 65535;                  // predictions of a record: the visited bits of a matching wave live in LDS
constexpr int AP_VISITED_WORDS = (AP_MAX_KEEP + 64) / 64;
constexpr int AP_LDS_COLUMNS = 4096;                // columns of a record whose class a matching wave keeps in LDS
constexpr int AP_MAX_CELLS = PBN_AP_MAX_CLASSES * PBN_AP_MAX_OVERLAPS;
// state block of the table (int32[PBN_AP_TABLE_SCALARS], the scalar block of the output)
constexpr int S_RECORDS = 0, S_RECORDS_WANTED = 1, S_ENTRIES_WANTED = 2, S_PREDS_WANTED = 3, S_OVERFLOW = 4, S_MALFORMED = 5,
              S_MALFORMED_AT = 6, S_LOG_OVERFLOW = 7, S_LOG_WANTED = 8, S_WORDS = 9, S_LOG_FIRST = 10, S_LOGS = 11;
constexpr int OVERFLOW_RECORDS = 1, OVERFLOW_ENTRIES = 2, OVERFLOW_PREDS = 4;

// the workspace, carved the same way by the size query and by every entry point
struct Table {
    int* state;                     // PBN_AP_TABLE_SCALARS
    int* cells;                     // AP_MAX_CELLS x 4: entries | true entries | hard_fn | distinct scores
    int* flags;                     // 2 x PBN_AP_MAX_CLASSES: has_gt | has_pred
    int* seg_start;                 // AP_MAX_CELLS + 1
    int* cursor;                    // AP_MAX_CELLS
    int* dir;                       // rec_cap x 4: offset | tag | status | n_keep
    int* rec_off;                   // rec_cap: the record's offset in ITS log
    int* pred_base;                 // rec_cap: first prediction row of the record (-1: the record takes no part)
    int* pred_vert;                 // entry_cap prediction rows of the log being added: vertex count,
    int* pred_ignore;               //   void + too-small same-class overlap,
    int* pred_class;                //   class (-1: not kept)
    unsigned long long* key;        // entry_cap entries: ordered score bits << 1 | true
    int* cell;                      // entry_cap: the entry's cell
    unsigned long long* seg;        // entry_cap: the keys segmented by cell (sorted in place by the global path)
    size_t bytes;
    bool ok;
};

Table carve(void* ws, size_t ws_bytes, int rec_cap, int entry_cap) {
    Carver c(ws, ws_bytes);
    Table t;
    t.state = c.take<int>(PBN_AP_TABLE_SCALARS);
    t.cells = c.take<int>(AP_MAX_CELLS * 4);
    t.flags = c.take<int>(2 * PBN_AP_MAX_CLASSES);
    t.seg_start = c.take<int>(AP_MAX_CELLS + 1);
    t.cursor = c.take<int>(AP_MAX_CELLS);
    t.dir = c.take<int>((size_t)rec_cap * 4);
    t.rec_off = c.take<int>(rec_cap);
    t.pred_base = c.take<int>(rec_cap);
    t.pred_vert = c.take<int>(entry_cap);
    t.pred_ignore = c.take<int>(entry_cap);
    t.pred_class = c.take<int>(entry_cap);
    t.key = c.take<unsigned long long>(entry_cap);
    t.cell = c.take<int>(entry_cap);
    t.seg = c.take<unsigned long long>(entry_cap);
    t.bytes = align_up(c.off, 256);
    t.ok = c.ok;
    return t;
}

// index of `id` in the by-value class table, -1 if absent (selects over constant indices: the table stays in scalar registers)
__device__ __forceinline__ int class_of(const pbn_ap_class_ids& classes, long long id) {
    int c = -1;
#pragma unroll
    for (int k = PBN_AP_MAX_CLASSES - 1; k >= 0; --k) c = (k < classes.n && (long long)classes.id[k] == id) ? k : c;
    return c;
}

__device__ __forceinline__ double overlap_of(const pbn_ap_overlaps& overlaps, int o) {
    double th = overlaps.th[0];
#pragma unroll
    for (int k = 1; k < PBN_AP_MAX_OVERLAPS; ++k) th = k == o ? overlaps.th[k] : th;
    return th;
}

// class of a ground-truth column (uid // 1000 in the class table), for uid >= 0; a negative id has no class
__device__ __forceinline__ int column_class(const pbn_ap_class_ids& classes, int uid) {
    return uid < 0 ? -1 : class_of(classes, uid / 1000);
}

// What matching asks of a column, in one byte: class + 1 in the low six bits -- 0 = a void column, anything else an instance
// column (class ids are >= 1, so id 0 and every id below 1000 is void) -- and COL_COUNTS for an instance that counts (gt_vert >=
// min_region, tools/eval.py:49-51; uid >= 1000 holds for every instance column)
constexpr unsigned COL_CLASS = 63u, COL_COUNTS = 64u;
__device__ __forceinline__ unsigned column_byte(const pbn_ap_class_ids& classes, int uid, int vert, int min_region) {
    const int c = column_class(classes, uid);
    if (c < 0) return 0u;
    return (unsigned)(c + 1) | (vert >= min_region ? COL_COUNTS : 0u);
}

// ---- a. the directory: _walk_association_log by ONE wave -----------------------------------------------------------------------
// Lanes 0..7 load a header at once; the walk itself is sequential.  A record that is not whole stops the walk (S_MALFORMED = 1 and
// its word), as does one with more predictions than a matching wave holds visited bits for (S_MALFORMED = 2).  Records with status
// bits or without predictions are listed and take no part (pred_base -1).
__global__ __launch_bounds__(64) void k_ap_walk(Table t, int rec_cap, int entry_cap, const int* __restrict__ log_state,
                                                const int* __restrict__ log, int log_words, int tag_base) {
    const int lane = lane_id();
    int* st = t.state;
    int n_dir = st[S_RECORDS], wanted = st[S_RECORDS_WANTED], over = st[S_OVERFLOW];
    const int first = n_dir;
    const unsigned words0 = (unsigned)st[S_WORDS];
    int end = log_state[ST_USED];
    end = end < 0 ? 0 : (end > log_words ? log_words : end);
    if (log_state[ST_OVERFLOW]) {                        // AssociationLog.read_log refuses such a log: so does the table
        if (lane == 0) {
            if (!st[S_LOG_OVERFLOW]) st[S_LOG_WANTED] = log_state[ST_WANTED];
            st[S_LOG_OVERFLOW] = 1;
            st[S_LOG_FIRST] = first;
            st[S_LOGS] += 1;
        }
        return;
    }
    long long preds = 0;
    int pos = 0, malformed = 0;
    while (pos < end) {                                  // uniform
        int w = 0;
        if (lane < AP_HDR && pos + lane < end) w = log[pos + lane];
        const int magic = __shfl(w, 0), tag = __shfl(w, 1), nk = __shfl(w, 2), ng = __shfl(w, 3), status = __shfl(w, 5),
                  size = __shfl(w, 6);
        if (end - pos < AP_HDR || magic != PBN_AP_RECORD_MAGIC || nk < 0 || ng < 0) { malformed = 1; break; }
        const long long want = ap_record_words(nk, ng);
        if ((long long)size != want || (long long)pos + want > (long long)end) { malformed = 1; break; }
        if (nk > AP_MAX_KEEP) { malformed = 2; break; }
        const bool usable = status == 0 && nk > 0;
        wanted = wanted < 0x7fffffff ? wanted + 1 : wanted;
        if (n_dir < rec_cap) {
            if (lane == 0) {
                t.dir[4 * n_dir + 0] = (int)(words0 + (unsigned)pos);
                t.dir[4 * n_dir + 1] = tag + tag_base;
                t.dir[4 * n_dir + 2] = status;
                t.dir[4 * n_dir + 3] = nk;
                t.rec_off[n_dir] = pos;
                t.pred_base[n_dir] = (usable && preds + nk <= (long long)entry_cap) ? (int)preds : -1;
            }
            ++n_dir;
            if (usable) preds += nk;
        } else {
            over |= OVERFLOW_RECORDS;
        }
        pos += size;
    }
    if (preds > (long long)entry_cap) over |= OVERFLOW_PREDS;
    if (lane == 0) {
        st[S_RECORDS] = n_dir;
        st[S_RECORDS_WANTED] = wanted;
        st[S_OVERFLOW] = over;
        if (preds > (long long)st[S_PREDS_WANTED]) st[S_PREDS_WANTED] = preds > 0x7fffffffLL ? 0x7fffffff : (int)preds;
        if (malformed && !st[S_MALFORMED]) {
            st[S_MALFORMED] = malformed;
            st[S_MALFORMED_AT] = pos;
        }
        st[S_WORDS] = (int)(words0 + (unsigned)end);
        st[S_LOG_FIRST] = first;
        st[S_LOGS] += 1;
    }
}

// the parts of a record
struct Record {
    const int* uid;
    const int* gt_vert;
    const int* label;
    const int* conf;
    const int* inter;
    int nk, ng;
};

__device__ __forceinline__ Record record_at(const int* __restrict__ log, int off) {
    const int* rec = log + off;
    Record r;
    r.nk = rec[2];
    r.ng = rec[3];
    r.uid = rec + AP_HDR;
    r.gt_vert = r.uid + r.ng;
    r.label = r.gt_vert + r.ng;
    r.conf = r.label + r.nk;
    r.inter = r.conf + r.nk;
    return r;
}

// ---- b1. one row per prediction: matches_from_table's counts, and the classes' has_gt / has_pred --------------------------------
// One workgroup per directory record of the log being added; a wave takes every fourth prediction, its lanes stride the columns.
__global__ __launch_bounds__(TPB) void k_ap_rows(Table t, const int* __restrict__ log, pbn_ap_class_ids classes, int min_region) {
    const int* st = t.state;
    const int d = st[S_LOG_FIRST] + (int)blockIdx.x;
    if (d >= st[S_RECORDS]) return;
    const int base = t.pred_base[d];
    if (base < 0) return;
    const Record r = record_at(log, t.rec_off[d]);
    const int lane = lane_id(), wave = (int)(threadIdx.x >> 6);
    for (int g = threadIdx.x; g < r.ng; g += TPB) {                       // has_gt: an instance that counts
        const unsigned b = column_byte(classes, r.uid[g], r.gt_vert[g], min_region);
        if (b & COL_COUNTS) atomicOr(&t.flags[(int)(b & COL_CLASS) - 1], 1);
    }
    for (int q = wave; q < r.nk; q += TPB / 64) {
        const int pc = class_of(classes, r.label[q]);
        const int* row = r.inter + (size_t)q * r.ng;
        int vert = 0, ignore = 0;
        for (int g = lane; g < r.ng; g += 64) {
            const int v = row[g];
            const unsigned b = column_byte(classes, r.uid[g], r.gt_vert[g], min_region);
            vert += v;
            // void columns, and same-class instances that do not count
            if ((b & COL_CLASS) == 0u || (!(b & COL_COUNTS) && (int)(b & COL_CLASS) - 1 == pc)) ignore += v;
        }
        vert = wave_reduce_add(vert);
        ignore = wave_reduce_add(ignore);
        if (lane == 0) {
            const bool kept = pc >= 0 && vert >= min_region;
            t.pred_vert[base + q] = vert;
            t.pred_ignore[base + q] = ignore;
            t.pred_class[base + q] = kept ? pc : -1;
            if (kept) atomicOr(&t.flags[PBN_AP_MAX_CLASSES + pc], 1);
        }
    }
}

// order-preserving key of a float32 score (-0 counts as +0, as numpy's comparisons have it), then the true bit
__device__ __forceinline__ unsigned long long entry_key(float score, int is_true) {
    if (score == 0.0f) score = 0.0f;
    const unsigned b = (unsigned)__float_as_int(score);
    const unsigned ordered = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
    return ((unsigned long long)ordered << 1) | (unsigned long long)(is_true & 1);
}

// one entry, by one lane: counted always, stored while the table has room
__device__ __forceinline__ void emit(const Table& t, int entry_cap, int cell, float score, int is_true) {
    atomicAdd(&t.cells[4 * cell + 0], 1);
    if (is_true) atomicAdd(&t.cells[4 * cell + 1], 1);
    const int slot = atomicAdd(&t.state[S_ENTRIES_WANTED], 1);
    if (slot >= 0 && slot < entry_cap) {
        t.key[slot] = entry_key(score, is_true);
        t.cell[slot] = cell;
    } else {
        atomicOr(&t.state[S_OVERFLOW], OVERFLOW_ENTRIES);
    }
}

// ---- b2. matching: _match_scene_class for every class of one record at one overlap, by ONE wave -------------------------------
// Instances in column order, predictions in 64s: the ballot's set bits are taken in prediction order.  visited (one bit per
// prediction, persistent across the record's instances) lives in LDS as ballot-shaped words; every lane writes the same word and
// reads back its own write, so no lane depends on another's store.
__global__ __launch_bounds__(64) void k_ap_match(Table t, int entry_cap, const int* __restrict__ log, pbn_ap_class_ids classes,
                                                 pbn_ap_overlaps overlaps, int min_region) {
    __shared__ unsigned long long s_visited[AP_VISITED_WORDS];
    __shared__ unsigned char s_column[AP_LDS_COLUMNS];
    const int* st = t.state;
    const int d = st[S_LOG_FIRST] + (int)blockIdx.x;
    if (d >= st[S_RECORDS]) return;
    const int base = t.pred_base[d];
    if (base < 0) return;
    const int o = (int)blockIdx.y, lane = lane_id();
    const double th = overlap_of(overlaps, o);
    const Record r = record_at(log, t.rec_off[d]);
    const int chunks = (r.nk + 63) / 64;
    for (int k = lane; k < chunks; k += 64) s_visited[k] = 0ull;
    // the columns' bytes once per wave: in LDS for the first AP_LDS_COLUMNS columns, recomputed for the columns beyond
    for (int g = lane; g < r.ng && g < AP_LDS_COLUMNS; g += 64)
        s_column[g] = (unsigned char)column_byte(classes, r.uid[g], r.gt_vert[g], min_region);
    __syncthreads();
    auto column = [&](int g) -> unsigned {
        return g < AP_LDS_COLUMNS ? (unsigned)s_column[g] : column_byte(classes, r.uid[g], r.gt_vert[g], min_region);
    };
    // the instances that count, in column order (tools/eval.py:60-100)
    for (int g = 0; g < r.ng; ++g) {                                     // uniform
        const unsigned cb = column(g);
        if (!(cb & COL_COUNTS)) continue;
        const int cg = (int)(cb & COL_CLASS) - 1, gv = r.gt_vert[g];
        const int cell = cg * overlaps.n + o;
        bool have = false;
        float best = 0.0f;
        for (int k = 0; k < chunks; ++k) {
            const int q = k * 64 + lane;
            const unsigned long long visited = s_visited[k];
            bool hit = false;
            float conf = 0.0f;
            if (q < r.nk && t.pred_class[base + q] == cg && !((visited >> lane) & 1ull)) {
                const int v = r.inter[(size_t)q * r.ng + g];
                if (v > 0) {
                    const int uni = t.pred_vert[base + q] + gv - v;
                    hit = (double)v / (double)(uni > 1 ? uni : 1) > th;
                    conf = __int_as_float(r.conf[q]);
                }
            }
            unsigned long long todo = __ballot(hit);
            while (todo) {                                               // uniform
                const int l = __ffsll((long long)todo) - 1;
                todo &= todo - 1ull;
                const float c = __shfl(conf, l);
                if (!have) {                                             // the first unvisited hit takes the instance
                    have = true;
                    best = c;
                    s_visited[k] = visited | (1ull << l);
                } else {                                                 // a later hit: the lower score is a false positive and the
                    if (lane == 0) emit(t, entry_cap, cell, c < best ? c : best, 0);   // prediction stays unvisited (:78-86)
                    best = c > best ? c : best;
                }
            }
        }
        if (lane == 0) {
            if (have) emit(t, entry_cap, cell, best, 1);
            else atomicAdd(&t.cells[4 * cell + 2], 1);
        }
    }
    // predictions without any same-class instance above the threshold, small instances included (:102-121)
    for (int q = 0; q < r.nk; ++q) {                                     // uniform
        const int pc = t.pred_class[base + q];
        if (pc < 0) continue;
        const int pv = t.pred_vert[base + q];
        const int* row = r.inter + (size_t)q * r.ng;
        bool any = false;
        for (int g0 = 0; g0 < r.ng; g0 += 64) {
            const int g = g0 + lane;
            bool over = false;
            if (g < r.ng) {
                const int v = row[g];
                const unsigned cb = v > 0 ? column(g) : 0u;
                if ((cb & COL_CLASS) != 0u && (int)(cb & COL_CLASS) - 1 == pc) {
                    const int uni = pv + r.gt_vert[g] - v;
                    over = (double)v / (double)(uni > 1 ? uni : 1) > th;
                }
            }
            any |= __ballot(over) != 0ull;
        }
        if (!any && lane == 0 && (double)t.pred_ignore[base + q] / (double)pv <= th)
            emit(t, entry_cap, pc * overlaps.n + o, __int_as_float(r.conf[q]), 0);
    }
}

// ---- c. integration ------------------------------------------------------------------------------------------------------------
// segment starts of the cells from their entry counts, cursors cleared; one thread over at most 512 cells
__global__ __launch_bounds__(64) void k_ap_segments(Table t, int n_cells) {
    if (threadIdx.x != 0) return;
    int at = 0;
    for (int c = 0; c < n_cells; ++c) {
        t.seg_start[c] = at;
        t.cursor[c] = 0;
        at += t.cells[4 * c + 0];
    }
    t.seg_start[n_cells] = at;
}

// the keys into their cells' segments.  The order inside a segment depends on the atomics; the sort that follows does not.
__global__ __launch_bounds__(TPB) void k_ap_scatter(Table t, int entry_cap, int n_cells) {
    if (t.state[S_OVERFLOW]) return;
    const int n = min(t.state[S_ENTRIES_WANTED], entry_cap);
    for (int e = blockIdx.x * TPB + threadIdx.x; e < n; e += gridDim.x * TPB) {
        const int c = t.cell[e];
        if (c < 0 || c >= n_cells) continue;
        const int slot = t.seg_start[c] + atomicAdd(&t.cursor[c], 1);
        if (slot >= 0 && slot < entry_cap) t.seg[slot] = t.key[e];
    }
}

// ascending bitonic network by one workgroup on a[0, n), n arbitrary: every compare-exchange leaves the smaller key at the lower
// index, so the places from n up to the next power of two behave as +infinity without being touched.  `a` is LDS or global memory.
__device__ __forceinline__ void sort_keys(unsigned long long* a, int n) {
    int p2 = 1;
    while (p2 < n) p2 <<= 1;
    const int pairs = p2 >> 1;
    for (int k = 2; k <= p2; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = threadIdx.x; i < pairs; i += TPB) {
                int lo, hi;
                if (j == (k >> 1)) {                         // first step of a merge: mirror within the block of k
                    const int b = i / j, r = i - b * j;
                    lo = b * k + r;
                    hi = b * k + k - 1 - r;
                } else {
                    const int b = i / j, r = i - b * j;
                    lo = b * 2 * j + r;
                    hi = lo + j;
                }
                if (hi < n) {
                    const unsigned long long x = a[lo], y = a[hi];
                    if (y < x) { a[lo] = y; a[hi] = x; }
                }
            }
            __syncthreads();
        }
    }
}

// _average_precision (tools/eval.py:131-176) on the sorted keys a[0, n) of one cell, by one workgroup.  Pass 1 packs, in place,
// for every distinct score in ascending order its first position and the true matches scored strictly lower; pass 2 sums
// precision * width in float64, each thread its strided terms and then a fixed tree.  Returns the area in every thread; *distinct
// gets the number of distinct scores.
__device__ __forceinline__ double integrate_keys(unsigned long long* a, int n, int n_true, int hard_fn, int* s_wave,
                                                 unsigned long long* s_carry, double* s_sum, int* distinct) {
    const int lane = lane_id(), wave = (int)(threadIdx.x >> 6);
    int base_first = 0, base_true = 0;
    for (int p0 = 0; p0 < n; p0 += TPB) {                                // uniform
        const int p = p0 + (int)threadIdx.x;
        unsigned long long cur = 0ull, prev = 0ull;
        if (p < n) {
            cur = a[p];
            if (p > 0) prev = threadIdx.x == 0 ? *s_carry : a[p - 1];     // a[p0 - 1] may hold a packed word by now
        }
        __syncthreads();                                                 // every key of this trip is read before any is replaced
        const bool first = p < n && (p == 0 || (cur >> 1) != (prev >> 1));
        const int mine = (first ? 1 << 16 : 0) | (int)(p < n ? cur & 1ull : 0ull);
        int incl = mine;
#pragma unroll
        for (int s = 1; s < 64; s <<= 1) {
            const int v = __shfl_up(incl, s, 64);
            if (lane >= s) incl += v;
        }
        if (lane == 63) s_wave[wave] = incl;
        if (threadIdx.x == TPB - 1) *s_carry = cur;
        __syncthreads();
        int before = 0, all = 0;
#pragma unroll
        for (int w = 0; w < TPB / 64; ++w) {
            before += w < wave ? s_wave[w] : 0;
            all += s_wave[w];
        }
        const int excl = before + incl - mine;
        if (first) a[base_first + (excl >> 16)] = ((unsigned long long)(unsigned)p << 32) | (unsigned)(base_true + (excl & 0xffff));
        base_first += all >> 16;
        base_true += all & 0xffff;
        __syncthreads();                                                 // s_wave and the carry are read before the next trip
    }
    const int d = base_first;
    const double denom = (double)(n_true + hard_fn);
    double acc = 0.0;
    for (int k = threadIdx.x; k <= d; k += TPB) {
        // recall of the distinct scores k - 1 (k itself at the curve's start) and k + 1; beyond the last one it is 0
        const int jl = k > 0 ? k - 1 : 0, jr = k + 1;
        const double rl = jl < d ? (double)(n_true - (int)(unsigned)a[jl]) / denom : 0.0;
        const double rr = jr < d ? (double)(n_true - (int)(unsigned)a[jr]) / denom : 0.0;
        double precision = 1.0;                                           // the artificial last point (:161-162)
        if (k < d) {
            const unsigned long long w = a[k];
            precision = (double)(n_true - (int)(unsigned)w) / (double)(n - (int)(w >> 32));
        }
        acc += precision * (0.5 * rl + -0.5 * rr);
    }
    s_sum[threadIdx.x] = acc;
    __syncthreads();
    for (int s = TPB / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) s_sum[threadIdx.x] += s_sum[threadIdx.x + s];
        __syncthreads();
    }
    *distinct = d;
    return s_sum[0];
}

// one workgroup per cell: sort the segment (in LDS up to AP_LDS_ENTRIES, in place in global memory above), integrate, publish
__global__ __launch_bounds__(TPB) void k_ap_integrate(Table t, int entry_cap, int n_classes, int n_overlaps,
                                                      float* __restrict__ ap, int* __restrict__ cells_out) {
    __shared__ unsigned long long s_keys[AP_LDS_ENTRIES];
    __shared__ double s_sum[TPB];
    __shared__ unsigned long long s_carry;
    __shared__ int s_wave[TPB / 64];
    const int cell = (int)blockIdx.x, cls = cell / n_overlaps;
    const int n = t.cells[4 * cell + 0], n_true = t.cells[4 * cell + 1], hard_fn = t.cells[4 * cell + 2];
    const bool has_gt = t.flags[cls] != 0, has_pred = t.flags[PBN_AP_MAX_CLASSES + cls] != 0;
    const int start = t.seg_start[cell];
    int distinct = 0;
    float value = has_gt ? 0.0f : __int_as_float(0x7fc00000);            // no ground truth: NaN; no prediction: 0
    const bool whole = !t.state[S_OVERFLOW] && start >= 0 && n >= 0 && (long long)start + n <= (long long)entry_cap;
    if (whole && n > 0) {                                                // uniform
        unsigned long long* seg = t.seg + start;
        double area;
        if (n <= AP_LDS_ENTRIES) {
            for (int i = threadIdx.x; i < n; i += TPB) s_keys[i] = seg[i];
            __syncthreads();
            sort_keys(s_keys, n);
            area = integrate_keys(s_keys, n, n_true, hard_fn, s_wave, &s_carry, s_sum, &distinct);
        } else {
            __syncthreads();
            sort_keys(seg, n);
            area = integrate_keys(seg, n, n_true, hard_fn, s_wave, &s_carry, s_sum, &distinct);
        }
        if (has_gt && has_pred) value = (float)area;
    }
    if (threadIdx.x == 0) {
        ap[cell] = value;
        cells_out[4 * cell + 0] = n;
        cells_out[4 * cell + 1] = n_true;
        cells_out[4 * cell + 2] = hard_fn;
        cells_out[4 * cell + 3] = distinct;
    }
}

// the scalar block, the classes' flags and the directory into the output
__global__ __launch_bounds__(TPB) void k_ap_publish(Table t, int rec_cap, int n_classes, int* __restrict__ scalars,
                                                    int* __restrict__ flags, int* __restrict__ dir) {
    const int n_dir = min(t.state[S_RECORDS], rec_cap);
    const long long total = PBN_AP_TABLE_SCALARS + 2LL * n_classes + 4LL * rec_cap, step = (long long)gridDim.x * TPB;
    for (long long e = (long long)blockIdx.x * TPB + threadIdx.x; e < total; e += step) {
        if (e < PBN_AP_TABLE_SCALARS) { scalars[e] = t.state[e]; continue; }
        long long i = e - PBN_AP_TABLE_SCALARS;
        if (i < 2LL * n_classes) {
            const int half = (int)(i / n_classes), c = (int)(i - (long long)half * n_classes);
            flags[i] = t.flags[half * PBN_AP_MAX_CLASSES + c];
            continue;
        }
        i -= 2LL * n_classes;
        dir[i] = i < 4LL * n_dir ? t.dir[i] : 0;
    }
}

int check_caps(int rec_cap, long long entry_cap) {
    if (rec_cap < 1 || entry_cap < 1) return PBN_ERR_ARG;
    if (entry_cap > 0x7fffffffLL / 2 || rec_cap > 0x7fffffff / 4) return PBN_ERR_RANGE;
    return PBN_OK;
}

}  // namespace
}  // namespace pbn

using namespace pbn;

extern "C" size_t pbn_ap_table_workspace_bytes(int rec_cap, int64_t entry_cap) {
    if (check_caps(rec_cap, entry_cap) != PBN_OK) return 0;
    return carve(nullptr, 0, rec_cap, (int)entry_cap).bytes;
}

extern "C" int pbn_ap_table_lds_entries(void) { return AP_LDS_ENTRIES; }

extern "C" int pbn_ap_table_reset(void* workspace, size_t workspace_bytes, int rec_cap, int64_t entry_cap, pbn_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    const int rc = check_caps(rec_cap, entry_cap);
    if (rc != PBN_OK) return rc;
    if (!workspace) return PBN_ERR_ARG;
    const Table t = carve(workspace, workspace_bytes, rec_cap, (int)entry_cap);
    if (!t.ok || t.bytes > workspace_bytes) return PBN_ERR_WORKSPACE;
    const FillRange ranges[3] = {{t.state, sizeof(int) * PBN_AP_TABLE_SCALARS, 0},
                                 {t.cells, sizeof(int) * AP_MAX_CELLS * 4, 0},
                                 {t.flags, sizeof(int) * 2 * PBN_AP_MAX_CLASSES, 0}};
    return fill_ranges(ranges, 3, stream);
}

extern "C" int pbn_ap_table_add_log(void* workspace, size_t workspace_bytes, int rec_cap, int64_t entry_cap,
                                    const int32_t* log_state, const int32_t* log, int64_t log_words, int tag_base,
                                    pbn_ap_class_ids classes, pbn_ap_overlaps overlaps, int min_region, pbn_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    const int rc = check_caps(rec_cap, entry_cap);
    if (rc != PBN_OK) return rc;
    if (!workspace || !log_state || log_words < 0 || (log_words > 0 && !log) || tag_base < 0 || min_region < 0) return PBN_ERR_ARG;
    if (classes.n < 1 || classes.n > PBN_AP_MAX_CLASSES || overlaps.n < 1 || overlaps.n > PBN_AP_MAX_OVERLAPS) return PBN_ERR_ARG;
    for (int k = 0; k < classes.n; ++k)
        if (classes.id[k] < 1) return PBN_ERR_ARG;         // id 0 is the unannotated id: a void column, never a class
    for (int k = 0; k < overlaps.n; ++k)
        if (!(overlaps.th[k] >= 0.0 && overlaps.th[k] <= 1.0)) return PBN_ERR_ARG;
    if (log_words > 0x7fffffffLL) return PBN_ERR_RANGE;
    const Table t = carve(workspace, workspace_bytes, rec_cap, (int)entry_cap);
    if (!t.ok || t.bytes > workspace_bytes) return PBN_ERR_WORKSPACE;
    hipLaunchKernelGGL(k_ap_walk, dim3(1), dim3(64), 0, stream, t, rec_cap, (int)entry_cap, log_state, log, (int)log_words, tag_base);
    if (log_words > 0) {
        hipLaunchKernelGGL(k_ap_rows, dim3(rec_cap), dim3(TPB), 0, stream, t, log, classes, min_region);
        hipLaunchKernelGGL(k_ap_match, dim3(rec_cap, overlaps.n), dim3(64), 0, stream, t, (int)entry_cap, log, classes, overlaps,
                           min_region);
    }
    PBN_LAUNCH_CHECK();
    return PBN_OK;
}

extern "C" int pbn_ap_table_finish(void* workspace, size_t workspace_bytes, int rec_cap, int64_t entry_cap, int n_classes,
                                   int n_overlaps, float* ap, int32_t* cells, int32_t* flags, int32_t* directory,
                                   int32_t* scalars, pbn_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    const int rc = check_caps(rec_cap, entry_cap);
    if (rc != PBN_OK) return rc;
    if (!workspace || !ap || !cells || !flags || !directory || !scalars) return PBN_ERR_ARG;
    if (n_classes < 1 || n_classes > PBN_AP_MAX_CLASSES || n_overlaps < 1 || n_overlaps > PBN_AP_MAX_OVERLAPS) return PBN_ERR_ARG;
    const Table t = carve(workspace, workspace_bytes, rec_cap, (int)entry_cap);
    if (!t.ok || t.bytes > workspace_bytes) return PBN_ERR_WORKSPACE;
    const int n_cells = n_classes * n_overlaps;
    hipLaunchKernelGGL(k_ap_segments, dim3(1), dim3(64), 0, stream, t, n_cells);
    hipLaunchKernelGGL(k_ap_scatter, dim3(stride_blocks(entry_cap)), dim3(TPB), 0, stream, t, (int)entry_cap, n_cells);
    hipLaunchKernelGGL(k_ap_integrate, dim3(n_cells), dim3(TPB), 0, stream, t, (int)entry_cap, n_classes, n_overlaps, ap, cells);
    hipLaunchKernelGGL(k_ap_publish, dim3(stride_blocks(PBN_AP_TABLE_SCALARS + 2LL * n_classes + 4LL * rec_cap)), dim3(TPB), 0,
                       stream, t, rec_cap, n_classes, scalars, flags, directory);
    PBN_LAUNCH_CHECK();
    return PBN_OK;
}
