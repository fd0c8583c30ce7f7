// unet_plan.h -- what the two executors of a U-Net plan (executor.hip: eval forward, train_exec.hip: train forward and
// backward) agree on, stated once: the element size, which tables an op's map kind means, the range check of an op's buffer
// and level indices, and where a symbolic buffer lives.  Host code only; the ABI is include/pbnet_hip.h.
#pragma once
#include "pbn_common.h"

namespace pbn {

inline int esize(int dtype) { return dtype == PBN_F32 ? 4 : 2; }

// the maps of one pyramid as every executor entry point receives them (levels 0..4 = tensor strides 1..16)
struct MapTables {
    const int32_t* const* k3; const int32_t* k5; const int32_t* const* down; const int32_t* const* up;
};

// fwd: the op's table (rows = output level); bwd: the table of its input gradient (rows = input level); K: offsets;
// pair_slot: its entry of pbn_pair_lists[14] (-1: identity pairs); ok: a known kind whose forward table exists
struct OpTables { const int32_t* fwd; const int32_t* bwd; int K; int pair_slot; bool ok; };

// levels must be in range (op_index_ok)
inline OpTables op_tables(int map_kind, int level_in, int level_out, const MapTables& t) {
    auto at = [](const int32_t* const* a, int l) -> const int32_t* { return a ? a[l] : nullptr; };
    OpTables r{nullptr, nullptr, 1, -1, false};
    switch (map_kind) {
        case 0: r.ok = true; return r;
        case 1: r.fwd = r.bwd = at(t.k3, level_out); r.K = 27; r.pair_slot = level_out; break;   // centred cube: the mirrored offsets of the same table
        case 2: r.fwd = r.bwd = t.k5; r.K = 125; r.pair_slot = 5; break;
        case 3: r.fwd = at(t.down, level_in); r.bwd = at(t.up, level_in); r.K = 8; r.pair_slot = 6 + level_in; break;      // k2s2: level_in = fine level
        case 4: r.fwd = at(t.up, level_out); r.bwd = at(t.down, level_out); r.K = 8; r.pair_slot = 10 + level_out; break;  // transposed: level_out = fine
        default: return r;
    }
    r.ok = r.fwd != nullptr;
    return r;
}

// an op reads buffer 0 (the caller's slab) or an arena buffer, writes an arena buffer, and may have no residual (-1)
inline bool op_index_ok(int in_buf, int res_buf, int out_buf, int level_in, int level_out, int n_bufs) {
    return in_buf >= 0 && in_buf < n_bufs && out_buf >= 1 && out_buf < n_bufs && res_buf < n_bufs && level_in >= 0 &&
           level_in <= 4 && level_out >= 0 && level_out <= 4;
}

// Symbolic buffers -> addresses and row strides (elements): buffer 0 is a slab of the caller's (`ext`, row stride `ld_ext`),
// buffer b >= 1 sits at offs[b] (pbn_unet_arena_bytes) of the arena and is as wide as the plan says.
struct PlanArena {
    char* arena; const int64_t* offs; const pbn_unet_buf* bufs; char* ext; int ld_ext; int es;
    PlanArena(const void* arena_, const int64_t* offs_, const pbn_unet_buf* bufs_, const void* ext_, int ld_ext_, int es_)
        : arena((char*)arena_), offs(offs_), bufs(bufs_), ext((char*)ext_), ld_ext(ld_ext_), es(es_) {}
    char* at(int b, int col = 0) const { return (b == 0 ? ext : arena + offs[b]) + (size_t)col * es; }
    int ld(int b) const { return b == 0 ? ld_ext : bufs[b].width; }
};

}  // namespace pbn
