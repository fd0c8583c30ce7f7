// wgrad_plan.h -- what pbn_spconv_wgrad (wgrad.hip) launches for a shape, stated once: the kernel form, its tile shape, the
// strip count, the pair splits and the grid.  The launch follows this plan and pbn_spconv_wgrad_plan reports it.  Host code
// only, no HIP type: a plain C++ compiler builds it alone; the ABI (pbn_wgrad_plan) is include/pbnet_hip.h.
#pragma once
#include "../../include/pbnet_hip.h"

namespace pbn {

constexpr int WGRAD_NTW = 4;   // k_wgrad<T>: output-channel tiles per wave

// environment knobs of the plan (wgrad_knobs() in wgrad.hip reads them); 0 = unset
struct WgradKnobs {
    int form;        // PBN_WGRAD_FORM: 32 = k_wgrad<T> for every slab; any other value: the automatic choice
    int maxt;        // PBN_WGRAD_MAXT: cap of WA and WB
    int wgs;         // PBN_WGRAD_WGS: workgroup target of the pair splits
    int min_pairs;   // PBN_WGRAD_MIN_PAIRS: pairs per workgroup below which no further split is made
    int dbg;         // PBN_WGRAD_DBG: measurement switches of k_wgrad_ring (WgradArgs::dbg); no part of the plan
};

struct WgradShape {
    int dtype, ld_x, ld_g;
    bool aligned16;   // both slab bases on a 16-byte boundary
    bool identity;    // no pair lists: pair p = row p (one offset)
    int n_offsets, n_pairs_total, cin, cout;
    bool has_workspace;
    size_t workspace_bytes;
};

// what both entries refuse as PBN_ERR_ARG before any arithmetic
inline bool wgrad_shape_ok(const WgradShape& s) {
    return s.n_offsets >= 1 && s.cin >= 1 && s.cout >= 1 && s.n_pairs_total >= 0 &&
           (s.dtype == PBN_F32 || s.dtype == PBN_BF16 || s.dtype == PBN_F16) && !(s.identity && s.n_offsets != 1);
}

// workgroups of a launch: wgrad_tile() (wgrad.hip) maps a flat id back to (strip, offset, split); from 8 splits on, the
// splits are padded to a multiple of the 8 XCDs
inline long long wgrad_grid(int strips, int K, int splits) {
    return (long long)strips * K * (splits < 8 ? splits : ((splits + 7) & ~7));
}

// s must pass wgrad_shape_ok
inline pbn_wgrad_plan wgrad_plan(const WgradShape& s, const WgradKnobs& kn) {
    auto cdiv = [](long long a, long long b) { return (int)((a + b - 1) / b); };
    const int cin = s.cin, cout = s.cout, n_offsets = s.n_offsets, n_pairs_total = s.n_pairs_total;
    const long long n_out = (long long)n_offsets * cin * cout;
    // 16-bit slabs whose rows can be read in 16-byte chunks take k_wgrad_ring on the bf16/f16 matrix cores; fp32 slabs, the
    // other 16-bit slabs and every slab under PBN_WGRAD_FORM=32 take k_wgrad<T> (f32 MFMA)
    const bool ring = kn.form != 32 && s.dtype != PBN_F32 && (s.ld_x % 8) == 0 && (s.ld_g % 8) == 0 &&
                      s.ld_x >= ((cin + 7) & ~7) && s.ld_g >= ((cout + 7) & ~7) && s.aligned16;
    int wa = 0, wb = 0, strips, co_groups;
    bool small_level = false;
    if (ring) {
        const int cit = cdiv(cin, 16), cot = cdiv(cout, 16);
        wa = cit >= 7 ? 4 : (cit + 1) / 2;            // waves are 2 x 2: a workgroup covers 2 wa x 2 wb tiles
        wb = cot >= 7 ? 4 : (cot + 1) / 2;
        // few pairs per offset (the stride-8/16 levels): quarter tiles instead of pair splits -- 4x the workgroups with no
        // partial slabs and no reduce launch (measured, stride-16 256->256: 23 -> 13 us; stride-8: 35 us either way)
        small_level = n_pairs_total / n_offsets < 3000 && cdiv(cit, 2 * wa) * cdiv(cot, 2 * wb) * n_offsets < 256;
        const int maxt = kn.maxt ? kn.maxt : (small_level ? 2 : 4);
        if (wa > maxt) wa = maxt;
        if (wb > maxt) wb = maxt;
        co_groups = cdiv(cot, 2 * wb);
        strips = cdiv(cit, 2 * wa) * co_groups;
    } else {
        co_groups = cdiv(cout, WGRAD_NTW * 16);
        strips = cdiv(cin, 16) * co_groups;
    }
    // pair splits: enough workgroups for the chip, enough pairs per workgroup to amortise its prologue, bounded by the
    // workspace.  k_wgrad_ring: ~1024 workgroups of >= 256 pairs (8 steps); k_wgrad<T>: ~2048 of >= 512
    const long long target = kn.wgs > 0 ? kn.wgs : (ring ? 1024 : 2048);
    const long long min_pairs = kn.min_pairs > 0 ? kn.min_pairs : (ring ? 256 : 512);
    const long long pairs_per_offset = n_pairs_total / n_offsets + 1;
    long long splits = target / ((long long)strips * n_offsets) + 1;
    if (splits > pairs_per_offset / min_pairs + 1) splits = pairs_per_offset / min_pairs + 1;
    // every split writes and re-reads a dW-sized partial: at most ~32 MB of partials (256->256 cubes: 4 splits)
    const long long by_traffic = (32LL << 20) / (long long)(sizeof(float) * (size_t)n_out) + 1;
    if (ring && splits > by_traffic) splits = by_traffic;
    if (small_level && kn.wgs <= 0) splits = 1;
    const long long by_ws = s.has_workspace ? (long long)(s.workspace_bytes / (sizeof(float) * (size_t)n_out)) : 1;
    if (splits > by_ws) splits = by_ws;
    if (splits > 64) splits = 64;
    if (splits < 1) splits = 1;
    pbn_wgrad_plan p;
    p.form = ring ? 1 : 0;
    p.wa = wa; p.wb = wb; p.small_level = small_level ? 1 : 0;
    p.strips = strips; p.co_groups = co_groups; p.splits = (int)splits;
    p.grid = wgrad_grid(strips, n_offsets, (int)splits);
    return p;
}

}  // namespace pbn
