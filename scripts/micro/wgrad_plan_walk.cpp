// wgrad_plan_walk.cpp -- the weight gradient's launch plan (pbnet_amd/csrc/wgrad_plan.h) walked on the CPU over the corners
// of its argument space, as a stand-alone host program for the sanitizers: no HIP, no library, no GPU.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all scripts/micro/wgrad_plan_walk.cpp -o wgrad_plan_walk
//   ./wgrad_plan_walk
// Shapes: every dtype, aligned or not, ld % 8 == 0 or not, cin / cout from 1 to 256 across the tile steps, K 1 / 8 / 27 / 125,
// pairs per offset from 0 to 150 000 and n_pairs_total at the limit of pbn_spconv_wgrad_checked (2^30 - 1), workspace absent /
// 0 bytes / one slab / 64 slabs / SIZE_MAX; knobs unset, PBN_WGRAD_FORM=32, and the forced values of the split tests.
// Every plan must keep what the kernels' index arithmetic relies on.
#include <cstdio>
#include <cstdlib>

#include "../../pbnet_amd/csrc/wgrad_plan.h"

using namespace pbn;

static long long n_checked = 0;

#define REQUIRE(c) do { if (!(c)) { std::printf("line %d: %s fails: dtype %d cin %d cout %d K %d pairs %d\n", __LINE__, #c, s.dtype, \
                                               s.cin, s.cout, s.n_offsets, s.n_pairs_total); std::exit(1); } } while (0)

static void check(const WgradShape& s, const WgradKnobs& kn) {
    if (!wgrad_shape_ok(s)) return;
    const pbn_wgrad_plan p = wgrad_plan(s, kn);
    ++n_checked;
    REQUIRE(p.splits >= 1 && p.splits <= 64);
    REQUIRE(p.strips >= 1 && p.co_groups >= 1 && p.strips % p.co_groups == 0);
    REQUIRE(p.grid == (long long)p.strips * s.n_offsets * (p.splits < 8 ? p.splits : (p.splits + 7) / 8 * 8));
    REQUIRE(p.grid >= 1 && p.grid <= 0x7fffffffLL);
    const long long n_out = (long long)s.n_offsets * s.cin * s.cout;
    if (p.splits > 1) REQUIRE(s.has_workspace && (unsigned long long)p.splits * 4ull * (unsigned long long)n_out <= s.workspace_bytes);
    if (p.form == 1) {
        REQUIRE(s.dtype != PBN_F32 && s.aligned16 && s.ld_x % 8 == 0 && s.ld_g % 8 == 0 && kn.form != 32);
        REQUIRE(p.wa >= 1 && p.wa <= 4 && p.wb >= 1 && p.wb <= 4);
        // the strips cover every channel tile
        REQUIRE((p.strips / p.co_groups) * 32 * p.wa >= s.cin && p.co_groups * 32 * p.wb >= s.cout);
        if (p.small_level && kn.wgs <= 0) REQUIRE(p.splits == 1);
    } else {
        REQUIRE(p.form == 0 && p.wa == 0 && p.wb == 0 && !p.small_level);
        REQUIRE((p.strips / p.co_groups) * 16 >= s.cin && p.co_groups * 16 * WGRAD_NTW >= s.cout);
    }
}

int main() {
    const int channels[] = {1, 3, 6, 15, 16, 17, 20, 32, 48, 56, 64, 90, 96, 97, 112, 120, 128, 136, 255, 256};
    const int ks[] = {1, 8, 27, 125};
    const int pairs[] = {0, 1, 31, 100, 2999, 3000, 12000, 150000};
    const WgradKnobs knobs[] = {{0, 0, 0, 0, 0}, {32, 0, 0, 0, 0}, {16, 0, 0, 0, 0}, {0, 1, 0, 0, 0}, {0, 4, 0, 0, 0}, {0, 0, 0, 1 << 30, 0},
                                {0, 0, 1, 1, 0}, {0, 0, 63 * 5, 1, 0}, {0, 0, 1 << 30, 1, 0}, {0, 2, 100000, 1, 31}};
    for (int dtype = 0; dtype < 3; ++dtype)
        for (int aligned = 0; aligned < 2; ++aligned)
            for (int ld8 = 0; ld8 < 2; ++ld8)
                for (int cin : channels)
                    for (int cout : channels)
                        for (int k : ks)
                            for (int ppo : pairs)
                                for (int ident = 0; ident < 2; ++ident)
                                    for (int ws = 0; ws < 5; ++ws) {
                                        const size_t slab = sizeof(float) * (size_t)k * cin * cout;
                                        const size_t bytes[] = {0, 0, slab, 64 * slab, (size_t)-1};
                                        const WgradShape s{dtype, ((cin + 7) & ~7) + (ld8 ? 0 : 4), ((cout + 7) & ~7) + (ld8 ? 0 : 2), aligned != 0,
                                                           ident != 0, k, ppo * k, cin, cout, ws != 0, bytes[ws]};
                                        for (const WgradKnobs& kn : knobs) check(s, kn);
                                    }
    // the largest pair count the checked entry lets through, with few and with many offsets
    for (int k : ks)
        for (int dtype = 0; dtype < 3; ++dtype) {
            const WgradShape s{dtype, 256, 256, true, false, k, (1 << 30) - 1, 256, 256, true, (size_t)-1};
            for (const WgradKnobs& kn : knobs) check(s, kn);
        }
    // refused shapes never reach the arithmetic
    const WgradShape bad[] = {{3, 8, 8, true, false, 1, 1, 8, 8, false, 0}, {1, 8, 8, true, false, 0, 1, 8, 8, false, 0},
                              {1, 8, 8, true, false, 1, -1, 8, 8, false, 0}, {1, 8, 8, true, true, 2, 1, 8, 8, false, 0},
                              {1, 8, 8, true, false, 1, 1, 0, 8, false, 0}, {1, 8, 8, true, false, 1, 1, 8, 0, false, 0}};
    for (const WgradShape& s : bad)
        if (wgrad_shape_ok(s)) { std::printf("a refused shape passes wgrad_shape_ok\n"); return 1; }
    std::printf("wgrad_plan_walk: %lld plans hold\n", n_checked);
    return 0;
}
