// tests/host_second_look_check.cpp -- the index rules two of the pair exclusion's small passes stand on, on the CPU:
//   * the second look (bound_low_exact_kernel) reads a low row as the input of Plan<13> BY REGISTER INDEX: for every thread and
//     register, "in the band" under the run-time rule of the body before it (in_index on the N/2 grid below N/8 or from 3N/8 on) is
//     sl_in_band of the register alone, the word the register loads is lslot_of_bin of its bin, and that word is sub-position
//     sl_sub of the 16-byte entry sl_entry -- a thread's eight band registers are two entries;
//   * the pair bound's window energies (slb_kernel): for a wave a pair and for a group of sixteen lanes a pair, the stretches the
//     lanes look up cover the pair's stretches exactly once, and what lies beyond them is past the last stretch (masked).
// usage: host_second_look_check        exit 1 with a message on the first violation
// Built with plain g++ (tests/test_second_look_host.py), no HIP; sushi_fft.hip includes the same headers.
#include <stdio.h>

#include <vector>

#include "../include/sushi_hip.h"
#include "../sushi_amd/csrc/fft_core.hpp"
#include "../sushi_amd/csrc/run_policy.hpp"
#include "../sushi_amd/csrc/sushi_geometry.hpp"

#define REQUIRE(cond, ...)                                                                                          \
    do {                                                                                                            \
        if (!(cond)) { fprintf(stderr, "second look: [%s] ", #cond); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); return 1; } \
    } while (0)

static int band_by_register() {
    using namespace sushi_fft;
    constexpr int LOGN = 13, N = Plan<LOGN>::N, NT = Plan<LOGN>::NT, FN = sushi::FFT_N;
    static_assert(2 * N == FN && NT * PER == N, "the low band sampled at every second position, sixteen points a thread");
    std::vector<int> seen((size_t)LB_BINS, 0);
    int in_band_registers = 0;
    for (int r = 0; r < PER; ++r) in_band_registers += sl_in_band(r) ? 1 : 0;
    REQUIRE(in_band_registers == 8, "%d registers in the band", in_band_registers);
    for (int tid = 0; tid < NT; ++tid) {
        for (int r = 0; r < PER; ++r) {
            // the run-time rule, as bound_low_exact_plain_kernel states it
            const int kin = in_index<LOGN>(tid, r);
            const bool in_band = kin < FN / 8 || kin >= 3 * FN / 8;
            REQUIRE(in_band == sl_in_band(r), "thread %d register %d: index %d", tid, r, kin);
            REQUIRE((kin == 0) == (tid == 0 && r == 0), "bin 0 is register 0 of thread 0: thread %d register %d", tid, r);
            if (!in_band) continue;
            const int bin = kin < FN / 8 ? kin : kin + FN / 2;
            const int word = lslot_of_bin(bin);                 // the word the body before loads
            REQUIRE(word >= 0 && word < LB_BINS, "thread %d register %d: word %d", tid, r, word);
            const int entry = sl_entry(tid, r >> 3), sub = sl_sub(r);
            REQUIRE(sub >= 0 && sub < 4 && entry >= 0 && entry < LB_ENTRIES, "thread %d register %d: entry %d sub %d", tid, r, entry, sub);
            REQUIRE(entry * 4 + sub == word, "thread %d register %d: entry %d sub %d, word %d", tid, r, entry, sub, word);
            REQUIRE(lb_bin_of(entry, sub) == bin, "thread %d register %d: bin %d", tid, r, bin);
            ++seen[(size_t)word];
        }
    }
    for (int w = 0; w < LB_BINS; ++w) REQUIRE(seen[(size_t)w] == 1, "word %d of a low row is loaded %d times", w, seen[(size_t)w]);
    return 0;
}

static int stretches_by_group() {
    using namespace sushi;
    REQUIRE(SLB_STRETCHES == 96, "%d stretches a pair", SLB_STRETCHES);
    for (int group : {64, 16}) {
        const int a_lane = slb_stretches_a_lane(group);
        REQUIRE(a_lane == (group == 64 ? 2 : 6), "group %d: %d stretches a lane", group, a_lane);
        std::vector<int> seen((size_t)SLB_STRETCHES, 0);
        for (int lane = 0; lane < group; ++lane) {
            for (int t = 0; t < a_lane; ++t) {
                const int sb = slb_stretch(lane, t, group);
                REQUIRE(sb >= 0, "group %d lane %d: stretch %d", group, lane, sb);
                if (sb < SLB_STRETCHES) ++seen[(size_t)sb];     // (the kernel's mask: sb < NSB)
                else REQUIRE(group == 64 && t == 1, "group %d lane %d: stretch %d beyond the pair", group, lane, sb);
            }
        }
        for (int sb = 0; sb < SLB_STRETCHES; ++sb)
            REQUIRE(seen[(size_t)sb] == 1, "group %d: stretch %d is looked up %d times", group, sb, seen[(size_t)sb]);
    }
    return 0;
}

static int routes() {
    using namespace sushi;
    REQUIRE(slb_route(nullptr) == SLB_BY_GROUP && slb_route("") == SLB_BY_GROUP && slb_route("group") == SLB_BY_GROUP, "the default");
    REQUIRE(slb_route("wave") == SLB_BY_WAVE && slb_by_wave(SLB_BY_WAVE) && !slb_by_wave(SLB_BY_GROUP), "a wave a pair");
    REQUIRE(second_look_route(nullptr) == SECOND_LOOK_AHEAD && second_look_route("") == SECOND_LOOK_AHEAD &&
            second_look_route("ahead") == SECOND_LOOK_AHEAD, "the default");
    REQUIRE(second_look_route("plain") == SECOND_LOOK_PLAIN && second_look_plain(SECOND_LOOK_PLAIN) && !second_look_plain(SECOND_LOOK_AHEAD),
            "the body before");
    // a value that names neither route is refused: an A/B run must not become an A/A run by a typo
    for (const char* bad : {"Wave", "wave ", " wave", "waves", "0", "1", "plain", "list"}) REQUIRE(slb_route(bad) < 0, "%s", bad);
    for (const char* bad : {"Plain", "plain ", " plain", "0", "1", "wave", "old"}) REQUIRE(second_look_route(bad) < 0, "%s", bad);
    REQUIRE(SLB_BY_GROUP == 0 && SECOND_LOOK_AHEAD == 0, "a zeroed handle takes the defaults");
    return 0;
}

int main() {
    if (band_by_register() || stretches_by_group() || routes()) return 1;
    return 0;
}
