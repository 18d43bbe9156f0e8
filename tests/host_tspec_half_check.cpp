// tests/host_tspec_half_check.cpp -- the HALF rows the real route stores of a pattern segment's spectrum (sushi_amd/csrc/fft_core.hpp
// "HALF ROWS"; tspec_real_kernel's stores, every reader's half_fetch, mac_rows_kernel's paired first pass) on the CPU.  Built with
// g++ and run as a program by tests/test_tspec_half_host.py; exit 1 with a message on the first violation.
//
// Whole rows are built that are conjugate-symmetric word for word by the kernel's own rule (real_conj_word), their half rows are
// taken the way tspec_real_kernel stores them, and half_fetch must give back every word of all 4096 entries.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <vector>

#include "../include/sushi_hip.h"
#include "../sushi_amd/csrc/fft_core.hpp"
#include "../sushi_amd/csrc/plan_core.hpp"
#include "../sushi_amd/csrc/run_policy.hpp"

using namespace sushi_fft;

#define REQUIRE(cond, ...) \
    do { \
        if (!(cond)) { fprintf(stderr, "tspec_half: [%s] ", #cond); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); return 1; } \
    } while (0)

struct alignas(16) Entry { unsigned x, y, z, w; };
constexpr int FULL_ENTRIES = RN / 4;
constexpr unsigned UNWRITTEN = 0xdeadbeefu;

static uint64_t g_rng = 0x9e3779b97f4a7c15ull;
static unsigned rnd() { g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17; return (unsigned)(g_rng >> 16); }

// a whole row from the words of bins 0 .. RN/2: bin RN - k is real_conj_word of bin k, bins 0 and RN/2 have a zero imaginary half
static std::vector<unsigned> whole_row(const std::vector<unsigned>& lower) {
    std::vector<unsigned> row(RN);
    for (int f = 0; f <= RN / 2; ++f) row[mslot_of_bin(f)] = (f == 0 || f == RN / 2) ? (lower[f] & 0xffffu) : lower[f];
    for (int f = RN / 2 + 1; f < RN; ++f) row[mslot_of_bin(f)] = real_conj_word(row[mslot_of_bin(RN - f)]);
    return row;
}

// What tspec_real_kernel stores of a whole row, restated: thread t the entries u = 0, 1 of its two rows (thread 0: of row 0 and,
// as row 1024, row 0's own bins 1 .. 7 and bin RN/2), the tail's lanes bins l and 7 - l of row 512.  writes[word] counts.
static int take_half(const std::vector<unsigned>& row, std::vector<unsigned>& half, std::vector<int>& writes) {
    half.assign(4 * HALF_ROWE, UNWRITTEN);
    writes.assign(4 * HALF_ROWE, 0);
    bool outside = false;
    auto put = [&](int word, unsigned v) { if (word >= 0 && word < 4 * HALF_ROWE) { ++writes[word]; half[word] = v; } else outside = true; };
    auto bin = [&](int f) { return row[mslot_of_bin(f)]; };
    for (int t = 0; t < RNT; ++t) {
        const int ra = real_row(t, 0), rb = real_row(t, 1);
        unsigned wa[8], wb[8];
        for (int d = 0; d < 8; ++d) {
            wa[d] = bin(ra + 1024 * d);
            wb[d] = t != 0 ? bin(rb + 1024 * d) : bin(1024 * (d + 1));
        }
        const unsigned x0[4] = {wa[1], wa[2], wa[3], wa[4]}, x1[4] = {wa[5], wa[6], wa[7], wb[7]};
        for (int j = 0; j < 4; ++j) {
            put(4 * half_entry(ra, 0) + j, wa[j]);
            put(4 * half_entry(ra, 1) + j, wa[4 + j]);
            put(4 * half_entry(rb, 0) + j, t != 0 ? wb[j] : x0[j]);
            put(4 * half_entry(rb, 1) + j, t != 0 ? wb[4 + j] : x1[j]);
        }
    }
    for (int l = 0; l < REAL_TAIL_LANES; ++l) {
        put(half_tail_word(l), bin(REAL_TAIL_ROW + 1024 * l));
        put(half_tail_word(7 - l), bin(REAL_TAIL_ROW + 1024 * (7 - l)));
    }
    REQUIRE(!outside, "a store outside the half row");
    return 0;
}

static int check_row(const char* name, const std::vector<unsigned>& lower) {
    const std::vector<unsigned> row = whole_row(lower);
    // (the row is what the kernel's rule makes it: every mirror the conj word of its bin, both ways)
    for (int f = 1; f < RN; ++f)
        REQUIRE(row[mslot_of_bin(RN - f)] == real_conj_word(row[mslot_of_bin(f)]), "%s: bin %d and its mirror", name, f);
    std::vector<unsigned> half;
    std::vector<int> writes;
    if (take_half(row, half, writes)) return 1;
    // every stored entry and both extras are written exactly once, the rest of the extra run never
    for (int h = 0; h < HALF_ROWE; ++h)
        for (int j = 0; j < 4; ++j)
            REQUIRE(writes[4 * h + j] == (h < HALF_STORED + 2 ? 1 : 0), "%s: word %d of half-row entry %d is written %d times", name, j, h, writes[4 * h + j]);
    // the stored entries are the whole row's entries u < 2 as they are
    for (int e = 0; e < FULL_ENTRIES; ++e)
        if ((e & 16) == 0) REQUIRE(memcmp(&half[4 * half_index(e)], &row[4 * e], 16) == 0, "%s: stored entry %d", name, e);
    // every reader's function gives back every word of the whole row
    const Entry* hrow = reinterpret_cast<const Entry*>(half.data());
    for (int e = 0; e < FULL_ENTRIES; ++e) {
        const Entry got = half_fetch(hrow, e);
        REQUIRE(memcmp(&got, &row[4 * e], 16) == 0, "%s: entry %d is %08x %08x %08x %08x, the whole row holds %08x %08x %08x %08x", name, e,
                got.x, got.y, got.z, got.w, row[4 * e], row[4 * e + 1], row[4 * e + 2], row[4 * e + 3]);
    }
    // the paired first pass: a stored entry's words (row 0's two: row 1024's), conj-reversed, are its mirror entry's
    for (int h = 0; h < HALF_STORED; ++h) {
        const int hx = (h & ~16) == 0 ? half_entry(1024, h >> 4) : h;
        const Entry got = real_conjrev(hrow[hx]);
        REQUIRE(memcmp(&got, &row[4 * half_mirror_of(h)], 16) == 0, "%s: the mirror of stored entry %d", name, h);
    }
    return 0;
}

static int check_geometry() {
    REQUIRE(HALF_ROWE == sushi::HROWE && HALF_ROWE * 16 == sushi::HROW_BYTES && (sushi::HROW_BYTES % 256) == 0 && HALF_STORED * 2 == FULL_ENTRIES, "sizes");
    // the entries u >= 2 are those whose index has bit 4 set; real_entry_row inverts real_entry; the half index keeps the order
    std::set<int> places;
    for (int row = 0; row < 1024; ++row)
        for (int u = 0; u < 4; ++u) {
            const int e = real_entry(row, u);
            int r2, u2;
            real_entry_row(e, &r2, &u2);
            REQUIRE(r2 == row && u2 == u, "real_entry_row(%d)", e);
            REQUIRE(((e & 16) != 0) == (u >= 2), "bit 4 of entry (%d, %d)", row, u);
            if (u < 2) {
                const int h = half_entry(row, u);
                REQUIRE(h >= 0 && h < HALF_STORED && half_to_full(h) == e && h == half_index(e), "half_entry(%d, %d)", row, u);
                REQUIRE(places.insert(h).second, "half_entry(%d, %d) twice", row, u);
                REQUIRE(!half_source(e).conjrev && half_source(e).index == h, "half_source of stored entry %d", e);
            }
        }
    REQUIRE(half_entry(1024, 0) == HALF_STORED && half_entry(1024, 1) == HALF_STORED + 1, "row 1024's entries");
    // 16-entry runs of the whole row stay runs of the half row, in order
    for (int e = 0; e < FULL_ENTRIES; e += 16)
        if ((e & 16) == 0) REQUIRE((half_index(e) & 15) == 0 && half_index(e + 15) == half_index(e) + 15, "run at %d", e);
    // sources of the mirrored entries: every stored entry but row 0's two and both of row 1024's, each once
    std::set<int> sources;
    int split_runs = 0;
    for (int run = 0; run < FULL_ENTRIES; run += 16) {
        if ((run & 16) == 0) continue;
        std::set<int> pieces;
        bool reversed = true;
        for (int m = 0; m < 16; ++m) {
            const HalfSource s = half_source(run + m);
            REQUIRE(s.conjrev && s.index >= 0 && s.index < HALF_STORED + 2, "source of entry %d", run + m);
            REQUIRE(sources.insert(s.index).second, "stored entry %d is the source of two entries", s.index);
            pieces.insert(s.index >> 4);
            reversed = reversed && s.index == (half_source(run).index | 15) - m;
        }
        // one whole stored run in reversed order -- but for the runs of the rows f0 = 0 mod 16 (n1 = 0), whose sources are two runs'
        const int n1 = run >> 8;
        if (n1 != 0) REQUIRE(pieces.size() == 1 && reversed && (half_source(run + 15).index & 15) == 0, "run %d: its sources are no whole run reversed", run);
        else { REQUIRE(pieces.size() == 2, "run %d: sources in %d runs", run, (int)pieces.size()); ++split_runs; }
        // the mirrors of part p (256 entries of the whole row) come from part (16 - p) mod 16 (row 1024's two: behind the parts)
        for (int m = 0; m < 16; ++m) {
            const int h = half_source(run + m).index;
            if (h < HALF_STORED) REQUIRE((half_to_full(h) >> 8) == ((16 - n1) & 15), "entry %d: its source's part", run + m);
        }
    }
    REQUIRE(split_runs == 8 && (int)sources.size() == HALF_STORED, "%d split runs, %d sources", split_runs, (int)sources.size());
    REQUIRE(!sources.count(half_entry(0, 0)) && !sources.count(half_entry(0, 1)) && sources.count(half_entry(1024, 0)) && sources.count(half_entry(1024, 1)),
            "row 0 mirrors from row 1024");
    // the paired first pass: the mirrors of the 2048 stored entries are the 2048 other entries, each once; a workgroup's 256
    // stored entries and their mirrors lie in two parts of the whole row each (16 lanes: one run, but for n1 = 0)
    std::set<int> mirrors;
    for (int h = 0; h < HALF_STORED; ++h) {
        const int e = half_mirror_of(h);
        REQUIRE(e >= 0 && e < FULL_ENTRIES && (e & 16) != 0 && mirrors.insert(e).second, "mirror of stored entry %d", h);
        const HalfSource s = half_source(e);
        REQUIRE(s.conjrev && s.index == ((h & ~16) == 0 ? half_entry(1024, h >> 4) : h), "mirror of stored entry %d comes from %d", h, s.index);
    }
    REQUIRE(half_entry(0, 0) == 0 && half_entry(0, 1) == 16, "row 0's two stored entries");
    return 0;
}

static int check_rule() {
    using namespace sushi;
    REQUIRE(tspec_half_rows(tspec_route(nullptr)) && tspec_half_rows(tspec_route("")) && tspec_half_rows(tspec_route("real")), "the real route stores half rows");
    REQUIRE(!tspec_half_rows(tspec_route("complex")), "the complex route stores whole rows");
    REQUIRE(tspec_half_rows(TSPEC_REAL) == tspec_real(TSPEC_REAL) && tspec_half_rows(TSPEC_COMPLEX) == tspec_real(TSPEC_COMPLEX), "the format is the route's");
    // the half rows of a sub-batch fit the room its workspace keeps for the pattern rows on either route
    const int64_t pairs = 1000, segs = 333, searches = 77;
    const WsLayout w = ws_layout(pairs, segs, searches);
    REQUIRE(w.y - w.tspec >= (size_t)segs * HROW_BYTES && HROW_BYTES < ROW_BYTES, "the pattern rows' region");
    return 0;
}

int main() {
    if (check_geometry() || check_rule()) return 1;
    std::vector<unsigned> lower(RN / 2 + 1);
    // an all-zero row
    std::fill(lower.begin(), lower.end(), 0u);
    if (check_row("zeros", lower)) return 1;
    // zero imaginary halves (+0 and -0) under real halves of either sign, zero real halves under imaginary halves of either sign
    for (int f = 0; f <= RN / 2; ++f) {
        const unsigned re = (rnd() & 0x7fffu) | ((f & 1) ? 0x8000u : 0u), im = (rnd() & 0x7fffu) | ((f & 2) ? 0x8000u : 0u);
        switch (f % 5) {
            case 0: lower[f] = re; break;                          // imaginary half +0
            case 1: lower[f] = re | 0x80000000u; break;            // imaginary half -0
            case 2: lower[f] = im << 16; break;                    // real half +0
            case 3: lower[f] = (im << 16) | 0x8000u; break;        // real half -0
            default: lower[f] = re | (im << 16);
        }
    }
    if (check_row("zero_halves", lower)) return 1;
    for (int round = 0; round < 3; ++round) {
        for (int f = 0; f <= RN / 2; ++f) lower[f] = rnd() ^ (rnd() << 16);
        if (check_row("random", lower)) return 1;
    }
    // rows 0 and 512 alone non-zero
    std::fill(lower.begin(), lower.end(), 0u);
    for (int d = 0; d <= 8; ++d) lower[1024 * d] = 0x3c003c00u + (unsigned)d;
    for (int d = 0; d < 8; ++d) lower[512 + 1024 * d] = 0xbc00c000u + (unsigned)d;
    if (check_row("rows_0_and_512", lower)) return 1;
    return 0;
}
