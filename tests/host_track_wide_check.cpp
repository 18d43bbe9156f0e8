// The wide tracking pass on the CPU (sushi_amd/csrc/track_wide_core.hpp): the call's host side -- stage_track_wide's and
// stage_margins_wide's refusals, the workspace's layout -- and its arithmetic: wide_combine, the tile pass and wide_near, held
// against the candidate loop of track_core.hpp (track_price, track_cand, track_replaces over every d), bit for bit.
// usage: host_track_wide_check validate
//          prints "<case> <return code>" for good and bad arguments, then the facts of staged calls.
//        host_track_wide_check near <step_cost> <reach> <row file> <output file>
//          step_cost: float64 as text (a hexadecimal literal keeps its bits; +-0.0); row: raw float64, one row X of n values.
//          near[j] and its move for every j, through wide_near -- divided as the kernels divide the work: per window tile the
//          records scanned as the tile kernel scans them (a thread's four values, a doubling scan over the wave's 64 threads, the
//          four waves' totals), compared with the element-by-element scan; per work item of track_split the whole tiles' records
//          staged into an array of WIDE_ITEM_TILES entries and read from there, the items and their indices taken backwards -- and
//          through the candidate loop; any difference is exit status 4.  The output file holds [near f64 x n][move i16 x n].
//        host_track_wide_check near_only <step_cost> <reach> <row file> <output file>
//          the same without the candidate loop (n x 2 reach candidates: too many on a long axis at the widest reach): the two
//          scans are still compared, and the test holds the output against _near_wide.
//        host_track_wide_check pass <sqdiff|ccoeff> <penalty> <step_cost> <n_shift> <curves file> <rows file> <reach file> <output>
//          host_track_check's pass with stage_track_wide: a row of a reach above TRACK_MAX_REACH through the tile pass and
//          wide_near, every other row through the candidate loop.  The output file holds [shift i32 x E][row_arg i32 x E]
//          [row_min f64 x E][moves i16 x E x n_shift].  The test compares it with sushi_amd.track.track_host(wide=True).
// Built by tests/test_track_wide_host.py with g++ -O2 -std=c++17 -ffp-contract=off -fsanitize=address,undefined.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "../include/sushi_hip.h"
#include "../sushi_amd/csrc/track_wide_core.hpp"
#include "host_check_io.hpp"

namespace {

using host_check::read_file;
using host_check::records;
using namespace sushi;

constexpr int32_t MAX32 = std::numeric_limits<int32_t>::max();
void* const MEM = reinterpret_cast<void*>((uintptr_t)1 << 20);      // aligned, never dereferenced
void* const MEM_ODD = reinterpret_cast<void*>(((uintptr_t)1 << 20) + 128);

struct Call {
    std::vector<SushiHipJointRow> rows;
    std::vector<int32_t> reach, guard;
    int n_rows;
    int32_t n_shift;
    int64_t n_curve;
    int method;
    double penalty, step_cost;
    int row0, n_total;
    const void* mem;
    size_t mem_bytes;
};

// rows 2 .. 4 of a sequence of 7 over 499 shifts, on a buffer of 1000 floats; free moves
Call good() {
    Call c;
    c.rows = {{0, 1.0}, {501, 0.0}, {333, 2.5}};
    c.reach = {0, 32767, 17, 1025};         // (the fourth: the row after the call's last, for a margins call)
    c.guard = {0, 120, 5};
    c.n_rows = 3; c.n_shift = 499; c.n_curve = 1000;
    c.method = SUSHI_HIP_METHOD_SQDIFF_NORMED;
    c.penalty = 0.5; c.step_cost = 0.0;
    c.row0 = 2; c.n_total = 7;
    c.mem = MEM; c.mem_bytes = (size_t)1 << 20;
    return c;
}

void report(const char* name, const Call& c) {
    TrackWideStage ts;
    MarginWideStage ms;
    const int t = stage_track_wide(c.rows.data(), c.reach.data(), c.n_rows, c.n_shift, c.n_curve, c.method, c.penalty, c.step_cost,
                                   c.row0, c.n_total, c.mem, c.mem_bytes, ts);
    const int m = stage_margins_wide(c.rows.data(), c.reach.data(), c.guard.data(), c.n_rows, c.n_shift, c.n_curve, c.method, c.penalty,
                                     c.step_cost, c.row0, c.n_total, c.mem, c.mem_bytes, ms);
    std::printf("%s %d %d\n", name, t, m);
}

int validate() {
    Call c = good();
    report("good", c);
    c = good(); c.step_cost = -0.0; report("step_cost_neg_zero", c);
    c = good(); c.reach = {0, 1024, 1024, 1024}; c.step_cost = 0.25; report("narrow_reaches_with_step_cost", c);
    c = good(); c.reach[1] = 32768; report("reach_32768", c);
    c = good(); c.reach[2] = -1; report("reach_negative", c);
    c = good(); c.reach[1] = MAX32; report("reach_int_max", c);
    c = good(); c.step_cost = 1e-300; report("wide_reach_with_step_cost", c);
    c = good(); c.reach = {0, 1024, 1025, 3}; c.step_cost = 0.001; report("reach_1025_with_step_cost", c);
    // reach[0]: a forward call that continues a sequence uses it, a margins call never does; reach[3]: a margins call that ends below
    // the sequence's last row uses it, a forward call never does
    c = good(); c.reach[0] = 32768; report("first_reach_32768", c);
    c = good(); c.reach[0] = 5000; c.step_cost = 0.5; c.reach[1] = 7; c.reach[3] = 7; report("first_reach_wide_with_step_cost", c);
    c = good(); c.row0 = 0; c.n_total = 3; c.reach[0] = 40000; report("reach_of_row_0_is_ignored", c);
    c = good(); c.reach[3] = 32768; report("reach_after_the_call_32768", c);
    c = good(); c.row0 = 4; c.reach[3] = 32768; report("reach_after_the_sequence_is_ignored", c);
    c = good(); c.reach[3] = 2000; c.reach[1] = 5; c.step_cost = 0.5; report("reach_after_the_call_wide_with_step_cost", c);
    c = good(); c.guard[1] = -1; report("guard_negative", c);
    c = good(); c.penalty = std::nan(""); report("penalty_nan", c);
    c = good(); c.step_cost = -1.0; report("step_cost_negative", c);
    c = good(); c.rows[1].curve_off = 502; report("row_one_past_curves_end", c);
    // the order: a bad reach before the workspace and its alignment
    c = good(); c.reach[1] = 32768; c.mem_bytes = 0; report("reach_32768_before_workspace", c);
    c = good(); c.step_cost = 0.5; c.mem = MEM_ODD; report("wide_reach_with_step_cost_before_alignment", c);
    c = good(); c.mem = MEM_ODD; c.mem_bytes = 0; report("workspace_misaligned_and_short", c);
    c = good(); c.mem_bytes = track_wide_layout_bytes(3, 499); report("workspace_exact_forward", c);
    c = good(); c.mem_bytes = margin_wide_layout_bytes(3, 499); report("workspace_exact_margins", c);
    c = good(); c.mem_bytes = track_wide_layout_bytes(3, 499) - 1; report("workspace_short", c);
    c = good(); c.mem_bytes = track_layout_bytes(3, 499); report("workspace_of_the_plain_call", c);

    std::printf("bytes %zu %zu %zu %zu %zu %zu\n", track_wide_layout_bytes(1, 1), track_wide_layout_bytes(200, 240001),
                track_wide_layout_bytes(16, 2880001), track_wide_layout_bytes(0, 5), track_wide_layout_bytes(5, 0),
                track_wide_layout_bytes(-1, -1));
    std::printf("margin_bytes %zu %zu %zu %zu\n", margin_wide_layout_bytes(1, 1), margin_wide_layout_bytes(200, 240001),
                margin_wide_layout_bytes(0, 5), margin_wide_layout_bytes(5, 0));
    std::printf("tile %d per=%d item_tiles=%d tiles=%lld,%lld,%lld grid=%u,%u\n", WIDE_TILE, WIDE_PER, WIDE_ITEM_TILES,
                (long long)wide_tiles(1), (long long)wide_tiles(1024), (long long)wide_tiles(1025), wide_tile_grid(240001),
                wide_tile_grid(MAX32));
    TrackWideStage ts;
    c = good();
    c.n_shift = 240001; c.n_curve = 1 << 20; c.rows = {{0, 1.0}, {3, 1.0}, {5, 1.0}}; c.mem_bytes = (size_t)1 << 30;
    const int rc = stage_track_wide(c.rows.data(), c.reach.data(), 3, c.n_shift, c.n_curve, c.method, c.penalty, c.step_cost, c.row0,
                                    c.n_total, c.mem, c.mem_bytes, ts);
    std::printf("facts_240001 rc=%d per=%d items=%lld grid=%u plain=%zu records=(%zu,%zu,%zu,%zu) bytes=%zu tile_grid=%u wide_rows=%d\n", rc,
                ts.plain.split.per, (long long)ts.plain.split.n_items, ts.plain.split.grid, ts.plain.lay.bytes, ts.wide.pv, ts.wide.sv,
                ts.wide.pi, ts.wide.si, ts.wide.bytes, ts.tile_grid, ts.n_wide);
    // the most tiles a work item asks for: the widest reach, the largest item, in the middle of a long axis
    long long most = 0;
    for (int64_t base = 0; base < 40 * 2048; base += 2048) {
        const long long count = wide_item_last_tile(base, 2048, 32767, MAX32) - wide_item_first_tile(base, 32767) + 1;
        most = count > most ? count : most;
    }
    std::printf("most_item_tiles %lld\n", most);
    return 0;
}

bool same_bits(double a, double b) { return !std::memcmp(&a, &b, sizeof a); }

// One window tile as the tile kernel scans it; the order of every combine differs from wide_tile_scan's.
void tile_scan_divided(const double* X, int32_t n_shift, int64_t tile, const WideRecords& w) {
    constexpr int T = TRACK_THREADS;
    const int64_t base = tile << WIDE_TILE_BITS;
    std::vector<WideRec> pl((size_t)WIDE_TILE), sl((size_t)WIDE_TILE), up((size_t)T), down((size_t)T), tmp((size_t)T);
    for (int i = 0; i < WIDE_TILE; ++i) pl[(size_t)i] = sl[(size_t)i] = base + i < n_shift ? wide_one(X[base + i], i) : wide_empty();
    for (int t = 0; t < T; ++t) {
        for (int k = 1; k < WIDE_PER; ++k) pl[(size_t)(t * WIDE_PER + k)] = wide_combine(pl[(size_t)(t * WIDE_PER + k - 1)], pl[(size_t)(t * WIDE_PER + k)]);
        for (int k = WIDE_PER - 2; k >= 0; --k) sl[(size_t)(t * WIDE_PER + k)] = wide_combine(sl[(size_t)(t * WIDE_PER + k)], sl[(size_t)(t * WIDE_PER + k + 1)]);
        up[(size_t)t] = pl[(size_t)(t * WIDE_PER + WIDE_PER - 1)];
        down[(size_t)t] = sl[(size_t)(t * WIDE_PER)];
    }
    for (int off = 1; off < 64; off <<= 1) {        // the doubling scans of a wave's 64 threads
        tmp = up;
        for (int t = 0; t < T; ++t) if ((t & 63) >= off) up[(size_t)t] = wide_combine(tmp[(size_t)(t - off)], tmp[(size_t)t]);
        tmp = down;
        for (int t = 0; t < T; ++t) if ((t & 63) + off < 64) down[(size_t)t] = wide_combine(tmp[(size_t)t], tmp[(size_t)(t + off)]);
    }
    for (int t = T - 1; t >= 0; --t) {
        const int wave = t >> 6, lane = t & 63;
        WideRec before = wide_empty(), after = wide_empty();
        for (int q = 0; q < T / 64; ++q) if (q < wave) before = wide_combine(before, up[(size_t)(q * 64 + 63)]);
        for (int q = T / 64 - 1; q >= 0; --q) if (q > wave) after = wide_combine(up[(size_t)(q * 64 + 63)], after);
        const WideRec carry_up = wide_combine(before, lane ? up[(size_t)(t - 1)] : wide_empty());
        const WideRec carry_down = wide_combine(lane < 63 ? down[(size_t)(t + 1)] : wide_empty(), after);
        for (int k = WIDE_PER - 1; k >= 0; --k) {
            const int64_t i = base + t * WIDE_PER + k;
            if (i >= n_shift) continue;
            const WideRec p = wide_combine(carry_up, pl[(size_t)(t * WIDE_PER + k)]), s = wide_combine(sl[(size_t)(t * WIDE_PER + k)], carry_down);
            w.pv[i] = p.v; w.pi[i] = wide_pack(p);
            w.sv[i] = s.v; w.si[i] = wide_pack(s);
        }
    }
}

struct Records {
    std::vector<double> pv, sv;
    std::vector<uint32_t> pi, si;
    explicit Records(int32_t n) : pv((size_t)n), sv((size_t)n), pi((size_t)n), si((size_t)n) {}
    WideRecords view() { return WideRecords{pv.data(), sv.data(), pi.data(), si.data()}; }
};

struct StagedTiles {
    const WideTileRec* s;
    int64_t first, count;
    WideTileRec operator()(int64_t t) const {
        if (t < first || t - first >= count) { std::fprintf(stderr, "a tile outside the staged ones\n"); std::exit(4); }
        return s[t - first];
    }
};

// near and its move for a whole row through the tile pass and wide_near; 0, or 4 where the two scans differ
int wide_row_near(const double* X, int32_t n_shift, int32_t reach, double mu, double* near, int32_t* nd) {
    Records a(n_shift), b(n_shift);
    for (int64_t t = wide_tiles(n_shift) - 1; t >= 0; --t) {
        tile_scan_divided(X, n_shift, t, a.view());
        wide_tile_scan(X, n_shift, t, b.view());
    }
    for (int32_t i = 0; i < n_shift; ++i)
        if (!same_bits(a.pv[(size_t)i], b.pv[(size_t)i]) || !same_bits(a.sv[(size_t)i], b.sv[(size_t)i]) || a.pi[(size_t)i] != b.pi[(size_t)i] ||
            a.si[(size_t)i] != b.si[(size_t)i]) {
            std::fprintf(stderr, "element %d: the divided scan and the element-by-element scan disagree\n", i);
            return 4;
        }
    const PathSplit split = track_split(n_shift);
    const int64_t span = (int64_t)split.per * TRACK_THREADS;
    WideTileRec staged[WIDE_ITEM_TILES];
    for (int64_t item = split.n_items - 1; item >= 0; --item) {
        const int64_t lo = item * span, hi = lo + span < n_shift ? lo + span : n_shift;
        const int64_t t_lo = wide_item_first_tile(lo, reach), t_hi = wide_item_last_tile(lo, span, reach, n_shift);
        if (t_hi - t_lo + 1 > WIDE_ITEM_TILES) { std::fprintf(stderr, "an item asks for %lld tiles\n", (long long)(t_hi - t_lo + 1)); return 4; }
        for (int64_t t = t_lo; t <= t_hi; ++t) {
            const int64_t end = wide_tile_end(t, n_shift);
            staged[t - t_lo] = WideTileRec{a.pv[(size_t)end], a.pi[(size_t)end]};
        }
        const StagedTiles tiles{staged, t_lo, t_hi - t_lo + 1};
        for (int64_t j = hi - 1; j >= lo; --j)
            near[j] = wide_near(X, a.pv.data(), a.sv.data(), a.pi.data(), a.si.data(), tiles, j, n_shift, reach, mu, &nd[j]);
    }
    return 0;
}

// the definition: every candidate, under track_replaces, from the widest move inwards
void loop_row_near(const double* X, int32_t n_shift, int32_t reach, double mu, double* near, int32_t* nd) {
    for (int64_t j = 0; j < n_shift; ++j) {
        double best = X[j]; int32_t bd = 0;
        const int32_t most = reach < n_shift ? reach : n_shift;
        for (int32_t a = most; a >= 1; --a) {
            const double price = track_price(mu, a);
            if (j + a < n_shift) { const double c = track_cand(X[j + a], price); if (track_replaces(c, a, best, bd)) { best = c; bd = a; } }
            if (j - a >= 0) { const double c = track_cand(X[j - a], price); if (track_replaces(c, -a, best, bd)) { best = c; bd = -a; } }
        }
        near[j] = best; nd[j] = bd;
    }
}

int near_mode(bool with_loop, const char* step_text, const char* reach_text, const char* row_path, const char* out_path) {
    const double mu = std::strtod(step_text, nullptr);
    const int32_t reach = (int32_t)std::strtol(reach_text, nullptr, 10);
    const std::vector<double> X = records<double>(read_file(row_path));
    const int32_t n = (int32_t)X.size();
    if (n < 1 || !wide_row(reach) || reach > TRACK_WIDE_MAX_REACH || !wide_step_cost_ok(mu)) { std::fprintf(stderr, "not a wide row\n"); return 3; }
    std::vector<double> near((size_t)n), want((size_t)n);
    std::vector<int32_t> nd((size_t)n), want_d((size_t)n);
    const int rc = wide_row_near(X.data(), n, reach, mu, near.data(), nd.data());
    if (rc) return rc;
    if (with_loop) loop_row_near(X.data(), n, reach, mu, want.data(), want_d.data());
    std::vector<int16_t> words((size_t)n);
    for (int32_t j = 0; j < n; ++j) {
        if (with_loop && (!same_bits(near[(size_t)j], want[(size_t)j]) || nd[(size_t)j] != want_d[(size_t)j])) {
            std::fprintf(stderr, "shift %d: wide_near gives (%a, %d), the candidate loop (%a, %d)\n", j, near[(size_t)j], nd[(size_t)j],
                         want[(size_t)j], want_d[(size_t)j]);
            return 4;
        }
        words[(size_t)j] = (int16_t)nd[(size_t)j];
    }
    using host_check::part;
    return host_check::write_file(out_path, {part(near), part(words)});
}

int pass(const char* method_name, const char* penalty_text, const char* step_text, const char* n_shift_text, const char* curves_path,
         const char* rows_path, const char* reach_path, const char* out_path) {
    const int method = !std::strcmp(method_name, "ccoeff") ? SUSHI_HIP_METHOD_CCOEFF_NORMED : SUSHI_HIP_METHOD_SQDIFF_NORMED;
    const double penalty = std::strtod(penalty_text, nullptr), step_cost = std::strtod(step_text, nullptr);
    const int32_t n_shift = (int32_t)std::strtol(n_shift_text, nullptr, 10);
    const std::vector<float> curves = records<float>(read_file(curves_path));
    const std::vector<SushiHipJointRow> rows = records<SushiHipJointRow>(read_file(rows_path));
    const std::vector<int32_t> reach_of = records<int32_t>(read_file(reach_path));
    const int E = (int)rows.size();
    if ((int)reach_of.size() != E) { std::fprintf(stderr, "as many reaches as rows\n"); return 3; }
    TrackWideStage st;
    const int rc = stage_track_wide(rows.data(), reach_of.data(), E, n_shift, (int64_t)curves.size(), method, penalty, step_cost, 0, E, MEM,
                                    (size_t)1 << 40, st);
    if (rc != SUSHI_HIP_OK) { std::fprintf(stderr, "stage_track_wide refused the call: %d\n", rc); return 3; }
    std::vector<double> D((size_t)2 * n_shift), row_min((size_t)E), near((size_t)n_shift);
    std::vector<int32_t> nd((size_t)n_shift), row_arg((size_t)E), shifts((size_t)E);
    std::vector<int16_t> moves((size_t)E * n_shift, 0);
    for (int e = 0; e < E; ++e) {
        const float* r = curves.data() + rows[(size_t)e].curve_off;
        const double jump = e ? row_min[(size_t)e - 1] + penalty : 0.0;
        const int32_t reach = e ? reach_of[(size_t)e] : 0;
        const double* Din = D.data() + (size_t)((e + 1) & 1) * n_shift;
        double* Dout = D.data() + (size_t)(e & 1) * n_shift;
        if (e) {
            if (wide_row(reach)) {
                const int bad = wide_row_near(Din, n_shift, reach, step_cost, near.data(), nd.data());
                if (bad) return bad;
            } else {
                loop_row_near(Din, n_shift, reach, step_cost, near.data(), nd.data());
            }
        }
        double best = INFINITY; int32_t at = PATH_NO_INDEX;
        for (int64_t j = n_shift - 1; j >= 0; --j) {
            const double u = path_cost(method, rows[(size_t)e].weight, r[j]);
            Dout[j] = e ? track_step(near[(size_t)j], nd[(size_t)j], u, jump, &moves[(size_t)e * n_shift + j]) : u;
            if (path_min_replaces(Dout[j], (int32_t)j, best, at)) { best = Dout[j]; at = (int32_t)j; }
        }
        row_min[(size_t)e] = best; row_arg[(size_t)e] = path_clamp(at, n_shift);
    }
    track_backtrack(moves.data(), row_arg.data(), E, n_shift, shifts.data());
    using host_check::part;
    return host_check::write_file(out_path, {part(shifts), part(row_arg), part(row_min), part(moves)});
}

}  // namespace

int main(int argc, char** argv) {
    if (argc == 2 && !std::strcmp(argv[1], "validate")) return validate();
    if (argc == 6 && !std::strcmp(argv[1], "near")) return near_mode(true, argv[2], argv[3], argv[4], argv[5]);
    if (argc == 6 && !std::strcmp(argv[1], "near_only")) return near_mode(false, argv[2], argv[3], argv[4], argv[5]);
    if (argc == 10 && !std::strcmp(argv[1], "pass")) return pass(argv[2], argv[3], argv[4], argv[5], argv[6], argv[7], argv[8], argv[9]);
    std::fprintf(stderr, "usage: %s validate | near[_only] <step_cost> <reach> <row> <output> | pass <sqdiff|ccoeff> <penalty> <step_cost> "
                 "<n_shift> <curves> <rows> <reach> <output>\n", argv[0]);
    return 2;
}
