// sushi_hip_track_margins on the CPU (sushi_amd/csrc/track_margin_core.hpp): the call's host side -- stage_margins' refusals and the
// workspace's layout -- and its arithmetic: track_price, track_cand, margin_back, margin_through, margin_suffix, margin_outside and
// the first-minimum rule, over whole sequences.
// usage: host_track_margins_check validate
//          prints "<case> <return code>" for good and bad arguments, then the facts of staged calls.
//        host_track_margins_check pass <sqdiff|ccoeff> <penalty> <step_cost> <n_shift> <curves file> <rows file> <reach file>
//                                      <guard file> <output file>
//          penalty, step_cost: float64 as text (a hexadecimal literal keeps its bits); curves: raw float32; rows: SushiHipJointRow
//          records, one sequence in event order; reach, guard: int32, one per row.  The forward pass is run plainly (its division is
//          tests/host_track_check.cpp's subject) with every row of D kept, then the backtrack, then the margins pass divided as the
//          kernel divides it: the axis into the work items of track_split, the items onto its workgroups, every item's values of
//          C_{e+1} and its halo staged into a tile (indices outside the axis moved onto an element inside it, and left out by a
//          select), C in two halves, one partial record of three first minima per workgroup -- with every order the device leaves
//          open taken BACKWARDS (a workgroup's items, an item's indices, the partial records), so the rule that makes the result
//          independent of the order is what is checked.  The sequence is walked in two calls where it has more than two rows (the
//          second continues from c_min and the C halves, as a later call does).  The output file holds [through f64 x E][best f64 x E]
//          [alt f64 x E][c_min f64 x E][best_arg i32 x E][alt_arg i32 x E][shift i32 x E][M f64 x E x n_shift][D f64 x E x n_shift].
//          The test compares it with sushi_amd.track.track_margins_host, bit for bit.
// Built by tests/test_track_margins_host.py with g++ -O2 -std=c++17 -ffp-contract=off -fsanitize=address,undefined.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "../include/sushi_hip.h"
#include "../sushi_amd/csrc/track_margin_core.hpp"
#include "host_check_io.hpp"

namespace {

using host_check::read_file;
using host_check::records;
using sushi::MarginStage;

constexpr int64_t MAX64 = std::numeric_limits<int64_t>::max();
constexpr int32_t MAX32 = std::numeric_limits<int32_t>::max();
void* const MEM = reinterpret_cast<void*>((uintptr_t)1 << 20);      // aligned, never dereferenced

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
    bool null_rows, null_reach, null_guard;
};

// rows 2 .. 4 of a sequence of 7 over 499 shifts, on a buffer of 1000 floats; the reach table carries row 5's
Call good() {
    Call c;
    c.rows = {{0, 1.0}, {501, 0.0}, {333, 2.5}};
    c.reach = {9999, 1024, 17, 3};
    c.guard = {0, 120, MAX32};
    c.n_rows = 3; c.n_shift = 499; c.n_curve = 1000;
    c.method = SUSHI_HIP_METHOD_SQDIFF_NORMED;
    c.penalty = 0.5; c.step_cost = 0.001;
    c.row0 = 2; c.n_total = 7;
    c.mem = MEM; c.mem_bytes = 1 << 20;
    c.null_rows = c.null_reach = c.null_guard = false;
    return c;
}

int stage(const Call& c, MarginStage& st) {
    return sushi::stage_margins(c.null_rows ? nullptr : c.rows.data(), c.null_reach ? nullptr : c.reach.data(),
                                c.null_guard ? nullptr : c.guard.data(), c.n_rows, c.n_shift, c.n_curve, c.method, c.penalty,
                                c.step_cost, c.row0, c.n_total, c.mem, c.mem_bytes, st);
}

void report(const char* name, const Call& c) {
    MarginStage st;
    std::printf("%s %d\n", name, stage(c, st));
}

void facts(const char* name, int32_t n_shift) {
    Call c = good();
    c.rows = {{0, 1.0}};
    c.reach = {0};
    c.guard = {0};
    c.n_rows = 1; c.row0 = 0; c.n_total = 1; c.n_shift = n_shift; c.n_curve = MAX64;
    MarginStage st;
    const int rc = stage(c, st);
    std::printf("%s rc=%d", name, rc);
    if (rc == SUSHI_HIP_OK)
        std::printf(" per=%d items=%lld grid=%u first=%d set=%zu bytes=%zu offsets=(%zu,%zu,%zu,%zu,%zu,%zu)", st.split.per,
                    (long long)st.split.n_items, st.split.grid, (int)st.first_call, st.lay.set_bytes, st.lay.bytes, st.lay.c_min,
                    st.lay.m_min, st.lay.a_min, st.lay.c_arg, st.lay.m_arg, st.lay.a_arg);
    std::printf("\n");
}

int validate() {
    Call c = good();
    report("good", c);
    c = good(); c.method = SUSHI_HIP_METHOD_CCOEFF_NORMED; report("good_ccoeff", c);
    c = good(); c.null_rows = true; report("null_rows", c);
    c = good(); c.null_reach = true; report("null_reach", c);
    c = good(); c.null_guard = true; report("null_guard", c);
    c = good(); c.mem = nullptr; report("null_mem", c);
    c = good(); c.method = 2; report("method_2", c);
    c = good(); c.n_rows = 0; report("no_rows", c);
    c = good(); c.n_shift = 0; report("no_shift", c);
    c = good(); c.n_curve = 0; report("empty_curves", c);
    c = good(); c.n_shift = 1001; report("shift_beyond_curves", c);
    // the rows inside the sequence
    c = good(); c.row0 = 0; c.n_total = 3; c.reach.pop_back(); report("whole_sequence", c);
    c = good(); c.row0 = 4; c.reach.pop_back(); report("rows_end_at_sequence_end", c);
    c = good(); c.row0 = 5; report("rows_past_sequence_end", c);
    c = good(); c.row0 = -1; report("row0_negative", c);
    c = good(); c.row0 = 7; report("row0_at_end", c);
    c = good(); c.n_total = 0; report("no_total", c);
    c = good(); c.row0 = MAX32 - 3; c.n_total = MAX32; c.reach.pop_back(); report("rows_end_at_int_max", c);
    c = good(); c.row0 = MAX32 - 2; c.n_total = MAX32; report("rows_sum_overflows_int", c);
    // the rows inside the curve buffer; sums that do not fit 64 bits are never formed
    c = good(); c.rows[0].curve_off = -1; report("row_before_curves", c);
    c = good(); c.rows[1].curve_off = 501; report("row_ends_at_curves_end", c);
    c = good(); c.rows[1].curve_off = 502; report("row_one_past_curves_end", c);
    c = good(); c.rows[2].curve_off = MAX64 - 498; report("row_sum_overflows", c);
    c = good(); c.rows[1].weight = std::nan(""); report("weight_nan", c);
    c = good(); c.rows[1].weight = -1e-300; report("weight_negative", c);
    c = good(); c.penalty = std::nan(""); report("penalty_nan", c);
    c = good(); c.penalty = -1e-300; report("penalty_negative", c);
    c = good(); c.step_cost = INFINITY; report("step_cost_inf", c);
    c = good(); c.step_cost = -1e-300; report("step_cost_negative", c);
    // the reach: entry 0 is not used; entries 1 .. n_rows are, the last only where the call ends before the sequence's last row
    c = good(); c.reach[0] = -5; report("reach_of_the_calls_first_row_is_ignored", c);
    c = good(); c.reach[1] = 1025; report("reach_1025", c);
    c = good(); c.reach[2] = -1; report("reach_negative", c);
    c = good(); c.reach[3] = 1025; report("reach_of_the_row_after_the_call", c);
    c = good(); c.reach[3] = -1; report("negative_reach_of_the_row_after_the_call", c);
    c = good(); c.row0 = 4; c.reach[3] = 1025; report("no_row_after_the_call_its_entry_is_not_read", c);
    c = good(); c.reach = {1024, 1024, 1024, 1024}; report("reach_all_widest", c);
    // the guard: >= 0 in every row
    c = good(); c.guard[0] = -1; report("guard_negative", c);
    c = good(); c.guard[2] = std::numeric_limits<int32_t>::min(); report("guard_int_min", c);
    c = good(); c.guard = {0, 0, 0}; report("guard_zero", c);
    // the workspace: one partial record of 36 bytes per set, each set padded to 256
    c = good(); c.mem_bytes = 512; report("workspace_exact", c);
    c = good(); c.mem_bytes = 511; report("workspace_short", c);
    c = good(); c.mem_bytes = 0; report("workspace_none", c);
    c = good(); c.mem = reinterpret_cast<void*>(((uintptr_t)1 << 20) + 128); report("workspace_misaligned", c);
    c = good(); c.mem = reinterpret_cast<void*>(((uintptr_t)1 << 20) + 128); c.mem_bytes = 0; report("workspace_misaligned_and_short", c);
    c = good(); c.guard[1] = -1; c.mem_bytes = 0; report("bad_guard_before_workspace", c);
    c = good(); c.reach[3] = 1025; c.mem = reinterpret_cast<void*>(((uintptr_t)1 << 20) + 128); report("bad_reach_before_alignment", c);

    std::printf("bytes %zu %zu %zu %zu %zu %zu %zu\n", sushi::margin_layout_bytes(1, 1), sushi::margin_layout_bytes(7, 513),
                sushi::margin_layout_bytes(200, 240001), sushi::margin_layout_bytes(1, MAX32), sushi::margin_layout_bytes(0, 5),
                sushi::margin_layout_bytes(5, 0), sushi::margin_layout_bytes(-1, -1));
    std::printf("outside %d %d %d %d %d %d %d\n", (int)sushi::margin_outside(5, 5, 0), (int)sushi::margin_outside(4, 5, 0),
                (int)sushi::margin_outside(6, 5, 0), (int)sushi::margin_outside(0, MAX32 - 1, MAX32), (int)sushi::margin_outside(MAX32 - 1, 0, MAX32),
                (int)sushi::margin_outside(125, 5, 120), (int)sushi::margin_outside(126, 5, 120));
    facts("facts_one", 1);
    facts("facts_513", 513);
    facts("facts_240001", 240001);
    facts("facts_int32_max", MAX32);
    return 0;
}

struct Min { double v; int32_t i; };
void meet(Min& m, double v, int32_t i) { if (sushi::path_min_replaces(v, i, m.v, m.i)) { m.v = v; m.i = i; } }

int pass(const char* method_name, const char* penalty_text, const char* step_text, const char* n_shift_text, const char* curves_path,
         const char* rows_path, const char* reach_path, const char* guard_path, const char* out_path) {
    const int method = !std::strcmp(method_name, "ccoeff") ? SUSHI_HIP_METHOD_CCOEFF_NORMED : SUSHI_HIP_METHOD_SQDIFF_NORMED;
    const double penalty = std::strtod(penalty_text, nullptr), step_cost = std::strtod(step_text, nullptr);
    const int32_t n_shift = (int32_t)std::strtol(n_shift_text, nullptr, 10);
    const std::vector<float> curves = records<float>(read_file(curves_path));
    const std::vector<SushiHipJointRow> rows = records<SushiHipJointRow>(read_file(rows_path));
    const std::vector<int32_t> reach_of = records<int32_t>(read_file(reach_path));
    const std::vector<int32_t> guard_of = records<int32_t>(read_file(guard_path));
    const int E = (int)rows.size();
    if ((int)reach_of.size() != E || (int)guard_of.size() != E) { std::fprintf(stderr, "as many reaches and guards as rows\n"); return 3; }
    sushi::TrackStage fwd;
    if (sushi::stage_track(rows.data(), reach_of.data(), E, n_shift, (int64_t)curves.size(), method, penalty, step_cost, 0, E, MEM,
                           (size_t)1 << 30, fwd) != SUSHI_HIP_OK) { std::fprintf(stderr, "stage_track refused the call\n"); return 3; }
    // ---- the forward pass, every row of D kept, and the backtrack
    const size_t n = (size_t)n_shift;
    std::vector<double> D((size_t)E * n), row_min((size_t)E);
    std::vector<int16_t> moves((size_t)E * n, 0);
    std::vector<int32_t> row_arg((size_t)E), shifts((size_t)E);
    for (int e = 0; e < E; ++e) {
        const float* r = curves.data() + rows[(size_t)e].curve_off;
        const double jump = e ? row_min[(size_t)e - 1] + penalty : 0.0;
        const int32_t reach = e ? reach_of[(size_t)e] : 0;
        Min best = {INFINITY, sushi::PATH_NO_INDEX};
        for (int64_t j = 0; j < n_shift; ++j) {
            const double u = sushi::path_cost(method, rows[(size_t)e].weight, r[j]);
            double dn = u;
            if (e) {
                const double* prev = D.data() + (size_t)(e - 1) * n;
                double near = prev[j]; int32_t nd = 0;
                for (int32_t a = 1; a <= reach; ++a) {
                    const double price = sushi::track_price(step_cost, a);
                    if (j - a >= 0) { const double v = sushi::track_cand(prev[j - a], price); if (sushi::track_replaces_in_order(v, near)) { near = v; nd = -a; } }
                    if (j + a < n_shift) { const double v = sushi::track_cand(prev[j + a], price); if (sushi::track_replaces_in_order(v, near)) { near = v; nd = a; } }
                }
                dn = sushi::track_step(near, nd, u, jump, &moves[(size_t)e * n + (size_t)j]);
            }
            D[(size_t)e * n + (size_t)j] = dn;
            meet(best, dn, (int32_t)j);
        }
        row_min[(size_t)e] = best.v; row_arg[(size_t)e] = sushi::path_clamp(best.i, n_shift);
    }
    sushi::track_backtrack(moves.data(), row_arg.data(), E, n_shift, shifts.data());

    // ---- the margins pass, in two calls where the sequence has more than two rows
    std::vector<double> C(2 * n), M((size_t)E * n), through((size_t)E), best_v((size_t)E), alt_v((size_t)E), c_min((size_t)E), tile;
    std::vector<int32_t> best_arg((size_t)E), alt_arg((size_t)E);
    const int cut = E > 2 ? E / 2 : 0;                                  // the second call walks rows cut - 1 .. 0
    const int firsts[2] = {cut, 0}, counts[2] = {E - cut, cut};
    for (int call = 0; call < 2; ++call) {
        const int row0 = firsts[call], n_rows = counts[call];
        if (n_rows < 1) continue;
        MarginStage st;
        const int rc = sushi::stage_margins(rows.data() + row0, reach_of.data() + row0, guard_of.data() + row0, n_rows, n_shift,
                                            (int64_t)curves.size(), method, penalty, step_cost, row0, E, MEM, (size_t)1 << 30, st);
        if (rc != SUSHI_HIP_OK) { std::fprintf(stderr, "stage_margins refused the call: %d\n", rc); return 3; }
        if (st.first_call != (row0 + n_rows == E)) { std::fprintf(stderr, "first_call is wrong\n"); return 4; }
        const int64_t span = (int64_t)st.split.per * sushi::TRACK_THREADS;
        const int grid = (int)st.split.grid;
        std::vector<Min> p_c((size_t)grid), p_m((size_t)grid), p_a((size_t)grid);
        for (int i = n_rows - 1; i >= 0; --i) {
            const int e = row0 + i;
            const bool last = e == E - 1;
            const float* r = curves.data() + rows[(size_t)e].curve_off;
            const int32_t reach = sushi::margin_reach_after(reach_of.data() + row0, i, n_rows, st.first_call);
            if (sushi::track_halo_rounds(reach) * sushi::TRACK_THREADS < 2 * reach) { std::fprintf(stderr, "halo rounds too few\n"); return 3; }
            const double jump = last ? 0.0 : c_min[(size_t)e + 1] + penalty;
            const double* Cin = C.data() + (size_t)((e + 1) & 1) * n;
            double* Cout = C.data() + (size_t)(e & 1) * n;
            const int32_t s_e = shifts[(size_t)e], guard = guard_of[(size_t)e];
            for (int b = grid - 1; b >= 0; --b) {                          // one partial record per workgroup
                Min bc = {INFINITY, sushi::PATH_NO_INDEX}, bm = bc, ba = bc;
                int64_t last_item = b;
                while (last_item + grid < st.split.n_items) last_item += grid;
                for (int64_t item = last_item; item >= b; item -= grid) {
                    const int64_t lo = item * span, hi = lo + span < n_shift ? lo + span : n_shift;
                    tile.assign((size_t)(span + 2 * reach), 0.0);
                    if (!last)
                        for (int64_t l = span + 2 * (int64_t)reach - 1; l >= 0; --l) {
                            int64_t g = lo - reach + l;
                            g = g < 0 ? 0 : g;
                            tile[(size_t)l] = Cin[sushi::axis_at(g, n_shift)];
                        }
                    for (int64_t j = hi - 1; j >= lo; --j) {
                        const int64_t l = reach + (j - lo);
                        double near = tile[(size_t)l];
                        for (int32_t a = 1; a <= reach; ++a) {
                            const double price = sushi::track_price(step_cost, a);
                            const double c_lo = sushi::track_cand(tile[(size_t)(l - a)], price);
                            if (j - a >= 0 && sushi::track_replaces_in_order(c_lo, near)) near = c_lo;
                            const double c_hi = sushi::track_cand(tile[(size_t)(l + a)], price);
                            if (j + a < n_shift && sushi::track_replaces_in_order(c_hi, near)) near = c_hi;
                        }
                        const double u = sushi::path_cost(method, rows[(size_t)e].weight, r[j]);
                        const double bk = sushi::margin_back(near, jump);
                        const double m = sushi::margin_through(D[(size_t)e * n + (size_t)j], bk, last);
                        const double cn = sushi::margin_suffix(u, bk, last);
                        Cout[j] = cn;
                        M[(size_t)e * n + (size_t)j] = m;
                        if (j == s_e) through[(size_t)e] = m;
                        meet(bc, cn, (int32_t)j);
                        meet(bm, m, (int32_t)j);
                        if (sushi::margin_outside(j, s_e, guard)) meet(ba, m, (int32_t)j);
                    }
                }
                p_c[(size_t)b] = bc; p_m[(size_t)b] = bm; p_a[(size_t)b] = ba;
            }
            Min bc = {INFINITY, sushi::PATH_NO_INDEX}, bm = bc, ba = bc;
            for (int b = grid - 1; b >= 0; --b) {
                meet(bc, p_c[(size_t)b].v, p_c[(size_t)b].i); meet(bm, p_m[(size_t)b].v, p_m[(size_t)b].i); meet(ba, p_a[(size_t)b].v, p_a[(size_t)b].i);
            }
            c_min[(size_t)e] = bc.v;
            best_v[(size_t)e] = bm.v; best_arg[(size_t)e] = sushi::path_clamp(bm.i, n_shift);
            alt_v[(size_t)e] = ba.i == sushi::PATH_NO_INDEX ? INFINITY : ba.v; alt_arg[(size_t)e] = sushi::margin_alt_index(ba.i, n_shift);
        }
    }
    using host_check::part;
    return host_check::write_file(out_path, {part(through), part(best_v), part(alt_v), part(c_min), part(best_arg), part(alt_arg),
                                             part(shifts), part(M), part(D)});
}

}  // namespace

int main(int argc, char** argv) {
    if (argc == 2 && !std::strcmp(argv[1], "validate")) return validate();
    if (argc == 11 && !std::strcmp(argv[1], "pass"))
        return pass(argv[2], argv[3], argv[4], argv[5], argv[6], argv[7], argv[8], argv[9], argv[10]);
    std::fprintf(stderr, "usage: %s validate | pass <sqdiff|ccoeff> <penalty> <step_cost> <n_shift> <curves> <rows> <reach> <guard> <output>\n",
                 argv[0]);
    return 2;
}
