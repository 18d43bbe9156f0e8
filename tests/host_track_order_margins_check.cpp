// sushi_hip_track_order_margins on the CPU (sushi_amd/csrc/track_order_margin_core.hpp): the call's host side --
// stage_order_margins' refusals and the workspace's layout -- and its arithmetic: track_core.hpp's candidates, margin_back /
// margin_through / margin_suffix / margin_outside with order_margin_from, order_margin_jump, order_combine over the items' records and
// order_suffix_combine inside an item, over whole sequences.
// usage: host_track_order_margins_check validate
//          prints "<case> <return code>" for good and bad arguments, then the facts of staged calls.
//        host_track_order_margins_check pass <sqdiff|ccoeff> <step_cost> <n_shift> <split> <curves file> <rows file> <reach file>
//                                            <back file> <penalty file> <guard file> <D file> <shifts file> <output file>
//          step_cost: float64 as text (a hexadecimal literal keeps its bits); curves: raw float32; rows: SushiHipJointRow records,
//          one sequence in event order; reach, back, guard: int32, one per row; penalty: float64, one per row; D: float64 [E][n_shift],
//          the ordered forward pass's rows; shifts: int32, the backtrack's output.  The walk is done in two backward calls, rows
//          split .. E - 1 and then rows 0 .. split - 1 (one call where split is 0), each staged by stage_order_margins from tables cut
//          as the entry point takes them, the second continuing from C and S as the first left them.  A call is divided as the
//          kernels divide it: the axis into the work items of the staged split, the items dealt to the grid's workgroups, three
//          first minima per workgroup, one (min, first index) record per item, an exclusive suffix scan of those records, and inside
//          an item waves of 64 indices -- but the orders the device leaves open are taken another way here (an item's record is
//          folded from its first index up, the scan of the records folds from the last item down one at a time, a wave's suffix is
//          folded from its last lane down, the totals behind a wave are folded left to right), so the rules that make the result
//          independent of the grouping are what is checked.  The output file holds [through f64 x E][best f64 x E][alt f64 x E]
//          [c_min f64 x E][best_arg i32 x E][alt_arg i32 x E][M f64 x E x n_shift][C f64 x 2 x n_shift][S f64 x n_shift].  The test
//          compares it with sushi_amd.track.track_ordered_margins_host, bit for bit.
// Built by tests/test_track_order_margins_host.py with g++ -O2 -std=c++17 -ffp-contract=off -fsanitize=address,undefined.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "../include/sushi_hip.h"
#include "../sushi_amd/csrc/track_order_margin_core.hpp"
#include "host_check_io.hpp"

namespace {

using host_check::read_file;
using host_check::records;
using sushi::OrderMarginStage;
using sushi::OrderMin;

constexpr int64_t MAX64 = std::numeric_limits<int64_t>::max();
constexpr int32_t MAX32 = std::numeric_limits<int32_t>::max();
void* const MEM = reinterpret_cast<void*>((uintptr_t)1 << 20);      // aligned, never dereferenced

struct Call {
    std::vector<SushiHipJointRow> rows;
    std::vector<int32_t> reach, back, guard;
    std::vector<double> penalty;
    int n_rows;
    int32_t n_shift;
    int64_t n_curve;
    int method;
    double step_cost;
    int row0, n_total;
    const void* mem;
    size_t mem_bytes;
    bool null_rows, null_reach, null_back, null_penalty, null_guard;
};

// rows 2 .. 4 of a sequence of 7 over 499 shifts, on a buffer of 1000 floats: entry 3 of reach, back and penalty is row 5's
Call good() {
    Call c;
    c.rows = {{0, 1.0}, {501, 0.0}, {333, 2.5}};
    c.reach = {0, 1024, 17, 3};
    c.back = {0, -1, 600, 0};
    c.penalty = {0.5, 0.0, 1e300, 0.25};
    c.guard = {0, 120, MAX32};
    c.n_rows = 3; c.n_shift = 499; c.n_curve = 1000;
    c.method = SUSHI_HIP_METHOD_SQDIFF_NORMED;
    c.step_cost = 0.001;
    c.row0 = 2; c.n_total = 7;
    c.mem = MEM; c.mem_bytes = 1 << 20;
    c.null_rows = c.null_reach = c.null_back = c.null_penalty = c.null_guard = false;
    return c;
}

int stage(const Call& c, OrderMarginStage& st) {
    return sushi::stage_order_margins(c.null_rows ? nullptr : c.rows.data(), c.null_reach ? nullptr : c.reach.data(),
                                      c.null_back ? nullptr : c.back.data(), c.null_penalty ? nullptr : c.penalty.data(),
                                      c.null_guard ? nullptr : c.guard.data(), c.n_rows, c.n_shift, c.n_curve, c.method, c.step_cost,
                                      c.row0, c.n_total, c.mem, c.mem_bytes, st);
}

void report(const char* name, const Call& c) {
    OrderMarginStage st;
    std::printf("%s %d\n", name, stage(c, st));
}

void facts(const char* name, int32_t n_shift) {
    Call c = good();
    c.rows = {{0, 1.0}};
    c.reach = {0}; c.back = {-1}; c.penalty = {0.0}; c.guard = {0};
    c.n_rows = 1; c.row0 = 0; c.n_total = 1; c.n_shift = n_shift; c.n_curve = MAX64;
    c.mem_bytes = (size_t)1 << 40;
    OrderMarginStage st;
    const int rc = stage(c, st);
    std::printf("%s rc=%d", name, rc);
    if (rc == SUSHI_HIP_OK)
        std::printf(" per=%d items=%lld grid=%u first=%d set=%zu offsets=(%zu,%zu,%zu) bytes=%zu", st.split.per,
                    (long long)st.split.n_items, st.split.grid, (int)st.first_call, st.lay.partials.set_bytes, st.lay.item_min,
                    st.lay.item_arg, st.lay.after_min, st.lay.bytes);
    std::printf("\n");
}

int validate() {
    Call c = good();
    report("good", c);
    c = good(); c.method = SUSHI_HIP_METHOD_CCOEFF_NORMED; report("good_ccoeff", c);
    // what stage_margins refuses
    c = good(); c.null_rows = true; report("null_rows", c);
    c = good(); c.null_reach = true; report("null_reach", c);
    c = good(); c.null_guard = true; report("null_guard", c);
    c = good(); c.mem = nullptr; report("null_mem", c);
    c = good(); c.method = 2; report("method_2", c);
    c = good(); c.n_rows = 0; report("no_rows", c);
    c = good(); c.n_shift = 0; report("no_shift", c);
    c = good(); c.n_curve = 0; report("empty_curves", c);
    c = good(); c.n_shift = 1001; report("shift_beyond_curves", c);
    c = good(); c.row0 = 4; report("rows_end_at_sequence_end", c);
    c = good(); c.row0 = 5; report("rows_past_sequence_end", c);
    c = good(); c.row0 = -1; report("row0_negative", c);
    c = good(); c.n_total = 0; report("no_total", c);
    c = good(); c.row0 = MAX32 - 2; c.n_total = MAX32; report("rows_sum_overflows_int", c);
    c = good(); c.rows[1].curve_off = 501; report("row_ends_at_curves_end", c);
    c = good(); c.rows[1].curve_off = 502; report("row_one_past_curves_end", c);
    c = good(); c.rows[2].curve_off = MAX64; report("row_at_int64_max", c);
    c = good(); c.rows[1].weight = std::nan(""); report("weight_nan", c);
    c = good(); c.rows[1].weight = -1e-300; report("weight_negative", c);
    c = good(); c.step_cost = std::nan(""); report("step_cost_nan", c);
    c = good(); c.step_cost = -1e-300; report("step_cost_negative", c);
    c = good(); c.reach[1] = 1025; report("reach_1025", c);
    c = good(); c.reach[2] = -1; report("reach_negative", c);
    c = good(); c.reach[0] = 1025; report("reach_entry_0_is_ignored", c);
    c = good(); c.reach[3] = 1025; report("reach_of_the_row_after_the_call", c);
    c = good(); c.row0 = 4; c.reach[3] = 1025; report("reach_after_the_last_row_is_not_read", c);
    c = good(); c.guard[1] = -1; report("guard_negative", c);
    // the backs: -1 (no limit) or >= 0, in every used entry
    c = good(); c.null_back = true; report("null_back", c);
    c = good(); c.back = {-1, -1, -1, -1}; report("back_all_any", c);
    c = good(); c.back = {0, 0, 0, 0}; report("back_all_zero", c);
    c = good(); c.back[1] = MAX32; report("back_int_max", c);
    c = good(); c.back[1] = -2; report("back_minus_two", c);
    c = good(); c.back[2] = std::numeric_limits<int32_t>::min(); report("back_int_min", c);
    c = good(); c.back[0] = -2; report("back_entry_0_is_ignored", c);
    c = good(); c.back[3] = -2; report("back_of_the_row_after_the_call", c);
    c = good(); c.row0 = 4; c.back[3] = -2; report("back_after_the_last_row_is_not_read", c);
    // the penalties: finite and >= 0 in every used entry
    c = good(); c.null_penalty = true; report("null_penalty", c);
    c = good(); c.penalty[1] = std::nan(""); report("penalty_nan", c);
    c = good(); c.penalty[2] = INFINITY; report("penalty_inf", c);
    c = good(); c.penalty[1] = -1e-300; report("penalty_negative", c);
    c = good(); c.penalty[1] = -0.0; report("penalty_neg_zero", c);
    c = good(); c.penalty[0] = std::nan(""); report("penalty_entry_0_is_ignored", c);
    c = good(); c.penalty[3] = -1.0; report("penalty_of_the_row_after_the_call", c);
    c = good(); c.row0 = 4; c.penalty[3] = std::nan(""); report("penalty_after_the_last_row_is_not_read", c);
    // the workspace: 256 bytes of partial records and three arrays of one item each, padded to 256
    c = good(); c.mem_bytes = 1024; report("workspace_exact", c);
    c = good(); c.mem_bytes = 1023; report("workspace_short", c);
    c = good(); c.mem_bytes = 512; report("workspace_of_the_plain_margins", c);
    c = good(); c.mem = reinterpret_cast<void*>(((uintptr_t)1 << 20) + 128); report("workspace_misaligned", c);
    c = good(); c.mem = reinterpret_cast<void*>(((uintptr_t)1 << 20) + 128); c.mem_bytes = 0; report("workspace_misaligned_and_short", c);
    c = good(); c.back[1] = -2; c.mem_bytes = 0; report("bad_back_before_workspace", c);
    c = good(); c.penalty[1] = -1.0; c.mem = reinterpret_cast<void*>(((uintptr_t)1 << 20) + 128); report("bad_penalty_before_alignment", c);
    c = good(); c.guard[0] = -1; c.back[1] = -2; c.mem_bytes = 0; report("bad_guard_and_back_before_workspace", c);

    std::printf("bytes %zu %zu %zu %zu %zu %zu\n", sushi::order_margin_layout_bytes(1, 1), sushi::order_margin_layout_bytes(7, 513),
                sushi::order_margin_layout_bytes(200, 240001), sushi::order_margin_layout_bytes(0, 5),
                sushi::order_margin_layout_bytes(5, 0), sushi::order_margin_layout_bytes(-1, -1));
    // t'_e(j): j - back in 64 bits, cut at 0; no limit: 0
    std::printf("from %d %d %d %d %d %d %d\n", sushi::order_margin_from(5, 0), sushi::order_margin_from(5, 4), sushi::order_margin_from(5, 5),
                sushi::order_margin_from(5, 6), sushi::order_margin_from(MAX32 - 1, MAX32), sushi::order_margin_from(9, -1),
                sushi::order_margin_from(0, 0));
    facts("facts_one", 1);
    facts("facts_513", 513);
    facts("facts_240001", 240001);
    facts("facts_2880001", 2880001);
    facts("facts_int32_max", MAX32);
    return 0;
}

struct Sequence {
    int method;
    double step_cost;
    int32_t n_shift;
    int E;
    std::vector<float> curves;
    std::vector<SushiHipJointRow> rows;
    std::vector<int32_t> reach, back, guard, shifts;
    std::vector<double> penalty, D;
    // the state and the outputs
    std::vector<double> C, S, M, through, best, alt, c_min;
    std::vector<int32_t> best_arg, alt_arg;
};

struct Three { OrderMin c, m, a; };

// one call: rows row0 + n_rows - 1 down to row0
int walk(Sequence& q, int row0, int n_rows) {
    const int32_t n_shift = q.n_shift;
    const bool more = row0 + n_rows < q.E;
    // the tables as the entry point takes them: entry i is row row0 + i's, one more where the row after the call exists
    const std::vector<SushiHipJointRow> rows(q.rows.begin() + row0, q.rows.begin() + row0 + n_rows);
    const std::vector<int32_t> guard(q.guard.begin() + row0, q.guard.begin() + row0 + n_rows);
    const std::vector<int32_t> reach(q.reach.begin() + row0, q.reach.begin() + row0 + n_rows + (more ? 1 : 0));
    const std::vector<int32_t> back(q.back.begin() + row0, q.back.begin() + row0 + n_rows + (more ? 1 : 0));
    const std::vector<double> penalty(q.penalty.begin() + row0, q.penalty.begin() + row0 + n_rows + (more ? 1 : 0));
    OrderMarginStage st;
    const int rc = sushi::stage_order_margins(rows.data(), reach.data(), back.data(), penalty.data(), guard.data(), n_rows, n_shift,
                                              (int64_t)q.curves.size(), q.method, q.step_cost, row0, q.E, MEM, (size_t)1 << 30, st);
    if (rc != SUSHI_HIP_OK) { std::fprintf(stderr, "stage_order_margins refused the call: %d\n", rc); return 3; }
    if (st.first_call == more) { std::fprintf(stderr, "first_call is wrong\n"); return 3; }
    const int64_t span = (int64_t)st.split.per * sushi::TRACK_THREADS, n_items = st.split.n_items;
    const unsigned grid = st.split.grid;
    std::vector<OrderMin> item((size_t)n_items);
    std::vector<double> after((size_t)n_items);
    std::vector<Three> partial((size_t)grid);
    for (int i = n_rows - 1; i >= 0; --i) {
        const int e = row0 + i;
        const bool last = e == q.E - 1;
        const float* r = q.curves.data() + rows[(size_t)i].curve_off;
        const int32_t rch = sushi::margin_reach_after(reach.data(), i, n_rows, st.first_call);
        const int32_t bck = sushi::order_margin_back_after(back.data(), i, n_rows, st.first_call);
        const double lam = sushi::order_margin_penalty_after(penalty.data(), i, n_rows, st.first_call);
        const double* Cin = q.C.data() + (size_t)((e + 1) & 1) * n_shift;
        double* Cout = q.C.data() + (size_t)(e & 1) * n_shift;
        const double* Drow = q.D.data() + (size_t)e * n_shift;
        double* Mrow = q.M.data() + (size_t)e * n_shift;
        const int32_t s_e = sushi::path_clamp(q.shifts[(size_t)e], n_shift);
        for (unsigned b = 0; b < grid; ++b) partial[b] = Three{sushi::order_none(), sushi::order_none(), sushi::order_none()};
        // the step: every item's indices from the first one up; the item's record, and its workgroup's three minima
        for (int64_t it = 0; it < n_items; ++it) {
            const int64_t lo = it * span, hi = lo + span < n_shift ? lo + span : n_shift;
            Three& p = partial[(size_t)(it % grid)];
            OrderMin mine = sushi::order_none();
            for (int64_t j = lo; j < hi; ++j) {
                const double u = sushi::path_cost(q.method, rows[(size_t)i].weight, r[j]);
                double b = 0.0;
                if (!last) {
                    double near = Cin[j];
                    for (int32_t a = 1; a <= rch; ++a) {
                        const double price = sushi::track_price(q.step_cost, a);
                        if (j - a >= 0) {
                            const double c_lo = sushi::track_cand(Cin[j - a], price);
                            if (sushi::track_replaces_in_order(c_lo, near)) near = c_lo;
                        }
                        if (j + a < n_shift) {
                            const double c_hi = sushi::track_cand(Cin[j + a], price);
                            if (sushi::track_replaces_in_order(c_hi, near)) near = c_hi;
                        }
                    }
                    b = sushi::margin_back(near, sushi::order_margin_jump(q.S[(size_t)sushi::order_margin_from(j, bck)], lam));
                }
                const double m = sushi::margin_through(Drow[j], b, last), cn = sushi::margin_suffix(u, b, last);
                Cout[j] = cn;
                Mrow[j] = m;
                if (j == s_e) q.through[(size_t)e] = m;
                mine = sushi::order_combine(mine, OrderMin{cn, (int32_t)j});
                p.m = sushi::order_combine(OrderMin{m, (int32_t)j}, p.m);
                if (sushi::margin_outside(j, s_e, guard[(size_t)i])) p.a = sushi::order_combine(OrderMin{m, (int32_t)j}, p.a);
            }
            item[(size_t)it] = mine;
            p.c = sushi::order_combine(mine, p.c);
        }
        // the scan: what lies after every item, one item at a time from the last one down; the row's outputs from the workgroups'
        // records, met from the last one down
        OrderMin carry = sushi::order_none();
        for (int64_t it = n_items - 1; it >= 0; --it) {
            after[(size_t)it] = carry.v;
            carry = sushi::order_combine(item[(size_t)it], carry);
        }
        Three all = Three{sushi::order_none(), sushi::order_none(), sushi::order_none()};
        for (int b = (int)grid - 1; b >= 0; --b) {
            all.c = sushi::order_combine(all.c, partial[(size_t)b].c);
            all.m = sushi::order_combine(all.m, partial[(size_t)b].m);
            all.a = sushi::order_combine(all.a, partial[(size_t)b].a);
        }
        if (all.c.v != carry.v || all.c.i != carry.i) { std::fprintf(stderr, "the two minima of C differ in row %d\n", e); return 4; }
        q.c_min[(size_t)e] = all.c.v;
        q.best[(size_t)e] = all.m.v;
        q.best_arg[(size_t)e] = sushi::path_clamp(all.m.i, n_shift);
        q.alt[(size_t)e] = all.a.i == sushi::PATH_NO_INDEX ? INFINITY : all.a.v;
        q.alt_arg[(size_t)e] = sushi::margin_alt_index(all.a.i, n_shift);
        // the apply: waves of 64 indices, values alone; a wave's suffix folded from its last lane down, the totals behind a wave
        // from the one next to it rightwards
        for (int64_t it = 0; it < n_items; ++it) {
            const int64_t lo = it * span, hi = lo + span < n_shift ? lo + span : n_shift;
            const int64_t waves = (hi - lo + 63) / 64;
            std::vector<double> total((size_t)waves);
            for (int64_t w = 0; w < waves; ++w) {
                const int64_t a = lo + 64 * w, b = a + 64 < hi ? a + 64 : hi;
                double t = Cout[a];
                for (int64_t j = a + 1; j < b; ++j) t = sushi::order_suffix_combine(t, Cout[j]);      // (a left fold: another grouping)
                total[(size_t)w] = t;
            }
            for (int64_t w = 0; w < waves; ++w) {
                double behind = INFINITY;
                bool any = false;
                for (int64_t k = w + 1; k < waves; ++k) {
                    behind = any ? sushi::order_suffix_combine(behind, total[(size_t)k]) : total[(size_t)k];
                    any = true;
                }
                behind = any ? sushi::order_suffix_combine(behind, after[(size_t)it]) : after[(size_t)it];
                const int64_t a = lo + 64 * w, b = a + 64 < hi ? a + 64 : hi;
                double run = behind;
                for (int64_t j = b - 1; j >= a; --j) {
                    run = sushi::order_suffix_combine(Cout[j], run);
                    q.S[(size_t)j] = run;
                }
            }
        }
    }
    return 0;
}

int pass(char** v) {
    Sequence q;
    q.method = !std::strcmp(v[0], "ccoeff") ? SUSHI_HIP_METHOD_CCOEFF_NORMED : SUSHI_HIP_METHOD_SQDIFF_NORMED;
    q.step_cost = std::strtod(v[1], nullptr);
    q.n_shift = (int32_t)std::strtol(v[2], nullptr, 10);
    const int split = (int)std::strtol(v[3], nullptr, 10);
    q.curves = records<float>(read_file(v[4]));
    q.rows = records<SushiHipJointRow>(read_file(v[5]));
    q.reach = records<int32_t>(read_file(v[6]));
    q.back = records<int32_t>(read_file(v[7]));
    q.penalty = records<double>(read_file(v[8]));
    q.guard = records<int32_t>(read_file(v[9]));
    q.D = records<double>(read_file(v[10]));
    q.shifts = records<int32_t>(read_file(v[11]));
    q.E = (int)q.rows.size();
    const size_t E = (size_t)q.E, n = (size_t)q.n_shift;
    if (q.reach.size() != E || q.back.size() != E || q.penalty.size() != E || q.guard.size() != E || q.shifts.size() != E ||
        q.D.size() != E * n || split < 0 || split >= q.E) {
        std::fprintf(stderr, "as many reaches, backs, penalties, guards and shifts as rows, D of E x n_shift, 0 <= split < E\n");
        return 3;
    }
    // (NaN: what a call does not write is seen)
    q.C.assign(2 * n, std::nan("")); q.S.assign(n, std::nan("")); q.M.assign(E * n, std::nan(""));
    q.through.assign(E, std::nan("")); q.best.assign(E, std::nan("")); q.alt.assign(E, std::nan("")); q.c_min.assign(E, std::nan(""));
    q.best_arg.assign(E, -7); q.alt_arg.assign(E, -7);
    int rc = walk(q, split, q.E - split);
    if (rc == 0 && split > 0) rc = walk(q, 0, split);
    if (rc) return rc;
    using host_check::part;
    return host_check::write_file(v[12], {part(q.through), part(q.best), part(q.alt), part(q.c_min), part(q.best_arg), part(q.alt_arg),
                                          part(q.M), part(q.C), part(q.S)});
}

}  // namespace

int main(int argc, char** argv) {
    if (argc == 2 && !std::strcmp(argv[1], "validate")) return validate();
    if (argc == 15 && !std::strcmp(argv[1], "pass")) return pass(argv + 2);
    std::fprintf(stderr, "usage: %s validate | pass <sqdiff|ccoeff> <step_cost> <n_shift> <split> <curves> <rows> <reach> <back> <penalty> "
                         "<guard> <D> <shifts> <output>\n", argv[0]);
    return 2;
}
