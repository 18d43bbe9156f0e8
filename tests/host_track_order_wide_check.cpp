// The wide ordered tracking pass on the CPU (sushi_amd/csrc/track_order_wide_core.hpp, and the arithmetic it joins: track_wide_core.hpp's
// wide_near beside track_order_core.hpp's / track_order_margin_core.hpp's jump term): the call's host side -- the refusals of
// stage_track_ordered_wide and stage_order_margins_wide in their order, and the workspace's layout -- and whole sequences, forward
// and backward, divided as the kernels divide the work.
// usage: host_track_order_wide_check validate
//          prints "<case> <stage_track_ordered_wide's return code> <stage_order_margins_wide's>" for good and bad arguments, then
//          the bytes of the two layouts.
//        host_track_order_wide_check pass <sqdiff|ccoeff> <step_cost> <n_shift> <curves file> <rows file> <reach file> <back file>
//                                         <penalty file> <output file>
//          step_cost: float64 as text (a hexadecimal literal keeps its bits); curves: raw float32; rows: SushiHipJointRow records,
//          one sequence in event order; reach, back: int32, one per row; penalty: float64, one per row.  Forward: the axis in the
//          work items of the staged split; per wide row the tile pass (element by element: tests/host_track_wide_check.cpp holds the
//          divided scan against it), per work item the staged whole tiles' records and wide_near with the jump read from P at
//          t_e(j), one (min, first index) record per item, the exclusive scan of the records, the apply in waves of 64.  Backward:
//          the same with C, S at t'_e(j), the records' exclusive suffix scan and the apply on values alone.  The orders the device
//          leaves open are taken another way here (an item from its last index down, a wave's total from its last lane down).
//          Every row's window minimum, wide or not, is held against the candidate loop of track_core.hpp in the kernels' order of
//          candidates (exit status 4 at the first difference).  The output file holds [shift i32 x E][row_arg i32 x E][row_min f64 x
//          E][c_min f64 x E][moves i16 x E x n_shift][from i32 x E x n_shift][D f64 x E x n_shift][M f64 x E x n_shift].  The test
//          compares it with sushi_amd.track.track_ordered_margins_host(wide=True), bit for bit.
// Built by tests/test_track_order_wide_host.py with g++ -O2 -std=c++17 -ffp-contract=off -fsanitize=address,undefined.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "../include/sushi_hip.h"
#include "../sushi_amd/csrc/track_order_wide_core.hpp"
#include "host_check_io.hpp"

namespace {

using host_check::read_file;
using host_check::records;
using namespace sushi;

void* const MEM = reinterpret_cast<void*>((uintptr_t)1 << 20);      // aligned, never dereferenced
void* const ODD = reinterpret_cast<void*>(((uintptr_t)1 << 20) + 128);

struct Call {
    std::vector<SushiHipJointRow> rows;
    std::vector<int32_t> reach, back, guard;        // reach, back, penalty: one more than rows (the row after a margins call)
    std::vector<double> penalty;
    double step_cost;
    int row0;
    const void* mem;
    size_t mem_bytes;
    bool null_back, null_penalty, null_reach;
};

// rows 2 .. 4 of a sequence of 7 over 499 shifts, on a buffer of 1000 floats
Call good() {
    Call c;
    c.rows = {{0, 1.0}, {501, 0.0}, {333, 2.5}};
    c.reach = {0, 32767, 1025, 2000};
    c.back = {0, -1, 600, 3};
    c.penalty = {0.5, 0.0, 1e300, 0.25};
    c.guard = {0, 120, 5};
    c.step_cost = 0.0;
    c.row0 = 2;
    c.mem = MEM; c.mem_bytes = (size_t)1 << 30;
    c.null_back = c.null_penalty = c.null_reach = false;
    return c;
}

void report(const char* name, const Call& c) {
    OrderWideStage f;
    OrderMarginWideStage m;
    const int32_t* reach = c.null_reach ? nullptr : c.reach.data();
    const int32_t* back = c.null_back ? nullptr : c.back.data();
    const double* penalty = c.null_penalty ? nullptr : c.penalty.data();
    const int rf = stage_track_ordered_wide(c.rows.data(), reach, back, penalty, 3, 499, 1000, SUSHI_HIP_METHOD_SQDIFF_NORMED, c.step_cost,
                                            c.row0, 7, c.mem, c.mem_bytes, f);
    const int rm = stage_order_margins_wide(c.rows.data(), reach, back, penalty, c.guard.data(), 3, 499, 1000,
                                            SUSHI_HIP_METHOD_SQDIFF_NORMED, c.step_cost, c.row0, 7, c.mem, c.mem_bytes, m);
    std::printf("%s %d %d\n", name, rf, rm);
}

int validate() {
    Call c = good();
    report("good", c);
    c = good(); c.step_cost = -0.0; report("step_cost_neg_zero", c);
    c = good(); c.reach = {0, 1024, 7, 1024}; c.step_cost = 1e-3; report("narrow_reaches_with_step_cost", c);
    c = good(); c.reach[1] = 32768; report("reach_32768", c);
    c = good(); c.reach[2] = -1; report("reach_negative", c);
    c = good(); c.step_cost = 1e-3; report("wide_reach_with_step_cost", c);
    c = good(); c.reach = {0, 1025, 0, 0}; c.step_cost = 1e-3; report("reach_1025_with_step_cost", c);
    c = good(); c.reach[0] = 32768; report("first_reach_32768", c);
    c = good(); c.reach[0] = 32768; c.row0 = 0; report("reach_of_row_0_is_ignored", c);
    c = good(); c.reach[3] = 32768; report("reach_after_the_call_32768", c);
    c = good(); c.reach[3] = 32768; c.row0 = 4; report("reach_after_the_sequence_is_ignored", c);
    c = good(); c.null_reach = true; report("null_reach", c);
    c = good(); c.null_back = true; report("null_back", c);
    c = good(); c.null_penalty = true; report("null_penalty", c);
    c = good(); c.back[1] = -2; report("back_minus_two", c);
    c = good(); c.penalty[2] = std::nan(""); report("penalty_nan", c);
    c = good(); c.step_cost = -1e-300; report("step_cost_negative", c);
    // the order: the reach and the step cost before the backs and the penalties, all of them before the workspace
    c = good(); c.reach[1] = 32768; c.null_back = false; c.back[1] = -2; c.mem = ODD; c.mem_bytes = 0; report("reach_32768_before_workspace", c);
    c = good(); c.step_cost = 1e-3; c.mem = ODD; report("wide_reach_with_step_cost_before_alignment", c);
    c = good(); c.back[1] = -2; c.mem_bytes = 0; report("bad_back_before_workspace", c);
    c = good(); c.mem = ODD; c.mem_bytes = 0; report("workspace_misaligned_and_short", c);
    c = good(); c.mem = ODD; report("workspace_misaligned", c);
    c = good(); c.mem = nullptr; report("null_mem", c);
    c = good(); c.mem_bytes = order_wide_layout_bytes(3, 499); report("workspace_exact_forward", c);
    c = good(); c.mem_bytes = order_margin_wide_layout_bytes(3, 499); report("workspace_exact_margins", c);
    c = good(); c.mem_bytes = order_wide_layout_bytes(3, 499) - 1; report("workspace_short", c);
    c = good(); c.mem_bytes = order_margin_layout_bytes(3, 499); report("workspace_of_the_ordered_call", c);
    std::printf("bytes %zu %zu %zu %zu %zu\n", order_wide_layout_bytes(1, 1), order_wide_layout_bytes(3, 499), order_wide_layout_bytes(200, 240001),
                order_wide_layout_bytes(0, 5), order_wide_layout_bytes(5, 0));
    std::printf("margin_bytes %zu %zu %zu %zu %zu\n", order_margin_wide_layout_bytes(1, 1), order_margin_wide_layout_bytes(3, 499),
                order_margin_wide_layout_bytes(200, 240001), order_margin_wide_layout_bytes(0, 5), order_margin_wide_layout_bytes(5, 0));
    OrderWideStage f;
    c = good();
    const int rc = stage_track_ordered_wide(c.rows.data(), c.reach.data(), c.back.data(), c.penalty.data(), 3, 499, 1000, 0, 0.0, 2, 7, MEM,
                                            (size_t)1 << 30, f);
    std::printf("facts_499 rc=%d per=%d items=%lld plain=%zu records=(%zu,%zu,%zu,%zu) bytes=%zu tile_grid=%u wide_rows=%d\n", rc, f.plain.split.per,
                (long long)f.plain.split.n_items, f.plain.lay.bytes, f.wide.pv, f.wide.sv, f.wide.pi, f.wide.si, f.wide.bytes, f.tile_grid,
                f.n_wide);
    return 0;
}

bool same_bits(double a, double b) { return !std::memcmp(&a, &b, sizeof a); }

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

// the kernels' own order of candidates, 0, -1, +1, -2, +2, ..., in which the rule is the strict comparison
double loop_near(const double* X, int64_t j, int32_t n_shift, int32_t reach, double mu, int32_t* d) {
    double near = X[j]; int32_t nd = 0;
    for (int32_t a = 1; a <= reach && a < n_shift; ++a) {
        const double price = track_price(mu, a);
        if (j - a >= 0) { const double c = track_cand(X[j - a], price); if (track_replaces_in_order(c, near)) { near = c; nd = -a; } }
        if (j + a < n_shift) { const double c = track_cand(X[j + a], price); if (track_replaces_in_order(c, near)) { near = c; nd = a; } }
    }
    *d = nd;
    return near;
}

// near and its move for the indices of one work item [lo, hi) of row X: through the staged tiles' records and wide_near for a wide
// row -- and then held against the loop --, the loop itself otherwise.  0, or 4 at a difference.
int item_near(const double* X, Records& rec, int32_t n_shift, int32_t reach, double mu, int64_t lo, int64_t hi, int64_t span, double* near,
              int32_t* nd) {
    if (!wide_row(reach)) {
        for (int64_t j = hi - 1; j >= lo; --j) near[j] = loop_near(X, j, n_shift, reach, mu, &nd[j]);
        return 0;
    }
    WideTileRec staged[WIDE_ITEM_TILES];
    const int64_t t_lo = wide_item_first_tile(lo, reach), t_hi = wide_item_last_tile(lo, span, reach, n_shift);
    if (t_hi - t_lo + 1 > WIDE_ITEM_TILES) { std::fprintf(stderr, "an item asks for %lld tiles\n", (long long)(t_hi - t_lo + 1)); return 4; }
    for (int64_t t = t_lo; t <= t_hi; ++t) {
        const int64_t end = wide_tile_end(t, n_shift);
        staged[t - t_lo] = WideTileRec{rec.pv[(size_t)end], rec.pi[(size_t)end]};
    }
    const StagedTiles tiles{staged, t_lo, t_hi - t_lo + 1};
    for (int64_t j = hi - 1; j >= lo; --j) {
        near[j] = wide_near(X, rec.pv.data(), rec.sv.data(), rec.pi.data(), rec.si.data(), tiles, j, n_shift, reach, mu, &nd[j]);
        int32_t want_d = 0;
        const double want = loop_near(X, j, n_shift, reach, mu, &want_d);
        if (!same_bits(near[j], want) || nd[j] != want_d) {
            std::fprintf(stderr, "shift %lld: wide_near gives (%a, %d), the candidate loop (%a, %d)\n", (long long)j, near[j], nd[j], want, want_d);
            return 4;
        }
    }
    return 0;
}

int pass(const char* method_name, const char* step_text, const char* n_shift_text, const char* curves_path, const char* rows_path,
         const char* reach_path, const char* back_path, const char* penalty_path, const char* out_path) {
    const int method = !std::strcmp(method_name, "ccoeff") ? SUSHI_HIP_METHOD_CCOEFF_NORMED : SUSHI_HIP_METHOD_SQDIFF_NORMED;
    const double step_cost = std::strtod(step_text, nullptr);
    const int32_t n_shift = (int32_t)std::strtol(n_shift_text, nullptr, 10);
    const std::vector<float> curves = records<float>(read_file(curves_path));
    const std::vector<SushiHipJointRow> rows = records<SushiHipJointRow>(read_file(rows_path));
    const std::vector<int32_t> reach_of = records<int32_t>(read_file(reach_path));
    const std::vector<int32_t> back_of = records<int32_t>(read_file(back_path));
    const std::vector<double> penalty_of = records<double>(read_file(penalty_path));
    const int E = (int)rows.size();
    if ((int)reach_of.size() != E || (int)back_of.size() != E || (int)penalty_of.size() != E) {
        std::fprintf(stderr, "as many reaches, backs and penalties as rows\n");
        return 3;
    }
    const std::vector<int32_t> guard((size_t)E, 0);
    OrderWideStage st;
    OrderMarginWideStage mst;
    int rc = stage_track_ordered_wide(rows.data(), reach_of.data(), back_of.data(), penalty_of.data(), E, n_shift, (int64_t)curves.size(),
                                      method, step_cost, 0, E, MEM, (size_t)1 << 40, st);
    if (rc == SUSHI_HIP_OK)
        rc = stage_order_margins_wide(rows.data(), reach_of.data(), back_of.data(), penalty_of.data(), guard.data(), E, n_shift,
                                      (int64_t)curves.size(), method, step_cost, 0, E, MEM, (size_t)1 << 40, mst);
    if (rc != SUSHI_HIP_OK) { std::fprintf(stderr, "the staging refused the call: %d\n", rc); return 3; }
    const int64_t span = (int64_t)st.plain.split.per * TRACK_THREADS, n_items = st.plain.split.n_items;
    if (mst.plain.split.n_items != n_items || mst.plain.split.per != st.plain.split.per) return 4;
    const size_t n = (size_t)n_shift;
    std::vector<double> D((size_t)E * n), M((size_t)E * n), C(2 * n), P(n), S(n), row_min((size_t)E), c_min((size_t)E), near(n);
    std::vector<int16_t> moves((size_t)E * n, 0);
    std::vector<int32_t> from((size_t)E * n), row_arg((size_t)E), shifts((size_t)E), nd(n);
    std::vector<OrderMin> item((size_t)n_items), before((size_t)n_items);
    std::vector<double> after((size_t)n_items);
    Records rec(n_shift);
    // ---- forward
    for (int e = 0; e < E; ++e) {
        const float* r = curves.data() + rows[(size_t)e].curve_off;
        const int32_t reach = e ? reach_of[(size_t)e] : 0;
        const double* Din = D.data() + (size_t)(e ? e - 1 : 0) * n;
        double* Dout = D.data() + (size_t)e * n;
        int16_t* mv = moves.data() + (size_t)e * n;
        if (wide_row(reach))
            for (int64_t t = wide_tiles(n_shift) - 1; t >= 0; --t) wide_tile_scan(Din, n_shift, t, rec.view());
        for (int64_t it = n_items - 1; it >= 0; --it) {
            const int64_t lo = it * span, hi = lo + span < n_shift ? lo + span : n_shift;
            if (e) { const int bad = item_near(Din, rec, n_shift, reach, step_cost, lo, hi, span, near.data(), nd.data()); if (bad) return bad; }
            double best = INFINITY; int32_t at = PATH_NO_INDEX;
            for (int64_t j = hi - 1; j >= lo; --j) {
                const double u = path_cost(method, rows[(size_t)e].weight, r[j]);
                double dn = u;
                if (e) {
                    const double jump = order_jump(P[(size_t)order_reach_back(j, back_of[(size_t)e], n_shift)], penalty_of[(size_t)e]);
                    dn = track_step(near[(size_t)j], nd[(size_t)j], u, jump, &mv[j]);
                }
                Dout[j] = dn;
                if (path_min_replaces(dn, (int32_t)j, best, at)) { best = dn; at = (int32_t)j; }
            }
            item[(size_t)it] = OrderMin{best, at};
        }
        OrderMin carry = order_none();
        for (int64_t it = 0; it < n_items; ++it) { before[(size_t)it] = carry; carry = order_combine(carry, item[(size_t)it]); }
        row_min[(size_t)e] = carry.v; row_arg[(size_t)e] = path_clamp(carry.i, n_shift);
        for (int64_t it = 0; it < n_items; ++it) {
            const int64_t lo = it * span, hi = lo + span < n_shift ? lo + span : n_shift;
            OrderMin pref = before[(size_t)it];
            for (int64_t a = lo; a < hi; a += 64) {         // a wave's total from its last lane down, then onto what lies before it
                const int64_t b = a + 64 < hi ? a + 64 : hi;
                OrderMin run = pref;
                for (int64_t j = a; j < b; ++j) {
                    run = order_combine(run, OrderMin{Dout[j], (int32_t)j});
                    P[(size_t)j] = run.v; from[(size_t)e * n + (size_t)j] = run.i;
                }
                OrderMin t = order_none();
                for (int64_t j = b - 1; j >= a; --j) t = order_combine(OrderMin{Dout[j], (int32_t)j}, t);
                pref = order_combine(pref, t);
            }
        }
    }
    order_backtrack(moves.data(), from.data(), back_of.data(), row_arg.data(), E, n_shift, shifts.data());
    // ---- backward
    for (int e = E - 1; e >= 0; --e) {
        const float* r = curves.data() + rows[(size_t)e].curve_off;
        const bool last = e == E - 1;
        const int32_t reach = last ? 0 : reach_of[(size_t)e + 1];
        const int32_t back = last ? TRACK_BACK_ANY : back_of[(size_t)e + 1];
        const double penalty = last ? 0.0 : penalty_of[(size_t)e + 1];
        const double* Cin = C.data() + (size_t)((e + 1) & 1) * n;
        double* Cout = C.data() + (size_t)(e & 1) * n;
        if (wide_row(reach))
            for (int64_t t = wide_tiles(n_shift) - 1; t >= 0; --t) wide_tile_scan(Cin, n_shift, t, rec.view());
        for (int64_t it = 0; it < n_items; ++it) {
            const int64_t lo = it * span, hi = lo + span < n_shift ? lo + span : n_shift;
            if (!last) { const int bad = item_near(Cin, rec, n_shift, reach, step_cost, lo, hi, span, near.data(), nd.data()); if (bad) return bad; }
            double best = INFINITY; int32_t at = PATH_NO_INDEX;
            for (int64_t j = hi - 1; j >= lo; --j) {
                const double u = path_cost(method, rows[(size_t)e].weight, r[j]);
                const double b = last ? 0.0 : margin_back(near[(size_t)j], order_margin_jump(S[(size_t)order_margin_from(j, back)], penalty));
                M[(size_t)e * n + (size_t)j] = margin_through(D[(size_t)e * n + (size_t)j], b, last);
                Cout[j] = margin_suffix(u, b, last);
                if (path_min_replaces(Cout[j], (int32_t)j, best, at)) { best = Cout[j]; at = (int32_t)j; }
            }
            item[(size_t)it] = OrderMin{best, at};
        }
        OrderMin carry = order_none();
        for (int64_t it = n_items - 1; it >= 0; --it) { after[(size_t)it] = carry.v; carry = order_combine(item[(size_t)it], carry); }
        c_min[(size_t)e] = carry.v;
        for (int64_t it = 0; it < n_items; ++it) {
            const int64_t lo = it * span, hi = lo + span < n_shift ? lo + span : n_shift;
            double behind = after[(size_t)it];
            for (int64_t j = hi - 1; j >= lo; --j) { behind = order_suffix_combine(Cout[j], behind); S[(size_t)j] = behind; }
        }
    }
    using host_check::part;
    return host_check::write_file(out_path, {part(shifts), part(row_arg), part(row_min), part(c_min), part(moves), part(from), part(D), part(M)});
}

}  // namespace

int main(int argc, char** argv) {
    if (argc == 2 && !std::strcmp(argv[1], "validate")) return validate();
    if (argc == 11 && !std::strcmp(argv[1], "pass"))
        return pass(argv[2], argv[3], argv[4], argv[5], argv[6], argv[7], argv[8], argv[9], argv[10]);
    std::fprintf(stderr, "usage: %s validate | pass <sqdiff|ccoeff> <step_cost> <n_shift> <curves> <rows> <reach> <back> <penalty> <output>\n",
                 argv[0]);
    return 2;
}
