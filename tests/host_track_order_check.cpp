// sushi_hip_track_forward_ordered / sushi_hip_track_backtrack_ordered on the CPU (sushi_amd/csrc/track_order_core.hpp): the call's
// host side -- stage_track_ordered's refusals and the workspace's layout -- and its arithmetic: track_core.hpp's candidates and
// track_step with order_jump, order_reach_back, the (value, index) combine rule and order_backtrack, over whole sequences.
// usage: host_track_order_check validate
//          prints "<case> <return code>" for good and bad arguments, then the facts of staged calls.
//        host_track_order_check pass <sqdiff|ccoeff> <step_cost> <n_shift> <curves file> <rows file> <reach file> <back file>
//                                    <penalty file> <output file>
//          step_cost: float64 as text (a hexadecimal literal keeps its bits); curves: raw float32; rows: SushiHipJointRow records,
//          one sequence in event order; reach, back: int32, one per row; penalty: float64, one per row.  The pass is divided as the
//          kernels divide it: the axis into the work items of the staged split, one (min, first index) record per item, an
//          exclusive scan of those records, and inside an item waves of 64 indices -- but the orders the device leaves open are
//          taken another way here (an item's record is folded from its last index down, a wave's total from its last lane down,
//          the waves' totals before a wave are folded right to left), so the rule that makes the result independent of the
//          grouping is what is checked.  The output file holds [shift i32 x E][row_arg i32 x E][own index i32 x E][own value f32 x E]
//          [row_min f64 x E][last D f64 x n_shift][moves i16 x E x n_shift][from i32 x E x n_shift].  The test compares it with
//          sushi_amd.track.track_ordered_host, bit for bit.
// Built by tests/test_track_order_host.py with g++ -O2 -std=c++17 -ffp-contract=off -fsanitize=address,undefined.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "../include/sushi_hip.h"
#include "../sushi_amd/csrc/track_order_core.hpp"
#include "host_check_io.hpp"

namespace {

using host_check::read_file;
using host_check::records;
using sushi::OrderMin;
using sushi::OrderStage;

constexpr int64_t MAX64 = std::numeric_limits<int64_t>::max();
constexpr int32_t MAX32 = std::numeric_limits<int32_t>::max();
void* const MEM = reinterpret_cast<void*>((uintptr_t)1 << 20);      // aligned, never dereferenced

struct Call {
    std::vector<SushiHipJointRow> rows;
    std::vector<int32_t> reach, back;
    std::vector<double> penalty;
    int n_rows;
    int32_t n_shift;
    int64_t n_curve;
    int method;
    double step_cost;
    int row0, n_total;
    const void* mem;
    size_t mem_bytes;
    bool null_rows, null_reach, null_back, null_penalty;
};

// rows 2 .. 4 of a sequence of 7 over 499 shifts, on a buffer of 1000 floats
Call good() {
    Call c;
    c.rows = {{0, 1.0}, {501, 0.0}, {333, 2.5}};
    c.reach = {0, 1024, 17};
    c.back = {0, -1, 600};
    c.penalty = {0.5, 0.0, 1e300};
    c.n_rows = 3; c.n_shift = 499; c.n_curve = 1000;
    c.method = SUSHI_HIP_METHOD_SQDIFF_NORMED;
    c.step_cost = 0.001;
    c.row0 = 2; c.n_total = 7;
    c.mem = MEM; c.mem_bytes = 1 << 20;
    c.null_rows = c.null_reach = c.null_back = c.null_penalty = false;
    return c;
}

int stage(const Call& c, OrderStage& st) {
    return sushi::stage_track_ordered(c.null_rows ? nullptr : c.rows.data(), c.null_reach ? nullptr : c.reach.data(),
                                      c.null_back ? nullptr : c.back.data(), c.null_penalty ? nullptr : c.penalty.data(), c.n_rows,
                                      c.n_shift, c.n_curve, c.method, c.step_cost, c.row0, c.n_total, c.mem, c.mem_bytes, st);
}

void report(const char* name, const Call& c) {
    OrderStage st;
    std::printf("%s %d\n", name, stage(c, st));
}

void facts(const char* name, int32_t n_shift) {
    Call c = good();
    c.rows = {{0, 1.0}};
    c.reach = {0}; c.back = {-1}; c.penalty = {0.0};
    c.n_rows = 1; c.row0 = 0; c.n_total = 1; c.n_shift = n_shift; c.n_curve = MAX64;
    c.mem_bytes = (size_t)1 << 40;
    OrderStage st;
    const int rc = stage(c, st);
    std::printf("%s rc=%d", name, rc);
    if (rc == SUSHI_HIP_OK)
        std::printf(" per=%d items=%lld grid=%u set=%zu offsets=(%zu,%zu,%zu,%zu) bytes=%zu", st.split.per, (long long)st.split.n_items,
                    st.split.grid, st.lay.partials.set_bytes, st.lay.item_min, st.lay.item_arg, st.lay.before_min, st.lay.before_arg,
                    st.lay.bytes);
    std::printf("\n");
}

int validate() {
    Call c = good();
    report("good", c);
    c = good(); c.method = SUSHI_HIP_METHOD_CCOEFF_NORMED; report("good_ccoeff", c);
    // what stage_track refuses
    c = good(); c.null_rows = true; report("null_rows", c);
    c = good(); c.null_reach = true; report("null_reach", c);
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
    c = good(); c.row0 = 0; c.reach[0] = 1025; report("reach_of_row_0_is_ignored", c);
    // the backs: -1 (no limit) or >= 0, in every row
    c = good(); c.null_back = true; report("null_back", c);
    c = good(); c.back = {-1, -1, -1}; report("back_all_any", c);
    c = good(); c.back = {0, 0, 0}; report("back_all_zero", c);
    c = good(); c.back[1] = MAX32; report("back_int_max", c);
    c = good(); c.back[1] = -2; report("back_minus_two", c);
    c = good(); c.back[2] = std::numeric_limits<int32_t>::min(); report("back_int_min", c);
    c = good(); c.back[0] = -2; report("back_of_a_later_calls_first_row", c);
    c = good(); c.row0 = 0; c.back[0] = -2; report("back_of_row_0_minus_two", c);
    // the penalties: finite and >= 0 in every row but the sequence's row 0
    c = good(); c.null_penalty = true; report("null_penalty", c);
    c = good(); c.penalty[1] = std::nan(""); report("penalty_nan", c);
    c = good(); c.penalty[2] = INFINITY; report("penalty_inf", c);
    c = good(); c.penalty[1] = -1e-300; report("penalty_negative", c);
    c = good(); c.penalty[1] = -0.0; report("penalty_neg_zero", c);
    c = good(); c.penalty[0] = std::nan(""); report("penalty_of_a_later_calls_first_row", c);
    c = good(); c.row0 = 0; c.penalty[0] = std::nan(""); report("penalty_of_row_0_is_ignored", c);
    c = good(); c.row0 = 0; c.penalty[0] = -1.0; report("negative_penalty_of_row_0_is_ignored", c);
    c = good(); c.row0 = 0; c.penalty[1] = -1.0; report("penalty_of_row_1", c);
    // the workspace: 256 bytes of partial records and four arrays of one item each, padded to 256
    c = good(); c.mem_bytes = 1280; report("workspace_exact", c);
    c = good(); c.mem_bytes = 1279; report("workspace_short", c);
    c = good(); c.mem_bytes = 512; report("workspace_of_the_plain_pass", c);
    c = good(); c.mem = reinterpret_cast<void*>(((uintptr_t)1 << 20) + 128); report("workspace_misaligned", c);
    c = good(); c.mem = reinterpret_cast<void*>(((uintptr_t)1 << 20) + 128); c.mem_bytes = 0; report("workspace_misaligned_and_short", c);
    c = good(); c.back[1] = -2; c.mem_bytes = 0; report("bad_back_before_workspace", c);
    c = good(); c.penalty[1] = -1.0; c.mem = reinterpret_cast<void*>(((uintptr_t)1 << 20) + 128); report("bad_penalty_before_alignment", c);

    std::printf("bytes %zu %zu %zu %zu %zu %zu\n", sushi::order_layout_bytes(1, 1), sushi::order_layout_bytes(7, 513),
                sushi::order_layout_bytes(200, 240001), sushi::order_layout_bytes(0, 5), sushi::order_layout_bytes(5, 0),
                sushi::order_layout_bytes(-1, -1));
    // t_e(j): j + back in 64 bits, cut at the axis's end; no limit: the axis's end
    std::printf("reach_back %d %d %d %d %d %d\n", sushi::order_reach_back(5, 0, 10), sushi::order_reach_back(5, 4, 10),
                sushi::order_reach_back(5, 5, 10), sushi::order_reach_back(MAX32 - 1, MAX32, MAX32), sushi::order_reach_back(0, -1, 10),
                sushi::order_reach_back(9, 0, 10));
    facts("facts_one", 1);
    facts("facts_513", 513);
    facts("facts_240001", 240001);
    facts("facts_2880001", 2880001);
    facts("facts_int32_max", MAX32);
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
    OrderStage st;
    const int rc = sushi::stage_track_ordered(rows.data(), reach_of.data(), back_of.data(), penalty_of.data(), E, n_shift,
                                              (int64_t)curves.size(), method, step_cost, 0, E, MEM, (size_t)1 << 30, st);
    if (rc != SUSHI_HIP_OK) { std::fprintf(stderr, "stage_track_ordered refused the call: %d\n", rc); return 3; }
    const int64_t span = (int64_t)st.split.per * sushi::TRACK_THREADS, n_items = st.split.n_items;
    std::vector<double> D((size_t)2 * n_shift), P((size_t)n_shift), row_min((size_t)E);
    std::vector<int16_t> moves((size_t)E * n_shift, 0);
    std::vector<int32_t> from((size_t)E * n_shift), row_arg((size_t)E), own_idx((size_t)E), shifts((size_t)E);
    std::vector<float> own_val((size_t)E);
    std::vector<OrderMin> item((size_t)n_items), before((size_t)n_items);
    const float worst = method == SUSHI_HIP_METHOD_CCOEFF_NORMED ? -INFINITY : INFINITY;
    for (int e = 0; e < E; ++e) {
        const float* r = curves.data() + rows[(size_t)e].curve_off;
        const int32_t reach = e ? reach_of[(size_t)e] : 0;
        const double* Din = D.data() + (size_t)((e + 1) & 1) * n_shift;
        double* Dout = D.data() + (size_t)(e & 1) * n_shift;
        int16_t* mv = moves.data() + (size_t)e * n_shift;
        float own = worst; int32_t own_at = sushi::PATH_NO_INDEX;
        // the step: every item's indices from the last one down, and the item's record
        for (int64_t it = n_items - 1; it >= 0; --it) {
            const int64_t lo = it * span, hi = lo + span < n_shift ? lo + span : n_shift;
            double best = INFINITY; int32_t at = sushi::PATH_NO_INDEX;
            for (int64_t j = hi - 1; j >= lo; --j) {
                const double u = sushi::path_cost(method, rows[(size_t)e].weight, r[j]);
                double dn = u;
                if (e) {
                    // the kernel's order of candidates, 0, -1, +1, -2, +2, ..., in which the rule is the strict comparison
                    // (tests/host_track_check.cpp holds it against the order-free rule)
                    double near = Din[j]; int32_t nd = 0;
                    for (int32_t a = 1; a <= reach; ++a) {
                        const double price = sushi::track_price(step_cost, a);
                        if (j - a >= 0) {
                            const double c_lo = sushi::track_cand(Din[j - a], price);
                            if (sushi::track_replaces_in_order(c_lo, near)) { near = c_lo; nd = -a; }
                        }
                        if (j + a < n_shift) {
                            const double c_hi = sushi::track_cand(Din[j + a], price);
                            if (sushi::track_replaces_in_order(c_hi, near)) { near = c_hi; nd = a; }
                        }
                    }
                    const double jump = sushi::order_jump(P[(size_t)sushi::order_reach_back(j, back_of[(size_t)e], n_shift)],
                                                          penalty_of[(size_t)e]);
                    dn = sushi::track_step(near, nd, u, jump, &mv[j]);
                }
                Dout[j] = dn;
                if (sushi::path_min_replaces(dn, (int32_t)j, best, at)) { best = dn; at = (int32_t)j; }
                if (sushi::path_own_replaces(method, r[j], (int32_t)j, own, own_at)) { own = r[j]; own_at = (int32_t)j; }
            }
            item[(size_t)it] = OrderMin{best, at};
        }
        // the scan: what lies before every item; what lies before the end is the row's minimum
        OrderMin carry = sushi::order_none();
        for (int64_t it = 0; it < n_items; ++it) {
            before[(size_t)it] = carry;
            carry = sushi::order_combine(carry, item[(size_t)it]);
        }
        row_min[(size_t)e] = carry.v; row_arg[(size_t)e] = sushi::path_clamp(carry.i, n_shift);
        own_idx[(size_t)e] = sushi::path_clamp(own_at, n_shift); own_val[(size_t)e] = own;
        // the apply: waves of 64 indices; a wave's total folded from its last lane down, the totals before a wave right to left
        for (int64_t it = 0; it < n_items; ++it) {
            const int64_t lo = it * span, hi = lo + span < n_shift ? lo + span : n_shift;
            const int64_t waves = (hi - lo + 63) / 64;
            std::vector<OrderMin> total((size_t)waves);
            for (int64_t w = 0; w < waves; ++w) {
                OrderMin t = sushi::order_none();
                const int64_t a = lo + 64 * w, b = a + 64 < hi ? a + 64 : hi;
                for (int64_t j = b - 1; j >= a; --j) t = sushi::order_combine(OrderMin{Dout[j], (int32_t)j}, t);
                total[(size_t)w] = t;
            }
            for (int64_t w = 0; w < waves; ++w) {
                OrderMin pref = sushi::order_none();
                for (int64_t k = w - 1; k >= 0; --k) pref = sushi::order_combine(total[(size_t)k], pref);
                pref = sushi::order_combine(before[(size_t)it], pref);
                const int64_t a = lo + 64 * w, b = a + 64 < hi ? a + 64 : hi;
                for (int64_t j = a; j < b; ++j) {
                    pref = sushi::order_combine(pref, OrderMin{Dout[j], (int32_t)j});
                    P[(size_t)j] = pref.v;
                    from[(size_t)e * n_shift + j] = pref.i;
                }
            }
        }
    }
    sushi::order_backtrack(moves.data(), from.data(), back_of.data(), row_arg.data(), E, n_shift, shifts.data());
    std::vector<double> last(D.begin() + (ptrdiff_t)((size_t)((E - 1) & 1) * n_shift), D.begin() + (ptrdiff_t)((size_t)((E - 1) & 1) * n_shift + n_shift));
    using host_check::part;
    return host_check::write_file(out_path, {part(shifts), part(row_arg), part(own_idx), part(own_val), part(row_min), part(last),
                                             part(moves), part(from)});
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
