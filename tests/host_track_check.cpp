// sushi_hip_track_forward / sushi_hip_track_backtrack on the CPU (sushi_amd/csrc/track_core.hpp): the call's host side --
// stage_track's refusals, the workspace's layout, the work split, the halo rounds and tile sizes -- and its arithmetic: path_cost,
// track_price, track_cand, track_replaces, track_step, the two first-extremum rules and track_backtrack, over whole sequences.
// usage: host_track_check validate
//          prints "<case> <return code>" for good and bad arguments (sizes up to INT64_MAX), then the facts of staged calls.
//        host_track_check pass <sqdiff|ccoeff> <penalty> <step_cost> <n_shift> <curves file> <rows file> <reach file> <output file>
//          penalty, step_cost: float64 as text (a hexadecimal literal keeps its bits); curves: raw float32; rows: SushiHipJointRow
//          records, one sequence in event order; reach: int32, one per row.  The pass is divided as the kernels divide it: the axis
//          into the work items of track_split, the items onto its workgroups, every item's values of D_{e-1} and its halo of reach_e
//          on each side staged into a tile (indices outside the axis moved onto an element inside it, and left out by a select),
//          every candidate read from the tile, D in two halves, one partial record per workgroup -- but every order the device
//          leaves open is taken BACKWARDS here (a workgroup's items, an item's indices, a shift's candidates from the widest move
//          inwards and +a before -a, the partial records), so the rules that make the result independent of the order are what is
//          checked; the kernel's own candidate order (0, -1, +1, -2, +2, ..., a strict comparison) is run beside it and has to
//          give the same winner, bit for bit.  The output file holds [shift i32 x E][row_arg i32 x E][own index i32 x E]
//          [own value f32 x E][row_min f64 x E][moves i16 x E x n_shift].  The test compares it with sushi_amd.track.track_host, bit for bit.
// Built by tests/test_track_host.py with g++ -O2 -std=c++17 -ffp-contract=off -fsanitize=address,undefined.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "../include/sushi_hip.h"
#include "../sushi_amd/csrc/track_core.hpp"
#include "host_check_io.hpp"

namespace {

using host_check::read_file;
using host_check::records;
using sushi::TrackStage;

constexpr int64_t MAX64 = std::numeric_limits<int64_t>::max();
constexpr int32_t MAX32 = std::numeric_limits<int32_t>::max();
void* const MEM = reinterpret_cast<void*>((uintptr_t)1 << 20);      // aligned, never dereferenced

struct Call {
    std::vector<SushiHipJointRow> rows;
    std::vector<int32_t> reach;
    int n_rows;
    int32_t n_shift;
    int64_t n_curve;
    int method;
    double penalty, step_cost;
    int row0, n_total;
    const void* mem;
    size_t mem_bytes;
    bool null_rows, null_reach;
};

// rows 2 .. 4 of a sequence of 7 over 499 shifts, on a buffer of 1000 floats
Call good() {
    Call c;
    c.rows = {{0, 1.0}, {501, 0.0}, {333, 2.5}};
    c.reach = {0, 1024, 17};
    c.n_rows = 3; c.n_shift = 499; c.n_curve = 1000;
    c.method = SUSHI_HIP_METHOD_SQDIFF_NORMED;
    c.penalty = 0.5; c.step_cost = 0.001;
    c.row0 = 2; c.n_total = 7;
    c.mem = MEM; c.mem_bytes = 1 << 20;
    c.null_rows = c.null_reach = false;
    return c;
}

int stage(const Call& c, TrackStage& st) {
    return sushi::stage_track(c.null_rows ? nullptr : c.rows.data(), c.null_reach ? nullptr : c.reach.data(), c.n_rows, c.n_shift,
                              c.n_curve, c.method, c.penalty, c.step_cost, c.row0, c.n_total, c.mem, c.mem_bytes, st);
}

void report(const char* name, const Call& c) {
    TrackStage st;
    std::printf("%s %d\n", name, stage(c, st));
}

void facts(const char* name, int32_t n_shift) {
    Call c = good();
    c.rows = {{0, 1.0}};
    c.reach = {0};
    c.n_rows = 1; c.row0 = 0; c.n_total = 1; c.n_shift = n_shift; c.n_curve = MAX64;
    TrackStage st;
    const int rc = stage(c, st);
    std::printf("%s rc=%d", name, rc);
    if (rc == SUSHI_HIP_OK)
        std::printf(" per=%d items=%lld grid=%u set=%zu bytes=%zu offsets=(%zu,%zu,%zu,%zu)", st.split.per,
                    (long long)st.split.n_items, st.split.grid, st.lay.set_bytes, st.lay.bytes, st.lay.d_min, st.lay.d_arg,
                    st.lay.own_idx, st.lay.own_val);
    std::printf("\n");
}

int validate() {
    Call c = good();
    report("good", c);
    c = good(); c.method = SUSHI_HIP_METHOD_CCOEFF_NORMED; report("good_ccoeff", c);
    c = good(); c.null_rows = true; report("null_rows", c);
    c = good(); c.null_reach = true; report("null_reach", c);
    c = good(); c.mem = nullptr; report("null_mem", c);
    c = good(); c.method = 2; report("method_2", c);
    c = good(); c.method = -1; report("method_neg", c);
    c = good(); c.n_rows = 0; report("no_rows", c);
    c = good(); c.n_rows = -3; report("negative_rows", c);
    c = good(); c.n_shift = 0; report("no_shift", c);
    c = good(); c.n_shift = -3; report("negative_shift", c);
    c = good(); c.n_curve = 0; report("empty_curves", c);
    c = good(); c.n_curve = -5; report("negative_curves", c);
    c = good(); c.n_shift = 1001; report("shift_beyond_curves", c);
    // the rows inside the sequence
    c = good(); c.row0 = 0; c.n_total = 3; report("whole_sequence", c);
    c = good(); c.row0 = 4; report("rows_end_at_sequence_end", c);
    c = good(); c.row0 = 5; report("rows_past_sequence_end", c);
    c = good(); c.row0 = -1; report("row0_negative", c);
    c = good(); c.row0 = 7; report("row0_at_end", c);
    c = good(); c.n_total = 0; report("no_total", c);
    c = good(); c.n_total = -7; report("negative_total", c);
    c = good(); c.row0 = MAX32 - 3; c.n_total = MAX32; report("rows_end_at_int_max", c);
    c = good(); c.row0 = MAX32 - 2; c.n_total = MAX32; report("rows_sum_overflows_int", c);
    c = good(); c.row0 = MAX32; c.n_total = MAX32; report("row0_int_max", c);
    // the rows inside the curve buffer; sums that do not fit 64 bits are never formed
    c = good(); c.rows[0].curve_off = -1; report("row_before_curves", c);
    c = good(); c.rows[1].curve_off = 501; report("row_ends_at_curves_end", c);
    c = good(); c.rows[1].curve_off = 502; report("row_one_past_curves_end", c);
    c = good(); c.n_shift = 1; c.rows[2].curve_off = 999; report("single_shift_last_float", c);
    c = good(); c.n_shift = 1; c.rows[2].curve_off = 1000; report("single_shift_past_end", c);
    c = good(); c.rows[2].curve_off = MAX64; report("row_at_int64_max", c);
    c = good(); c.rows[2].curve_off = MAX64 - 498; report("row_sum_overflows", c);
    c = good(); c.n_curve = MAX64; c.rows[2].curve_off = MAX64 - 499; report("huge_curves_row_at_end", c);
    c = good(); c.n_curve = MAX64; c.rows[2].curve_off = MAX64 - 498; report("huge_curves_row_past_end", c);
    c = good(); c.n_curve = MAX64; c.n_shift = MAX32; c.rows[2].curve_off = MAX64 / 2; report("huge_curves_int32_max_shifts", c);
    // weights, the penalty and the step cost
    c = good(); c.rows[1].weight = std::nan(""); report("weight_nan", c);
    c = good(); c.rows[1].weight = INFINITY; report("weight_inf", c);
    c = good(); c.rows[1].weight = -1e-300; report("weight_negative", c);
    c = good(); c.rows[1].weight = -0.0; report("weight_neg_zero", c);
    c = good(); c.penalty = std::nan(""); report("penalty_nan", c);
    c = good(); c.penalty = INFINITY; report("penalty_inf", c);
    c = good(); c.penalty = -1e-300; report("penalty_negative", c);
    c = good(); c.penalty = 0.0; report("penalty_zero", c);
    c = good(); c.penalty = 1e300; report("penalty_large", c);
    c = good(); c.step_cost = std::nan(""); report("step_cost_nan", c);
    c = good(); c.step_cost = INFINITY; report("step_cost_inf", c);
    c = good(); c.step_cost = -INFINITY; report("step_cost_neg_inf", c);
    c = good(); c.step_cost = -1e-300; report("step_cost_negative", c);
    c = good(); c.step_cost = 0.0; report("step_cost_zero", c);
    c = good(); c.step_cost = -0.0; report("step_cost_neg_zero", c);
    c = good(); c.step_cost = 1e300; report("step_cost_large", c);
    // the reach: 0 .. 1024 in every row but the sequence's row 0
    c = good(); c.reach = {1024, 1024, 1024}; report("reach_all_widest", c);
    c = good(); c.reach[1] = 1025; report("reach_1025", c);
    c = good(); c.reach[2] = -1; report("reach_negative", c);
    c = good(); c.reach[0] = 1025; report("reach_of_a_later_calls_first_row", c);
    c = good(); c.reach[2] = MAX32; report("reach_int_max", c);
    c = good(); c.reach[1] = std::numeric_limits<int32_t>::min(); report("reach_int_min", c);
    c = good(); c.row0 = 0; c.reach[0] = 1025; report("reach_of_row_0_is_ignored", c);
    c = good(); c.row0 = 0; c.reach[0] = -5; report("negative_reach_of_row_0_is_ignored", c);
    c = good(); c.row0 = 0; c.reach[1] = 1025; report("reach_of_row_1", c);
    // the workspace: one partial record of 20 bytes per set, each set padded to 256
    c = good(); c.mem_bytes = 512; report("workspace_exact", c);
    c = good(); c.mem_bytes = 511; report("workspace_short", c);
    c = good(); c.mem_bytes = 0; report("workspace_none", c);
    c = good(); c.mem = reinterpret_cast<void*>(((uintptr_t)1 << 20) + 128); report("workspace_misaligned", c);
    c = good(); c.mem = reinterpret_cast<void*>(((uintptr_t)1 << 20) + 128); c.mem_bytes = 0; report("workspace_misaligned_and_short", c);
    c = good(); c.reach[1] = 1025; c.mem_bytes = 0; report("bad_reach_before_workspace", c);
    c = good(); c.step_cost = -1.0; c.mem = reinterpret_cast<void*>(((uintptr_t)1 << 20) + 128); report("bad_step_cost_before_alignment", c);

    std::printf("bytes %zu %zu %zu %zu %zu %zu %zu\n", sushi::track_layout_bytes(1, 1), sushi::track_layout_bytes(7, 513),
                sushi::track_layout_bytes(200, 240001), sushi::track_layout_bytes(1, MAX32), sushi::track_layout_bytes(0, 5),
                sushi::track_layout_bytes(5, 0), sushi::track_layout_bytes(-1, -1));
    std::printf("halo %d %d %d %d %d %d\n", sushi::track_halo_rounds(0), sushi::track_halo_rounds(1), sushi::track_halo_rounds(256),
                sushi::track_halo_rounds(257), sushi::track_halo_rounds(1024), sushi::TRACK_HALO_LARGE * sushi::TRACK_THREADS);
    std::printf("tile %zu %zu %zu %zu %zu\n", sushi::track_tile_bytes(2, 0), sushi::track_tile_bytes(2, 1), sushi::track_tile_bytes(2, 1024),
                sushi::track_tile_bytes(8, 16), sushi::track_tile_bytes(8, 1024));
    facts("facts_one", 1);
    facts("facts_512", 512);
    facts("facts_513", 513);
    facts("facts_240001", 240001);
    // the size from which on the large items are taken, and one shift below it
    facts("facts_large_items", 1023 * 2048 + 1);
    facts("facts_small_items", 1023 * 2048);
    facts("facts_2880001", 2880001);
    facts("facts_int32_max", MAX32);
    return 0;
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
    TrackStage st;
    const int rc = sushi::stage_track(rows.data(), reach_of.data(), E, n_shift, (int64_t)curves.size(), method, penalty, step_cost, 0, E,
                                      MEM, (size_t)1 << 30, st);
    if (rc != SUSHI_HIP_OK) { std::fprintf(stderr, "stage_track refused the call: %d\n", rc); return 3; }
    const int64_t span = (int64_t)st.split.per * sushi::TRACK_THREADS;
    const int grid = (int)st.split.grid;
    std::vector<double> D((size_t)2 * n_shift), row_min((size_t)E), p_min((size_t)grid), tile;
    std::vector<int16_t> moves((size_t)E * n_shift, 0);
    std::vector<int32_t> row_arg((size_t)E), own_idx((size_t)E), shifts((size_t)E), p_arg((size_t)grid), p_own_idx((size_t)grid);
    std::vector<float> own_val((size_t)E), p_own_val((size_t)grid);
    const float worst = method == SUSHI_HIP_METHOD_CCOEFF_NORMED ? -INFINITY : INFINITY;
    for (int e = 0; e < E; ++e) {
        const float* r = curves.data() + rows[(size_t)e].curve_off;
        const double jump = e ? row_min[(size_t)e - 1] + penalty : 0.0;
        const int32_t reach = e ? reach_of[(size_t)e] : 0;
        const double* Din = D.data() + (size_t)((e + 1) & 1) * n_shift;
        double* Dout = D.data() + (size_t)(e & 1) * n_shift;
        int16_t* mv = moves.data() + (size_t)e * n_shift;
        if (sushi::track_halo_rounds(reach) * sushi::TRACK_THREADS < 2 * reach) { std::fprintf(stderr, "halo rounds too few\n"); return 3; }
        for (int b = grid - 1; b >= 0; --b) {                              // one partial record per workgroup
            double best = INFINITY; int32_t at = sushi::PATH_NO_INDEX;
            float own = worst; int32_t own_at = sushi::PATH_NO_INDEX;
            int64_t last_item = b;
            while (last_item + grid < st.split.n_items) last_item += grid;
            for (int64_t item = last_item; item >= b; item -= grid) {
                const int64_t lo = item * span, hi = lo + span < n_shift ? lo + span : n_shift;
                // the tile: entry l is D_{e-1}[lo - reach + l], the indices outside the axis moved onto an element inside it
                tile.assign((size_t)(span + 2 * reach), 0.0);
                if (e)
                    for (int64_t l = span + 2 * (int64_t)reach - 1; l >= 0; --l) {
                        int64_t g = lo - reach + l;
                        g = g < 0 ? 0 : g;
                        tile[(size_t)l] = Din[sushi::axis_at(g, n_shift)];
                    }
                for (int64_t j = hi - 1; j >= lo; --j) {
                    const double u = sushi::path_cost(method, rows[(size_t)e].weight, r[j]);
                    double dn = u;
                    if (e) {
                        const int64_t l = reach + (j - lo);
                        // the widest move first, +a before -a, the value itself last
                        bool have = false;
                        double near = 0.0; int32_t nd = 0;
                        for (int32_t a = reach; a >= 1; --a) {
                            const double price = sushi::track_price(step_cost, a);
                            const double c_hi = sushi::track_cand(tile[(size_t)(l + a)], price);
                            const double c_lo = sushi::track_cand(tile[(size_t)(l - a)], price);
                            if (j + a < n_shift && (!have || sushi::track_replaces(c_hi, a, near, nd))) { near = c_hi; nd = a; have = true; }
                            if (j - a >= 0 && (!have || sushi::track_replaces(c_lo, -a, near, nd))) { near = c_lo; nd = -a; have = true; }
                        }
                        if (!have || sushi::track_replaces(tile[(size_t)l], 0, near, nd)) { near = tile[(size_t)l]; nd = 0; }
                        // the kernel's order, 0, -1, +1, -2, +2, ..., in which the rule is the strict comparison: the same winner
                        double near_fwd = tile[(size_t)l]; int32_t nd_fwd = 0;
                        for (int32_t a = 1; a <= reach; ++a) {
                            const double price = sushi::track_price(step_cost, a);
                            const double c_lo = sushi::track_cand(tile[(size_t)(l - a)], price);
                            if (j - a >= 0 && sushi::track_replaces_in_order(c_lo, near_fwd)) { near_fwd = c_lo; nd_fwd = -a; }
                            const double c_hi = sushi::track_cand(tile[(size_t)(l + a)], price);
                            if (j + a < n_shift && sushi::track_replaces_in_order(c_hi, near_fwd)) { near_fwd = c_hi; nd_fwd = a; }
                        }
                        if (nd_fwd != nd || std::memcmp(&near_fwd, &near, sizeof near)) {
                            std::fprintf(stderr, "row %d shift %lld: the two candidate orders disagree\n", e, (long long)j);
                            return 4;
                        }
                        dn = sushi::track_step(near, nd, u, jump, &mv[j]);
                    }
                    Dout[j] = dn;
                    if (sushi::path_min_replaces(dn, (int32_t)j, best, at)) { best = dn; at = (int32_t)j; }
                    if (sushi::path_own_replaces(method, r[j], (int32_t)j, own, own_at)) { own = r[j]; own_at = (int32_t)j; }
                }
            }
            p_min[(size_t)b] = best; p_arg[(size_t)b] = at; p_own_idx[(size_t)b] = own_at; p_own_val[(size_t)b] = own;
        }
        double best = INFINITY; int32_t at = sushi::PATH_NO_INDEX;
        float own = worst; int32_t own_at = sushi::PATH_NO_INDEX;
        for (int b = grid - 1; b >= 0; --b) {
            if (sushi::path_min_replaces(p_min[(size_t)b], p_arg[(size_t)b], best, at)) { best = p_min[(size_t)b]; at = p_arg[(size_t)b]; }
            if (sushi::path_own_replaces(method, p_own_val[(size_t)b], p_own_idx[(size_t)b], own, own_at)) {
                own = p_own_val[(size_t)b]; own_at = p_own_idx[(size_t)b];
            }
        }
        row_min[(size_t)e] = best; row_arg[(size_t)e] = sushi::path_clamp(at, n_shift);
        own_idx[(size_t)e] = sushi::path_clamp(own_at, n_shift); own_val[(size_t)e] = own;
    }
    sushi::track_backtrack(moves.data(), row_arg.data(), E, n_shift, shifts.data());
    using host_check::part;
    return host_check::write_file(out_path, {part(shifts), part(row_arg), part(own_idx), part(own_val), part(row_min), part(moves)});
}

}  // namespace

int main(int argc, char** argv) {
    if (argc == 2 && !std::strcmp(argv[1], "validate")) return validate();
    if (argc == 10 && !std::strcmp(argv[1], "pass")) return pass(argv[2], argv[3], argv[4], argv[5], argv[6], argv[7], argv[8], argv[9]);
    std::fprintf(stderr, "usage: %s validate | pass <sqdiff|ccoeff> <penalty> <step_cost> <n_shift> <curves> <rows> <reach> <output>\n",
                 argv[0]);
    return 2;
}
