// sushi_hip_drift_reduce on the CPU (sushi_amd/csrc/drift_core.hpp): the call's host side -- stage_drift's refusals, the workspace's
// layout, the work split -- and its arithmetic, drift_value and the first-extremum rule, over whole offset tables.
// usage: host_drift_check validate
//          prints "<case> <return code>" for good and bad tables (offsets up to INT32_MIN, sizes up to INT64_MAX), then the facts of
//          staged calls.
//        host_drift_check reduce <sqdiff|ccoeff> <n_shift> <curves file> <rows file> <offsets file> <output file>
//          curves: raw float32; rows: SushiHipJointRow records; offsets: int32 [n_drifts][n_rows].  The output file holds
//          [drift i32, index i32][score f32][row score f32 x rows][candidate index i32 x drifts][candidate score f32 x drifts]
//          [the lines, n_drifts x n_shift f32]: what sushi_hip_drift_reduce returns.  The test compares it with
//          sushi_amd.drift.drift_host, bit for bit.
// Built by tests/test_drift_host.py with g++ -O2 -std=c++17 -ffp-contract=off -fsanitize=address,undefined.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "../include/sushi_hip.h"
#include "../sushi_amd/csrc/drift_core.hpp"
#include "host_check_io.hpp"

namespace {

using host_check::read_file;
using host_check::records;
using sushi::DriftStage;

constexpr int64_t MAX64 = std::numeric_limits<int64_t>::max();
constexpr int32_t MIN32 = std::numeric_limits<int32_t>::min(), MAX32 = std::numeric_limits<int32_t>::max();

struct Tables {
    std::vector<SushiHipJointRow> rows;
    std::vector<int32_t> offsets;       // [n_drifts][rows]
    int n_drifts;
    int32_t n_shift;
    int64_t n_curve;
    int method;
};

// three rows of 93 shifts on a buffer of 1000 floats, six candidates
Tables good() {
    Tables t;
    t.rows = {{0, 0.5}, {7, 1.0 / 3.0}, {907, 0.0}};
    t.offsets = {0, 0, 0, /**/ -3, 2, 0, /**/ 5, 1, 9, /**/ -4, -1, -92, /**/ 92, 0, 0, /**/ -46, 46, 0};
    t.n_drifts = 6;
    t.n_shift = 93;
    t.n_curve = 1000;
    t.method = SUSHI_HIP_METHOD_SQDIFF_NORMED;
    return t;
}

int stage_counts(const Tables& t, DriftStage& st, int n_rows, int n_drifts) {
    return sushi::stage_drift(t.rows.data(), n_rows, t.n_shift, t.offsets.data(), n_drifts, t.n_curve, t.method, st);
}
int stage(const Tables& t, DriftStage& st) { return stage_counts(t, st, (int)t.rows.size(), t.n_drifts); }

void report(const char* name, int rc) { std::printf("%s %d\n", name, rc); }

void facts(const char* name, const Tables& t) {
    DriftStage st;
    const int rc = stage(t, st);
    std::printf("%s rc=%d", name, rc);
    if (rc == SUSHI_HIP_OK) {
        const int n_rows = (int)t.rows.size();
        std::printf(" per=%d jitems=%lld items=%lld grid=%u bytes=%zu", st.per, (long long)st.n_jitems, (long long)st.n_items, st.grid,
                    st.image.size());
        const SushiHipJointRow* r = reinterpret_cast<const SushiHipJointRow*>(st.image.data() + st.lay.rows);
        const int32_t* o = reinterpret_cast<const int32_t*>(st.image.data() + st.lay.offs);
        const sushi::DriftRange* g = reinterpret_cast<const sushi::DriftRange*>(st.image.data() + st.lay.ranges);
        const int64_t slots = sushi::drift_blocks(t.n_drifts) * sushi::DRIFT_DB;
        for (int d = 0; d < t.n_drifts && d < 8; ++d) std::printf(" r%d=[%d,%d)", d, g[d].lo, g[d].hi);
        bool rows_ok = true, offs_ok = true, pad_ok = true, keys_ok = true;
        for (int e = 0; e < n_rows; ++e)
            rows_ok = rows_ok && r[e].curve_off == t.rows[(size_t)e].curve_off && r[e].weight == t.rows[(size_t)e].weight;
        for (int64_t d = 0; d < slots; ++d)
            for (int e = 0; e < n_rows; ++e) {
                const int64_t from = d < t.n_drifts ? d : t.n_drifts - 1;
                offs_ok = offs_ok && o[sushi::drift_offset_at(n_rows, (int)d, e)] == t.offsets[(size_t)(from * n_rows + e)];
            }
        for (int64_t d = t.n_drifts; d < slots; ++d) pad_ok = pad_ok && g[d].lo == 0 && g[d].hi == 0;
        for (size_t b = st.lay.keys; b < st.lay.bytes; ++b) keys_ok = keys_ok && (unsigned char)st.image[b] == 0xff;
        std::printf(" rows_ok=%d offs_ok=%d pad_ok=%d keys_ok=%d", (int)rows_ok, (int)offs_ok, (int)pad_ok, (int)keys_ok);
    }
    std::printf("\n");
}

int validate() {
    DriftStage st;
    Tables t = good();
    report("good", stage(t, st));
    t = good(); t.method = SUSHI_HIP_METHOD_CCOEFF_NORMED; report("good_ccoeff", stage(t, st));
    t = good(); t.method = 2; report("method_2", stage(t, st));
    t = good(); t.method = -1; report("method_neg", stage(t, st));
    t = good(); report("null_rows", sushi::stage_drift(nullptr, 3, t.n_shift, t.offsets.data(), 6, t.n_curve, t.method, st));
    t = good(); report("null_offsets", sushi::stage_drift(t.rows.data(), 3, t.n_shift, nullptr, 6, t.n_curve, t.method, st));
    t = good(); report("no_rows", stage_counts(t, st, 0, 6));
    t = good(); report("negative_rows", stage_counts(t, st, -3, 6));
    t = good(); report("no_drifts", stage_counts(t, st, 3, 0));
    t = good(); report("negative_drifts", stage_counts(t, st, 3, -1));
    t = good(); report("drifts_65536", stage_counts(t, st, 3, 65536));
    t = good(); report("drifts_int32_max", stage_counts(t, st, 3, MAX32));
    t = good(); t.n_shift = 0; report("no_shift", stage(t, st));
    t = good(); t.n_shift = -93; report("negative_shift", stage(t, st));
    t = good(); t.n_curve = 0; report("empty_curves", stage(t, st));
    t = good(); t.n_curve = -5; report("negative_curves", stage(t, st));
    t = good(); t.n_curve = 92; report("shift_beyond_curves", stage(t, st));
    t = good(); t.rows[0].curve_off = -1; report("row_before_curves", stage(t, st));
    t = good(); t.rows[2].curve_off = 907; report("row_ends_at_curves_end", stage(t, st));
    t = good(); t.rows[2].curve_off = 908; report("row_one_past_curves_end", stage(t, st));
    // sums that do not fit 64 bits are never formed
    t = good(); t.rows[2].curve_off = MAX64; report("row_at_int64_max", stage(t, st));
    t = good(); t.rows[2].curve_off = MAX64 - 92; report("row_sum_overflows", stage(t, st));
    t = good(); t.n_curve = MAX64; t.rows[2].curve_off = MAX64 - 93; report("huge_curves_row_at_end", stage(t, st));
    t = good(); t.n_curve = MAX64; t.rows[2].curve_off = MAX64 - 92; report("huge_curves_row_past_end", stage(t, st));
    t = good(); t.rows[1].weight = std::nan(""); report("weight_nan", stage(t, st));
    t = good(); t.rows[1].weight = INFINITY; report("weight_inf", stage(t, st));
    t = good(); t.rows[1].weight = -INFINITY; report("weight_neg_inf", stage(t, st));
    t = good(); t.rows[1].weight = -1e-300; report("weight_negative", stage(t, st));
    t = good(); t.rows[1].weight = -0.0; report("weight_neg_zero", stage(t, st));
    t = good(); t.rows[1].weight = 1e300; report("weight_large", stage(t, st));
    // valid ranges: a single index is one, an empty one is refused, whatever the offsets' size
    t = good(); t.offsets[9 + 2] = -93; report("offset_minus_n_shift", stage(t, st));
    t = good(); t.offsets[12] = 93; report("offset_n_shift", stage(t, st));
    t = good(); t.offsets[15] = -47; report("reach_is_n_shift", stage(t, st));
    t = good(); t.offsets[16] = 47; report("reach_is_n_shift_above", stage(t, st));
    t = good(); t.offsets[4] = MIN32; report("offset_int32_min", stage(t, st));
    t = good(); t.offsets[4] = MAX32; report("offset_int32_max", stage(t, st));
    t = good(); t.offsets[3] = MIN32; t.offsets[4] = MAX32; report("offsets_int32_min_and_max", stage(t, st));
    t = good(); t.n_shift = 1; t.n_curve = 1000; report("one_shift_offsets_not_zero", stage(t, st));
    t = good(); t.n_shift = 1; t.offsets.assign(18, 0); report("one_shift_offsets_zero", stage(t, st));
    t = good(); t.n_shift = MAX32; t.n_curve = MAX64; t.offsets[4] = MAX32 - 1; t.offsets[3] = 0; report("int32_max_shifts_single_index", stage(t, st));
    t = good(); t.n_shift = MAX32; t.n_curve = MAX64; t.offsets[4] = MAX32 - 1; report("int32_max_shifts_empty", stage(t, st));
    t = good(); report("bad_candidate_behind_n_drifts", stage_counts(t, st, 3, 5));
    t = good(); t.offsets[15] = -47; report("bad_candidate_not_counted", stage_counts(t, st, 3, 5));

    std::printf("bytes %zu %zu %zu %zu %zu %zu %zu\n", sushi::drift_layout_bytes(1, 1), sushi::drift_layout_bytes(3, 6),
                sushi::drift_layout_bytes(64, 8641), sushi::drift_layout_bytes(0, 5), sushi::drift_layout_bytes(5, 0),
                sushi::drift_layout_bytes(5, 65536), sushi::drift_layout_bytes(-1, -1));
    facts("facts_good", good());
    // the size from which on the large items are taken (2048 items of 2048 shifts x blocks), and one block below it
    Tables big;
    big.rows = {{0, 1.0}, {1, 1.0}};
    big.n_shift = 2048 * 8;
    big.n_curve = (int64_t)1 << 40;
    big.method = SUSHI_HIP_METHOD_SQDIFF_NORMED;
    big.n_drifts = 256 * sushi::DRIFT_DB;
    big.offsets.assign((size_t)big.n_drifts * 2, 1);
    facts("facts_large_items", big);
    big.n_drifts = 255 * sushi::DRIFT_DB;
    facts("facts_small_items", big);
    big.n_drifts = 65535;
    big.offsets.assign((size_t)big.n_drifts * 2, -1);
    big.n_shift = MAX32;
    facts("facts_int32_max", big);
    return 0;
}

int reduce(const char* method_name, const char* n_shift_text, const char* curves_path, const char* rows_path, const char* offsets_path,
           const char* out_path) {
    const int method = !std::strcmp(method_name, "ccoeff") ? SUSHI_HIP_METHOD_CCOEFF_NORMED : SUSHI_HIP_METHOD_SQDIFF_NORMED;
    const int32_t n_shift = (int32_t)std::atol(n_shift_text);
    const std::vector<float> curves = records<float>(read_file(curves_path));
    const std::vector<SushiHipJointRow> rows = records<SushiHipJointRow>(read_file(rows_path));
    const std::vector<int32_t> offsets = records<int32_t>(read_file(offsets_path));
    const int n_rows = (int)rows.size();
    if (n_rows < 1 || offsets.size() % rows.size()) { std::fprintf(stderr, "offsets are [n_drifts][n_rows]\n"); return 3; }
    const int n_drifts = (int)(offsets.size() / rows.size());
    DriftStage st;
    const int rc = sushi::stage_drift(rows.data(), n_rows, n_shift, offsets.data(), n_drifts, (int64_t)curves.size(), method, st);
    if (rc != SUSHI_HIP_OK) { std::fprintf(stderr, "stage_drift refused the tables: %d\n", rc); return 3; }
    // from here on the staged image is what is read, as on the device
    const SushiHipJointRow* rd = reinterpret_cast<const SushiHipJointRow*>(st.image.data() + st.lay.rows);
    const int32_t* od = reinterpret_cast<const int32_t*>(st.image.data() + st.lay.offs);
    const sushi::DriftRange* gd = reinterpret_cast<const sushi::DriftRange*>(st.image.data() + st.lay.ranges);
    std::vector<int32_t> best(2), drift_idx((size_t)n_drifts);
    std::vector<float> score(1), row_score((size_t)n_rows), drift_score((size_t)n_drifts);
    std::vector<float> lines((size_t)n_drifts * (size_t)n_shift, method == SUSHI_HIP_METHOD_CCOEFF_NORMED ? -INFINITY : INFINITY);
    for (int d = 0; d < n_drifts; ++d) {
        float* line = lines.data() + (size_t)d * (size_t)n_shift;
        for (int32_t j = gd[d].lo; j < gd[d].hi; ++j) line[j] = sushi::drift_value(curves.data(), rd, n_rows, od, d, j);
        drift_idx[(size_t)d] = gd[d].lo + sushi::joint_first_extremum(line + gd[d].lo, gd[d].hi - gd[d].lo, method);
        drift_score[(size_t)d] = line[drift_idx[(size_t)d]];
    }
    best[0] = sushi::joint_first_extremum(drift_score.data(), n_drifts, method);
    best[1] = drift_idx[(size_t)best[0]];
    score[0] = drift_score[(size_t)best[0]];
    for (int e = 0; e < n_rows; ++e)
        row_score[(size_t)e] = curves[(size_t)(rd[e].curve_off + best[1] + od[sushi::drift_offset_at(n_rows, best[0], e)])];
    using host_check::part;
    return host_check::write_file(out_path, {part(best), part(score), part(row_score), part(drift_idx), part(drift_score), part(lines)});
}

}  // namespace

int main(int argc, char** argv) {
    if (argc == 2 && !std::strcmp(argv[1], "validate")) return validate();
    if (argc == 8 && !std::strcmp(argv[1], "reduce")) return reduce(argv[2], argv[3], argv[4], argv[5], argv[6], argv[7]);
    std::fprintf(stderr, "usage: %s validate | reduce <sqdiff|ccoeff> <n_shift> <curves> <rows> <offsets> <output>\n", argv[0]);
    return 2;
}
