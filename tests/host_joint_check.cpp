// sushi_hip_joint_reduce on the CPU (sushi_amd/csrc/joint_core.hpp): the call's host side -- stage_joint's refusals, the workspace's
// layout, the work split -- and its arithmetic, joint_value and the first-extremum rule, over whole groups.
// usage: host_joint_check validate
//          prints "<case> <return code>" for good and bad tables (sizes up to INT64_MAX), then the facts of staged calls.
//        host_joint_check reduce <sqdiff|ccoeff> <curves file> <rows file> <groups file> <output file>
//          curves: raw float32; rows: SushiHipJointRow records; groups: SushiHipJointGroup records.  The output file holds
//          [index i32 x groups][score f32 x groups][row score f32 x rows][row own index i32 x rows][row own value f32 x rows]
//          [the joint rows, back to back]: what sushi_hip_joint_reduce returns.  The test compares it with
//          sushi_amd.joint.joint_host, bit for bit.
// Built by tests/test_joint_host.py with g++ -O2 -std=c++17 -ffp-contract=off -fsanitize=address,undefined.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "../include/sushi_hip.h"
#include "../sushi_amd/csrc/joint_core.hpp"
#include "host_check_io.hpp"

namespace {

using host_check::read_file;
using host_check::records;
using sushi::JointStage;

constexpr int64_t MAX64 = std::numeric_limits<int64_t>::max();

struct Tables {
    std::vector<SushiHipJointRow> rows;
    std::vector<SushiHipJointGroup> groups;
    int64_t n_curve;
    int method;
};

// three groups of 2, 1 and 3 rows on a buffer of 1000 floats
Tables good() {
    Tables t;
    t.rows = {{0, 0.5}, {7, 0.5}, {100, 1.0}, {500, 1.0 / 3.0}, {501, 0.0}, {333, 2.0}};
    t.groups = {{0, 2, 93, 0}, {2, 1, 1, 0}, {3, 3, 499, 0}};
    t.n_curve = 1000;
    t.method = SUSHI_HIP_METHOD_SQDIFF_NORMED;
    return t;
}

int stage_counts(const Tables& t, JointStage& st, int n_rows, int n_groups) {
    return sushi::stage_joint(t.rows.data(), n_rows, t.groups.data(), n_groups, t.n_curve, t.method, st);
}
int stage(const Tables& t, JointStage& st) { return stage_counts(t, st, (int)t.rows.size(), (int)t.groups.size()); }

void report(const char* name, int rc) { std::printf("%s %d\n", name, rc); }

void facts(const char* name, const Tables& t) {
    JointStage st;
    const int rc = stage(t, st);
    std::printf("%s rc=%d", name, rc);
    if (rc == SUSHI_HIP_OK) {
        std::printf(" per=%d items=%lld joint=%lld grid=%u bytes=%zu", st.per, (long long)st.n_items, (long long)st.n_joint, st.grid,
                    st.image.size());
        const sushi::JointGroupDev* g = reinterpret_cast<const sushi::JointGroupDev*>(st.image.data() + st.lay.groups);
        const sushi::JointRowDev* r = reinterpret_cast<const sushi::JointRowDev*>(st.image.data() + st.lay.rows);
        for (size_t k = 0; k < t.groups.size(); ++k)
            std::printf(" g%zu=(%lld,%lld,%d,%d,%d)", k, (long long)g[k].first_item, (long long)g[k].joint_off, g[k].first_row, g[k].n_rows,
                        g[k].n_shift);
        bool rows_ok = true, keys_ok = true;
        for (size_t k = 0; k < t.rows.size(); ++k)
            rows_ok = rows_ok && r[k].curve_off == t.rows[k].curve_off && r[k].weight == t.rows[k].weight &&
                      t.groups[(size_t)r[k].group].first_row <= (int)k &&
                      (int)k < t.groups[(size_t)r[k].group].first_row + t.groups[(size_t)r[k].group].n_rows;
        for (size_t b = st.lay.group_keys; b < st.lay.bytes; ++b) keys_ok = keys_ok && (unsigned char)st.image[b] == 0xff;
        std::printf(" rows_ok=%d keys_ok=%d", (int)rows_ok, (int)keys_ok);
    }
    std::printf("\n");
}

int validate() {
    JointStage st;
    Tables t = good();
    report("good", stage(t, st));
    t = good(); t.method = SUSHI_HIP_METHOD_CCOEFF_NORMED; report("good_ccoeff", stage(t, st));
    t = good(); t.method = 2; report("method_2", stage(t, st));
    t = good(); t.method = -1; report("method_neg", stage(t, st));
    t = good(); report("no_groups", stage_counts(t, st, 6, 0));
    t = good(); report("no_rows", stage_counts(t, st, 0, 3));
    t = good(); report("negative_counts", stage_counts(t, st, -6, -3));
    t = good(); report("fewer_rows_than_groups", stage_counts(t, st, 2, 3));
    t = good(); t.n_curve = 0; report("empty_curves", stage(t, st));
    t = good(); t.n_curve = -5; report("negative_curves", stage(t, st));
    t = good(); t.groups[1].first_row = 1; report("group_overlaps", stage(t, st));
    t = good(); t.groups[1].first_row = 3; report("group_gap", stage(t, st));
    t = good(); t.groups[0].first_row = 1; report("first_group_not_at_0", stage(t, st));
    t = good(); std::swap(t.groups[0], t.groups[1]); report("groups_out_of_order", stage(t, st));
    t = good(); t.groups[1].n_rows = 0; report("group_without_rows", stage(t, st));
    t = good(); t.groups[1].n_rows = -1; report("group_negative_rows", stage(t, st));
    t = good(); t.groups[2].n_rows = 2; report("rows_left_over", stage(t, st));
    t = good(); t.groups[2].n_rows = 4; report("rows_missing", stage(t, st));
    t = good(); t.groups[2].n_rows = std::numeric_limits<int32_t>::max(); report("rows_int32_max", stage(t, st));
    t = good(); t.groups[0].n_shift = 0; report("no_shift", stage(t, st));
    t = good(); t.groups[0].n_shift = -3; report("negative_shift", stage(t, st));
    t = good(); t.groups[0].n_shift = 1001; report("shift_beyond_curves", stage(t, st));
    t = good(); t.rows[0].curve_off = -1; report("row_before_curves", stage(t, st));
    t = good(); t.rows[5].curve_off = 501; report("row_ends_at_curves_end", stage(t, st));
    t = good(); t.rows[5].curve_off = 502; report("row_one_past_curves_end", stage(t, st));
    t = good(); t.rows[2].curve_off = 999; report("single_shift_last_float", stage(t, st));
    t = good(); t.rows[2].curve_off = 1000; report("single_shift_past_end", stage(t, st));
    // sums that do not fit 64 bits are never formed
    t = good(); t.rows[5].curve_off = MAX64; report("row_at_int64_max", stage(t, st));
    t = good(); t.rows[5].curve_off = MAX64 - 498; report("row_sum_overflows", stage(t, st));
    t = good(); t.n_curve = MAX64; t.rows[5].curve_off = MAX64 - 499; report("huge_curves_row_at_end", stage(t, st));
    t = good(); t.n_curve = MAX64; t.rows[5].curve_off = MAX64 - 498; report("huge_curves_row_past_end", stage(t, st));
    t = good(); t.n_curve = MAX64; t.groups[2].n_shift = std::numeric_limits<int32_t>::max(); t.rows[3].curve_off = MAX64 / 2;
    report("huge_curves_int32_max_shifts", stage(t, st));
    t = good(); t.rows[1].weight = std::nan(""); report("weight_nan", stage(t, st));
    t = good(); t.rows[1].weight = INFINITY; report("weight_inf", stage(t, st));
    t = good(); t.rows[1].weight = -INFINITY; report("weight_neg_inf", stage(t, st));
    t = good(); t.rows[1].weight = -1e-300; report("weight_negative", stage(t, st));
    t = good(); t.rows[1].weight = -0.0; report("weight_neg_zero", stage(t, st));
    t = good(); t.rows[1].weight = 1e300; report("weight_large", stage(t, st));

    std::printf("bytes %zu %zu %zu %zu %zu %zu\n", sushi::joint_layout_bytes(1, 1), sushi::joint_layout_bytes(3, 6),
                sushi::joint_layout_bytes(17, 40), sushi::joint_layout_bytes(0, 5), sushi::joint_layout_bytes(2, 1),
                sushi::joint_layout_bytes(-1, -1));
    facts("facts_good", good());
    // one group at the size from which on the large items are taken, and one shift below it
    Tables big;
    big.rows = {{0, 1.0}, {1, 1.0}};
    big.groups = {{0, 2, 2048 * 2048, 0}};
    big.n_curve = (int64_t)1 << 40;
    big.method = SUSHI_HIP_METHOD_SQDIFF_NORMED;
    facts("facts_large_items", big);
    big.groups[0].n_shift = 2048 * 2047;
    facts("facts_small_items", big);
    big.groups[0].n_shift = std::numeric_limits<int32_t>::max();
    facts("facts_int32_max", big);
    return 0;
}

int reduce(const char* method_name, const char* curves_path, const char* rows_path, const char* groups_path, const char* out_path) {
    const int method = !std::strcmp(method_name, "ccoeff") ? SUSHI_HIP_METHOD_CCOEFF_NORMED : SUSHI_HIP_METHOD_SQDIFF_NORMED;
    const std::vector<float> curves = records<float>(read_file(curves_path));
    const std::vector<SushiHipJointRow> rows = records<SushiHipJointRow>(read_file(rows_path));
    const std::vector<SushiHipJointGroup> groups = records<SushiHipJointGroup>(read_file(groups_path));
    JointStage st;
    const int rc = sushi::stage_joint(rows.data(), (int)rows.size(), groups.data(), (int)groups.size(), (int64_t)curves.size(), method, st);
    if (rc != SUSHI_HIP_OK) { std::fprintf(stderr, "stage_joint refused the tables: %d\n", rc); return 3; }
    // from here on the staged image is what is read, as on the device
    const sushi::JointGroupDev* gd = reinterpret_cast<const sushi::JointGroupDev*>(st.image.data() + st.lay.groups);
    const sushi::JointRowDev* rd = reinterpret_cast<const sushi::JointRowDev*>(st.image.data() + st.lay.rows);
    std::vector<int32_t> idx(groups.size()), row_idx(rows.size());
    std::vector<float> score(groups.size()), row_score(rows.size()), row_best(rows.size()), joint((size_t)st.n_joint);
    for (size_t g = 0; g < groups.size(); ++g) {
        const sushi::JointGroupDev& G = gd[g];
        float* jr = joint.data() + G.joint_off;
        for (int32_t j = 0; j < G.n_shift; ++j) jr[j] = sushi::joint_value(curves.data(), rd, G.first_row, G.n_rows, j);
        idx[g] = sushi::joint_first_extremum(jr, G.n_shift, method);
        score[g] = jr[idx[g]];
        for (int i = G.first_row; i < G.first_row + G.n_rows; ++i) {
            const float* r = curves.data() + rd[i].curve_off;
            row_idx[(size_t)i] = sushi::joint_first_extremum(r, G.n_shift, method);
            row_best[(size_t)i] = r[row_idx[(size_t)i]];
            row_score[(size_t)i] = r[idx[g]];
        }
    }
    using host_check::part;
    return host_check::write_file(out_path, {part(idx), part(score), part(row_score), part(row_idx), part(row_best), part(joint)});
}

}  // namespace

int main(int argc, char** argv) {
    if (argc == 2 && !std::strcmp(argv[1], "validate")) return validate();
    if (argc == 7 && !std::strcmp(argv[1], "reduce")) return reduce(argv[2], argv[3], argv[4], argv[5], argv[6]);
    std::fprintf(stderr, "usage: %s validate | reduce <sqdiff|ccoeff> <curves> <rows> <groups> <output>\n", argv[0]);
    return 2;
}
