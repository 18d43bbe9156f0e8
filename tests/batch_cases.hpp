// The table of batches that the stand-alone CPU checks of the batch's host side share: tests/host_plan_check.cpp (what a plan must
// be) and tests/host_batch_check.cpp (what a staged batch must be) both include this file and go through the same cases.
#ifndef SUSHI_TESTS_BATCH_CASES_HPP
#define SUSHI_TESTS_BATCH_CASES_HPP

#include "../sushi_amd/csrc/sushi_geometry.hpp"
#include "../sushi_amd/csrc/plan_core.hpp"

#include <string>
#include <vector>

namespace batch_cases {

using namespace sushi;

constexpr int FFT_PATH_TILE = 16384;      // the direct path's tile the FFT path's descriptors are made with (its largest variant's)

// ---- the cases ----
enum CapKind { CAP_GIVEN, CAP_HALFWAY };  // HALFWAY: between ws_extremes' need_one and need_all -- a greedy cut into several sub-batches
struct Case {
    std::string name;
    std::vector<SushiHipRequest> req;
    CapKind cap_kind;
    size_t cap;
    std::string lanes;                    // the override ("": none)
};

inline SushiHipRequest request(int64_t tmpl_off, int64_t win_start, int32_t tmpl_len, int32_t n_pos) {
    SushiHipRequest r;
    memset(&r, 0, sizeof(r));
    r.tmpl_off = tmpl_off; r.win_start = win_start; r.tmpl_len = tmpl_len; r.n_pos = n_pos;
    return r;
}

inline std::vector<Case> cases() {
    std::vector<Case> c;
    const int64_t PAIR = (int64_t)FFT_STEP * FFT_SEG;                       // samples between two pairs of the absolute grid
    // a. one search of one position
    c.push_back({"a_one", {request(0, 0, 1, 1)}, CAP_GIVEN, 0, ""});
    // b. the four requests of tests/test_native_abi.py::test_host_only_entry_points
    std::vector<SushiHipRequest> four;
    const int64_t four_win[4] = {100000, 140000, 190000, 300000};
    for (int k = 0; k < 4; ++k) four.push_back(request(40000 * k, four_win[k], 36000, 240001));
    c.push_back({"b_four_cap0", four, CAP_GIVEN, 0, ""});
    c.push_back({"b_four_cap1", four, CAP_GIVEN, 1, ""});
    c.push_back({"b_four_cap2p40", four, CAP_GIVEN, (size_t)1 << 40, ""});
    c.push_back({"b_four_4x2_cap0", four, CAP_GIVEN, 0, "4:2"});
    c.push_back({"b_four_4x2_cap1", four, CAP_GIVEN, 1, "4:2"});
    c.push_back({"b_four_1x1", four, CAP_GIVEN, 0, "1:1"});
    // c. its 3000 requests: nine parts on three lanes by themselves, and the pending whole cut
    std::vector<SushiHipRequest> big;
    for (int k = 0; k < 3000; ++k) big.push_back(request(28000 * (int64_t)k, 28000 * (int64_t)k, 36000, 2880001));
    c.push_back({"c_3000_auto", big, CAP_GIVEN, 0, ""});
    c.push_back({"c_3000_1x1", big, CAP_GIVEN, 0, "1:1"});
    // d. 24 searches: every mac_class at least twice, two patterns of more than 30 segments, window starts out of order, two
    // windows (2 and 5) that begin in the same pair
    const int d_segs[24] = {1, 6, 7, 12, 13, 18, 19, 24, 25, 30, 31, 40, 3, 9, 15, 21, 27, 2, 8, 14, 20, 26, 5, 11};
    std::vector<SushiHipRequest> mixed;
    for (int k = 0; k < 24; ++k) {
        int64_t win = (int64_t)((k * 7) % 24) * 150000 + 13 * k;
        if (k == 2) win = 10 * PAIR + 100;
        if (k == 5) win = 10 * PAIR + 5000;
        mixed.push_back(request(1000 * k, win, (d_segs[k] - 1) * FFT_SEG + 1 + (k * 977) % (FFT_SEG - 1), 50000 + 9001 * k));
    }
    c.push_back({"d_mixed_cap0", mixed, CAP_GIVEN, 0, ""});
    c.push_back({"d_mixed_halfway", mixed, CAP_HALFWAY, 0, ""});
    // e. 130 searches whose pairs just reach LANES_MIN_PAIRS (6 x 190 + 124 x 189 = 24576), and the same without the last
    std::vector<SushiHipRequest> edge;
    for (int k = 0; k < 130; ++k) edge.push_back(request(0, 3 * PAIR * k, 5000, (int32_t)((k < 6 ? 190 : 189) * PAIR)));
    c.push_back({"e_130_reaches", edge, CAP_GIVEN, 0, ""});
    // (and cut into eight parts on two lanes under a cap that does not hold the batch as one: a whole cut of several sub-batches)
    c.push_back({"e_130_8x2_halfway", edge, CAP_HALFWAY, 0, "8:2"});
    edge.pop_back();
    c.push_back({"e_129_below", edge, CAP_GIVEN, 0, ""});
    // f. overrides that are ignored or clamped
    c.push_back({"f_0x1", four, CAP_GIVEN, 0, "0:1"});
    c.push_back({"f_3x9", four, CAP_GIVEN, 0, "3:9"});
    c.push_back({"f_65x2", four, CAP_GIVEN, 0, "65:2"});
    c.push_back({"f_2", four, CAP_GIVEN, 0, "2"});
    c.push_back({"f_empty", four, CAP_GIVEN, 0, ""});
    c.push_back({"f_5x4_of_3", std::vector<SushiHipRequest>(four.begin(), four.begin() + 3), CAP_GIVEN, 0, "5:4"});
    // g. refusals
    std::vector<SushiHipRequest> bad = four;
    bad[2].n_pos = 0;
    c.push_back({"g_n_pos_0", bad, CAP_GIVEN, 0, ""});
    bad = four; bad[1].tmpl_off = -1;
    c.push_back({"g_tmpl_off_neg", bad, CAP_GIVEN, 0, ""});
    bad = four; bad[3].n_pos = 0x7fffffff - 65536 + 1;
    c.push_back({"g_n_pos_large", bad, CAP_GIVEN, 0, ""});
    // (87379 pairs each: 13000 of them pass 0x7fffffff / 2 -- make_plan refuses before it builds anything)
    c.push_back({"g_pairs_past_int", std::vector<SushiHipRequest>(13000, request(0, 0, 1, 0x7fffffff - 65536)), CAP_GIVEN, 0, ""});
    return c;
}

// the workspace cap a case is planned under
inline size_t case_cap(const Case& c, const std::vector<SearchDesc>& descs) {
    if (c.cap_kind != CAP_HALFWAY) return c.cap;
    size_t need_one = 0, need_all = 0;
    ws_extremes(search_layouts(descs), &need_one, &need_all);
    return need_one + (need_all - need_one) / 2;
}

}  // namespace batch_cases
#endif
