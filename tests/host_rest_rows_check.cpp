// tests/host_rest_rows_check.cpp -- run_policy.hpp's rules for the survivors' pass of the band-split form, on the CPU: which unit of
// work the pass takes (rest_rows_route: SUSHI_HIP_REST_ROWS) and how a search's pairs to form are cut into work items
// (rest_pair_to_form, rest_item_starts, rest_item_take: the three functions dense_search_kernel and mac_rows_kernel call).
// usage: host_rest_rows_check          the route rule; exit 1 with a message on the first violation
//        host_rest_rows_check cut      reads cases from stdin, one a line: "<pairs per item, 0: REST_ITEM_PAIRS> <audit pair, -1: none>
//                                      <marks: a string of 0 / 1, one per pair of the search>"; prints per case one line, the items
//                                      separated by '|', each the pairs it forms: what the device forms, walked the way the
//                                      device walks -- the builder 64 pairs at a time from the search's first pair, the consumer
//                                      64 pairs at a time from the item's first pair
// Built with plain g++ (tests/test_rest_rows_host.py), no HIP; sushi_fft.hip includes the same header.
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "../include/sushi_hip.h"
#include "../sushi_amd/csrc/run_policy.hpp"

using namespace sushi;

#define REQUIRE(cond, what)                                                             \
    do {                                                                                \
        if (!(cond)) { fprintf(stderr, "rest_rows_route: %s [%s]\n", what, #cond); return 1; } \
    } while (0)

// which of the 64 pairs from `base` on are to form (the device: one lane per pair, a ballot)
static unsigned long long form_mask(const std::string& marks, int base, int audit) {
    unsigned long long form = 0;
    for (int j = 0; j < 64; ++j) {
        const int i = base + j;
        const int listed = i < (int)marks.size() && marks[(size_t)i] == '1' ? 2 : 0;          // (MARK_LISTED)
        if (i < (int)marks.size() && rest_pair_to_form(listed, i, audit)) form |= 1ull << j;
    }
    return form;
}

static int cut_cases() {
    char line[8192];
    while (fgets(line, sizeof line, stdin)) {
        int per_item = 0, audit = -1;
        char marks_c[8000];
        marks_c[0] = 0;
        if (sscanf(line, "%d %d %7999s", &per_item, &audit, marks_c) < 2) { fprintf(stderr, "bad case: %s", line); return 1; }
        const std::string marks = strcmp(marks_c, "-") ? marks_c : "";
        if (per_item == 0) per_item = REST_ITEM_PAIRS;
        const int n = (int)marks.size();
        // the builder (dense_search_kernel)
        std::vector<int> items;
        int formed = 0;
        for (int base = 0; base < n; base += 64) {
            const unsigned long long form = form_mask(marks, base, audit);
            unsigned long long starts = rest_item_starts(form, formed, per_item);
            formed += __builtin_popcountll(form);
            for (; starts; starts &= starts - 1) items.push_back(base + __builtin_ctzll(starts));
        }
        // the consumer (mac_rows_kernel, ROWS_ITEMS)
        std::string out;
        for (size_t it = 0; it < items.size(); ++it) {
            if (it) out += "|";
            int room = per_item;
            bool first = true;
            for (int base = items[it]; base < n && room > 0; base += 64) {
                unsigned long long take = rest_item_take(form_mask(marks, base, audit), room);
                room -= __builtin_popcountll(take);
                for (; take; take &= take - 1) {
                    out += (first ? "" : " ") + std::to_string(base + __builtin_ctzll(take));
                    first = false;
                }
            }
        }
        printf("%s\n", out.c_str());
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc > 1 && !strcmp(argv[1], "cut")) return cut_cases();
    if (argc > 1 && !strcmp(argv[1], "pairs")) { printf("%d\n", REST_ITEM_PAIRS); return 0; }
    // nothing set, or set to nothing: by items
    REQUIRE(rest_rows_route(nullptr) == REST_ROWS_BY_ITEM && rest_rows_route("") == REST_ROWS_BY_ITEM, "the default");
    REQUIRE(rest_rows_route("items") == REST_ROWS_BY_ITEM, "the default by its name");
    REQUIRE(rest_rows_route("search") == REST_ROWS_BY_SEARCH, "the earlier route");
    // a value that names neither route is refused, not read as the default: an A/B run must not become an A/A run by a typo
    for (const char* bad : {"Search", "search ", " search", "searches", "sear", "0", "1", "item", "list", "rows"})
        REQUIRE(rest_rows_route(bad) < 0, bad);
    REQUIRE(rest_rows_by_item(REST_ROWS_BY_ITEM) && !rest_rows_by_item(REST_ROWS_BY_SEARCH), "which route strides over items");
    REQUIRE(REST_ROWS_BY_ITEM == 0, "a zeroed handle takes the default");
    REQUIRE(REST_ITEM_PAIRS == 2 || REST_ITEM_PAIRS == 4 || REST_ITEM_PAIRS == 8, "one of the measured values");
    return 0;
}
