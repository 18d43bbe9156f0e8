// tests/host_pilot_rows_check.cpp -- run_policy.hpp's rule for how the band-split form's pilots get their whole rows, on the CPU.
// usage: host_pilot_rows_check     exit 1 with a message on the first violation
// Built with plain g++ (tests/test_pilot_rows_host.py), no HIP; sushi_fft.hip includes the same header.
#include <stdio.h>

#include "../include/sushi_hip.h"
#include "../sushi_amd/csrc/run_policy.hpp"

using namespace sushi;

#define REQUIRE(cond, what)                                                              \
    do {                                                                                 \
        if (!(cond)) { fprintf(stderr, "pilot_rows_route: %s [%s]\n", what, #cond); return 1; } \
    } while (0)

int main() {
    // nothing set, or set to nothing: search by search
    REQUIRE(pilot_rows_route(nullptr) == PILOT_ROWS_BY_SEARCH && pilot_rows_route("") == PILOT_ROWS_BY_SEARCH, "the default");
    REQUIRE(pilot_rows_route("search") == PILOT_ROWS_BY_SEARCH, "the default by its name");
    REQUIRE(pilot_rows_route("list") == PILOT_ROWS_LIST, "the earlier route");
    // a value that names neither route is refused, not read as the default: an A/B run must not become an A/A run by a typo
    for (const char* bad : {"List", "list ", " list", "lists", "lis", "0", "1", "searches", "rows"})
        REQUIRE(pilot_rows_route(bad) < 0, bad);
    REQUIRE(pilot_rows_by_search(PILOT_ROWS_BY_SEARCH) && !pilot_rows_by_search(PILOT_ROWS_LIST), "which route forms the pilots search by search");
    REQUIRE(PILOT_ROWS_BY_SEARCH == 0, "a zeroed handle takes the default");
    return 0;
}
