// Clamped score rows on the CPU (sushi_amd/csrc/rows_core.hpp): the calls' host side -- stage_rows' refusals, the work split, the
// in-place rule -- and their arithmetic: the pass / fill rule, the tile-range search and the checks of a hit list, tile by tile as
// the kernel goes.
// usage: host_rows_check validate
//          prints "<case> <return code>" for good and bad tables (sizes up to INT64_MAX), then the facts of staged calls.
//        host_rows_check form <fill bits, hex> <capacity> <n_out> <hits file> <counts file> <table file> <output file>
//          hits: SushiHipHit records [n][capacity]; counts: int64 [n]; table: SushiHipRowsRow records.  The output file holds
//          [n_out floats, 0x7fc00123 where no row lies][flags i32 x n]: what sushi_hip_rows_from_hits leaves.
//        host_rows_check clamp <sqdiff|ccoeff> <fill bits, hex> <input file> <output file>
//          raw float32 in, every value through rows_clamped, raw float32 out.
// Built by tests/test_clamped_rows_host.py with g++ -O2 -std=c++17 -ffp-contract=off -fsanitize=address,undefined.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "../include/sushi_hip.h"
#include "../sushi_amd/csrc/rows_core.hpp"
#include "host_check_io.hpp"

namespace {

using host_check::read_file;
using host_check::records;
using sushi::RowsStage;

constexpr int64_t MAX64 = std::numeric_limits<int64_t>::max();
constexpr uint32_t SENTINEL = 0x7fc00123u;

float from_bits(uint32_t b) { float f; std::memcpy(&f, &b, 4); return f; }

void report(const char* name, int rc) { std::printf("%s %d\n", name, rc); }

std::vector<SushiHipRowsRow> good() { return {{1, 0, 5, 0}, {7, 3, 4096, 0}, {5001, 9000, 12293, 0}}; }

int validate() {
    RowsStage st;
    std::vector<SushiHipRowsRow> t = good();
    const int n = (int)t.size();
    report("good", sushi::stage_rows(t.data(), n, 20000, false, 0, 0.5f, st));
    report("good_with_in", sushi::stage_rows(t.data(), n, 20000, true, 21293, 0.5f, st));
    report("no_rows", sushi::stage_rows(t.data(), 0, 20000, false, 0, 0.5f, st));
    report("negative_rows", sushi::stage_rows(t.data(), -1, 20000, false, 0, 0.5f, st));
    report("empty_out", sushi::stage_rows(t.data(), n, 0, false, 0, 0.5f, st));
    report("empty_in", sushi::stage_rows(t.data(), n, 20000, true, 0, 0.5f, st));
    report("fill_nan", sushi::stage_rows(t.data(), n, 20000, false, 0, from_bits(0x7fc00000u), st));
    report("fill_inf", sushi::stage_rows(t.data(), n, 20000, false, 0, from_bits(0x7f800000u), st));
    report("fill_neg_zero", sushi::stage_rows(t.data(), n, 20000, false, 0, -0.0f, st));
    t = good(); t[0].n_pos = 0; report("row_empty", sushi::stage_rows(t.data(), n, 20000, false, 0, 0.5f, st));
    t = good(); t[0].n_pos = -4; report("row_negative", sushi::stage_rows(t.data(), n, 20000, false, 0, 0.5f, st));
    t = good(); t[1].out_off = -1; report("row_before_out", sushi::stage_rows(t.data(), n, 20000, false, 0, 0.5f, st));
    t = good(); report("row_ends_at_out_end", sushi::stage_rows(t.data(), n, 17294, false, 0, 0.5f, st));
    t = good(); report("row_one_past_out_end", sushi::stage_rows(t.data(), n, 17293, false, 0, 0.5f, st));
    t = good(); report("row_one_past_in_end", sushi::stage_rows(t.data(), n, 20000, true, 21292, 0.5f, st));
    t = good(); t[1].in_off = -1; report("row_before_in", sushi::stage_rows(t.data(), n, 20000, true, 21293, 0.5f, st));
    t = good(); t[1].in_off = -1; report("in_not_read_without_in", sushi::stage_rows(t.data(), n, 20000, false, 0, 0.5f, st));
    // sums that do not fit 64 bits are never formed
    t = good(); t[2].out_off = MAX64; report("row_at_int64_max", sushi::stage_rows(t.data(), n, 20000, false, 0, 0.5f, st));
    t = good(); t[2].out_off = MAX64 - 12293; report("huge_out_row_at_end", sushi::stage_rows(t.data(), n, MAX64, false, 0, 0.5f, st));
    t = good(); t[2].out_off = MAX64 - 12292; report("huge_out_row_past_end", sushi::stage_rows(t.data(), n, MAX64, false, 0, 0.5f, st));
    t = good(); t[2].n_pos = std::numeric_limits<int32_t>::max();
    report("int32_max_floats", sushi::stage_rows(t.data(), n, MAX64, false, 0, 0.5f, st));
    std::printf("facts_int32_max items=%lld grid=%u tiles=%d\n", (long long)st.n_items, st.grid,
                reinterpret_cast<const sushi::RowsRowDev*>(st.image.data())[2].n_tiles);

    t = good();
    const int rc = sushi::stage_rows(t.data(), n, 20000, true, 21293, 0.5f, st);
    const sushi::RowsRowDev* rd = reinterpret_cast<const sushi::RowsRowDev*>(st.image.data());
    std::printf("facts_good rc=%d items=%lld grid=%u bytes=%zu", rc, (long long)st.n_items, st.grid, st.image.size());
    for (int k = 0; k < n; ++k)
        std::printf(" r%d=(%lld,%lld,%lld,%d,%d)", k, (long long)rd[k].out_off, (long long)rd[k].in_off, (long long)rd[k].first_item,
                    rd[k].n_pos, rd[k].n_tiles);
    std::printf("\nrow_of");
    for (int64_t item = 0; item < st.n_items; ++item) std::printf(" %d", sushi::rows_row_of(rd, n, item));
    std::printf("\nbytes %zu %zu %zu %zu\n", sushi::rows_layout_bytes(1), sushi::rows_layout_bytes(8), sushi::rows_layout_bytes(9),
                sushi::rows_layout_bytes(0));
    // buffers that share bytes: apart, in place, the same first float with a row moved, one float apart
    std::vector<float> buf(40000);
    t = good();
    for (auto& r : t) r.in_off = r.out_off;
    std::printf("overlap %d %d", (int)sushi::rows_overlap_ok(buf.data(), 20000, buf.data() + 20000, 20000, t.data(), n),
                (int)sushi::rows_overlap_ok(buf.data(), 20000, buf.data(), 20000, t.data(), n));
    t[1].in_off = 8;
    std::printf(" %d", (int)sushi::rows_overlap_ok(buf.data(), 20000, buf.data(), 20000, t.data(), n));
    t[1].in_off = 7;
    std::printf(" %d %d\n", (int)sushi::rows_overlap_ok(buf.data(), 20000, buf.data() + 1, 20000, t.data(), n),
                (int)sushi::rows_overlap_ok(buf.data(), 20000, buf.data() + 19999, 20000, t.data(), n));
    return 0;
}

int form(const char* fill_hex, const char* capacity_s, const char* n_out_s, const char* hits_path, const char* counts_path,
         const char* table_path, const char* out_path) {
    const float f = from_bits((uint32_t)std::strtoul(fill_hex, nullptr, 16));
    const int32_t capacity = (int32_t)std::atol(capacity_s);
    const int64_t n_out = std::atoll(n_out_s);
    const std::vector<SushiHipHit> hits = records<SushiHipHit>(read_file(hits_path));
    const std::vector<int64_t> counts = records<int64_t>(read_file(counts_path));
    const std::vector<SushiHipRowsRow> table = records<SushiHipRowsRow>(read_file(table_path));
    const int n = (int)table.size();
    if (counts.size() != (size_t)n || hits.size() != (size_t)n * (size_t)capacity) { std::fprintf(stderr, "sizes do not agree\n"); return 3; }
    RowsStage st;
    const int rc = sushi::stage_rows(table.data(), n, n_out, false, 0, f, st);
    if (rc != SUSHI_HIP_OK) { std::fprintf(stderr, "stage_rows refused the table: %d\n", rc); return 3; }
    const sushi::RowsRowDev* rd = reinterpret_cast<const sushi::RowsRowDev*>(st.image.data());
    std::vector<float> out((size_t)n_out, from_bits(SENTINEL));
    std::vector<int32_t> flags((size_t)n, 0);
    // every work item, as the grid strides over them: its row by bisection, its tile, the definition of a tile
    for (int64_t item = 0; item < st.n_items; ++item) {
        const int k = sushi::rows_row_of(rd, n, item);
        // (an exact-size copy of the request's list: a read past it is caught)
        std::vector<SushiHipHit> list(hits.begin() + (ptrdiff_t)k * capacity, hits.begin() + (ptrdiff_t)(k + 1) * capacity);
        flags[(size_t)k] |= sushi::rows_form_tile(list.data(), counts[(size_t)k], capacity, rd[k].n_pos, (int32_t)(item - rd[k].first_item), f,
                                                  out.data() + rd[k].out_off);
    }
    using host_check::part;
    return host_check::write_file(out_path, {part(out), part(flags)});
}

int clamp(const char* method_name, const char* fill_hex, const char* in_path, const char* out_path) {
    const int method = !std::strcmp(method_name, "ccoeff") ? SUSHI_HIP_METHOD_CCOEFF_NORMED : SUSHI_HIP_METHOD_SQDIFF_NORMED;
    const float f = from_bits((uint32_t)std::strtoul(fill_hex, nullptr, 16));
    std::vector<float> v = records<float>(read_file(in_path));
    for (float& x : v) x = sushi::rows_clamped(method, x, f);
    return host_check::write_file(out_path, {host_check::part(v)});
}

}  // namespace

int main(int argc, char** argv) {
    if (argc == 2 && !std::strcmp(argv[1], "validate")) return validate();
    if (argc == 9 && !std::strcmp(argv[1], "form")) return form(argv[2], argv[3], argv[4], argv[5], argv[6], argv[7], argv[8]);
    if (argc == 6 && !std::strcmp(argv[1], "clamp")) return clamp(argv[2], argv[3], argv[4], argv[5]);
    std::fprintf(stderr, "usage: %s validate | form <fill> <capacity> <n_out> <hits> <counts> <table> <output> | "
                         "clamp <sqdiff|ccoeff> <fill> <input> <output>\n", argv[0]);
    return 2;
}
