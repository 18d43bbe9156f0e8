// sushi_hip_filter's arithmetic (sushi_amd/csrc/filter_core.hpp) on the CPU: every output of every case straight from the row with
// both clamps (filter_sample: the deviations, the products and the sum in ascending tap order, and the finish the kernel runs on
// its staged tile), and what stage_filter makes of the case.
// usage: host_filter_check <u8|f32> <input file> <taps file> <case file> <output file> <stage file>
//   input file: raw samples; taps file: float64 taps of every case back to back; case file: records of seven int64 (in_start,
//   first tap in the taps file, n_taps, out_len, null pointers: 1 the row | 2 the taps | 4 the output, dtype or -1 for the row's,
//   n_in or 0 for the row's); output file: the cases' outputs back to back; stage file: per case four int64 (return code, tile,
//   n_tiles, grid).  A case stage_filter refuses writes no outputs, and one with a pointer, dtype or n_in of its own is only staged.
//   The test compares the outputs with sushi_amd.filter.filter_host, bit for bit.
// Built by tests/test_filter_host.py with g++ -O2 -std=c++17 -ffp-contract=off -fsanitize=address,undefined.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../include/sushi_hip.h"
#include "../sushi_amd/csrc/filter_core.hpp"
#include "host_check_io.hpp"

namespace {

struct Case { int64_t in_start, tap_off, n_taps, out_len, nulls, dtype, n_in; };
static_assert(sizeof(Case) == 56, "Case layout");

template <class T>
int run(int dtype, const char* in_path, const char* taps_path, const char* case_path, const char* out_path, const char* stage_path) {
    const std::vector<T> x = host_check::records<T>(host_check::read_file(in_path));
    const std::vector<double> taps = host_check::records<double>(host_check::read_file(taps_path));
    const std::vector<Case> cases = host_check::records<Case>(host_check::read_file(case_path));
    std::vector<T> out;
    std::vector<int64_t> stages;
    T sink = 0;
    for (const Case& c : cases) {
        const bool probe = c.nulls || c.dtype >= 0 || c.n_in;
        const int64_t n_in = c.n_in ? c.n_in : (int64_t)x.size();
        const bool taps_inside = c.tap_off >= 0 && c.n_taps >= 0 && c.tap_off + c.n_taps <= (int64_t)taps.size();
        if (!probe && !taps_inside) { std::fprintf(stderr, "a case's taps lie outside the taps file\n"); return 2; }
        const double* h = taps.data() + (taps_inside ? c.tap_off : 0);
        sushi::FilterStage st{0, 0, 0, 0};
        const int rc = sushi::stage_filter((c.nulls & 1) ? nullptr : (const void*)x.data(), c.dtype >= 0 ? (int)c.dtype : dtype, n_in,
                                           c.in_start, (c.nulls & 2) ? nullptr : (const void*)h, (int32_t)c.n_taps,
                                           (c.nulls & 4) ? nullptr : (const void*)&sink, c.out_len, st);
        stages.push_back(rc);
        stages.push_back(rc == SUSHI_HIP_OK ? st.tile : 0);
        stages.push_back(rc == SUSHI_HIP_OK ? st.n_tiles : 0);
        stages.push_back(rc == SUSHI_HIP_OK ? (int64_t)st.grid : 0);
        if (rc != SUSHI_HIP_OK || probe) continue;
        for (int64_t i = 0; i < c.out_len; ++i)
            out.push_back(sushi::filter_sample<T>(x.data(), n_in, c.in_start, h, (int32_t)c.n_taps, i));
    }
    const int rc = host_check::write_file(out_path, {host_check::part(out)});
    return rc ? rc : host_check::write_file(stage_path, {host_check::part(stages)});
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 7) { std::fprintf(stderr, "usage: %s <u8|f32> <input> <taps> <cases> <output> <stages>\n", argv[0]); return 2; }
    if (!std::strcmp(argv[1], "u8")) return run<uint8_t>(SUSHI_HIP_U8, argv[2], argv[3], argv[4], argv[5], argv[6]);
    if (!std::strcmp(argv[1], "f32")) return run<float>(SUSHI_HIP_F32, argv[2], argv[3], argv[4], argv[5], argv[6]);
    return 2;
}
