// sushi_hip_level's arithmetic (sushi_amd/csrc/level_core.hpp) on the CPU: every output of every case straight from the row with
// both clamps (level_window: the deviation and the window sum in ascending t; level_output: the quotient and the finish the kernels
// run on their staged tile; together they are level_sample), and what stage_level makes of the case.
// usage: host_level_check <u8|f32> <input file> <pairs file> <case file> <output file> <stage file>
//   input file: raw samples; pairs file: float64 (floor, peak) pairs of every case back to back; case file: records of eight int64
//   (in_start, window, out_len, first pair in the pairs file, pairs, flags: 1 a null row | 2 a null output | 4 a row off its
//   alignment | 8 an output off its alignment, dtype or -1 for the row's, n_in or 0 for the row's); output file: per case and per
//   pair, in that order, out_len outputs; stage file: per case and per pair five int64 (return code, tile, n_tiles, grid, LDS
//   bytes).  A window's sum does not depend on the pair, so a case forms it once per output and finishes it for every pair.  A
//   pair stage_level refuses writes no outputs, and a case with flags, a dtype or an n_in of its own is only staged.
//   The test compares the outputs with sushi_amd.level.level_host, bit for bit.
// Built by tests/test_level_host.py with g++ -O2 -std=c++17 -ffp-contract=off -fsanitize=address,undefined.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../include/sushi_hip.h"
#include "../sushi_amd/csrc/level_core.hpp"
#include "host_check_io.hpp"

namespace {

struct Case { int64_t in_start, window, out_len, pair_off, n_pairs, flags, dtype, n_in; };
static_assert(sizeof(Case) == 64, "Case layout");

template <class T>
int run(int dtype, const char* in_path, const char* pairs_path, const char* case_path, const char* out_path, const char* stage_path) {
    const std::vector<T> x = host_check::records<T>(host_check::read_file(in_path));
    const std::vector<double> pairs = host_check::records<double>(host_check::read_file(pairs_path));
    const std::vector<Case> cases = host_check::records<Case>(host_check::read_file(case_path));
    std::vector<T> out;
    std::vector<int64_t> stages;
    T sink[2] = {0, 0};
    for (const Case& c : cases) {
        const bool probe = c.flags || c.dtype >= 0 || c.n_in;
        const int64_t n_in = c.n_in ? c.n_in : (int64_t)x.size();
        if (c.pair_off < 0 || c.n_pairs < 1 || 2 * (c.pair_off + c.n_pairs) > (int64_t)pairs.size()) {
            std::fprintf(stderr, "a case's pairs lie outside the pairs file\n");
            return 2;
        }
        const char* xp = (c.flags & 1) ? nullptr : (const char*)x.data() + ((c.flags & 4) ? 1 : 0);       // (never dereferenced by stage_level)
        const char* yp = (c.flags & 2) ? nullptr : (const char*)sink + ((c.flags & 8) ? 1 : 0);
        std::vector<bool> fine;
        bool any = false;
        for (int64_t p = 0; p < c.n_pairs; ++p) {
            const double floor_ = pairs[2 * (c.pair_off + p)], peak = pairs[2 * (c.pair_off + p) + 1];
            sushi::LevelStage st{0, 0, 0, 0};
            const int rc = sushi::stage_level(xp, c.dtype >= 0 ? (int)c.dtype : dtype, n_in, c.in_start, (int32_t)c.window, floor_, peak,
                                              yp, c.out_len, st);
            const bool ok = rc == SUSHI_HIP_OK;
            stages.push_back(rc);
            stages.push_back(ok ? st.tile : 0);
            stages.push_back(ok ? st.n_tiles : 0);
            stages.push_back(ok ? (int64_t)st.grid : 0);
            stages.push_back(ok ? (int64_t)st.lds_bytes : 0);
            fine.push_back(ok && !probe);
            any = any || (ok && !probe);
        }
        if (!any) continue;
        std::vector<sushi::LevelWindow<T>> w((size_t)c.out_len);
        for (int64_t i = 0; i < c.out_len; ++i) w[(size_t)i] = sushi::level_window(x.data(), n_in, c.in_start, (int32_t)c.window, i);
        for (int64_t p = 0; p < c.n_pairs; ++p) {
            if (!fine[(size_t)p]) continue;
            const double floor_ = pairs[2 * (c.pair_off + p)], peak = pairs[2 * (c.pair_off + p) + 1];
            const double fw = sushi::level_floor_term<T>(floor_, (int32_t)c.window);
            for (int64_t i = 0; i < c.out_len; ++i)
                out.push_back(sushi::level_output<T>(w[(size_t)i].d, w[(size_t)i].e, (int32_t)c.window, fw, peak));
            // level_sample is the two together
            if (out.back() != sushi::level_sample(x.data(), n_in, c.in_start, (int32_t)c.window, floor_, peak, c.out_len - 1) &&
                out.back() == out.back()) {
                std::fprintf(stderr, "level_sample differs from level_window and level_output\n");
                return 3;
            }
        }
    }
    const int rc = host_check::write_file(out_path, {host_check::part(out)});
    return rc ? rc : host_check::write_file(stage_path, {host_check::part(stages)});
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 7) { std::fprintf(stderr, "usage: %s <u8|f32> <input> <pairs> <cases> <output> <stages>\n", argv[0]); return 2; }
    if (!std::strcmp(argv[1], "u8")) return run<uint8_t>(SUSHI_HIP_U8, argv[2], argv[3], argv[4], argv[5], argv[6]);
    if (!std::strcmp(argv[1], "f32")) return run<float>(SUSHI_HIP_F32, argv[2], argv[3], argv[4], argv[5], argv[6]);
    return 2;
}
