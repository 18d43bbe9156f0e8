// sushi_hip_load_resample_fir's arithmetic (sushi_amd/csrc/resample_core.hpp) on the CPU: what a thread of fir_body_kernel does
// for its outputs -- one division per run (resample_seek), then advances of HOP outputs -- over the whole body, in runs of RUN.
// usage: host_resample_check <input file> <table file> <output file> <num> <den> <half_width> <n_body>
//   input file: raw float32 frames; table file: float64 [den][2 * half_width]; output file: n_body float32 body samples.
// The test compares it with sushi_amd.resample.resample_host, bit for bit.
// Built by tests/test_resample_host.py with g++ -O2 -std=c++17 -ffp-contract=off -fsanitize=address,undefined.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../sushi_amd/csrc/resample_core.hpp"
#include "host_check_io.hpp"

namespace {

constexpr int RUN = 1024;    // outputs of a workgroup's run
constexpr int HOP = 256;     // outputs between two of one thread

}  // namespace

int main(int argc, char** argv) {
    if (argc != 8) { std::fprintf(stderr, "usage: %s <input> <table> <output> <num> <den> <half_width> <n_body>\n", argv[0]); return 2; }
    const int32_t num = (int32_t)std::atol(argv[4]), den = (int32_t)std::atol(argv[5]), W = (int32_t)std::atol(argv[6]);
    const int64_t n_body = std::atoll(argv[7]);
    if (num < 1 || num > sushi::RESAMPLE_MAX_TERM || den < 1 || den > sushi::RESAMPLE_MAX_TERM || W < 1 ||
        (int64_t)den * 2 * W > sushi::RESAMPLE_MAX_TABLE || n_body < 1 || n_body >= sushi::RESAMPLE_MAX_BODY)
        return 2;
    const std::vector<float> x = host_check::records<float>(host_check::read_file(argv[1]));
    const std::vector<unsigned char> table_bytes = host_check::read_file(argv[2]);
    const int64_t n_raw = (int64_t)x.size();
    const int32_t taps = 2 * W;
    if (n_raw < 1 || table_bytes.size() != (size_t)den * taps * sizeof(double)) return 2;
    if ((n_body - 1) * (int64_t)num / den > n_raw - 1) return 2;
    const std::vector<double> table = host_check::records<double>(table_bytes);
    std::vector<float> out((size_t)n_body);
    const int64_t hop = (int64_t)HOP * num;
    const int32_t qhop = (int32_t)(hop / den), rhop = (int32_t)(hop % den);
    for (int64_t i0 = 0; i0 < n_body; i0 += RUN) {
        const int64_t i1 = i0 + RUN < n_body ? i0 + RUN : n_body;
        for (int tid = 0; tid < HOP && i0 + tid < i1; ++tid) {
            sushi::ResampleCursor cur = sushi::resample_seek(i0 + tid, num, den);
            for (int64_t i = i0 + tid; i < i1; i += HOP) {
                const double* row = table.data() + (size_t)cur.r * taps;
                out.at((size_t)i) = sushi::resample_output(
                    taps, [&](int32_t c) { return (double)x.at((size_t)sushi::resample_tap_index(cur.j, W, c, n_raw)); },
                    [&](int32_t c) { return row[c]; });
                sushi::resample_advance(cur, qhop, rhop, den);
            }
        }
    }
    return host_check::write_file(argv[3], {host_check::part(out)});
}
