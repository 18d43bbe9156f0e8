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

namespace {

constexpr int RUN = 1024;    // outputs of a workgroup's run
constexpr int HOP = 256;     // outputs between two of one thread

std::vector<unsigned char> read_file(const char* path) {
    std::vector<unsigned char> buf;
    FILE* f = std::fopen(path, "rb");
    if (!f) { std::fprintf(stderr, "cannot open %s\n", path); std::exit(2); }
    unsigned char tmp[65536];
    size_t got;
    while ((got = std::fread(tmp, 1, sizeof(tmp), f)) > 0) buf.insert(buf.end(), tmp, tmp + got);
    std::fclose(f);
    return buf;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 8) { std::fprintf(stderr, "usage: %s <input> <table> <output> <num> <den> <half_width> <n_body>\n", argv[0]); return 2; }
    const int32_t num = (int32_t)std::atol(argv[4]), den = (int32_t)std::atol(argv[5]), W = (int32_t)std::atol(argv[6]);
    const int64_t n_body = std::atoll(argv[7]);
    if (num < 1 || num > sushi::RESAMPLE_MAX_TERM || den < 1 || den > sushi::RESAMPLE_MAX_TERM || W < 1 ||
        (int64_t)den * 2 * W > sushi::RESAMPLE_MAX_TABLE || n_body < 1 || n_body >= sushi::RESAMPLE_MAX_BODY)
        return 2;
    const std::vector<unsigned char> in_bytes = read_file(argv[1]), table_bytes = read_file(argv[2]);
    const int64_t n_raw = (int64_t)(in_bytes.size() / sizeof(float));
    const int32_t taps = 2 * W;
    if (n_raw < 1 || table_bytes.size() != (size_t)den * taps * sizeof(double)) return 2;
    if ((n_body - 1) * (int64_t)num / den > n_raw - 1) return 2;
    std::vector<float> x((size_t)n_raw);
    std::memcpy(x.data(), in_bytes.data(), (size_t)n_raw * sizeof(float));
    std::vector<double> table((size_t)den * taps);
    std::memcpy(table.data(), table_bytes.data(), table.size() * sizeof(double));
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
    FILE* f = std::fopen(argv[3], "wb");
    if (!f) { std::fprintf(stderr, "cannot write %s\n", argv[3]); return 2; }
    const size_t put = std::fwrite(out.data(), sizeof(float), out.size(), f);
    std::fclose(f);
    return put == out.size() ? 0 : 2;
}
