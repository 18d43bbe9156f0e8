// sushi_hip_retime's arithmetic (sushi_amd/csrc/retime_core.hpp) on the CPU: what a thread of retime_kernel does for its run of
// outputs -- one division (retime_seek), then incremental advances -- over whole segments, in runs of RUN outputs.
// usage: host_retime_check <u8|f32> <input file> <segment file> <output file> <n_out>
//   input file: raw samples; segment file: SushiHipRetimeSegment records (32 bytes each); output file: n_out samples, zero
//   outside the segments.  The test compares it with sushi_amd.retime.retime_host, bit for bit.
// Built by tests/test_retime_host.py with g++ -O2 -std=c++17 -ffp-contract=off -fsanitize=address,undefined.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../include/sushi_hip.h"
#include "../sushi_amd/csrc/retime_core.hpp"
#include "host_check_io.hpp"

namespace {

constexpr int RUN = 16;      // outputs between two divisions (a thread's chunk in the kernel)

template <class T>
int run(const char* in_path, const char* seg_path, const char* out_path, int64_t n_out) {
    const std::vector<T> x = host_check::records<T>(host_check::read_file(in_path));
    const std::vector<SushiHipRetimeSegment> seg = host_check::records<SushiHipRetimeSegment>(host_check::read_file(seg_path));
    const int64_t n_in = (int64_t)x.size();
    std::vector<T> out((size_t)n_out, (T)0);
    for (const SushiHipRetimeSegment& s : seg) {
        const int32_t qstep = s.num / s.den, rstep = s.num % s.den;
        for (int64_t i0 = 0; i0 < s.out_len; i0 += RUN) {
            const int64_t i1 = i0 + RUN < s.out_len ? i0 + RUN : s.out_len;
            sushi::RetimeCursor c = sushi::retime_seek(s.in_start, i0, s.num, s.den);
            for (int64_t i = i0; i < i1; ++i) {
                out.at((size_t)(s.out_off + i)) = sushi::retime_sample<T>(x.data(), n_in, c.j, c.r, s.den);
                sushi::retime_advance(c, qstep, rstep, s.den);
            }
        }
    }
    return host_check::write_file(out_path, {host_check::part(out)});
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 6) { std::fprintf(stderr, "usage: %s <u8|f32> <input> <segments> <output> <n_out>\n", argv[0]); return 2; }
    const int64_t n_out = std::atoll(argv[5]);
    if (n_out < 1) return 2;
    if (!std::strcmp(argv[1], "u8")) return run<uint8_t>(argv[2], argv[3], argv[4], n_out);
    if (!std::strcmp(argv[1], "f32")) return run<float>(argv[2], argv[3], argv[4], n_out);
    return 2;
}
