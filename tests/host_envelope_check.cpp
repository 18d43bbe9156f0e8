// sushi_hip_envelope's arithmetic (sushi_amd/csrc/envelope_core.hpp) on the CPU: every output of every case straight from the row
// with both clamps (envelope_sample: the block sums, the window sum and the finish the kernel runs on its staged tile), and what
// stage_envelope makes of the case.
// usage: host_envelope_check <u8|f32> <input file> <case file> <output file> <stage file>
//   input file: raw samples; case file: records of four int64 (in_start, hop, span, out_len); output file: the cases' outputs
//   back to back; stage file: per case four int64 (return code, tile, n_tiles, grid).  A case stage_envelope refuses writes no
//   outputs.  The test compares the outputs with sushi_amd.envelope.envelope_host, bit for bit.
// Built by tests/test_envelope_host.py with g++ -O2 -std=c++17 -ffp-contract=off -fsanitize=address,undefined.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../include/sushi_hip.h"
#include "../sushi_amd/csrc/envelope_core.hpp"
#include "host_check_io.hpp"

namespace {

struct Case { int64_t in_start, hop, span, out_len; };
static_assert(sizeof(Case) == 32, "Case layout");

template <class T>
int run(int dtype, const char* in_path, const char* case_path, const char* out_path, const char* stage_path) {
    const std::vector<T> x = host_check::records<T>(host_check::read_file(in_path));
    const std::vector<Case> cases = host_check::records<Case>(host_check::read_file(case_path));
    const int64_t n_in = (int64_t)x.size();
    std::vector<T> out;
    std::vector<int64_t> stages;
    for (const Case& c : cases) {
        sushi::EnvelopeStage st{0, 0, 0};
        const int rc = sushi::stage_envelope(dtype, n_in, c.in_start, (int32_t)c.hop, (int32_t)c.span, c.out_len, st);
        stages.push_back(rc);
        stages.push_back(rc == SUSHI_HIP_OK ? st.tile : 0);
        stages.push_back(rc == SUSHI_HIP_OK ? st.n_tiles : 0);
        stages.push_back(rc == SUSHI_HIP_OK ? (int64_t)st.grid : 0);
        if (rc != SUSHI_HIP_OK) continue;
        for (int64_t i = 0; i < c.out_len; ++i)
            out.push_back(sushi::envelope_sample<T>(x.data(), n_in, c.in_start, (int32_t)c.hop, (int32_t)c.span, i));
    }
    const int rc = host_check::write_file(out_path, {host_check::part(out)});
    return rc ? rc : host_check::write_file(stage_path, {host_check::part(stages)});
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 6) { std::fprintf(stderr, "usage: %s <u8|f32> <input> <cases> <output> <stages>\n", argv[0]); return 2; }
    if (!std::strcmp(argv[1], "u8")) return run<uint8_t>(SUSHI_HIP_U8, argv[2], argv[3], argv[4], argv[5]);
    if (!std::strcmp(argv[1], "f32")) return run<float>(SUSHI_HIP_F32, argv[2], argv[3], argv[4], argv[5]);
    return 2;
}
