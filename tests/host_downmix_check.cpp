// sushi_hip_load_decode_mix's arithmetic (sushi_amd/csrc/downmix_core.hpp) on the CPU: what a thread of decode_mix_kernel does for
// its frame (downmix_frame: every output, each sample read once) and the statement per (frame, output) it rests on (downmix_value);
// the two must agree to the bit.
// usage: host_downmix_check <sample width 2|3> <channels> <n_out> <pcm file> <weights file> <output file>
//   pcm file: raw interleaved frames (bytes behind the last whole frame are ignored); weights file: n_out x channels float32,
//   row-major, as the entry point takes them; output file: n_out rows of n_frames float32.  The test compares it with
//   sushi_amd.downmix.mix_host, bit for bit.  The PCM bytes sit in a heap block of exactly their size, one byte off any alignment.
// Built by tests/test_downmix_host.py with g++ -O2 -std=c++17 -ffp-contract=off -fsanitize=address,undefined.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../include/sushi_hip.h"
#include "../sushi_amd/csrc/downmix_core.hpp"
#include "host_check_io.hpp"

namespace {

template <int WIDTH>
int run(int channels, int n_out, const char* pcm_path, const char* w_path, const char* out_path) {
    const std::vector<unsigned char> file = host_check::read_file(pcm_path), w_bytes = host_check::read_file(w_path);
    const int fs = channels * WIDTH;
    const int64_t n_frames = (int64_t)(file.size() / (size_t)fs);
    if (w_bytes.size() != (size_t)n_out * channels * sizeof(float)) { std::fprintf(stderr, "weights: wrong size\n"); return 2; }
    const std::vector<float> w_rows = host_check::records<float>(w_bytes);
    // as the entry point lays them out for the kernel: w[c * 8 + o], zero elsewhere
    std::vector<float> w((size_t)sushi::DOWNMIX_MAX_CHANNELS * sushi::DOWNMIX_MAX_OUTPUTS, 0.f);
    for (int c = 0; c < channels; ++c)
        for (int o = 0; o < n_out; ++o) w[(size_t)c * sushi::DOWNMIX_MAX_OUTPUTS + o] = w_rows[(size_t)o * channels + c];
    // exactly the frames' bytes, at an odd address: a read outside them is the sanitizer's
    const size_t nbytes = (size_t)n_frames * fs;
    unsigned char* block = (unsigned char*)std::malloc(nbytes + 1);
    if (!block) return 2;
    unsigned char* odd = block + 1;
    std::memcpy(odd, file.data(), nbytes);
    unsigned char* exact = (unsigned char*)std::malloc(nbytes ? nbytes : 1);
    if (!exact) return 2;
    std::memcpy(exact, file.data(), nbytes);
    std::vector<float> out((size_t)n_out * n_frames);
    int rc = 0;
    for (int64_t f = 0; f < n_frames && rc == 0; ++f) {
        float acc[sushi::DOWNMIX_MAX_OUTPUTS];
        sushi::downmix_frame<WIDTH>(exact + f * fs, channels, w.data(), acc);
        for (int o = 0; o < n_out; ++o) {
            const float one = sushi::downmix_value<WIDTH>(odd + f * fs, channels, w.data() + o, sushi::DOWNMIX_MAX_OUTPUTS);
            const float row = sushi::downmix_value<WIDTH>(exact + f * fs, channels, w_rows.data() + (size_t)o * channels, 1);
            if (std::memcmp(&one, &acc[o], 4) || std::memcmp(&row, &acc[o], 4)) {
                std::fprintf(stderr, "frame %lld output %d: downmix_frame and downmix_value differ\n", (long long)f, o);
                rc = 3;
            }
            out[(size_t)o * n_frames + f] = acc[o];
        }
    }
    std::free(block);
    std::free(exact);
    if (rc) return rc;
    return host_check::write_file(out_path, {host_check::part(out)});
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 7) { std::fprintf(stderr, "usage: %s <2|3> <channels> <n_out> <pcm> <weights> <output>\n", argv[0]); return 2; }
    const int width = std::atoi(argv[1]), channels = std::atoi(argv[2]), n_out = std::atoi(argv[3]);
    if (channels < 1 || channels > SUSHI_HIP_MIX_MAX_CHANNELS || n_out < 1 || n_out > SUSHI_HIP_MIX_MAX_OUTPUTS) return 2;
    if (width == 2) return run<2>(channels, n_out, argv[4], argv[5], argv[6]);
    if (width == 3) return run<3>(channels, n_out, argv[4], argv[5], argv[6]);
    return 2;
}
