// The sample rule of sushi_hip_load_decode_format / _decode_mix_format (sushi_amd/csrc/pcm_core.hpp) on the CPU: what a thread of
// decode_format_kernel and of decode_mix_format_kernel does for its frame (pcm_mean, pcm_mix_frame), the samples they rest on
// (pcm_sample) and the statement per (frame, output) (pcm_mix_value); pcm_mix_frame and pcm_mix_value must agree to the bit.
// usage: host_pcm_check <format 1..6> <channels> <n_out> <pcm file> <weights file>
//   pcm file: raw interleaved frames (bytes behind the last whole frame are ignored); weights file: n_out x channels float32,
//   row-major, as the entry point takes them.  Everything is computed three times, on heap blocks that END with the last frame's
//   last byte and hold the frames 0, 1 and 3 bytes into the block: a read outside a sample's container is the sanitizer's, and the
//   three must agree.  Prints the values as float32 bit patterns in hex, one line each: "samples" (frame-major, n_frames x
//   channels), "mean" (n_frames), then "mix <o>" (n_frames) per output.  The test compares them with
//   sushi_amd.downmix.samples_from_bytes, mean_host and mix_host.
// Built by tests/test_wav_formats_host.py with g++ -O2 -std=c++17 -ffp-contract=off -fsanitize=address,undefined.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../include/sushi_hip.h"
#include "../sushi_amd/csrc/pcm_core.hpp"
#include "host_check_io.hpp"

namespace {

void print_row(const char* name, int o, const std::vector<float>& v) {
    if (o < 0) std::printf("%s", name); else std::printf("%s %d", name, o);
    for (float x : v) {
        uint32_t bits;
        std::memcpy(&bits, &x, 4);
        std::printf(" %08x", bits);
    }
    std::printf("\n");
}

template <int FMT>
int run(int channels, int n_out, const char* pcm_path, const char* w_path) {
    constexpr int W = sushi::pcm_width(FMT);
    const std::vector<unsigned char> file = host_check::read_file(pcm_path), w_bytes = host_check::read_file(w_path);
    const int fs = channels * W;
    const int64_t n_frames = (int64_t)(file.size() / (size_t)fs);
    if (w_bytes.size() != (size_t)n_out * channels * sizeof(float)) { std::fprintf(stderr, "weights: wrong size\n"); return 2; }
    const std::vector<float> w_rows = host_check::records<float>(w_bytes);
    // as the entry point lays them out for the kernel: w[c * 8 + o], zero elsewhere
    std::vector<float> w((size_t)sushi::DOWNMIX_MAX_CHANNELS * sushi::DOWNMIX_MAX_OUTPUTS, 0.f);
    for (int c = 0; c < channels; ++c)
        for (int o = 0; o < n_out; ++o) w[(size_t)c * sushi::DOWNMIX_MAX_OUTPUTS + o] = w_rows[(size_t)o * channels + c];
    const size_t nbytes = (size_t)n_frames * fs;
    std::vector<float> samples, mean, mix;
    for (size_t start : {(size_t)0, (size_t)1, (size_t)3}) {
        unsigned char* block = (unsigned char*)std::malloc(start + nbytes ? start + nbytes : 1);
        if (!block) return 2;
        const unsigned char* pcm = block + start;
        std::memcpy(block + start, file.data(), nbytes);
        std::vector<float> s((size_t)n_frames * channels), m((size_t)n_frames), x((size_t)n_out * n_frames);
        int rc = 0;
        for (int64_t f = 0; f < n_frames && rc == 0; ++f) {
            const uint8_t* frame = pcm + f * fs;
            for (int c = 0; c < channels; ++c) s[(size_t)f * channels + c] = sushi::pcm_sample<FMT>(frame + c * W);
            m[(size_t)f] = sushi::pcm_mean<FMT>(frame, channels);
            float acc[sushi::DOWNMIX_MAX_OUTPUTS];
            sushi::pcm_mix_frame<FMT>(frame, channels, w.data(), acc);
            for (int o = 0; o < n_out; ++o) {
                const float one = sushi::pcm_mix_value<FMT>(frame, channels, w.data() + o, sushi::DOWNMIX_MAX_OUTPUTS);
                const float row = sushi::pcm_mix_value<FMT>(frame, channels, w_rows.data() + (size_t)o * channels, 1);
                if (std::memcmp(&one, &acc[o], 4) || std::memcmp(&row, &acc[o], 4)) {
                    std::fprintf(stderr, "frame %lld output %d: pcm_mix_frame and pcm_mix_value differ\n", (long long)f, o);
                    rc = 3;
                }
                x[(size_t)o * n_frames + f] = acc[o];
            }
        }
        std::free(block);
        if (rc) return rc;
        if (start == 0) { samples = s; mean = m; mix = x; continue; }
        if ((nbytes && (std::memcmp(samples.data(), s.data(), s.size() * 4) || std::memcmp(mean.data(), m.data(), m.size() * 4) ||
                        std::memcmp(mix.data(), x.data(), x.size() * 4)))) {
            std::fprintf(stderr, "the values depend on where the frames start (%zu bytes in)\n", start);
            return 4;
        }
    }
    print_row("samples", -1, samples);
    print_row("mean", -1, mean);
    for (int o = 0; o < n_out; ++o)
        print_row("mix", o, std::vector<float>(mix.begin() + (size_t)o * n_frames, mix.begin() + (size_t)(o + 1) * n_frames));
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 6) { std::fprintf(stderr, "usage: %s <format 1..6> <channels> <n_out> <pcm> <weights>\n", argv[0]); return 2; }
    const int format = std::atoi(argv[1]), channels = std::atoi(argv[2]), n_out = std::atoi(argv[3]);
    if (channels < 1 || channels > SUSHI_HIP_MIX_MAX_CHANNELS || n_out < 1 || n_out > SUSHI_HIP_MIX_MAX_OUTPUTS) return 2;
    switch (format) {
        case SUSHI_HIP_PCM_U8: return run<sushi::PCM_U8>(channels, n_out, argv[4], argv[5]);
        case SUSHI_HIP_PCM_S16: return run<sushi::PCM_S16>(channels, n_out, argv[4], argv[5]);
        case SUSHI_HIP_PCM_S24: return run<sushi::PCM_S24>(channels, n_out, argv[4], argv[5]);
        case SUSHI_HIP_PCM_S32: return run<sushi::PCM_S32>(channels, n_out, argv[4], argv[5]);
        case SUSHI_HIP_PCM_F32: return run<sushi::PCM_F32>(channels, n_out, argv[4], argv[5]);
        case SUSHI_HIP_PCM_F64: return run<sushi::PCM_F64>(channels, n_out, argv[4], argv[5]);
    }
    return 2;
}
