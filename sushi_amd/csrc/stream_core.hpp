// sushi_amd/csrc/stream_core.hpp -- what a prepared stream is made of and where its parts lie, host only: no HIP header.  ONE table
// (stream_layout) says which parts there are, how large each is and which buffer holds it; the size of a stream's buffer, the
// pointers of its handle, those of its spectra and sushi_hip_stream_view's answers are all read from that table.  sushi_stream.hip
// and sushi_fft.hip make the HIP calls around it; tests/host_stream_check.cpp (plain g++) holds the table to the sizes the library
// has always had.
#ifndef SUSHI_STREAM_CORE_HPP
#define SUSHI_STREAM_CORE_HPP

#include <stddef.h>
#include <stdint.h>

#include "../../include/sushi_hip.h"
#include "sushi_geometry.hpp"
#include "row_core.hpp"            // row_dtype_ok

// The opaque stream handle of the C ABI: where the parts of a prepared stream live (all inside the caller's buffers).
struct SushiHipStream {
    const void* raw;          // the samples as they are (uint8 / float32), caller-owned
    int dtype;
    int64_t n;
    char* mem;                // the caller's buffer the parts up to `coarse` lie in
    float* xc;                // [n]      sample - centre
    double* s1;               // [n + 1]  prefix sums of the samples
    double* s2;               // [n + 1]  prefix sums of their squares
    float* urel;              // [n + 1]  s2 relative to the block base
    float* usrel;             // [n + 1][2]  (urel[e], s1 relative to the block base): TM_CCOEFF_NORMED on the FFT path, one 8-byte load per window end
    double* base;             // [nb + 1] block bases of s2; right behind them:
    double* base1;            // [nb + 1] block bases of s1; right behind them:
    double* stats;            // [2] FFT path: largest centred energy of seven consecutive blocks; the centring constant
    double* coarse;           // [2][nc] s2 and s1 at every COARSE_G-th sample (nc = n / COARSE_G + 2; entries past the end hold the
                              //         totals): bound_kernel's lower bound of a block pair's window energies
    int64_t nc;
    void* spec;               // [(nb + 1) * N] block spectra as packed halves, or null; behind them:
    void* spec_low;           // [(nb + 1) * N / 4] the low band (|f| < N / 8) of every block spectrum again, in bound_low_kernel's order
    float* znorm_rest;        // [3][norm_stride] norms over the bins OUTSIDE the band of a block spectrum's stored halves: of Z itself, of
                              // the spectrum of its real block at j B, of the one at j B + H (sushi_fft.hip real_block_rest_norms)
    int64_t norm_stride;
    int64_t blocks;           // nb
};

namespace sushi {

constexpr int PB = FFT_HOP;   // samples per block of the prefix sums' passes and of the relative prefix (urel / base)

// The parts, in the order they lie in.  Those from PART_SPECTRA on lie in the spectra buffer (sushi_hip_stream_add_spectra's; a
// searchable stream's is the tail of its own buffer), the others in the stream's.
enum StreamPartId { PART_XC, PART_S1, PART_S2, PART_UREL, PART_USREL, PART_BASE, PART_BASE1, PART_STATS, PART_COARSE,
                    PART_SPECTRA, PART_SPECTRA_LOW, PART_ZNORM_REST, STREAM_PARTS };
constexpr int NO_VIEW = -1;
struct StreamPart {
    int view;                 // its SUSHI_HIP_VIEW_*, or NO_VIEW
    bool in_spectra;          // which buffer `offset` counts from
    size_t offset, bytes;
};
struct StreamLayout {
    int64_t nb, nc;           // blocks of PB samples; entries of each coarse table
    StreamPart part[STREAM_PARTS];
    size_t spec;              // where a searchable stream's spectra buffer begins in the stream's buffer: the end of its own parts
    size_t total;             // bytes of the stream's buffer
};

inline StreamLayout stream_layout(int64_t n, int searchable) {
    StreamLayout l;
    l.nb = (n + PB - 1) / PB;
    l.nc = n / COARSE_G + 2;
    const size_t n0 = (size_t)n, n1 = (size_t)(n + 1), nb1 = (size_t)(l.nb + 1), F = sizeof(float), D = sizeof(double);
    const SpectraLayout sp = spectra_layout(n);
    // a part begins at the next multiple of 256 bytes behind the one before it in its buffer; a PACKED one right behind it
    constexpr bool PACKED = true, STREAM = false, SPECTRA = true;
    const struct { int view; bool in_spectra, packed; size_t bytes; } rows[STREAM_PARTS] = {
        {SUSHI_HIP_VIEW_XC, STREAM, false, n0 * F},
        {SUSHI_HIP_VIEW_S1, STREAM, false, n1 * D},
        {SUSHI_HIP_VIEW_S2, STREAM, false, n1 * D},
        {SUSHI_HIP_VIEW_UREL, STREAM, false, n1 * F},
        {SUSHI_HIP_VIEW_USREL, STREAM, false, n1 * 2 * F},                   // (urel, srel) interleaved
        {SUSHI_HIP_VIEW_BASE, STREAM, false, nb1 * D},                       // what the FFT path's scoring reads
        {SUSHI_HIP_VIEW_BASE1, STREAM, PACKED, nb1 * D},
        {NO_VIEW, STREAM, PACKED, 2 * D},                                    // stats
        {SUSHI_HIP_VIEW_COARSE, STREAM, false, 2 * (size_t)l.nc * D},
        {SUSHI_HIP_VIEW_SPECTRA, SPECTRA, false, sp.low},                    // the whole rows
        {SUSHI_HIP_VIEW_SPECTRA_LOW, SPECTRA, false, sp.norms - sp.low},
        {SUSHI_HIP_VIEW_ZNORM_REST, SPECTRA, false, sp.total - sp.norms},
    };
    size_t end[2] = {0, 0};
    for (int p = 0; p < STREAM_PARTS; ++p) {
        size_t& e = end[rows[p].in_spectra];
        const size_t at = rows[p].packed ? e : align_up(e, 256);
        l.part[p] = {rows[p].view, rows[p].in_spectra, at, rows[p].bytes};
        e = at + rows[p].bytes;
    }
    l.spec = align_up(end[STREAM], 256);
    l.total = l.spec + (searchable ? align_up(end[SPECTRA], 256) : 0);
    return l;
}

inline bool stream_dtype_ok(int dtype) { return row_dtype_ok(dtype); }

// sushi_hip_stream_bytes
inline size_t stream_bytes(int64_t n, int dtype, int searchable) { return n <= 0 || !stream_dtype_ok(dtype) ? 0 : stream_layout(n, searchable).total; }

// the handle of a stream built into `mem`, without spectra
inline void fill_stream(SushiHipStream& s, const void* raw, int dtype, int64_t n, void* mem, const StreamLayout& l) {
    s.raw = raw; s.dtype = dtype; s.n = n; s.mem = (char*)mem; s.blocks = l.nb; s.nc = l.nc;
    auto at = [&](StreamPartId p) { return (void*)(s.mem + l.part[p].offset); };
    s.xc = (float*)at(PART_XC); s.s1 = (double*)at(PART_S1); s.s2 = (double*)at(PART_S2);
    s.urel = (float*)at(PART_UREL); s.usrel = (float*)at(PART_USREL);
    s.base = (double*)at(PART_BASE); s.base1 = (double*)at(PART_BASE1); s.stats = (double*)at(PART_STATS);
    s.coarse = (double*)at(PART_COARSE);
    s.spec = nullptr; s.spec_low = nullptr; s.znorm_rest = nullptr; s.norm_stride = 0;
}

// ... and its spectra, in `mem`
inline void fill_spectra(SushiHipStream& s, void* mem, const StreamLayout& l) {
    auto at = [&](StreamPartId p) { return (void*)((char*)mem + l.part[p].offset); };
    s.spec = at(PART_SPECTRA); s.spec_low = at(PART_SPECTRA_LOW); s.znorm_rest = (float*)at(PART_ZNORM_REST);
    s.norm_stride = spectra_layout(s.n).norm_stride;
}

// sushi_hip_stream_view: a part of the spectra is NULL / 0 before they exist
inline int stream_view(const SushiHipStream& s, int which, const void** ptr, size_t* bytes) {
    const StreamLayout l = stream_layout(s.n, 0);
    for (const StreamPart& p : l.part) {
        if (p.view != which || which == NO_VIEW) continue;
        const char* buf = p.in_spectra ? (const char*)s.spec : s.mem;
        *ptr = buf ? buf + p.offset : nullptr;
        *bytes = buf ? p.bytes : 0;
        return SUSHI_HIP_OK;
    }
    return SUSHI_HIP_EINVAL;
}

}  // namespace sushi
#endif
