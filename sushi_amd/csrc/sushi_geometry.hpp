// sushi_amd/csrc/sushi_geometry.hpp -- the sizes and small records the host's plan of a batch and the device code agree on:
// overlap-save geometry, segment-count classes, the records a workgroup finds its work by, the rows and work items of the
// multiply-accumulate.  Each defined once, here.  Compiles with plain g++ (tests/host_plan_check.cpp, through plan_core.hpp)
// and with hipcc (every translation unit of the library, through sushi_common.hpp).
#ifndef SUSHI_GEOMETRY_HPP
#define SUSHI_GEOMETRY_HPP

#include <stddef.h>
#include <stdint.h>

#include "../../include/sushi_hip.h"

#ifdef __HIPCC__
#define SUSHI_GEOM_HD __host__ __device__
#else
#define SUSHI_GEOM_HD
#endif

namespace sushi {

// ---- overlap-save geometry ------------------------------------------------------------
// Transform length N = 2^FFT_LOGN complex points; patterns are cut into segments of FFT_SEG samples, so a real
// block of N samples yields FFT_H = N - FFT_SEG valid positions; two real blocks FFT_H apart are packed into one
// complex block (a "pair": 2 * FFT_H positions per transform).  Spectra are kept at every multiple of FFT_SEG
// ("block" j = samples from j * FFT_SEG on); consecutive pairs of a search are FFT_STEP blocks apart.
constexpr int FFT_LOGN = 14;
constexpr int FFT_N = 1 << FFT_LOGN;
constexpr int FFT_SEG = 4096;
constexpr int FFT_HOP = FFT_SEG;                   // also the block size of the relative window-energy prefix (urel / base)
constexpr int FFT_VB = FFT_N / FFT_SEG - 1;        // valid blocks per half of a pair: 3
constexpr int FFT_H = FFT_VB * FFT_SEG;            // result positions per half
constexpr int FFT_STEP = 2 * FFT_VB;               // blocks between consecutive pairs
constexpr int FFT_CAND = 8;                        // candidate slots per block pair (+ overflow marker + error bound + audit positions)
constexpr int FFT_AUDIT = 4;                       // positions of an audit run: consecutive (one exact evaluation's worth of loads)
constexpr int AUDIT_RUNS = 4;                      // audit runs a transformed pair leaves, and audit runs refine_kernel evaluates per search
constexpr int FFT_ROW = 32;                        // 64-bit entries per pair in the candidate array: two 128-byte lines
static_assert(FFT_CAND + 2 + AUDIT_RUNS * FFT_AUDIT <= FFT_ROW, "candidates, overflow marker, error bound, audit runs");
constexpr int TILE = 1024;                         // positions per exact-evaluation tile (aligned to the absolute grid)
constexpr int TILES_PER_PAIR = 2 * FFT_H / TILE;
constexpr int COARSE_G = 256;                      // granularity of the coarse prefix table (SushiHipStream.coarse)
// The pair bound's window energies (slb_kernel): a pair's positions are SLB_STRETCHES stretches of COARSE_G, looked up by the
// `group` lanes that take the pair -- a wave, or a row of sixteen --, lane l the stretches l, l + group, ... (one beyond the last
// stretch is masked: a wave's last lanes have no second one).
constexpr int SLB_STRETCHES = 2 * FFT_H / COARSE_G;
SUSHI_GEOM_HD constexpr int slb_stretches_a_lane(int group) { return (SLB_STRETCHES + group - 1) / group; }
SUSHI_GEOM_HD constexpr int slb_stretch(int lane, int t, int group) { return lane + group * t; }

// Overlap-save layout of one search (DESIGN.md "FFT path"): its block pairs sit on the ABSOLUTE pair grid (pair I
// starts at block FFT_STEP * I), from the pair holding the window's first position to the one holding its last.
struct FftLayout { int64_t pair0; int n_pairs; int n_seg; };
SUSHI_GEOM_HD inline FftLayout fft_layout(int64_t win_start, int n_pos, int tmpl_len) {
    FftLayout l;
    l.pair0 = (win_start / FFT_SEG) / FFT_STEP;
    const int64_t pair_last = ((win_start + n_pos - 1) / FFT_SEG) / FFT_STEP;
    l.n_pairs = (int)(pair_last - l.pair0 + 1);
    l.n_seg = (tmpl_len + FFT_SEG - 1) / FFT_SEG;
    return l;
}

// segment-count class of a search: the smallest SMAX (a multiple of FFT_STEP) that holds the whole pattern.  Classes
// 0 .. MAC_SHORT_CLASSES-1 (up to 18 segments) run in mac_kernel, the others (up to 30: a 5 s pattern at 24 kHz, BASELINE
// configs[4]'s longest) in mac_long_kernel, which keeps more pattern spectra per lane at a lower occupancy; still longer
// patterns use the largest class and several chunks of its SMAX segments, the output accumulating.  (A sixth class of 36
// segments made mac_long_kernel spill at its 256 registers: 144 of them were pattern spectra.)
constexpr int MAC_CLASSES = 5;
constexpr int MAC_SHORT_CLASSES = 3;
SUSHI_GEOM_HD constexpr int mac_class_smax(int c) { return FFT_STEP * (c + 1); }
SUSHI_GEOM_HD inline int mac_class(int n_seg) {
    for (int c = 0; c < MAC_CLASSES - 1; ++c)
        if (n_seg <= mac_class_smax(c)) return c;
    return MAC_CLASSES - 1;
}

// the two matching methods (include/sushi_hip.h): what every entry point that takes a method refuses by
SUSHI_GEOM_HD inline bool method_known(int method) {
    return method == SUSHI_HIP_METHOD_SQDIFF_NORMED || method == SUSHI_HIP_METHOD_CCOEFF_NORMED;
}

// sizes of device-memory parts are rounded up to 256 bytes
inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

// What a request must be, for every entry point that takes requests: a pattern and a window of at least one sample / position,
// both short enough that no count derived from them (tiles, pairs, positions past the window) leaves 32 bits, the pattern inside
// its source stream of `src_n` samples and the window's last read inside the destination's `dst_n`.  (Written without a sum that
// could overflow.)  sushi_amd/device.py _checked_requests restates it for its messages.
constexpr int32_t REQUEST_MAX_TERM = 0x7fffffff - 65536;      // n_pos, tmpl_len
inline bool request_fits(const SushiHipRequest& r, int64_t dst_n, int64_t src_n) {
    if (r.tmpl_len < 1 || r.n_pos < 1 || r.win_start < 0 || r.tmpl_off < 0) return false;
    if (r.n_pos > REQUEST_MAX_TERM || r.tmpl_len > REQUEST_MAX_TERM) return false;
    return r.tmpl_len <= src_n - r.tmpl_off && (int64_t)r.n_pos + r.tmpl_len - 1 <= dst_n - r.win_start;
}

// One search on the device: a SushiHipRequest plus the running sums that let a workgroup find its work.
struct SearchDesc {
    int64_t tmpl_off;
    int64_t win_start;
    int32_t tmpl_len;
    int32_t n_pos;
    int32_t first_tile;   // direct path: tiles of the searches before this one
    int32_t first_pair;   // FFT path: block pairs of the searches before this one
    int32_t first_seg;    // FFT path: pattern segments of the searches before this one
    int32_t reserved;
};
static_assert(sizeof(SearchDesc) == 40, "SearchDesc layout");

// One exact-evaluation work item: TILE consecutive positions of one search, aligned to the absolute grid.
constexpr int SPARSE_TILE_MAX = 256;   // candidates per tile up to which collect_kernel lists them; beyond: every position of the tile
constexpr int SPARSE_UNIT = 64;        // a listed tile is handed to exact_tiles_kernel in entries of at most this many candidates
struct TileDesc {
    int32_t search;       // global search index
    int32_t p0;           // first position of the tile relative to the search's window (may be < 0 for the first tile)
    int32_t off;          // sparse: first entry of the tile's candidate list in the candidate buffer
    int32_t cnt;          // sparse: candidates of this entry (<= SPARSE_UNIT: a tile of more is several entries); dense (every valid position of the tile): -1
};

// Counters of one run, in device memory (zeroed at the start of a run).
// What the exact stages of ONE sub-batch count with: every sub-batch of a plan has its own (sub-batches of a batch may run side by
// side on several HIP streams: plan_core.hpp "Lanes"); cleared by the run's first launch.
struct SubCounters {
    int32_t n_tiles;          // entries of the tile list
    int32_t tile_next;        // exact_tiles_kernel's queue: the next entry to hand out
    int32_t n_cand;           // entries of the candidate buffer
    int32_t sub_flagged;      // searches of this sub-batch refine_kernel flagged (entries of its part of the flag list)
};

// (of the whole run; the batch's layout keeps room for one: plan_core.hpp batch_layout)
struct RunCounters {
    int32_t n_flagged;        // searches refine_kernel could not finish from the per-pair lists
    int32_t n_all_positions;  // of those: every position (bound violated)
    unsigned long long tiles_dense, tiles_sparse, candidates;    // totals of the run
    uint32_t max_ratio_bits;  // float bits of SushiHipBatchDiag.max_bound_ratio
    uint32_t max_ratio_audit_bits;  // float bits of SushiHipBatchDiag.max_bound_ratio_noncandidate
    unsigned long long audited;     // non-candidate positions evaluated exactly (SushiHipBatchDiag.audited)
    unsigned long long pairs_transformed;   // block pairs whose inverse transform was run (the others were excluded by bound_kernel's bound)
    unsigned long long excluded_audited;    // of those: pairs the bound HAD excluded, transformed as a check of the bound
    uint32_t max_slb_ratio_bits;            // float bits: largest (lower bound / upper bound of the pair's real best score) over the audited excluded pairs
    int32_t slb_violations;                 // pairs whose lower bound turned out above a real score (their searches go to every position)
    unsigned long long second_look_audited; // of excluded_audited: pairs the second look had excluded (survivor2_kernel's sample)
};

// per-search constants of the f32 scoring epilogue, computed once (float64) by tspec_kernel
struct TemplConsts {
    double tU;           // sum T^2 (uncentred)
    float inv_tnorm;     // 1 / sqrt(sum T^2)
    float tnorm;         // sqrt(sum T^2)
    // TM_CCOEFF_NORMED (cv2's numType == 1 statistics, sushi_common.hpp templ_stats)
    float tmean;         // mean T
    float inv_tnorm_c;   // 1 / sqrt(sum (T - mean T)^2); 0 for a flat pattern
    float inv_m;         // 1 / M
    int flat;            // the pattern has no variance: cv2's result is all ones
    float c_sum_t;       // c * sum T: sum T I = y' + c_sum_t (block spectra are of the centred destination samples)
    float inv_scale;     // 1 / the power-of-two scale of this search's stored products Y
    float mac_scale;     // what mac_kernel multiplies its float32 sums by when it stores them: scale of Y / (scale of Tt * scale of Z)
};

// ---- stored rows (sushi_fft_store.inc): block spectra, pattern spectra and their products as packed halves ----
constexpr int ROW_BYTES = FFT_N * 4;           // a stored spectrum: one 32-bit word per bin
constexpr int ROWE = FFT_N / 4;                // ... as 16-byte entries (four bins: what a lane of mac_kernel owns, sushi_mac::BINS)
// The low band of every spectrum (bins |f| < N/8) is kept a second time, as rows of LROWE entries in the order bound_low_kernel
// loads them (fft_core.hpp "LOW BAND"): the band-split exclusion multiplies, stores and transforms only these.
constexpr int LROWE = FFT_N / 16;              // 16-byte entries of a low row (sushi_fft::LB_ENTRIES)
constexpr int LROW_BYTES = LROWE * 16;
// A pattern segment's whole row is stored as a HALF row where its transform leaves it conjugate-symmetric word for word (the real
// route: run_policy.hpp tspec_half_rows): half the entries and one run of sixteen more (fft_core.hpp "HALF ROWS").
constexpr int HROWE = ROWE / 2 + 16;           // 16-byte entries of a half row (sushi_fft::HALF_ROWE)
constexpr int HROW_BYTES = HROWE * 16;         // (a workspace keeps a whole row's room per segment on either route: plan_core.hpp ws_layout)
// The spectra of a searchable stream of n samples (sushi_hip_stream_add_spectra), as they lie in the memory it is given: a whole
// row per block and one more (its samples are all past the end, so its spectrum is zero), from `low` on their low rows, from
// `norms` on three arrays of `norm_stride` floats -- the rows' norms outside the band: of Z, of its two real blocks.
struct SpectraLayout { size_t low, norms, total; int64_t norm_stride; };
inline SpectraLayout spectra_layout(int64_t n) {
    const size_t rows = (size_t)((n + FFT_SEG - 1) / FFT_SEG + 1), norm_bytes = align_up(rows * sizeof(float), 256);
    SpectraLayout l;
    l.low = rows * ROW_BYTES; l.norms = l.low + rows * LROW_BYTES; l.total = l.norms + 3 * norm_bytes;
    l.norm_stride = (int64_t)(norm_bytes / sizeof(float));
    return l;
}

// ---- the multiply-accumulate's work items (sushi_fft_mac.inc) ----
constexpr int MAC_SPW = 8;                       // searches per wave
constexpr int MAC_BPW = 64 / MAC_SPW;            // 4-bin entries per wave
constexpr int MAC_WAVES = 4;
constexpr int MAC_THREADS = MAC_WAVES * 64;
constexpr int MAC_BW = MAC_BPW * MAC_WAVES;      // entries per workgroup
constexpr int MAC_DUMMY_LINES = 1024;
constexpr int MAC_CHUNKS = ROWE / MAC_BW;
static_assert(MAC_CHUNKS % 8 == 0, "every XCD owns the same number of bin chunks");

constexpr int VOTE_SLOTS = 64, VOTE_STRIDE = 32;      // the form prediction's counters (sushi_fft_bound.inc): 64 pairs of ints, 128 bytes apart

}  // namespace sushi
#endif
