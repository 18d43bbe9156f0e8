// sushi_amd/csrc/sushi_internal.hpp -- types and launchers shared between the translation units of
// libsushi_hip.so (hidden visibility: not part of the C ABI).
#ifndef SUSHI_INTERNAL_HPP
#define SUSHI_INTERNAL_HPP

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <new>
#include <type_traits>
#include <utility>

#include "../../include/sushi_hip.h"
#include "sushi_common.hpp"
#include "stream_core.hpp"         // SushiHipStream

namespace sushi {

// what every launcher returns after its last launch
inline int launch_ok() { return hipGetLastError() == hipSuccess ? SUSHI_HIP_OK : SUSHI_HIP_ELAUNCH; }

// Nothing crosses the C boundary: an entry point that may allocate runs its body in here.
template <class F, class R = decltype(std::declval<F>()())>
R c_boundary(F&& body, std::common_type_t<R> no_memory = SUSHI_HIP_ENOMEM, std::common_type_t<R> other = SUSHI_HIP_EINTERNAL) {   // (R: the body's alone)
    try { return body(); } catch (const std::bad_alloc&) { return no_memory; } catch (...) { return other; }
}

// FFT path: the pairs of a sub-batch are numbered from its first search's first pair (`sub_first_pair`: that pair's number in the
// batch); `pr` is a pair of the sub-batch, `sd` its search.
// pair `pr` as a pair of its search (0 .. n_pairs - 1)
__host__ __device__ inline int pair_of_search(int sub_first_pair, int pr, const SearchDesc& sd) { return sub_first_pair + pr - sd.first_pair; }
// the search's first pair as a pair of the sub-batch
__host__ __device__ inline int first_pair_in_sub(int sub_first_pair, const SearchDesc& sd) { return sd.first_pair - sub_first_pair; }
// pair `pr` on the absolute pair grid (fft_layout)
__host__ __device__ inline int64_t absolute_pair(const FftLayout& lay, int sub_first_pair, int pr, const SearchDesc& sd) {
    return lay.pair0 + (sub_first_pair + pr - sd.first_pair);
}

struct StreamRefs {
    const float* dst_xc; const double* dst_s1; const double* dst_s2; int64_t dst_len;
    const float* src_xc; const double* src_s1; const double* src_s2; int64_t src_len;
    double centre;
    const void* dst_raw; const void* src_raw; int dtype;     // the samples as they are (exact evaluation)
};

int direct_variant_count();
int direct_variant_tile(int variant);

// direct path (sushi_direct.hip): one launch of the MFMA kernel + unpack
int launch_direct(const StreamRefs& r, const SearchDesc* searches_dev, int n_search, int n_tiles, int variant, int method,
                  unsigned long long* keys_dev, int32_t* out_idx_dev, float* out_score_dev, int32_t* out_packed_dev, hipStream_t st);

// FFT path, exact stages (sushi_exact.hip):
// refine: exact float64 evaluation of the listed candidates of searches [first_search, first_search + n_sub).
// flags_dev[s] = 0 done / 1 needs tiles / 2 every position; flag_list_dev receives the flagged searches of this sub-batch.
struct RefineParams {
    StreamRefs r;
    const SearchDesc* searches;       // all searches of the batch
    int first_search, n_sub, sub_first_pair;
    const unsigned long long* cand;   // [pairs of the sub-batch][FFT_ROW]
    const float* pair_lb;             // [pairs of the sub-batch] smallest lower bound of each pair
    unsigned long long* gkeys;        // [all searches] in: min over pairs of (f32 score + bound); out: |f32 - exact| bits
    unsigned long long* keys;         // [all searches] result keys
    int* flags;                       // [all searches]
    int* flag_list;                   // [n_sub] flagged searches of this sub-batch (global indices)
    SubCounters* sub;                 // this sub-batch's counters (sub_flagged: how many)
    int* citems;                      // [pairs of the sub-batch] out: the pairs of flagged searches collect_kernel has to look at
    int* n_citems;                    // [1] how many
    RunCounters* counters;
    float delta;
    int method;                       // SUSHI_HIP_METHOD_*
    const int* viol;                  // [all searches] or NULL: 1 = a pair's lower bound was found above a real score (ifft_kernel's audit)
    int4* early;                      // [all searches] or NULL: sushi_hip_batch_set_early_output's records (host memory mapped to the device)
};
int launch_refine(const RefineParams& p, hipStream_t st);

// Up to FILL_RANGES ranges of 32-bit words set to a value each, in ONE launch: what a run clears before its first kernel (result
// keys, flags, counters, the candidate rows of a small batch) used to be half a dozen hipMemsetAsync calls -- a third of the
// launches of a drop-in find_substream call, whose cost IS its launches.
constexpr int FILL_RANGES = 8;
struct FillArgs { uint32_t* p[FILL_RANGES]; uint32_t words[FILL_RANGES]; uint32_t value[FILL_RANGES]; int n; };
int launch_fill(const FillArgs& a, hipStream_t st);

struct TileParams {
    StreamRefs r;
    const SearchDesc* searches;
    const TileDesc* tiles;
    const int32_t* cand;              // candidate positions (relative to the search window)
    unsigned long long* keys;
    RunCounters* counters;
    SubCounters* sub;                 // this sub-batch's tile list length and queue head (read / advanced on the device)
    int method;                       // SUSHI_HIP_METHOD_*
};
int launch_tiles(const TileParams& p, hipStream_t st);

// A pair's byte of a sub-batch's `audit_mark` array (FFT path: what the bound decided about the pair in this run), as bits:
constexpr int MARK_AUDITED = 1;        // the bound had excluded the pair; it is transformed / evaluated all the same, as a check of the bound
constexpr int MARK_LISTED = 2;         // the pair is listed: its row is formed, or (a listed-pair run) it is evaluated
constexpr int MARK_SECOND_LOOK = 4;    // an audited pair that the second look (not the first bound) had excluded
constexpr int MARK_BEST_FINAL = 8;     // a best-K run: an audited pair that best_final_kernel listed

// FFT path, the listed-pair runs: threshold (sushi_hip_batch_run_threshold) and best-K (sushi_hip_batch_run_best;
// DESIGN.md 3.11).  A listed block pair is evaluated exactly at each of its 2 FFT_H positions, as TILES_PER_PAIR tiles of TILE
// consecutive ones (the curves' tile bodies, sushi_curve.hip).  What a pair leaves lies in its own 64 KB row of the sub-batch's Y
// region (neither run forms whole rows after the bound has read them).
constexpr int THR_SLOT_WORDS = FFT_N;                          // 32-bit words of a pair's row (FFT_N packed-half bins)
// What the tile kernels of both runs read to find their work (sushi_fft.hip listed_pairs fills it, sushi_curve.hip listed_tile
// decodes a work item from it): the streams, the sub-batch's searches, the list of pairs to evaluate, the pairs' rows.
struct ListedPairs {
    StreamRefs r;
    const SearchDesc* searches;       // the sub-batch's searches
    const int* pairmap;               // [pairs of the sub-batch] -> search of the sub-batch
    int sub_first_pair;
    int first_search;                 // global index of searches[0]: its output slot
    const int* list;                  // the pairs to evaluate: list[0 .. *list_count), or [0 .. list_max) where list_count is NULL
    const int* list_count;
    int list_max;                     // the sub-batch's pairs: every list holds distinct pairs of it, so no list is longer
    uint32_t* rows;                   // [pairs of the sub-batch][THR_SLOT_WORDS]
    int method;
};

// Threshold run: a pair's row
constexpr int THR_MASK = 0;                                    // [TILES_PER_PAIR * TILE / 32] bit i: position i of the pair passes
constexpr int THR_COUNT = TILES_PER_PAIR * TILE / 32;          // [TILES_PER_PAIR] hits per tile
constexpr int THR_MIN = THR_COUNT + TILES_PER_PAIR;            // [TILES_PER_PAIR] float bits: smallest ranking score of the tile
constexpr int THR_OFF = THR_MIN + TILES_PER_PAIR;              // the pair's first hit in its search's output (thr_scan_kernel)
static_assert(THR_OFF < THR_SLOT_WORDS, "a pair's hit mask and counts fit its row");
struct ThresholdTileParams {
    ListedPairs lp;
    double threshold;                 // SQDIFF_NORMED: score <= threshold; CCOEFF_NORMED: score >= threshold
    int pass;                         // 0: hit masks, counts and minima; 1: (index, score) of every hit into `hits`
    SushiHipHit* hits;                // [searches][capacity]
    int32_t capacity;
};
int launch_threshold_tiles(const ThresholdTileParams& p, hipStream_t st);

// Best-K run.  An evaluated pair's row holds, per tile, the best eligible position of the tile as a 64-bit pick key -- the smaller
// key is the better pick: the float32 score under the order-preserving map of its bits (ordered_bits; negated for TM_CCOEFF_NORMED;
// -0.0 and 0.0 tie), then the lower index -- once as evaluated (BEST_KEY: no pick masked) and once as the selection works on it
// (BEST_WORK: dead tiles NO_KEY, tiles a pick's window cuts evaluated again with the picks masked); and the tile's smallest ranking
// score over ALL its positions (THR_MIN: the bound's audit, as in a threshold run).
constexpr int BEST_KEY = 0;                                    // [TILES_PER_PAIR] 64-bit keys
constexpr int BEST_WORK = 2 * TILES_PER_PAIR;                  // [TILES_PER_PAIR] 64-bit keys
static_assert(BEST_WORK + 2 * TILES_PER_PAIR <= THR_COUNT, "the pick keys lie in front of the tile minima");
constexpr int BEST_MAX_K = SUSHI_HIP_BEST_MAX_K;
struct BestParams {
    ListedPairs lp;                   // (the list: best_tiles_kernel's)
    int n_sub;
    const unsigned char* audit_mark;  // MARK_LISTED: the pair is evaluated; NULL: every pair is
    int has_threshold;
    double threshold;                 // eligible: score <= threshold (SQDIFF_NORMED) / >= threshold (CCOEFF_NORMED)
    unsigned long long tkey;          // the threshold in ranking units, rounded up, as a search key; NO_KEY: none
    int k;                            // picks per search
    int min_separation;               // 0: the search's own tmpl_len
    const int* stamp_flags;           // [all searches] best_select_kernel works on the searches whose word is `stamp`; NULL: on all
    int stamp;
    unsigned long long* gkeys;        // [all searches] out: what a pair's bound is compared with from now on
    SushiHipHit* hits;                // [all searches][k]
    int32_t* counts;                  // [all searches]
    int* reset0; int* reset1;         // list lengths best_select_kernel clears for the round after it (or NULL)
};
int launch_best_tiles(const BestParams& p, hipStream_t st);
int launch_best_select(const BestParams& p, hipStream_t st);
int launch_unpack(const unsigned long long* keys_dev, int n, int method, int32_t* out_idx_dev, float* out_score_dev,
                  int32_t* out_packed_dev, hipStream_t st);

}  // namespace sushi
#endif
