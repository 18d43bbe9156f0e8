/*
 * include/sushi_hip.h -- C ABI of libsushi_hip.so (MI355X / gfx950 only)
 *
 * The reference (tp7/Sushi) has no FFI on this path: `wav.WavStream.find_substream`
 * (wav.py:177-188) calls `cv2.matchTemplate(..., cv2.TM_SQDIFF_NORMED)` (wav.py:185) and
 * `ndarray.argmin` (wav.py:186) in-process.  These entry points are what a ctypes binding
 * inside a drop-in `wav.py` binds instead of `import cv2`:
 *
 *   sushi_hip_stream_create    once per WavStream, right after wav.py:108-162 has built `self.data`:
 *                              what cv2 redoes inside every matchTemplate call on the search image
 *                              (the CV_64F integral of common_matchTemplate, the block DFTs of crossCorr)
 *                              is done once per stream and kept in HBM.
 *   sushi_hip_batch_create     a batch of find_substream calls after their window arithmetic
 *                              (wav.py:178-184): one SushiHipRequest per call.
 *   sushi_hip_batch_run        replaces wav.py:185-186 for the whole batch: one (index, score) per request.
 *
 * Conventions: extern "C", plain pointers and sizes, no C++ or torch types.  Every pointer named *_dev is a
 * device (HBM) pointer owned by the caller; *_host pointers are host memory read during the call only.
 * The library allocates NO device memory: a handle is built inside a buffer the caller provides
 * (sushi_hip_*_bytes tells its size) and the caller keeps that buffer -- and, for a stream, the samples --
 * alive until the handle is destroyed.  `hip_stream` is a hipStream_t passed as void* (NULL = the default
 * stream).  Calls are asynchronous with respect to the host and return 0 or a negative SUSHI_HIP_E* code;
 * no exception crosses the boundary.  A handle may be used from one host thread at a time.
 */
#ifndef SUSHI_HIP_H
#define SUSHI_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SUSHI_HIP_ABI_VERSION 13  /* 10: band-split exclusion (low-band rows + row norms behind the spectra, SUSHI_HIP_EXCLUDE_BAND / _WHOLE,
                                     SushiHipBatchDiag.excluded_audited / .max_slb_ratio_excluded / .slb_violations / .band / .band_votes);
                                     11: SushiHipBatchDiag.second_look_audited (appended);
                                     12: sushi_hip_batch_set_bound_model (the excluded side of the pair exclusion is a worst-case bound by
                                     default), the band is |f| < N/8 strictly (bin 7N/8 of a low row is zero and counted with the rest), sushi_hip_batch_reset,
                                     sushi_hip_batch_workspace_view, SUSHI_HIP_ENOMEM / _EINTERNAL;
                                     13: SushiHipBatchInfo.lanes (appended): a large batch's sub-batches run side by side on HIP streams
                                     of the library's own, forked off and joined back into the stream a run is given;
                                     sushi_hip_batch_set_early_output, sushi_hip_device_prepare;
                                     13 (additive): sushi_hip_curve_bytes, sushi_hip_match_curves;
                                     13 (additive): SushiHipHit, sushi_hip_batch_run_threshold;
                                     13 (additive): SUSHI_HIP_BEST_MAX_K, sushi_hip_batch_run_best;
                                     13 (additive): SushiHipRetimeSegment, sushi_hip_retime_bytes, sushi_hip_retime;
                                     13 (additive): SUSHI_HIP_MIX_MAX_CHANNELS / _OUTPUTS, sushi_hip_load_decode_mix;
                                     13 (additive): sushi_hip_load_resample_fir;
                                     13 (additive): SushiHipJointRow, SushiHipJointGroup, sushi_hip_joint_bytes, sushi_hip_joint_reduce;
                                     13 (additive): sushi_hip_path_bytes, sushi_hip_path_stay_words, sushi_hip_path_forward,
                                     sushi_hip_path_backtrack;
                                     13 (additive): sushi_hip_drift_bytes, sushi_hip_drift_reduce;
                                     13 (additive): SUSHI_HIP_TRACK_MAX_REACH, SUSHI_HIP_TRACK_JUMP, sushi_hip_track_bytes,
                                     sushi_hip_track_forward, sushi_hip_track_backtrack;
                                     13 (additive): sushi_hip_track_forward_keep, sushi_hip_track_margins_bytes, sushi_hip_track_margins;
                                     13 (additive): SUSHI_HIP_TRACK_BACK_ANY, sushi_hip_track_order_bytes,
                                     sushi_hip_track_forward_ordered, sushi_hip_track_backtrack_ordered;
                                     13 (additive): sushi_hip_track_forward_ordered_keep, sushi_hip_track_order_margins_bytes,
                                     sushi_hip_track_order_margins;
                                     13 (additive): SUSHI_HIP_TRACK_WIDE_MAX_REACH, sushi_hip_track_wide_bytes,
                                     sushi_hip_track_margins_wide_bytes, sushi_hip_track_forward_wide,
                                     sushi_hip_track_forward_wide_keep, sushi_hip_track_margins_wide;
                                     13 (additive): sushi_hip_track_order_wide_bytes, sushi_hip_track_order_margins_wide_bytes,
                                     sushi_hip_track_forward_ordered_wide, sushi_hip_track_forward_ordered_wide_keep,
                                     sushi_hip_track_order_margins_wide;
                                     13 (additive): SUSHI_HIP_PCM_*, sushi_hip_load_decode_format, sushi_hip_load_decode_mix_format;
                                     13 (additive): sushi_hip_envelope;
                                     13 (additive): sushi_hip_filter;
                                     13 (additive): sushi_hip_level */

#if defined(__GNUC__)
#define SUSHI_HIP_API __attribute__((visibility("default")))
#else
#define SUSHI_HIP_API
#endif

/* error codes */
#define SUSHI_HIP_OK 0
#define SUSHI_HIP_EINVAL (-1)    /* bad argument (null pointer, negative size, unknown dtype/path/variant, request outside its stream) */
#define SUSHI_HIP_EALIGN (-2)    /* a device pointer is not aligned as documented */
#define SUSHI_HIP_ELAUNCH (-3)   /* the HIP runtime rejected a launch / copy / memset (see hipGetLastError) */
#define SUSHI_HIP_ENOSPACE (-4)  /* buffer or workspace too small */
#define SUSHI_HIP_ENODEV (-5)    /* no gfx950 device visible */
#define SUSHI_HIP_ENOMEM (-6)    /* the host ran out of memory while a handle, a plan or an upload was built (std::bad_alloc caught at the
                                    boundary; sushi_hip_stream_create and sushi_hip_batch_create alike) */
#define SUSHI_HIP_EINTERNAL (-7) /* any other C++ exception caught at the boundary: a bug, never a property of the input */

/* sample types of WavStream.data (wav.py:109: 'uint8' or 'float32') */
#define SUSHI_HIP_U8 0
#define SUSHI_HIP_F32 1

/* how a batch is matched.  Both give the same results (tests/test_gpu_parity.py). */
#define SUSHI_HIP_PATH_FFT 0     /* overlap-save FFT ranking + exact float64 evaluation of the near-minimum positions */
#define SUSHI_HIP_PATH_DIRECT 1  /* exact-f32 MFMA sliding dot product, O(P*M) */

/* what cv2.matchTemplate's `method` argument selects (and which extremum the caller takes) */
#define SUSHI_HIP_METHOD_SQDIFF_NORMED 0  /* cv2.TM_SQDIFF_NORMED + argmin: what wav.py:185-186 does; both paths */
#define SUSHI_HIP_METHOD_CCOEFF_NORMED 1  /* cv2.TM_CCOEFF_NORMED + argmax (BASELINE.json's wording); both paths */

SUSHI_HIP_API int sushi_hip_abi_version(void);
SUSHI_HIP_API const char* sushi_hip_strerror(int code);

/* 0 if a gfx950 device is current, SUSHI_HIP_ENODEV otherwise. */
SUSHI_HIP_API int sushi_hip_device_ok(void);
/* What a batch's first run would otherwise create on the current device, made NOW (v13): the HIP streams the lanes of large batches
 * run on (a stream is a hardware queue: ~5 ms each) and the pinned words a run's counts come back through.  Optional -- a process
 * that calls it while it is busy elsewhere (sushi_amd.device.warm_up does, behind the demux) takes 11 ms off its first large batch. */
SUSHI_HIP_API int sushi_hip_device_prepare(void);

/* ---- streams --------------------------------------------------------------------------------------------
 * raw_dev: the n samples of the row WavStream.data[0] (`dtype`), already in HBM; they stay the caller's and
 * are read again by every batch (pattern spectra, exact evaluation).  Built into mem_dev (256-byte aligned,
 * >= sushi_hip_stream_bytes(n, dtype, searchable) bytes):
 *   xc[n]      float32  sample - centre (0.5 for float32 data in [0,1], 128 for uint8): the direct path's operand
 *   s1[n+1], s2[n+1]  float64 exclusive prefix sums of the samples and of their squares AS THEY ARE (the CV_64F
 *              integral cv2 builds per call; exact for uint8)
 *   urel[n+1]  float32 + base[nb+1] float64, nb = ceil(n / B), B = sushi_hip_fft_block():
 *              s2[e] = base[e / B] + urel[e]   (the window energies in the cheap form the FFT scoring reads)
 *   usrel[n+1][2] float32 + base1[nb+1] float64: (urel[e], srel[e]) interleaved, srel = the same for s1 (the window sums of
 *              TM_CCOEFF_NORMED, which reads both prefixes with one 8-byte load per window end)
 *   spectra    (searchable streams only; sushi_hip_stream_add_spectra attaches them later)  for every block
 *              j = 0 .. nb-1 the N-point complex DFT, N = sushi_hip_fft_size(), H = N - B, of
 *                  (x - mean)[jB .. jB+N) + i * (x - mean)[jB+H .. jB+H+N)         (zeros past the end)
 *              as packed halves (float16 re, float16 im: 4 bytes per bin) times one power of two per stream, bin f at
 *              sushi_hip_fft_slot_of_bin(f), followed by one all-zero block:
 *              (nb + 1) * N * 4 bytes; behind them, for the band-split form of the pair exclusion:
 *              the LOW BAND (bins |f| < N/8; the slot of bin 7N/8 is zero) of every block spectrum once more, (nb + 1) * N bytes, in the order
 *              the bound's transform loads it, and float32[nb + 1]: the norm of each block spectrum's stored halves
 *              OUTSIDE that band.  sushi_hip_stream_spectra_bytes(n) is the sum.
 * A stream that is only a source of patterns does not need spectra. */
typedef struct SushiHipStream SushiHipStream;

SUSHI_HIP_API int sushi_hip_fft_size(void);      /* N: complex points per transform */
SUSHI_HIP_API int sushi_hip_fft_block(void);     /* B: samples per block = per pattern segment */
/* Where bin f (0 <= f < N) of a block spectrum sits inside its N stored complex values (4 bytes each): spectra are kept
 * in the order the inverse transform loads them (coalesced 16-byte loads), not in natural order.  -1 for an invalid bin. */
SUSHI_HIP_API int sushi_hip_fft_slot_of_bin(int bin);
/* The same for the low-band rows behind the spectra (bins f < N/8 and f >= 7N/8 only; N/4 complex values of 4 bytes per row):
 * their order is the one the band-split bound's transform loads them in.  -1 for a bin outside the band. */
SUSHI_HIP_API int sushi_hip_fft_low_slot_of_bin(int bin);
SUSHI_HIP_API double sushi_hip_centre(int dtype);
SUSHI_HIP_API size_t sushi_hip_stream_bytes(int64_t n, int dtype, int searchable);
SUSHI_HIP_API size_t sushi_hip_stream_spectra_bytes(int64_t n);
SUSHI_HIP_API int sushi_hip_stream_create(const void* raw_dev, int dtype, int64_t n, int searchable,
                                          void* mem_dev, size_t mem_bytes, void* hip_stream, SushiHipStream** out);
SUSHI_HIP_API int sushi_hip_stream_add_spectra(SushiHipStream* stream, void* mem_dev, size_t mem_bytes, void* hip_stream);
/* Where a part lives (for tests and diagnostics): which = SUSHI_HIP_VIEW_*; SPECTRA gives NULL / 0 before they exist. */
#define SUSHI_HIP_VIEW_XC 0
#define SUSHI_HIP_VIEW_S1 1
#define SUSHI_HIP_VIEW_S2 2
#define SUSHI_HIP_VIEW_UREL 3
#define SUSHI_HIP_VIEW_BASE 4
#define SUSHI_HIP_VIEW_SPECTRA 5
#define SUSHI_HIP_VIEW_USREL 6    /* float32[n+1][2]: (urel[e], srel[e]), s1[e] = base1[e / B] + srel[e] (TM_CCOEFF_NORMED's window sums on the FFT path) */
#define SUSHI_HIP_VIEW_BASE1 7    /* float64[nb+1] */
#define SUSHI_HIP_VIEW_COARSE 8   /* float64[2][n / 256 + 2]: s2, then s1, at every 256th sample (entries past the end: the totals) --
                                    what the FFT path's lower bound of a block pair's window energies reads */
#define SUSHI_HIP_VIEW_SPECTRA_LOW 9   /* the low-band rows behind the spectra (packed halves, N bytes per block) */
#define SUSHI_HIP_VIEW_ZNORM_REST 10   /* float32[nb + 1]: norm of each block spectrum outside the band */
SUSHI_HIP_API int sushi_hip_stream_view(const SushiHipStream* stream, int which, const void** ptr_dev, size_t* bytes);
SUSHI_HIP_API void sushi_hip_stream_destroy(SushiHipStream* stream);

/* ---- batches --------------------------------------------------------------------------------------------
 * One request = one call of WavStream.find_substream (wav.py:177-188) after its window arithmetic: `pattern` is
 * src.data[0, tmpl_off : tmpl_off + tmpl_len] and `search_source` is
 * dst.data[0, win_start : win_start + n_pos + tmpl_len - 1]; n_pos = result.shape[1]. */
typedef struct SushiHipRequest {
    int64_t tmpl_off;
    int64_t win_start;
    int32_t tmpl_len;
    int32_t n_pos;
} SushiHipRequest;        /* 24 bytes */

typedef struct SushiHipBatchInfo {
    int32_t n_search;
    int32_t path;
    int32_t variant;          /* direct path: tile-size variant in use */
    int32_t sub_batches;      /* FFT path: launches of each kernel per run (the batch is cut to fit the workspace, or -- a large batch --
                                 into parts that run side by side: `lanes`) */
    int64_t direct_tiles;
    int64_t fft_pairs;        /* FFT path: block pairs (inverse transforms) of the whole batch */
    int64_t fft_segments;     /* FFT path: pattern segments (forward transforms) of the whole batch */
    uint64_t workspace_bytes; /* of mem_bytes: scratch reused by the sub-batches */
    uint64_t mem_bytes;       /* what sushi_hip_batch_bytes returned */
    double flops;             /* 2 * P * M summed over the requests (the direct form's work) */
    double algorithmic_bytes; /* every search and pattern sample once + 8 bytes out per request */
    int32_t lanes;            /* FFT path: HIP streams the sub-batches of a run are spread over (1: all on the stream the run is given).
                                 Lane 0 IS that stream; the others are the library's own (one set per device, made by the first run
                                 that needs them or by sushi_hip_device_prepare), start behind the run's first launch and are joined
                                 before its last, so the caller sees one stream's ordering.  The stages of the path are bound by
                                 different things (stores, instruction issue, LDS, HBM reads): side by side they fill each other's gaps.
                                 SUSHI_HIP_LANES="subs:lanes" in the environment when the batch is created overrides the choice. */
    int32_t reserved;
} SushiHipBatchInfo;

typedef struct SushiHipBatchDiag {
    int32_t flagged;          /* searches with more near-minimum positions than the per-pair / per-search lists hold */
    int32_t all_positions;    /* of those: searches evaluated at every position (a candidate violated its error bound) */
    int64_t tiles_dense;      /* 1024-position tiles evaluated exactly at every position */
    int64_t tiles_sparse;     /* tiles evaluated exactly at listed candidate positions only */
    int64_t candidates;       /* listed candidate positions */
    float max_bound_ratio;    /* max over the exactly evaluated candidates of |f32 score - exact score| / the pair's
                                 modelled error bound (without the delta/2 floor); < 1 or the search went to all_positions */
    float max_bound_ratio_noncandidate; /* the same over the AUDITED positions: per search the audit runs (4 consecutive
                                 positions at a hashed place) of 4 hashed pairs spread over the window -- up to 16 positions that
                                 were NOT selected, evaluated exactly and held to the bound they were ranked with: the error
                                 model checked where it was not already believed.  A violation there sends the search to
                                 all_positions too.  The bound is a statistical model (8 standard deviations of the packed-half
                                 roundings), not a worst-case proof: this field is what watches it. */
    int64_t audited;          /* audited non-candidate positions of the run */
    int64_t pairs_transformed; /* FFT path: block pairs whose inverse transform was run and scored; the other
                                 info.fft_pairs - this were excluded by a lower bound of their scores */
    int64_t excluded_audited; /* of those: pairs the bound HAD excluded, transformed all the same -- per run one hashed pair of every
                                 audited search (all of them by default), a different one every run -- so that the lower bound is held
                                 to what such a pair really scores, not only to the pairs it let through */
    float max_slb_ratio_excluded; /* max over the audited excluded pairs of (the pair's lower bound) / (an upper bound of the exact
                                 score of its best position); < 1 or the search went to all_positions */
    int32_t slb_violations;   /* transformed pairs (audited or not) whose lower bound was found above a real score: 0 */
    int32_t band;             /* form of the exclusion the last run used (its last sub-batch that went through it): 0 whole rows,
                                 1 band-split, -1 none */
    int32_t suspended;        /* 1: AUTO left the exclusion out of the last run -- an earlier run of this batch had excluded next to
                                 nothing (searches without a match anywhere: no bound can help), so the passes that compute the bounds
                                 would only be overhead; every 64th run looks again */
    int32_t band_votes[2];    /* what AUTO / ALWAYS decided the form from (first run of a batch): block pairs looked at (all of them; those of
                                 the first sub-batch where there are several), and those whose
                                 bound -- with nothing but the rows' norms outside the band -- already leaves room to exclude; the
                                 band-split form is taken when that is >= 75 % */
    int64_t second_look_audited; /* of excluded_audited: pairs the FIRST bound had let through and the second look (band-split form:
                                 the low band's samples themselves) then excluded -- a hashed 1/32 of them per run
                                 (1/16 with SUSHI_HIP_AUDIT_EVERY=1, none with 0), other ones every run -- transformed all the same and
                                 held to what they really score, like the others */
} SushiHipBatchDiag;

typedef struct SushiHipBatch SushiHipBatch;

/* Bytes of device memory a batch of these requests needs: descriptors, schedules, result keys and a workspace of
 * at most workspace_cap_bytes (0 = as much as one sub-batch for all requests needs; the minimum is what the most
 * demanding single request needs -- the batch is cut into sub-batches that fit).  variant: -1 = choose. */
SUSHI_HIP_API size_t sushi_hip_batch_bytes(const SushiHipRequest* req_host, int n, int path, int variant,
                                           size_t workspace_cap_bytes);
/* dst: the stream find_substream is called on (searchable for the FFT path); src: the stream the patterns are slices
 * of (may be dst itself); same dtype.  Requests must lie inside their streams (EINVAL otherwise: the reference gets a
 * cv2.error for a pattern longer than the window).  mem_dev: 256-byte aligned, >= sushi_hip_batch_bytes(...) with the
 * same arguments.  The handle keeps pointers to dst and src: destroy it before them. */
SUSHI_HIP_API int sushi_hip_batch_create(const SushiHipStream* dst, const SushiHipStream* src,
                                         const SushiHipRequest* req_host, int n, int path, int variant,
                                         size_t workspace_cap_bytes, void* mem_dev, size_t mem_bytes,
                                         void* hip_stream, SushiHipBatch** out);
/* The same handle for OTHER requests (equally many, same streams, path and settings): descriptors, plan and schedule are redone
 * in place and uploaded in one copy -- what a caller that issues one small batch after another (sushi.calculate_shifts: one
 * find_substream call at a time, sushi.py:432,450-452) does instead of destroy + create.  ENOSPACE if the new requests need more
 * than the memory the batch was created in (the handle is then unchanged and still runs its old requests); so is it after EINVAL,
 * and after an ELAUNCH from the wait for the previous upload.  Only the new plan's own upload comes after the point of no return:
 * if the HIP runtime rejects that copy (ELAUNCH), the handle holds a plan the device has not got -- every run entry point returns
 * EINVAL until a sushi_hip_batch_reset succeeds.  A run still in flight on another stream than `hip_stream` must have finished.
 * What the batch had learnt about its searches (exclusion form, suspension) is reset. */
SUSHI_HIP_API int sushi_hip_batch_reset(SushiHipBatch* batch, const SushiHipRequest* req_host, int n, void* hip_stream);
SUSHI_HIP_API int sushi_hip_batch_info(const SushiHipBatch* batch, SushiHipBatchInfo* info);
/* Matching method of the following runs (default after create: SUSHI_HIP_METHOD_SQDIFF_NORMED).
 * SUSHI_HIP_METHOD_CCOEFF_NORMED: out_idx = first index of the MAXIMUM of cv2.matchTemplate(..., TM_CCOEFF_NORMED),
 * out_score = that float32. */
SUSHI_HIP_API int sushi_hip_batch_set_method(SushiHipBatch* batch, int method);
/* FFT path: whether block pairs are excluded by a lower bound of their scores before they are transformed.
 * Results are the same either way; what differs is time.  AUTO (default after create): a sub-batch uses the exclusion when it has
 * enough pairs for the bound pass and its extra launches to pay (more than 3000 + 2 x its searches: one find_substream call
 * over a small window is a dozen pairs and a dozen launches -- 0.17 ms without, 0.23 with); ALWAYS / NEVER: for tests and measurements. */
#define SUSHI_HIP_EXCLUDE_AUTO 0
#define SUSHI_HIP_EXCLUDE_ALWAYS 1
#define SUSHI_HIP_EXCLUDE_NEVER 2
/* The exclusion has two forms with the same results.  WHOLE: the bound is taken from the products of whole spectra (every pair's
 * 64 KB row written and read back once).  BAND: only the low band (|f| < N/8, a quarter of the bins) is multiplied, stored and
 * transformed; what the other bins can add is bounded from the norms of the rows that meet (Cauchy-Schwarz), and whole rows are
 * formed only for the few pairs that are transformed after all.  BAND needs streams that keep most of their energy in the band
 * (audio does): AUTO and ALWAYS decide per batch, from the streams' own norms, which form to use; these two force one. */
#define SUSHI_HIP_EXCLUDE_BAND 3
#define SUSHI_HIP_EXCLUDE_WHOLE 4
SUSHI_HIP_API int sushi_hip_batch_set_exclusion(SushiHipBatch* batch, int mode);
/* How the roundings of the stored spectra and products (packed halves) enter the LOWER BOUND by which a block pair is excluded
 * without being transformed.  WORST_CASE (default after create): every rounding at its largest, all of them in phase -- triangle
 * inequality over the bins, Cauchy-Schwarz, a proven error bound of the float32 transforms; no independence is assumed, so a
 * pair is excluded only if NO position of it can reach the search's minimum.  STATISTICAL: round 5's model (8
 * standard deviations of independent roundings), kept for A/B measurements.  Results are the same either way wherever the
 * model holds; what differs is how many pairs are left to transform. */
#define SUSHI_HIP_BOUND_WORST_CASE 0
#define SUSHI_HIP_BOUND_STATISTICAL 1
SUSHI_HIP_API int sushi_hip_batch_set_bound_model(SushiHipBatch* batch, int model);
/* Multi-GPU callers: every following run ALSO writes its results as n 8-byte records (int32 index, float32 score bits) to
 * out_packed_dev (8-byte aligned, n records; NULL = off) -- the block a rank contributes to the one all-gather of the path, written
 * by the kernel that writes out_idx / out_score instead of by two copies afterwards. */
SUSHI_HIP_API int sushi_hip_batch_set_packed_output(SushiHipBatch* batch, int32_t* out_packed_dev);
/* The answer as soon as it exists (FFT path; v13).  early: n 16-byte records {int32 index, float32 score bits, int32 ready, int32
 * flagged} in memory BOTH sides can touch -- pinned host memory mapped to the device (16-byte aligned; NULL = off).  The kernel that
 * finishes a search from its candidate lists (refine_kernel) writes the search's record with ONE 16-byte store: ready = 1 and either
 * the final (index, score bits) -- the very values out_idx / out_score receive -- or flagged = 1: the search goes on to the tile stage
 * and its answer is in out_idx / out_score when the run's stream has drained.  A caller that sets ready = 0 in every record before a
 * run can poll the records instead of synchronising the stream: a drop-in find_substream call then does not wait for the three
 * launches behind refine_kernel (collection pass, exact tiles, unpack), which find nothing to do for it (~30 of ~140 us a call).
 * The direct path writes no early records. */
SUSHI_HIP_API int sushi_hip_batch_set_early_output(SushiHipBatch* batch, int32_t* early);
/* One pass of the hot path over the batch.  Asynchronous, with ONE exception: the first run of a batch (and the first after its
 * method changed) that goes through the pair exclusion in AUTO or ALWAYS mode reads 8 bytes back to decide the exclusion's form and
 * synchronises `hip_stream` once for that (not capturable in a hipGraph; BAND, WHOLE and NEVER never synchronise, nor does a
 * batch too small for AUTO to use the exclusion -- a drop-in find_substream call).  Environment variables are read when a batch is
 * created, never here.  A batch on lanes (SushiHipBatchInfo.lanes > 1) launches its sub-batches on streams of the library's own between the
 * run's first launch and its last on `hip_stream`: what is ordered behind the run on `hip_stream` is ordered behind all of it.  The
 * first run of such a batch that forms whole rows for every pair (whole-row form, no exclusion) builds the plan's one-sub-batch
 * cut on the host first (milliseconds, once).
 *   out_idx_dev[n]   = result.argmin(axis=1)[0]        (wav.py:186)
 *   out_score_dev[n] = result[0][min_idx], float32     (wav.py:188)
 * delta (FFT path; > 0, <= 1): floor of the score margin inside which positions are re-evaluated exactly -- every
 * position whose f32 FFT score minus its error bound is not above the smallest (score plus bound) of the search.
 * The bound of a pair is max(delta / 2, modelled f32 error); 2e-5 is the default of the Python layer. */
SUSHI_HIP_API int sushi_hip_batch_run(SushiHipBatch* batch, double delta, int32_t* out_idx_dev, float* out_score_dev,
                                      void* hip_stream);
/* What the last run did (FFT path).  Waits for that run.  ranking_err_host (n floats or NULL): |f32 FFT score - exact
 * score| at every request's result position (0 where a tile kernel found it); flagged_host (n int32 or NULL): 0 = the
 * candidate list sufficed, 1 = tiles, 2 = every position. */
SUSHI_HIP_API int sushi_hip_batch_diagnostics(SushiHipBatch* batch, SushiHipBatchDiag* diag, float* ranking_err_host,
                                              int32_t* flagged_host);
/* FFT path, after a run: the lower bound of the scores of every block pair of the LAST sub-batch (slb_host[pairs]; -inf = no
 * bound) and what it was put together from (acc_host[pairs][2], in the units of the stored products.  Whole-row form: the bound of
 * the cross term's magnitude, the largest row energy of a wave; band-split form: the SIGNED upper bound of the low band's part of the
 * cross term -- sqrt(2) and bin 0 in it --, the low row's energy; the energies only under SUSHI_HIP_BOUND_STATISTICAL, whose term they
 * feed: the worst-case bound does not form them) -- for tests and tools that look at how sharp the exclusion is.  *n_pairs
 * in: the capacity of the arrays, out: how many pairs there are.  Synchronises. */
SUSHI_HIP_API int sushi_hip_batch_pair_bounds(SushiHipBatch* batch, float* slb_host, float* acc_host, int64_t* n_pairs);
/* FFT path, for the tests of the bound pass: after a run that went through the pair exclusion, launch the LAST sub-batch's bound
 * pass once more on what the run left in the workspace -- the same accumulators, norms and tables, bit for bit, whichever route is
 * asked for, which two runs do not have (several of those are float atomic sums) -- and return every pair's bound.  by_wave: 0 four
 * pairs a wave where the patterns allow it (the default route), 1 a wave a pair (SUSHI_HIP_SLB=wave).  pass: 0 slb_kernel over
 * every pair; 1 slb_list_kernel over the list the second look left (band-split form only; EINVAL otherwise); 2 slb_kernel in
 * prediction mode, votes_host[2] = pairs looked at, pairs whose bound leaves room.  Overwrites the stored bounds (a following run
 * makes them again).  *n_pairs in: the capacity of slb_host (NULL: not wanted), out: the pairs; 0 where no run left a bound pass.
 * Synchronises. */
SUSHI_HIP_API int sushi_hip_batch_bounds_again(SushiHipBatch* batch, int by_wave, int pass, float* slb_host, int32_t* votes_host,
                                               int64_t* n_pairs);
/* FFT path, after a run, for tests and tools: where the LAST sub-batch's pattern spectra and products live in the batch's workspace
 * (packed halves, 4 bytes per bin, bin f of a whole row at sushi_hip_fft_slot_of_bin(f), of a low row at
 * sushi_hip_fft_low_slot_of_bin(f)): TSPEC [segments][N], Y [block pairs][N] -- whole rows exist only for the pairs that were
 * transformed --, TSPEC_LOW [segments][N/4], Y_LOW [block pairs][N/4] (band-split form only).  Synchronises; the memory is the
 * caller's own batch buffer, valid until the next run.
 * The real route of the pattern transform (the default; SUSHI_HIP_TSPEC) STORES half rows: TSPEC is then a whole-row copy made on
 * request, in a buffer the batch allocates at the first request and frees with itself (ENOMEM: it could not), valid until the next
 * request or run; TSPEC_HALF is what is stored, [segments][N/2 + 64] words -- the entries whose index has bit 4 clear, in order, then
 * a run of sixteen entries whose first two are the conj-reversals of row 0's entries 3 and 2.  EINVAL under SUSHI_HIP_TSPEC=complex,
 * whose rows are stored whole. */
#define SUSHI_HIP_WS_TSPEC 0
#define SUSHI_HIP_WS_Y 1
#define SUSHI_HIP_WS_TSPEC_LOW 2
#define SUSHI_HIP_WS_Y_LOW 3
#define SUSHI_HIP_WS_TNORM_REST 4   /* float32 per pattern segment: the SQUARED norm of its stored halves outside the band */
#define SUSHI_HIP_WS_TSPEC_HALF 5
/* ... and what the pair exclusion left of the LAST sub-batch, for the tests of its passes: SLIST [block pairs] int32, the pairs the
 * first bound left (indices inside the sub-batch, in no fixed order; an argmin run in the band-split form writes its survivors'
 * work items over it unless SUSHI_HIP_REST_ROWS=search); SLIST2 the same behind the second look (band-split form); SCOUNT the
 * sub-batch's eight int32 count words, [0] the entries of SLIST and [5] those of SLIST2; MARKS [block pairs] bytes, bit 0 the pair
 * is audited, bit 1 it is listed, bit 2 by the second look's audit; PAIR_LB [block pairs] float32, +inf for an excluded pair. */
#define SUSHI_HIP_WS_SLIST 6
#define SUSHI_HIP_WS_SLIST2 7
#define SUSHI_HIP_WS_SCOUNT 8
#define SUSHI_HIP_WS_MARKS 9
#define SUSHI_HIP_WS_PAIR_LB 10
SUSHI_HIP_API int sushi_hip_batch_workspace_view(SushiHipBatch* batch, int which, void** ptr_dev, size_t* bytes);
SUSHI_HIP_API void sushi_hip_batch_destroy(SushiHipBatch* batch);

/* ---- threshold runs: every position that passes a threshold (13, additive) ----------------------------------
 * What np.where(result >= t) answers on cv2.matchTemplate's result row: all occurrences of a pattern in its window, not only the
 * best one.  FFT path only.  For request k of the batch (same requests, streams and method as sushi_hip_batch_run), every index p
 * in [0, n_pos) whose score passes `threshold`:
 *   SUSHI_HIP_METHOD_SQDIFF_NORMED  score(p) <= threshold;
 *   SUSHI_HIP_METHOD_CCOEFF_NORMED  score(p) >= threshold   (the coefficient itself, as sushi_hip_match_curves returns it).
 * out_hits_dev[k * capacity + j], j < min(count, capacity): the hits of request k in ascending index order, each with its float32
 * score -- bit-identical to sushi_hip_match_curves at that position; the slots behind them are not written.  out_counts_dev[k]:
 * how many hits request k has, also when that exceeds `capacity` (then only the first `capacity` by index are written; capacity 0
 * counts only).  The output depends on nothing but the requests, the method and the threshold: not on sub-batches, lanes, the
 * exclusion's mode or form, or earlier runs.
 * Completeness rests on the pair exclusion's WORST_CASE bound alone (the default): a block pair is skipped only if
 * no exact score in it can pass; every other pair is evaluated exactly at every position.  SUSHI_HIP_EXCLUDE_NEVER evaluates every
 * pair.  An audited excluded pair (the audit of sushi_hip_batch_run) that is found to hold a hit, or a score below its bound, is a
 * bound violation (slb_violations): every pair of that search is then evaluated in the same run.
 * EINVAL before any HIP call: NULL batch or outputs, capacity < 0, a threshold that is not finite, a direct-path batch; EALIGN:
 * out_hits_dev not 4-byte or out_counts_dev not 8-byte aligned.  Synchronisation as for sushi_hip_batch_run: asynchronous, except
 * that a threshold run may take the batch's one decision of the exclusion's form (one 8-byte read-back, once per batch and method)
 * if no run has taken it yet.  No device memory besides the batch's own (sushi_hip_batch_bytes is what it was).  Afterwards
 * sushi_hip_batch_diagnostics reports pairs_transformed (pairs evaluated exactly), excluded_audited, max_slb_ratio_excluded,
 * slb_violations and band as for a run, and 0 in every other field.  Neither the early nor the packed records are written, and
 * what AUTO has learnt from the batch's runs is not changed. */
typedef struct SushiHipHit {
    int32_t index;            /* position in the request's result row */
    float score;              /* its float32 score */
} SushiHipHit;                /* 8 bytes */
/* FFT path.  out_hits_dev: [n][capacity] hits; out_counts_dev: [n] int64. */
SUSHI_HIP_API int sushi_hip_batch_run_threshold(SushiHipBatch* batch, double threshold, int32_t capacity,
                                                SushiHipHit* out_hits_dev, int64_t* out_counts_dev, void* hip_stream);

/* ---- the K best distinct matches of every search -----------------------------------------
 * Is the best match the only one, and if not, where are the others, best first?  FFT path only.  For request k of the batch with
 * curve c (sushi_hip_match_curves of that request, same method), separation S >= 1 and K in 1 .. SUSHI_HIP_BEST_MAX_K, the first K
 * picks of greedy suppression over the whole score row:
 *   eligible positions: all of [0, n_pos), or with a threshold only those that pass it, compared as sushi_hip_batch_run_threshold
 *   compares (c[p] <= *threshold for SQDIFF_NORMED, c[p] >= *threshold for CCOEFF_NORMED);
 *   pick j = 1, 2, ...: among the eligible positions at least S away from every earlier pick (|p - g_i| >= S), the best float32
 *   score VALUE (lowest for SQDIFF_NORMED, highest for CCOEFF_NORMED: the score itself, not 1 - score; -0.0 and 0.0 are one
 *   value), ties by the lower index; the picks end after K of them or when no position is left.
 * out_hits_dev[k * K + j], j < out_counts_dev[k]: pick j + 1 of request k (best first), its score bit-identical to c[index];
 * out_counts_dev[k]: picks made (<= K); the slots behind them are not written.  min_separation 0 means each request's own tmpl_len
 * (occurrences that do not overlap).  The output depends on the requests, the method, K, S and the threshold only: not on
 * sub-batches, lanes, the exclusion's mode or form, or earlier runs.  With K = 1 and no threshold, index and score bits are
 * sushi_hip_batch_run's.
 * Exactness rests on the pair exclusion's WORST_CASE bound alone: a block pair is left unevaluated only if its bound is above the
 * score, in ranking units rounded up to a float, of the K-th pick made from the evaluated pairs (or above the threshold); that is
 * checked again whenever more pairs have been evaluated, since the K-th pick's score is not monotone in the evaluated set.
 * SUSHI_HIP_EXCLUDE_NEVER evaluates every pair.  An audited excluded pair is evaluated all the same; one that holds a position as
 * good as its search's K-th pick, or a score below its bound, is a bound violation (slb_violations): every pair of that search is
 * then evaluated in the same run.
 * K beyond the number of real occurrences makes the K-th pick a chance-level score that no bound excludes much under: the run then
 * evaluates most of the window exactly.  Callers who want a runner-up "if there is one" pass a threshold.
 * EINVAL before any HIP call: NULL batch or outputs, k < 1 or > SUSHI_HIP_BEST_MAX_K, min_separation < 0, a *threshold that is not
 * finite, a direct-path batch; EALIGN: an output that is not 4-byte aligned.  Synchronisation, device memory, diagnostics, early and
 * packed records, what AUTO has learnt: as for sushi_hip_batch_run_threshold; flagged_host[k] of sushi_hip_batch_diagnostics is the
 * last round that evaluated a pair of request k (1: the first pairs, 2 and 3: the rounds behind them, 4: the last stage, which
 * evaluates every pair of a request still unsettled and the audit's; 0 under SUSHI_HIP_EXCLUDE_NEVER). */
#define SUSHI_HIP_BEST_MAX_K 32
/* FFT path.  threshold: NULL = none.  out_hits_dev: [n][k] picks; out_counts_dev: [n] int32. */
SUSHI_HIP_API int sushi_hip_batch_run_best(SushiHipBatch* batch, int32_t k, int32_t min_separation, const double* threshold,
                                           SushiHipHit* out_hits_dev, int32_t* out_counts_dev, void* hip_stream);

/* FFT path geometry of one request: block pairs (inverse transforms) and pattern segments (forward transforms). */
SUSHI_HIP_API int sushi_hip_fft_layout(int64_t win_start, int32_t n_pos, int32_t tmpl_len,
                                       int32_t* n_pairs, int32_t* n_seg);

/* ---- whole score curves (DESIGN.md "Curves") -------------------------------------------------------------
 * The row cv2.matchTemplate returns (wav.py:185 `result`), not only its extremum.  A request is a SushiHipRequest with the
 * meaning and validation of sushi_hip_batch_create; the curve of request k is its n_pos float32 values
 * cv2.matchTemplate(search_source, pattern, method)[0]:
 *   SUSHI_HIP_METHOD_SQDIFF_NORMED  the TM_SQDIFF_NORMED value;
 *   SUSHI_HIP_METHOD_CCOEFF_NORMED  the TM_CCOEFF_NORMED value itself (not the 1 - value the ranking minimises): a flat pattern
 *                                   gives 1, a window cv2 takes for flat 0.
 * Every value is bit-identical to what the exact stages of sushi_hip_batch_run produce for that position: curve[out_idx] ==
 * out_score, the first arg-min (arg-max for CCOEFF) of a curve is the batch's out_idx, and uint8 curves equal cv2's direct
 * (non-FFT) evaluation.  Request k's curve starts at out_dev + off_k, off_k = sum of n_pos of the requests before it (a
 * 64-bit count).  Only the samples and the float64 prefix sums are read: dst and src need not be searchable, and no batch
 * handle is involved. */
/* workspace a curve call needs (request table, tile queue); 0 for n <= 0 */
SUSHI_HIP_API size_t sushi_hip_curve_bytes(const SushiHipRequest* req_host, int n);
/* out_dev[off_k + p] = result row of request k (contract above); dst/src need not be searchable; same dtype;
 * mem_dev 256-byte aligned, >= sushi_hip_curve_bytes; out_dev 4-byte aligned, >= sum of n_pos floats.
 * EINVAL / EALIGN / ENOSPACE checked before any HIP call; asynchronous; stateless (any thread, own workspace). */
SUSHI_HIP_API int sushi_hip_match_curves(const SushiHipStream* dst, const SushiHipStream* src,
                                         const SushiHipRequest* req_host, int n, int method,
                                         void* mem_dev, size_t mem_bytes, float* out_dev, void* hip_stream);

/* ---- retiming: a stream read at another speed (13, additive) -----------------------------------
 * A source that plays faster or slower than the destination (PAL / NTSC: 25/24, 1001/960, 1001/1000 and their inverses) is put on
 * the destination's clock by reading it at a rational step: linear interpolation, in an arithmetic stated to the bit.  A segment
 * reads in_dev[in_start ...] at `num / den` input samples per output sample and writes out_len outputs from out_dev[out_off] on.
 * Output i of a segment, 0 <= i < out_len:
 *     t = i * num                          (int64)
 *     j = in_start + t / den,  r = t % den,  j1 = min(j + 1, n_in - 1)
 *     w = (double)r / (double)den
 *     y = x[j] + w * (x[j1] - x[j])        (x[.] converted to double; the product and the sum round separately, no fused multiply-add)
 *     SUSHI_HIP_F32: out = (float)y        SUSHI_HIP_U8: out = (uint8_t)(y + 0.5)
 * so a NumPy float64 restatement equals the result bit for bit, and a step of 1 / 1 copies (uint8: always; float32: every finite
 * sample but -0.0, which y = x + 0 * 0 turns into 0.0).  in_dev / out_dev: n_in / n_out samples of `dtype`, naturally aligned,
 * not overlapping.  Output ranges of different segments that overlap are the caller's business: which segment's value such a
 * sample ends with is not defined.  Samples of out_dev outside every segment are not written. */
typedef struct SushiHipRetimeSegment {
    int64_t in_start;   /* first input sample read */
    int64_t out_off;    /* where the segment's outputs go in out_dev */
    int64_t out_len;    /* outputs of this segment */
    int32_t num, den;   /* input samples advanced per output sample = num / den */
} SushiHipRetimeSegment;    /* 32 bytes */
/* workspace a retime call needs (the segment table); 0 for n_seg <= 0 */
SUSHI_HIP_API size_t sushi_hip_retime_bytes(int n_seg);
/* One launch for the whole table (many short segments, or one of 10^8 samples).  No device allocation: the table is uploaded
 * into mem_dev (256-byte aligned, >= sushi_hip_retime_bytes(n_seg)).  Asynchronous; stateless (any thread, own workspace).
 * Checked before any HIP call -- EINVAL: a null pointer, an unknown dtype, n_seg < 1, n_in < 1, n_out < 1; a segment with num or
 * den outside [1, 2^20], num / den outside [1/8, 8], out_len < 1 or >= 2^40, in_start < 0, a last read
 * in_start + ((out_len - 1) * num) / den beyond n_in - 1, or outputs outside [0, n_out); EALIGN: mem_dev not 256-byte aligned
 * (in_dev / out_dev not aligned to their sample type); ENOSPACE: mem_bytes too small. */
SUSHI_HIP_API int sushi_hip_retime(const void* in_dev, int dtype, int64_t n_in,
                                   const SushiHipRetimeSegment* seg_host, int n_seg,
                                   void* out_dev, int64_t n_out,
                                   void* mem_dev, size_t mem_bytes, void* hip_stream);

/* ---- loudness contour: a row's mean absolute deviation, decimated (13, additive) --------------
 * Two releases of one programme whose waveforms differ -- inverted polarity, a speed change with the pitch kept, another carrier
 * under the same contour -- still share their loudness contour.  This call turns a row into that contour at 1 / hop of its rate,
 * in an arithmetic stated to the bit.  hop h in [1, 256], span m in [1, 64], W = h * m <= 4096, a = (m - 1) / 2 (integer
 * division), c = sushi_hip_centre(dtype).  For a block index b, which may be negative,
 *     B_b = sum over t = 0 .. h - 1, in that order, of |x[clamp(in_start + b * h + t, 0, n_in - 1)] - c|
 * and output i, 0 <= i < out_len, is
 *     E_i = B_{i-a} + B_{i-a+1} + ... + B_{i-a+m-1}, summed in that order
 *     SUSHI_HIP_U8:  everything in integers (E <= 524288);  out = min(255, (4 * E + W) / (2 * W))    (2 E / W rounded half up)
 *     SUSHI_HIP_F32: d = fabs((double)x - 0.5); B and E are float64 running sums from 0.0, every addition rounded once (no fused
 *                    multiply-add, no pairwise sum);  out = (float)((E + E) / (double)W)
 * so a NumPy restatement equals the result bit for bit; there is no square root and no logarithm.  Output i covers the input
 * samples in_start + (i - a) * h .. in_start + (i - a + m) * h - 1; reads outside the row see its edge samples.
 * in_dev / out_dev: n_in / out_len samples of `dtype`, naturally aligned, not overlapping.  One launch, no workspace, no device
 * allocation.  Asynchronous; stateless (any thread).  Checked before any HIP call -- EINVAL: a null pointer, an unknown dtype,
 * n_in < 1 (or >= 2^62), out_len < 1 or >= 2^40, in_start outside [0, n_in - 1], hop outside [1, 256], span outside [1, 64],
 * hop * span > 4096; EALIGN: in_dev / out_dev not aligned to their sample type. */
SUSHI_HIP_API int sushi_hip_envelope(const void* in_dev, int dtype, int64_t n_in, int64_t in_start,
                                     int32_t hop, int32_t span, void* out_dev, int64_t out_len, void* hip_stream);

/* ---- FIR filter: a row with a band removed, at its own rate (13, additive) --------------------
 * Mains hum, DC wander, rumble or a dub's own speech correlate with themselves and hide what two streams share.  This call
 * correlates a row with T float64 taps in an arithmetic stated to the bit.  T odd in [1, 2047], a = (T - 1) / 2,
 * c = sushi_hip_centre(dtype), d(g) = (double)x[clamp(g, 0, n_in - 1)] - c (SUSHI_HIP_F32: one float64 subtraction;
 * SUSHI_HIP_U8: exact).  Output i, 0 <= i < out_len:
 *     acc = 0.0
 *     p = taps[k] * d(in_start + i + k - a);  acc = acc + p      for k = 0 .. T - 1, in that order (the product and the sum round
 *                                                                separately: no fused multiply-add, no pairwise sum)
 *     SUSHI_HIP_F32: out = (float)(acc + 0.5)
 *     SUSHI_HIP_U8:  v = floor(acc + 128.5);  out = v >= 255 ? 255 : (v >= 0 ? v : 0)      (a NaN gives 0)
 * so a NumPy float64 restatement equals the result bit for bit.  Correlation orientation: taps[0] meets the sample a places in
 * front of the output; reads outside the row see its edge samples.  Taps are not checked for being finite.
 * in_dev / out_dev: n_in / out_len samples of `dtype`, naturally aligned, not overlapping; taps_dev: T doubles in device memory.
 * One launch, no workspace, no device allocation.  Asynchronous; stateless (any thread).  Checked before any HIP call -- EINVAL: a
 * null pointer, an unknown dtype, n_in < 1 (or >= 2^62), in_start outside [0, n_in - 1], out_len < 1 or >= 2^40, n_taps even or
 * outside [1, 2047]; EALIGN: in_dev / out_dev not aligned to their sample type, taps_dev not to 8 bytes. */
SUSHI_HIP_API int sushi_hip_filter(const void* in_dev, int dtype, int64_t n_in, int64_t in_start,
                                   const double* taps_dev, int32_t n_taps, void* out_dev, int64_t out_len, void* hip_stream);

/* ---- levelling: a row divided by its local level, at its own rate (13, additive) ---------------
 * A normalised score weights each instant by its energy.  Two mono dubs share the music-and-effects bed and carry a louder speech
 * of their own: the unrelated speech decides the score, and the bed in the pauses between words counts for nothing; a capture
 * through an AGC or a broadcast compressor loses the same.  This call divides every sample's deviation by the mean absolute
 * deviation over W samples around it, in an arithmetic stated to the bit, so that the pauses count as much as the words.
 * W = window, odd in [1, 1023]; h = (W - 1) / 2; c = sushi_hip_centre(dtype); H the type's half range (SUSHI_HIP_U8: 128.0;
 * SUSHI_HIP_F32: 0.5); d(j) = x[clamp(j, 0, n_in - 1)] - c (SUSHI_HIP_U8: an integer; SUSHI_HIP_F32: one float64 subtraction).
 * Output i, 0 <= i < out_len, with g = in_start + i:
 *     E   = |d(g - h)| + |d(g - h + 1)| + ... + |d(g - h + W - 1)|
 *           SUSHI_HIP_U8:  an exact integer (at most 128 * 1023), whichever way it is summed
 *           SUSHI_HIP_F32: a float64 running sum from 0.0 in that order, every addition rounded once (no pairwise sum, no sliding
 *                          update)
 *     fw  = (floor * H) * (double)W                     two float64 multiplications, in that order
 *     den = ((double)E + fw) * peak
 *     q   = ((double)d(g) * (double)W) / den            one product, one division; a NaN q becomes 0; then q is held to [-1, 1]
 *     SUSHI_HIP_F32: out = (float)(0.5 + 0.5 * q)
 *     SUSHI_HIP_U8:  out = min(255, (int)floor(q * 128.0 + 128.5))
 * so a NumPy restatement equals the result bit for bit.  floor, a fraction of the half range, keeps digital silence at the centre
 * and quantisation noise from being blown up to full scale (1.0 / 128: one step of a uint8 stream); the local level times peak
 * maps to full scale (8.0 leaves the clamp to a few samples in a million of programme material).  Reads outside the row see its edge samples.
 * in_dev / out_dev: n_in / out_len samples of `dtype`, naturally aligned, not overlapping.  One launch, no workspace, no device
 * allocation.  Asynchronous; stateless (any thread).  Checked before any HIP call -- EINVAL: a null pointer, an unknown dtype,
 * n_in < 1 (or >= 2^62), in_start outside [0, n_in - 1], out_len < 1 or >= 2^40, window even or outside [1, 1023], floor or peak
 * not finite or not > 0; EALIGN: in_dev / out_dev not aligned to their sample type. */
SUSHI_HIP_API int sushi_hip_level(const void* in_dev, int dtype, int64_t n_in, int64_t in_start,
                                  int32_t window, double floor, double peak, void* out_dev, int64_t out_len, void* hip_stream);

/* ---- joint search: the one shift a group of score rows shares (13, additive) -----------------
 * Events of one scene share one shift, and a lone search of a short or repeated pattern may prefer a decoy in its window.  The
 * rows of a group are therefore put on one shift axis and reduced together.  A group is m >= 1 rows; a row is n_shift consecutive
 * float32 values of a sushi_hip_match_curves output (all rows of a call by the same method), starting at a curve_off of its own,
 * with a float64 weight w_i, finite and >= 0.  Joint index j in [0, n_shift) addresses element j of every row R_i.  In row order:
 *     acc = 0.0
 *     acc = acc + w_i * (double)R_i[j]     for i = 0 .. m - 1 (the product and the sum round separately, no fused multiply-add)
 *     joint[j] = (float)acc
 * so a NumPy float64 restatement equals the result bit for bit.  The group's answer is the FIRST index of the minimum of joint
 * (SUSHI_HIP_METHOD_SQDIFF_NORMED) or of its maximum (SUSHI_HIP_METHOD_CCOEFF_NORMED; 0.0 and -0.0 tie, as in NumPy), and that
 * float32 value.  Per row the same pass returns R_i[answer] -- each row's own score at the joint index -- and the row's own first
 * extremum over [0, n_shift), as index and value: what a lone search over that range returns.  Row values are assumed finite, and
 * under SQDIFF_NORMED not negative (-0.0 included), as curves are; with a NaN the results are unspecified, but no access leaves
 * the buffers. */
typedef struct SushiHipJointRow {
    int64_t curve_off;  /* first float of the row in curves_dev */
    double weight;      /* finite, >= 0 */
} SushiHipJointRow;         /* 16 bytes */
typedef struct SushiHipJointGroup {
    int32_t first_row;  /* the groups tile the rows in order: the sum of n_rows of the groups before this one */
    int32_t n_rows;     /* m >= 1 */
    int32_t n_shift;    /* >= 1 */
    int32_t reserved;
} SushiHipJointGroup;       /* 16 bytes */
/* workspace a joint call needs (both tables, the extremum keys); 0 for n_groups < 1 or n_rows < n_groups */
SUSHI_HIP_API size_t sushi_hip_joint_bytes(int n_groups, int n_rows);
/* out_idx_dev / out_score_dev: [n_groups] the answers; out_row_score_dev: [n_rows] R_i[answer of its group]; out_row_idx_dev /
 * out_row_best_dev: [n_rows] every row's own first extremum; out_joint_dev: NULL, or the joint rows back to back (group g's starts
 * at the sum of n_shift of the groups before it).  No device allocation: one upload of the tables into mem_dev (256-byte aligned,
 * >= sushi_hip_joint_bytes), then two launches (the reduce; the gather of R_i[answer]).  Asynchronous; stateless (any thread, own
 * workspace).  Checked before any HIP call -- EINVAL: a null pointer (but out_joint_dev), an unknown method, n_groups < 1,
 * n_rows < n_groups, n_curve < 1, groups that do not tile the rows in order, n_shift < 1, curve_off < 0 or curve_off + n_shift >
 * n_curve (decided without forming the sum), a weight that is not finite or is negative; EALIGN: mem_dev not 256-byte aligned, a
 * float / int32 pointer not 4-byte aligned; ENOSPACE: mem_bytes too small. */
SUSHI_HIP_API int sushi_hip_joint_reduce(const float* curves_dev, int64_t n_curve,
                                         const SushiHipJointRow* rows_host, int n_rows,
                                         const SushiHipJointGroup* groups_host, int n_groups, int method,
                                         void* mem_dev, size_t mem_bytes,
                                         int32_t* out_idx_dev, float* out_score_dev,
                                         float* out_row_score_dev, int32_t* out_row_idx_dev, float* out_row_best_dev,
                                         float* out_joint_dev, void* hip_stream);

/* ---- segmentation: where the shift a sequence of score rows shares changes (13, additive) -----------------
 * A joint search needs its groups named.  Here the rows of consecutive events lie on one shift axis in event order, and a shift is
 * chosen per event that minimises the sum of the events' weighted scores plus a fixed price `penalty` for every change of shift
 * between consecutive events (a Potts model: a Viterbi pass of O(events x shifts)).  The groups and their borders are what the
 * backtrack finds.  A sequence is E >= 1 rows R_e; a row is n_shift >= 1 consecutive float32 values of a sushi_hip_match_curves
 * output (all rows by one method) at a curve_off of its own, with a float64 weight w_e, finite and >= 0 (a SushiHipJointRow);
 * penalty is a finite float64 >= 0.  Everything is float64; products and sums round separately (no fused multiply-add):
 *     c_e[j] = (double)R_e[j] (SQDIFF_NORMED) or -(double)R_e[j] (CCOEFF_NORMED: an exact negation);  u_e[j] = w_e * c_e[j]
 *     D_0[j] = u_0[j]
 *     m_e = min_j D_e[j], a_e = the FIRST index of it (0.0 and -0.0 tie, as in NumPy)
 *     for e >= 1:  jump_e = m_{e-1} + penalty;  stay_e[j] = (D_{e-1}[j] <= jump_e)  (a tie stays);
 *                  D_e[j] = u_e[j] + (stay_e[j] ? D_{e-1}[j] : jump_e)
 *     backtrack:   s_{E-1} = a_{E-1};  for e = E-1 .. 1:  s_{e-1} = stay_e[s_e] ? s_e : a_{e-1}
 * The total cost is m_{E-1}.  Because floating-point addition is monotone, it equals the minimum over ALL n_shift^E paths of the
 * path's cost accumulated in this order: c = u_0[s_0]; per event c = c + penalty if the shift changed, then c = c + u_e[s_e].
 * Per row the pass also returns the row's own first extremum over the axis (minimum / maximum by method; 0.0 and -0.0 tie), as
 * index and float32 value with its own bits: what a lone search over that range returns.  Rows are assumed finite; with a NaN the
 * results are unspecified, but no access leaves the buffers (indices are clamped into [0, n_shift)).
 * Stay bits: row e's occupy sushi_hip_path_stay_words(n_shift) = ceil(n_shift / 64) 64-bit words from word e * that on; shift j is
 * bit j % 64 of word j / 64; tail bits and all of row 0's are zero. */
/* workspace of a forward call (two sets of per-workgroup partial minima, used by turns; a row's curve_off and weight travel with
 * its launch, nothing is uploaded); 0 for n_rows < 1 or n_shift < 1 */
SUSHI_HIP_API size_t sushi_hip_path_bytes(int n_rows, int32_t n_shift);
/* 64-bit words of one row's stay bits; 0 for n_shift < 1 */
SUSHI_HIP_API int64_t sushi_hip_path_stay_words(int32_t n_shift);
/* Advances rows row0 .. row0 + n_rows - 1 of a sequence of n_total rows: rows_host[i] is row row0 + i.  The output arrays are the
 * whole sequence's -- D_dev: [n_shift] float64, updated in place; stay_dev: [n_total][words]; row_min_dev (m_e) float64,
 * row_arg_dev (a_e) int32, row_own_index_dev int32, row_own_score_dev float32: [n_total] -- and the call writes rows row0 ..
 * row0 + n_rows - 1 of them.  row0 > 0 continues from D_dev and row_min_dev[row0 - 1] as the call before it on the same stream left
 * them, so a sequence whose curves do not fit in memory at once is streamed through in chunks of events, with the bits of one
 * call.  No device allocation, no upload: one launch per row, stream-ordered, and one that closes the last row.  Asynchronous;
 * stateless (any thread, own workspace and arrays).  Checked before any HIP call -- EINVAL: a null pointer, an unknown method,
 * n_rows < 1, n_shift < 1, n_curve < 1, n_shift > n_curve, n_total < 1, row0 < 0, row0 + n_rows > n_total, curve_off < 0 or
 * curve_off + n_shift > n_curve (decided without forming the sum), a weight or a penalty that is not finite or is negative;
 * EALIGN: mem_dev not 256-byte aligned; ENOSPACE: mem_bytes < sushi_hip_path_bytes; EALIGN: D_dev / stay_dev / row_min_dev not
 * 8-byte aligned, a float / int32 pointer not 4-byte aligned. */
SUSHI_HIP_API int sushi_hip_path_forward(const float* curves_dev, int64_t n_curve,
                                         const SushiHipJointRow* rows_host, int n_rows, int32_t n_shift,
                                         int method, double penalty, int row0, int n_total,
                                         double* D_dev, unsigned long long* stay_dev,
                                         double* row_min_dev, int32_t* row_arg_dev,
                                         int32_t* row_own_index_dev, float* row_own_score_dev,
                                         void* mem_dev, size_t mem_bytes, void* hip_stream);
/* out_shift_dev[e] = s_e for the n_total rows of a sequence whose forward calls lie before it on the stream.  One wave, one lane
 * walking n_total dependent bit reads.  EINVAL: a null pointer, n_total < 1, n_shift < 1; EALIGN: stay_dev not 8-byte aligned, an
 * int32 pointer not 4-byte aligned. */
SUSHI_HIP_API int sushi_hip_path_backtrack(const unsigned long long* stay_dev, const int32_t* row_arg_dev, int n_total,
                                           int32_t n_shift, int32_t* out_shift_dev, void* hip_stream);

/* ---- drift search: score rows summed along a sloped line of shifts (13, additive) -----------------
 * A joint search sums a group's rows at one displacement.  Where source and destination run at slightly different rates the shared
 * shift moves along the programme, and the rows have to be summed along a sloped line instead: row e at k + round(r * (pos_e -
 * anchor)) for a candidate rate r.  The native side does not know rates: it is given E >= 1 rows R_e (SushiHipJointRow: n_shift >= 1
 * consecutive float32 values of a sushi_hip_match_curves output at a curve_off of its own, all by one method, with a float64 weight
 * w_e, finite and >= 0) and a table of int32 offsets o[d][e], [n_drifts][n_rows] row-major, n_drifts in 1 .. 65535: the
 * displacement of row e under candidate d relative to the axis index.  Candidate d is valid on j in [lo_d, hi_d),
 *     lo_d = max(0, max_e(-o[d][e])),  hi_d = n_shift - max(0, max_e o[d][e]),
 * where every row is addressed inside itself.  For a valid j, in row order (joint_accumulate, unchanged):
 *     acc = 0.0
 *     acc = acc + w_e * (double)R_e[j + o[d][e]]     for e = 0 .. E - 1 (the product and the sum round separately, no fused multiply-add)
 *     line[d][j] = (float)acc
 * so a NumPy float64 restatement equals the result bit for bit.  Per candidate the call returns the FIRST index of the minimum
 * (SUSHI_HIP_METHOD_SQDIFF_NORMED) or maximum (SUSHI_HIP_METHOD_CCOEFF_NORMED) of line[d] over its valid range and that float32
 * value.  The answer is the best of those: a tie goes to the first candidate in table order, then to the first j; 0.0 and -0.0 tie,
 * as in NumPy.  Per row it returns R_e[j* + o[d*][e]], the row's own score on the answer's line, read where it lies (-0.0 keeps its
 * bits).  Row values are assumed finite, and under SQDIFF_NORMED not negative (-0.0 included), as curves are; with a NaN the results
 * are unspecified, but no access leaves the buffers. */
/* workspace a drift call needs (the rows, the offset table in blocks of candidates, their valid ranges, the extremum keys); 0 for
 * n_rows < 1 or n_drifts outside 1 .. 65535 */
SUSHI_HIP_API size_t sushi_hip_drift_bytes(int n_rows, int n_drifts);
/* out_best_dev: int32[2], the answer's candidate d* and index j*; out_score_dev: float32[1], line[d*][j*]; out_row_score_dev:
 * [n_rows] R_e[j* + o[d*][e]]; out_drift_idx_dev / out_drift_score_dev: [n_drifts] every candidate's own first extremum over its
 * valid range; out_lines_dev: NULL, or [n_drifts][n_shift] the lines, +inf (SQDIFF_NORMED) / -inf (CCOEFF_NORMED) outside a
 * candidate's valid range.  No device allocation: one upload of the tables into mem_dev (256-byte aligned, >=
 * sushi_hip_drift_bytes), then three launches (the reduce; keys to the per-candidate outputs and the answer's key; the gather of
 * the rows' scores).  Asynchronous; stateless (any thread, own workspace).  Checked before any HIP call -- EINVAL: a null pointer
 * (but out_lines_dev), an unknown method, n_rows < 1, n_drifts outside 1 .. 65535, n_shift < 1, curve_off < 0 or curve_off +
 * n_shift > n_curve (decided without forming the sum), a weight that is not finite or is negative, a candidate whose valid range is
 * empty (hi_d <= lo_d, decided in 64 bits: any |o| >= n_shift is one); EALIGN: mem_dev not 256-byte aligned, a float / int32 device
 * pointer not 4-byte aligned; ENOSPACE: mem_bytes too small. */
SUSHI_HIP_API int sushi_hip_drift_reduce(const float* curves_dev, int64_t n_curve,
                                         const SushiHipJointRow* rows_host, int n_rows, int32_t n_shift,
                                         const int32_t* offsets_host, int n_drifts, int method,
                                         void* mem_dev, size_t mem_bytes,
                                         int32_t* out_best_dev, float* out_score_dev, float* out_row_score_dev,
                                         int32_t* out_drift_idx_dev, float* out_drift_score_dev,
                                         float* out_lines_dev, void* hip_stream);

/* ---- tracking: a shift that wanders from event to event, and may jump (13, additive) -----------------
 * The segmentation pass charges the full `penalty` for every change of shift, however small, and the drift search follows one
 * straight line.  Here the shift may, between consecutive events, either MOVE by at most reach_e samples at step_cost a sample,
 * or JUMP anywhere at `penalty` (a Viterbi pass with bounded moves: O(events x shifts x reach)).  A sequence is E >= 1 rows R_e in
 * event order, as for sushi_hip_path_forward: n_shift >= 1 consecutive float32 values of a sushi_hip_match_curves output (all rows
 * by one method) at a curve_off of its own, with a float64 weight w_e, finite and >= 0 (a SushiHipJointRow).  In addition an
 * int32 reach_e per row, in 0 .. SUSHI_HIP_TRACK_MAX_REACH (row 0's is ignored), and penalty and step_cost, finite float64 >= 0.
 * Everything is float64; products and sums round separately (no fused multiply-add):
 *     u_e[j] = w_e * c_e[j] as in "segmentation";  D_0[j] = u_0[j]
 *     m_e = min_j D_e[j], a_e = the FIRST index of it (0.0 and -0.0 tie)
 *     for e >= 1:  jump_e = m_{e-1} + penalty
 *         the candidates of j are every d with |d| <= reach_e and 0 <= j + d < n_shift:
 *             cand(0) = D_{e-1}[j] itself (nothing is added: -0.0 keeps its bits, and reach 0 is the segmentation pass)
 *             cand(d) = D_{e-1}[j + d] + step_cost * (double)|d|  for d != 0 (the product rounds once, then the sum rounds once)
 *         near_e[j] = the smallest candidate; of equal candidates the one with the smaller |d| wins, and of those the negative d
 *                     (a total order on (value, |d|, d > 0): the result does not depend on the order the candidates meet in)
 *         take_near = (near_e[j] <= jump_e)  (a tie moves);  D_e[j] = u_e[j] + (take_near ? near_e[j] : jump_e)
 *         move_e[j] = the winning d (int16), or SUSHI_HIP_TRACK_JUMP;  row 0's moves are 0
 *     backtrack:   s_{E-1} = a_{E-1};  for e = E-1 .. 1:  s_{e-1} = move_e[s_e] == SUSHI_HIP_TRACK_JUMP ? a_{e-1} : s_e + move_e[s_e]
 * The total cost is m_{E-1}.  Because floating-point addition is monotone, it equals the minimum over ALL n_shift^E paths of the
 * path's cost accumulated in this order: c = u_0[s_0]; per event c = c + step_cost * |d| (a move within reach, d != 0), or c
 * unchanged (d = 0), or c + penalty (a jump, allowed for any pair), whichever allowed choice is cheaper; then c = u_e[s_e] + c.
 * With every reach_e = 0 the pass is sushi_hip_path_forward bit for bit.  Per row the pass also returns the row's own first
 * extremum, as the segmentation pass does.  Rows are assumed finite; with a NaN the results are unspecified, but no access leaves
 * the buffers (indices are clamped into [0, n_shift)). */
#define SUSHI_HIP_TRACK_MAX_REACH 1024
#define SUSHI_HIP_TRACK_JUMP (-32768)
/* workspace of a forward call (two sets of per-workgroup partial minima, used by turns; a row's curve_off, weight and reach travel
 * with its launch, nothing is uploaded); 0 for n_rows < 1 or n_shift < 1 */
SUSHI_HIP_API size_t sushi_hip_track_bytes(int n_rows, int32_t n_shift);
/* Advances rows row0 .. row0 + n_rows - 1 of a sequence of n_total rows: rows_host[i] and reach_host[i] are row row0 + i's.  The
 * output arrays are the whole sequence's -- D_dev: [2][n_shift] float64 in two halves (row e reads half (e - 1) & 1 and writes
 * half e & 1: a row reads its neighbours' costs, so it cannot be updated in place); move_dev: [n_total][n_shift] int16;
 * row_min_dev (m_e) float64, row_arg_dev (a_e) int32, row_own_index_dev int32, row_own_score_dev float32: [n_total] -- and the
 * call writes rows row0 .. row0 + n_rows - 1 of them.  row0 > 0 continues from D_dev and row_min_dev[row0 - 1] as the call before
 * it on the same stream left them: a sequence in chunks has the bits of one call, whether row0 is odd or even.  No device
 * allocation, no upload: one launch per row, stream-ordered, and one that closes the last row.  Asynchronous; stateless (any
 * thread, own workspace and arrays).  Checked before any HIP call -- EINVAL: a null pointer, an unknown method, n_rows < 1,
 * n_shift < 1, n_curve < 1, n_shift > n_curve, n_total < 1, row0 < 0, row0 + n_rows > n_total, curve_off < 0 or curve_off +
 * n_shift > n_curve (decided without forming the sum), a weight, a penalty or a step_cost that is not finite or is negative, a
 * reach outside 0 .. SUSHI_HIP_TRACK_MAX_REACH in any row but the sequence's row 0; EALIGN: mem_dev not 256-byte aligned;
 * ENOSPACE: mem_bytes < sushi_hip_track_bytes; EALIGN: D_dev / row_min_dev not 8-byte aligned, a float / int32 pointer not 4-byte
 * aligned, move_dev not 2-byte aligned. */
SUSHI_HIP_API int sushi_hip_track_forward(const float* curves_dev, int64_t n_curve,
                                          const SushiHipJointRow* rows_host, const int32_t* reach_host, int n_rows, int32_t n_shift,
                                          int method, double penalty, double step_cost, int row0, int n_total,
                                          double* D_dev, int16_t* move_dev,
                                          double* row_min_dev, int32_t* row_arg_dev,
                                          int32_t* row_own_index_dev, float* row_own_score_dev,
                                          void* mem_dev, size_t mem_bytes, void* hip_stream);
/* out_shift_dev[e] = s_e for the n_total rows of a sequence whose forward calls lie before it on the stream.  One wave, one lane
 * walking n_total dependent reads.  EINVAL: a null pointer, n_total < 1, n_shift < 1; EALIGN: move_dev not 2-byte aligned, an
 * int32 pointer not 4-byte aligned. */
SUSHI_HIP_API int sushi_hip_track_backtrack(const int16_t* move_dev, const int32_t* row_arg_dev, int n_total,
                                            int32_t n_shift, int32_t* out_shift_dev, void* hip_stream);

/* ---- margins: how firmly the tracking pass places each event -- its min-marginals (13, additive) --------------
 * For event e and shift j the MIN-MARGINAL M_e[j] is the cost of the best whole path that puts event e at shift j.  The best
 * value of M_e more than guard_e samples away from the chosen shift s_e is the cost of the best alternative explanation that moves
 * this event; its excess over M_e[s_e] is the event's margin, its index where the event would go instead.  The forward half, D_e, is
 * what the tracking pass computes (sushi_hip_track_forward_keep keeps every row of it); the backward half is the same recurrence
 * run from the last event down.  Inputs: those of "tracking" (u_e, reach_e, penalty, step_cost), D_e, the backtrack's s_e, and an
 * int32 guard_e >= 0 per row.  Everything is float64; products and sums round separately:
 *     C_{E-1}[j] = u_{E-1}[j];   M_{E-1}[j] = D_{E-1}[j]            (nothing is added: the bits of D)
 *     for e = E-2 .. 0, with r = reach_{e+1}:
 *         n_{e+1}  = min_j C_{e+1}[j];   jumpB = n_{e+1} + penalty
 *         nearB[j] = the smallest of cand(0) = C_{e+1}[j] itself and cand(d) = C_{e+1}[j + d] + step_cost * (double)|d|,
 *                    0 < |d| <= r, 0 <= j + d < n_shift  (the candidates and the tie rule of "tracking"; only the value is kept)
 *         B_e[j]   = nearB[j] <= jumpB ? nearB[j] : jumpB
 *         M_e[j]   = D_e[j] + B_e[j]   (one rounding);   C_e[j] = u_e[j] + B_e[j]   (one rounding)
 *     per row e:
 *         through_e          = M_e[s_e]
 *         best_e, best_arg_e = the minimum of M_e and its FIRST index (0.0 and -0.0 tie)
 *         alt_e,  alt_arg_e  = the minimum of M_e over { j : |j - s_e| > guard_e } and its first index; (+inf, -1) where that set is
 *                              empty
 *         c_min_e            = n_e  (kept per row so that a later call can continue)
 * Three facts.  EXACT PATH MINIMUM: floating-point addition is monotone, so M_e[j] is bitwise the minimum, over all paths with
 * s_e = j, of (the prefix cost, accumulated forwards as "tracking" states it) + (the suffix cost, accumulated backwards in the
 * mirrored order -- c = u_{E-1}[s_{E-1}]; per event from E-2 down to e + 1 the cheaper allowed choice of a move's price, nothing,
 * or the penalty is added, then c = u_i[s_i] + c -- ending, at event e, before u_e is added).  REVERSAL: n_0 is bitwise the
 * tracking pass's total cost of the reversed sequence, with reach_rev[i] = reach[E - i] for i >= 1.  CONSISTENCY WITH THE TOTAL:
 * best_e <= through_e exactly; through_e equals the total m_{E-1} only up to summation order: |through_e - m_{E-1}| <=
 * 6 E 2^-53 S, S the sum of the absolute values of the optimal path's terms (w_e |R_e[s_e]|, its prices and its penalties) --
 * Higham's bound for two recursive sums of at most 3 E terms each.
 * With every reach 0 this is the same statement about the segmentation model. */
/* sushi_hip_track_forward with D kept: D_all_dev is [n_total][n_shift] float64, row e reads row e - 1 and writes row e.  Everything
 * else -- the kernels, the other outputs, their bits, the refusals, the workspace (sushi_hip_track_bytes) and the continuation of
 * a sequence in chunks -- is sushi_hip_track_forward's. */
SUSHI_HIP_API int sushi_hip_track_forward_keep(const float* curves_dev, int64_t n_curve,
                                               const SushiHipJointRow* rows_host, const int32_t* reach_host, int n_rows, int32_t n_shift,
                                               int method, double penalty, double step_cost, int row0, int n_total,
                                               double* D_all_dev, int16_t* move_dev,
                                               double* row_min_dev, int32_t* row_arg_dev,
                                               int32_t* row_own_index_dev, float* row_own_score_dev,
                                               void* mem_dev, size_t mem_bytes, void* hip_stream);
/* workspace of a margins call (two sets of per-workgroup partial minima, used by turns); 0 for n_rows < 1 or n_shift < 1 */
SUSHI_HIP_API size_t sushi_hip_track_margins_bytes(int n_rows, int32_t n_shift);
/* Walks rows row0 + n_rows - 1 down to row0 of a sequence of n_total rows whose forward_keep calls and backtrack lie before it on
 * the stream.  rows_host[i] and guard_host[i] are row row0 + i's; reach_host[i] is row row0 + i's for i = 0 .. n_rows, the last
 * only where row0 + n_rows < n_total (reach_host[0] is not used and is ignored: the step into row row0 is priced by the call that
 * walks row row0 - 1).  D_all_dev: [n_total][n_shift] as sushi_hip_track_forward_keep left it; shift_dev: [n_total], the
 * backtrack's output; C_dev: [2][n_shift] float64 in two halves (row e reads half (e + 1) & 1 and writes half e & 1).  The outputs
 * are the whole sequence's -- c_min_dev, through_dev, best_dev, alt_dev float64 and best_arg_dev, alt_arg_dev int32: [n_total];
 * M_dev: [n_total][n_shift] float64 or NULL -- and the call writes rows row0 .. row0 + n_rows - 1 of them.  The first call of a
 * sequence has row0 + n_rows == n_total; a later one continues from C_dev and c_min_dev[row0 + n_rows] as the call before it on the
 * same stream left them: a sequence in chunks has the bits of one call, whatever the parity of the boundary.  No device
 * allocation, no upload: one launch per row, stream-ordered, and one that closes row row0.  Asynchronous; stateless.  Checked
 * before any HIP call -- EINVAL: a null pointer (M_dev may be null), an unknown method, n_rows < 1, n_shift < 1, n_curve < 1,
 * n_shift > n_curve, n_total < 1, row0 < 0, row0 + n_rows > n_total (no sum is formed), a row outside the curve buffer, a weight, a
 * penalty or a step_cost that is not finite or is negative, a used reach outside 0 .. SUSHI_HIP_TRACK_MAX_REACH, a guard < 0;
 * EALIGN: mem_dev not 256-byte aligned; ENOSPACE: mem_bytes < sushi_hip_track_margins_bytes; EALIGN: a float64 pointer not 8-byte
 * aligned, a float / int32 pointer not 4-byte aligned. */
SUSHI_HIP_API int sushi_hip_track_margins(const float* curves_dev, int64_t n_curve,
                                          const SushiHipJointRow* rows_host, const int32_t* reach_host, const int32_t* guard_host,
                                          int n_rows, int32_t n_shift, int method, double penalty, double step_cost,
                                          int row0, int n_total,
                                          const double* D_all_dev, const int32_t* shift_dev, double* C_dev, double* c_min_dev,
                                          double* through_dev, double* best_dev, int32_t* best_arg_dev,
                                          double* alt_dev, int32_t* alt_arg_dev, double* M_dev,
                                          void* mem_dev, size_t mem_bytes, void* hip_stream);

/* ---- ordered tracking: tracked events kept in order -- one-sided jumps, a penalty per event (13, additive) -------
 * "tracking" lets a jump go anywhere at one fixed penalty.  But no cut puts an event in the destination before the end of the event
 * in front of it: inserted material raises the shift by any amount, removed material lowers it by at most what lay between the two
 * events.  And a caller may know where a cut is cheap (a chapter mark, a long silence) and where it is dear.  So here a jump into
 * row e may lower the shift index by at most back_e (int32 >= 0, or SUSHI_HIP_TRACK_BACK_ANY: no limit), and costs penalty_e, row
 * e's own (float64, finite and >= 0); row 0's back and penalty are ignored.  Moves are not restricted by the backs: a reach says how
 * far the clock may wander either way.  Everything else -- u_e, D_0, m_e, a_e, reach_e, step_cost, the candidates cand(d) and
 * near_e[j] with its tie rule, the move words -- is "tracking"'s; float64, products and sums round separately.  For e >= 1:
 *     P_{e-1}[t] = min D_{e-1}[0 .. t];  A_{e-1}[t] = the FIRST index that attains it (scanning upwards with a strict <: 0.0 and
 *                  -0.0 tie);  P_{e-1}[t] is D_{e-1}[A_{e-1}[t]] itself, so a zero keeps its sign
 *     t_e(j)     = min(j + back_e, n_shift - 1), formed in 64 bits;  n_shift - 1 where back_e is SUSHI_HIP_TRACK_BACK_ANY
 *     jump_e[j]  = P_{e-1}[t_e(j)] + penalty_e
 *     take_near  = (near_e[j] <= jump_e[j])  (a tie moves);  D_e[j] = u_e[j] + (take_near ? near_e[j] : jump_e[j])
 *     move_e[j]  = the winning d (int16), or SUSHI_HIP_TRACK_JUMP
 *     backtrack:   s_{E-1} = a_{E-1};  for e = E-1 .. 1:
 *                  s_{e-1} = move_e[s_e] == SUSHI_HIP_TRACK_JUMP ? A_{e-1}[t_e(s_e)] : s_e + move_e[s_e]
 * The total cost is m_{E-1}: the minimum over all paths whose jumps obey s_e >= s_{e-1} - back_e, accumulated in "tracking"'s order
 * with penalty_e for a jump into event e.  With every back SUSHI_HIP_TRACK_BACK_ANY (or >= n_shift - 1) and one penalty the pass is
 * sushi_hip_track_forward + sushi_hip_track_backtrack bit for bit.  Rows are assumed finite; with a NaN the results are
 * unspecified, but no access leaves the buffers. */
#define SUSHI_HIP_TRACK_BACK_ANY (-1)
/* workspace of an ordered forward call (one set of per-workgroup partial records, and per work item of the axis one (minimum, first
 * index) record and the same of everything before the item); 0 for n_rows < 1 or n_shift < 1 */
SUSHI_HIP_API size_t sushi_hip_track_order_bytes(int n_rows, int32_t n_shift);
/* sushi_hip_track_forward for the ordered pass.  penalty_host[i] and back_host[i] are row row0 + i's, as rows_host[i] and
 * reach_host[i] are.  The state it adds to sushi_hip_track_forward's: P_dev, [n_shift] float64 (P of the last row advanced);
 * from_dev, [n_total][n_shift] int32 (row e holds A_e); back_dev, [n_total] int32 (every advanced row's back, left there for the
 * backtrack).  row0 > 0 continues from D_dev and P_dev as the call before it on the same stream left them: a sequence in chunks has
 * the bits of one call.  No device allocation, no upload: three launches per row, stream-ordered -- the step, a scan of one record
 * per work item, and the prefix minimum of the row just written -- and the launch boundary is their only synchronisation.
 * Asynchronous; stateless.  Checked before any HIP call -- EINVAL: everything sushi_hip_track_forward refuses (the penalty: per
 * row, in any row but the sequence's row 0), a null back or penalty table, a null P_dev / from_dev / back_dev, a back below
 * SUSHI_HIP_TRACK_BACK_ANY; EALIGN: mem_dev not 256-byte aligned; ENOSPACE: mem_bytes < sushi_hip_track_order_bytes; EALIGN: D_dev
 * / P_dev / row_min_dev not 8-byte aligned, a float / int32 pointer not 4-byte aligned, move_dev not 2-byte aligned. */
SUSHI_HIP_API int sushi_hip_track_forward_ordered(const float* curves_dev, int64_t n_curve,
                                                  const SushiHipJointRow* rows_host, const int32_t* reach_host,
                                                  const int32_t* back_host, int n_rows, int32_t n_shift,
                                                  int method, const double* penalty_host, double step_cost, int row0, int n_total,
                                                  double* D_dev, int16_t* move_dev,
                                                  double* P_dev, int32_t* from_dev, int32_t* back_dev,
                                                  double* row_min_dev, int32_t* row_arg_dev,
                                                  int32_t* row_own_index_dev, float* row_own_score_dev,
                                                  void* mem_dev, size_t mem_bytes, void* hip_stream);
/* out_shift_dev[e] = s_e for the n_total rows of a sequence whose ordered forward calls lie before it on the stream.  One wave,
 * one lane walking n_total dependent reads.  EINVAL: a null pointer, n_total < 1, n_shift < 1; EALIGN: move_dev not 2-byte aligned,
 * an int32 pointer not 4-byte aligned. */
SUSHI_HIP_API int sushi_hip_track_backtrack_ordered(const int16_t* move_dev, const int32_t* from_dev, const int32_t* back_dev,
                                                    const int32_t* row_arg_dev, int n_total, int32_t n_shift,
                                                    int32_t* out_shift_dev, void* hip_stream);

/* ---- ordered margins: how firmly ordered tracking places each event -- its min-marginals (13, additive) --------
 * "margins" for the pass of "ordered tracking": M_e[j] is the cost of the best whole path that puts event e at shift j among the
 * paths whose jumps obey the backs, with penalty_{i+1} for a jump out of event i.  Everything not named here is theirs, unchanged:
 * u_e, near / cand and their tie rule, the price of a move, B, M and C from nearB and jumpB (a tie moves), the guard window, the
 * stored index of an alternative, the (min, first index) combine rule; float64, products and sums round separately, one rounding
 * per sum.  A jump from (e, i) into (e + 1, j) exists iff j >= i - back_{e+1}.  So, backwards, with D_e the ordered forward pass's
 * row (sushi_hip_track_forward_ordered_keep keeps every one):
 *     C_{E-1} = u_{E-1};   M_{E-1} = D_{E-1}                          (nothing is added: the bits of D)
 *     S_e[t]     = min C_e[t .. n_shift - 1], the value at the FIRST (lowest) index that attains it (0.0 and -0.0 tie; a zero keeps
 *                  its sign): the (min, first index) combine over the span, in any grouping
 *     for e = E-2 .. 0, with r = reach_{e+1}, b = back_{e+1}, penalty_{e+1}:
 *         t'_e(j)  = max(j - b, 0), formed in 64 bits;  0 where b is SUSHI_HIP_TRACK_BACK_ANY
 *         jumpB[j] = S_{e+1}[t'_e(j)] + penalty_{e+1}                 (one rounding)
 *         nearB[j] = "margins"' window minimum over C_{e+1} with reach r (the value only)
 *         B_e[j]   = nearB[j] <= jumpB[j] ? nearB[j] : jumpB[j]       (a tie moves)
 *         M_e[j]   = D_e[j] + B_e[j];   C_e[j] = u_e[j] + B_e[j]
 *     per row e:   through_e, best_e / best_arg_e, alt_e / alt_arg_e as in "margins";  c_min_e = S_e[0]
 * Four facts.  EXACT PATH MINIMUM: M_e[j] is bitwise the minimum, over all paths with s_e = j whose jumps obey the backs, of (the
 * prefix cost, accumulated forwards as "ordered tracking" states it) + (the suffix cost, accumulated backwards in the mirrored
 * order as "margins" states it, with penalty_{i+1} per jump out of event i).  REVERSAL: c_min_0 == the ordered forward pass's total
 * on the reversed sequence -- the rows in reverse order and every row flipped end to end, reach_rev[i] = reach[E - i], back_rev[i] =
 * back[E - i], penalty_rev[i] = penalty[E - i]; a zero may differ in sign, since the window's tie order is mirrored.  CONSISTENCY
 * WITH THE TOTAL: best_e <= through_e exactly; |through_e - m_{E-1}| <= 6 E 2^-53 S as in "margins".  NO LIMIT: with every used back
 * SUSHI_HIP_TRACK_BACK_ANY or >= n_shift - 1 and one penalty, every output -- M, C, c_min, through, best, alt and their indices --
 * is sushi_hip_track_margins' bit for bit (S[0] with the first-index rule is n_{e+1} of "margins"). */
/* sushi_hip_track_forward_ordered with D kept: D_all_dev is [n_total][n_shift] float64, row e reads row e - 1 and writes row e.
 * Everything else -- the kernels, the other outputs, their bits, the refusals, the workspace (sushi_hip_track_order_bytes) and the
 * continuation of a sequence in chunks -- is sushi_hip_track_forward_ordered's. */
SUSHI_HIP_API int sushi_hip_track_forward_ordered_keep(const float* curves_dev, int64_t n_curve,
                                                       const SushiHipJointRow* rows_host, const int32_t* reach_host,
                                                       const int32_t* back_host, int n_rows, int32_t n_shift,
                                                       int method, const double* penalty_host, double step_cost, int row0, int n_total,
                                                       double* D_all_dev, int16_t* move_dev,
                                                       double* P_dev, int32_t* from_dev, int32_t* back_dev,
                                                       double* row_min_dev, int32_t* row_arg_dev,
                                                       int32_t* row_own_index_dev, float* row_own_score_dev,
                                                       void* mem_dev, size_t mem_bytes, void* hip_stream);
/* workspace of an ordered margins call (one set of per-workgroup partial minima, and per work item of the axis one (minimum, first
 * index) record and the minimum of everything after the item); 0 for n_rows < 1 or n_shift < 1 */
SUSHI_HIP_API size_t sushi_hip_track_order_margins_bytes(int n_rows, int32_t n_shift);
/* sushi_hip_track_margins for the ordered pass: walks rows row0 + n_rows - 1 down to row0 of a sequence whose
 * forward_ordered_keep calls and ordered backtrack lie before it on the stream.  rows_host[i] and guard_host[i] are row row0 + i's;
 * reach_host[i], back_host[i] and penalty_host[i] are row row0 + i's for i = 0 .. n_rows, the last only where row0 + n_rows <
 * n_total; entry 0 is not used and is ignored.  S_dev: [n_shift] float64, S of the last row walked; the other buffers are
 * sushi_hip_track_margins'.  The first call of a sequence has row0 + n_rows == n_total; a later one continues from C_dev and S_dev
 * as the call before it on the same stream left them: a sequence in chunks has the bits of one call, whatever the parity of the
 * boundary.  No device allocation, no upload: three launches per row, stream-ordered -- the step, a scan of one record per work
 * item (which also writes the row's outputs), and the suffix minimum of the row just written -- and the launch boundary is their
 * only synchronisation.  Asynchronous; stateless.  Checked before any HIP call -- EINVAL: everything sushi_hip_track_margins
 * refuses (it has no penalty of its own), a null back or penalty table, a null S_dev, a used back below
 * SUSHI_HIP_TRACK_BACK_ANY, a used penalty that is not finite or is negative; EALIGN: mem_dev not 256-byte aligned; ENOSPACE:
 * mem_bytes < sushi_hip_track_order_margins_bytes; EALIGN: a float64 pointer not 8-byte aligned, a float / int32 pointer not 4-byte
 * aligned. */
SUSHI_HIP_API int sushi_hip_track_order_margins(const float* curves_dev, int64_t n_curve,
                                                const SushiHipJointRow* rows_host, const int32_t* reach_host,
                                                const int32_t* back_host, const int32_t* guard_host,
                                                int n_rows, int32_t n_shift, int method, const double* penalty_host, double step_cost,
                                                int row0, int n_total,
                                                const double* D_all_dev, const int32_t* shift_dev, double* C_dev, double* S_dev,
                                                double* c_min_dev, double* through_dev, double* best_dev, int32_t* best_arg_dev,
                                                double* alt_dev, int32_t* alt_arg_dev, double* M_dev,
                                                void* mem_dev, size_t mem_bytes, void* hip_stream);

/* ---- wide tracking: a reach up to 32767 where moves are free (13, additive) -----------------------------------
 * "tracking" and "margins" word for word, with one bound raised: a row's reach may be 0 .. SUSHI_HIP_TRACK_WIDE_MAX_REACH, and every
 * used reach above SUSHI_HIP_TRACK_MAX_REACH requires a step_cost of +0.0 or -0.0 (with a price per sample a move of more than
 * penalty / step_cost samples never beats a jump: clip the reach instead).  A move word is an int16 and SUSHI_HIP_TRACK_JUMP is
 * -32768, so +-32767 fits; sushi_hip_track_backtrack is used as it is.  For a row X (D_{e-1} forwards, C_{e+1} backwards), a reach
 * r above SUSHI_HIP_TRACK_MAX_REACH and mu = step_cost, near[j] is what the candidate-by-candidate definition gives, bit for bit:
 *     cand(0) = X[j] itself;  cand(d) = X[j + d] + mu * (double)|d| for 0 < |d| <= r, 0 <= j + d < n_shift
 *     (mu = +0.0: a winning -0.0 at d != 0 becomes +0.0;  mu = -0.0: it keeps its bits)
 *     near[j] = the smallest candidate under the order (value, |d|, d > 0).  Adding +-0.0 changes no order, so this is:
 *         left  = the minimum of X[j - r .. j - 1], of equal values the LARGEST index
 *         right = the minimum of X[j + 1 .. j + r], of equal values the SMALLEST index        (0.0 and -0.0 are equal)
 *         own, left and right combined under the same order; the price is added once, to the winner
 * computed in a time that does not grow with r.  A row whose reach is at most SUSHI_HIP_TRACK_MAX_REACH goes through the kernels of
 * sushi_hip_track_forward / sushi_hip_track_margins themselves: with every reach <= SUSHI_HIP_TRACK_MAX_REACH each wide call gives
 * the plain call's outputs bit for bit. */
#define SUSHI_HIP_TRACK_WIDE_MAX_REACH 32767
/* workspace of a wide forward / a wide margins call: the plain call's, then one row's window records (24 bytes per shift: per
 * element the minimum of its 1024-value tile up to it and from it on, each a float64 and two 16-bit indices); 0 wherever
 * sushi_hip_track_bytes / sushi_hip_track_margins_bytes is 0 */
SUSHI_HIP_API size_t sushi_hip_track_wide_bytes(int n_rows, int32_t n_shift);
SUSHI_HIP_API size_t sushi_hip_track_margins_wide_bytes(int n_rows, int32_t n_shift);
/* sushi_hip_track_forward / sushi_hip_track_forward_keep with a reach up to SUSHI_HIP_TRACK_WIDE_MAX_REACH: the arguments, the
 * outputs, chunks (a sequence may mix plain and wide calls: the state is the same) and the refusals in their order, but -- EINVAL: a
 * reach outside 0 .. SUSHI_HIP_TRACK_WIDE_MAX_REACH in any row but the sequence's row 0, or such a reach above
 * SUSHI_HIP_TRACK_MAX_REACH beside a step_cost that is not +-0.0; ENOSPACE: mem_bytes < sushi_hip_track_wide_bytes.  A wide row
 * takes two launches, stream-ordered; no grid waits on itself and there are no atomics. */
SUSHI_HIP_API int sushi_hip_track_forward_wide(const float* curves_dev, int64_t n_curve,
                                               const SushiHipJointRow* rows_host, const int32_t* reach_host, int n_rows, int32_t n_shift,
                                               int method, double penalty, double step_cost, int row0, int n_total,
                                               double* D_dev, int16_t* move_dev,
                                               double* row_min_dev, int32_t* row_arg_dev,
                                               int32_t* row_own_index_dev, float* row_own_score_dev,
                                               void* mem_dev, size_t mem_bytes, void* hip_stream);
SUSHI_HIP_API int sushi_hip_track_forward_wide_keep(const float* curves_dev, int64_t n_curve,
                                                    const SushiHipJointRow* rows_host, const int32_t* reach_host, int n_rows,
                                                    int32_t n_shift, int method, double penalty, double step_cost, int row0, int n_total,
                                                    double* D_all_dev, int16_t* move_dev,
                                                    double* row_min_dev, int32_t* row_arg_dev,
                                                    int32_t* row_own_index_dev, float* row_own_score_dev,
                                                    void* mem_dev, size_t mem_bytes, void* hip_stream);
/* sushi_hip_track_margins in the same way: a used reach outside 0 .. SUSHI_HIP_TRACK_WIDE_MAX_REACH, or one above
 * SUSHI_HIP_TRACK_MAX_REACH beside a step_cost that is not +-0.0, is EINVAL; ENOSPACE: mem_bytes <
 * sushi_hip_track_margins_wide_bytes. */
SUSHI_HIP_API int sushi_hip_track_margins_wide(const float* curves_dev, int64_t n_curve,
                                               const SushiHipJointRow* rows_host, const int32_t* reach_host, const int32_t* guard_host,
                                               int n_rows, int32_t n_shift, int method, double penalty, double step_cost,
                                               int row0, int n_total,
                                               const double* D_all_dev, const int32_t* shift_dev, double* C_dev, double* c_min_dev,
                                               double* through_dev, double* best_dev, int32_t* best_arg_dev,
                                               double* alt_dev, int32_t* alt_arg_dev, double* M_dev,
                                               void* mem_dev, size_t mem_bytes, void* hip_stream);

/* ---- wide ordered tracking: the ordered pass and its margins with a reach up to 32767 where moves are free (13,
 * additive) ---------------------------------------------------------------------------------------------------------------------
 * "ordered tracking" and "ordered margins" word for word, with "wide tracking"'s one bound raised: a row's reach may be 0 ..
 * SUSHI_HIP_TRACK_WIDE_MAX_REACH, and every used reach above SUSHI_HIP_TRACK_MAX_REACH requires a step_cost of +0.0 or -0.0.  The
 * recurrences, the tie rules, the move words, P / A / S, chunks and every output are unchanged; near[j] of a row of a reach above
 * SUSHI_HIP_TRACK_MAX_REACH is "wide tracking"'s, bit for bit the candidate-by-candidate definition's, and its jump term is the
 * ordered pass's own: P_{e-1}[t_e(j)] + penalty_e forwards, S_{e+1}[t'_e(j)] + penalty_{e+1} backwards.  A row whose reach is at
 * most SUSHI_HIP_TRACK_MAX_REACH goes through the ordered calls' own kernels: with no reach above it each call gives the ordered
 * call's outputs bit for bit; with every back without a limit and one penalty each gives the wide call's.
 * sushi_hip_track_backtrack_ordered is used as it is.  The state is the ordered calls': a sequence may mix them. */
/* workspace: the ordered call's, then one row's window records (24 bytes per shift); 0 wherever sushi_hip_track_order_bytes /
 * sushi_hip_track_order_margins_bytes is 0 */
SUSHI_HIP_API size_t sushi_hip_track_order_wide_bytes(int n_rows, int32_t n_shift);
SUSHI_HIP_API size_t sushi_hip_track_order_margins_wide_bytes(int n_rows, int32_t n_shift);
/* sushi_hip_track_forward_ordered / _ordered_keep: the arguments, the outputs and the refusals in their order, but -- EINVAL: a reach
 * outside 0 .. SUSHI_HIP_TRACK_WIDE_MAX_REACH in any row but the sequence's row 0, or such a reach above SUSHI_HIP_TRACK_MAX_REACH
 * beside a step_cost that is not +-0.0 (both where the ordered call checks a row's reach); ENOSPACE: mem_bytes <
 * sushi_hip_track_order_wide_bytes.  A wide row takes four launches (tile pass, step, scan, apply), stream-ordered; no grid waits
 * on itself and there are no atomics. */
SUSHI_HIP_API int sushi_hip_track_forward_ordered_wide(const float* curves_dev, int64_t n_curve,
                                                       const SushiHipJointRow* rows_host, const int32_t* reach_host,
                                                       const int32_t* back_host, int n_rows, int32_t n_shift, int method,
                                                       const double* penalty_host, double step_cost, int row0, int n_total,
                                                       double* D_dev, int16_t* move_dev, double* P_dev, int32_t* from_dev,
                                                       int32_t* back_dev, double* row_min_dev, int32_t* row_arg_dev,
                                                       int32_t* row_own_index_dev, float* row_own_score_dev,
                                                       void* mem_dev, size_t mem_bytes, void* hip_stream);
SUSHI_HIP_API int sushi_hip_track_forward_ordered_wide_keep(const float* curves_dev, int64_t n_curve,
                                                            const SushiHipJointRow* rows_host, const int32_t* reach_host,
                                                            const int32_t* back_host, int n_rows, int32_t n_shift, int method,
                                                            const double* penalty_host, double step_cost, int row0, int n_total,
                                                            double* D_all_dev, int16_t* move_dev, double* P_dev, int32_t* from_dev,
                                                            int32_t* back_dev, double* row_min_dev, int32_t* row_arg_dev,
                                                            int32_t* row_own_index_dev, float* row_own_score_dev,
                                                            void* mem_dev, size_t mem_bytes, void* hip_stream);
/* sushi_hip_track_order_margins in the same way: a used reach outside 0 .. SUSHI_HIP_TRACK_WIDE_MAX_REACH, or one above
 * SUSHI_HIP_TRACK_MAX_REACH beside a step_cost that is not +-0.0, is EINVAL; ENOSPACE: mem_bytes <
 * sushi_hip_track_order_margins_wide_bytes. */
SUSHI_HIP_API int sushi_hip_track_order_margins_wide(const float* curves_dev, int64_t n_curve,
                                                     const SushiHipJointRow* rows_host, const int32_t* reach_host,
                                                     const int32_t* back_host, const int32_t* guard_host, int n_rows, int32_t n_shift,
                                                     int method, const double* penalty_host, double step_cost, int row0, int n_total,
                                                     const double* D_all_dev, const int32_t* shift_dev, double* C_dev, double* S_dev,
                                                     double* c_min_dev, double* through_dev, double* best_dev, int32_t* best_arg_dev,
                                                     double* alt_dev, int32_t* alt_arg_dev, double* M_dev,
                                                     void* mem_dev, size_t mem_bytes, void* hip_stream);

/* ---- rows: score rows clamped at a threshold, formed from a threshold run's hits (13, additive) ---------------
 * A pass over a shift axis needs to know where a row is good and how good; how bad the rest is only feeds decoys.  The CLAMPED row
 * of a score row R at a float32 value f keeps every value that passes f and holds f everywhere else:
 *     SUSHI_HIP_METHOD_SQDIFF_NORMED   C[p] = R[p] <= f ? R[p] : f      (min(R, f), the bits of a passing value kept, -0.0 included)
 *     SUSHI_HIP_METHOD_CCOEFF_NORMED   C[p] = R[p] >= f ? R[p] : f      (max(R, f))
 * (a NaN does not pass).  A float32 score passes a threshold run's double comparison with (double)f exactly when it passes f, so
 * "the hits of sushi_hip_batch_run_threshold(batch, (double)f, ...), and f everywhere else" is C bit for bit: that is
 * sushi_hip_rows_from_hits, a fill and a scatter, no score formed.  sushi_hip_rows_clamp applies the rule to rows that exist.
 * A row record names where a row lies in each buffer of a call; rows of one call that overlap are the caller's business. */
typedef struct SushiHipRowsRow {
    int64_t out_off;    /* first float of the row in out_dev */
    int64_t in_off;     /* sushi_hip_rows_clamp: first float of the row in in_dev; sushi_hip_rows_from_hits: not read */
    int32_t n_pos;      /* floats of the row, >= 1 */
    int32_t reserved;
} SushiHipRowsRow;          /* 24 bytes */
#define SUSHI_HIP_ROWS_OVERFLOW 1   /* flag bit 0: the request has more hits than `capacity`; its row is all f */
#define SUSHI_HIP_ROWS_BAD_HITS 2   /* flag bit 1: a hit index outside [0, n_pos), hits not in ascending index order, a count < 0 */
/* floats of a tile: one workgroup fills a tile of consecutive floats of one row, then writes the hits that fall into it */
SUSHI_HIP_API int sushi_hip_rows_tile(void);
/* workspace of either call (the row table); 0 for n < 1 */
SUSHI_HIP_API size_t sushi_hip_rows_bytes(int n);
/* hits_dev: [n][capacity] records and counts_dev: [n], as sushi_hip_batch_run_threshold leaves them (request k's hits in ascending
 * index order in the first min(counts[k], capacity) records).  Row k, rows_host[k].n_pos floats from out_dev + rows_host[k].out_off
 * on, becomes f over [0, n_pos) and then hits[k][j].score at hits[k][j].index for every j < counts[k]; flags_dev[k] (int32) becomes
 * 0, or SUSHI_HIP_ROWS_OVERFLOW where counts[k] > capacity -- that row is all f: it has to be formed densely --, or
 * SUSHI_HIP_ROWS_BAD_HITS where the list is not what a threshold run leaves: such a row holds f and an unspecified subset of its
 * hits, and no access leaves the row or the list.  Floats of out_dev outside every row are not written.  A tile of a row is
 * written by one workgroup only, which finds its hits by bisection of the list: no atomics on the rows, and the result does not
 * depend on the launch geometry.  No device allocation: one upload of the table into mem_dev, one memset of the flags, one launch.
 * Asynchronous; stateless (any thread, own workspace).  Checked before any HIP call -- EINVAL: a null pointer, n < 1, capacity < 0,
 * n_out < 1, an f that is not finite, n_pos < 1, out_off < 0 or out_off + n_pos > n_out (decided without forming the sum); EALIGN:
 * mem_dev not 256-byte aligned, counts_dev not 8-byte aligned, another pointer not 4-byte aligned; ENOSPACE: mem_bytes too small. */
SUSHI_HIP_API int sushi_hip_rows_from_hits(const SushiHipHit* hits_dev, const int64_t* counts_dev, int n, int32_t capacity,
                                           const SushiHipRowsRow* rows_host, float f, float* out_dev, int64_t n_out,
                                           int32_t* flags_dev, void* mem_dev, size_t mem_bytes, void* hip_stream);
/* out_dev[out_off + p] = C[p] of R = in_dev[in_off ..], for every row of the table and p in [0, n_pos).  in_dev == out_dev with
 * in_off == out_off in every row clamps in place; buffers that overlap in any other way are refused.  One upload of the table, one
 * launch.  Asynchronous; stateless.  Checked before any HIP call -- EINVAL: a null pointer, n < 1, n_in < 1, n_out < 1, an unknown
 * method, an f that is not finite, n_pos < 1, a row that leaves either buffer, buffers that overlap other than in place; EALIGN:
 * mem_dev not 256-byte aligned, a float pointer not 4-byte aligned; ENOSPACE: mem_bytes too small. */
SUSHI_HIP_API int sushi_hip_rows_clamp(const float* in_dev, int64_t n_in, float* out_dev, int64_t n_out,
                                       const SushiHipRowsRow* rows_host, int n, int method, float f,
                                       void* mem_dev, size_t mem_bytes, void* hip_stream);

/* ---- WavStream.__init__ on the GPU (wav.py:64-91 decode + downmix, wav.py:113-156 value pipeline) ----
 * sushi_hip_load_decode   : interleaved little-endian PCM frames (sample_width 2 or 3 bytes, `channels` per frame)
 *     -> float32 mono: the int16 (for 24-bit: the top two bytes, wav.py:70-74) of every channel converted to
 *     float32, summed left to right in float32 and divided by float(channels) (wav.py:78-91).  Frames
 *     [0, n_frames) of pcm_dev go to mono_dev[0 .. n_frames): callers upload and decode a file in bounded chunks.
 * sushi_hip_load_resample : data[pad + u] = nearest-neighbour decimation of the one-second chunks of the
 *     downmixed frames (cv2.resize INTER_NEAREST, wav.py:125-137: sx = min(floor(x * scale), chunk - 1) in
 *     float64), zeros where the reference never writes, and both pads filled with the nearest inner sample
 *     (wav.py:140-141).  n_full chunks of `chunk` frames become nl_full samples each (scale_full =
 *     1 / (nl_full / chunk)); a last partial chunk of `rest` frames becomes nl_rest samples.
 * sushi_hip_load_histogram: 256-bin histogram (uint64) of key byte `shift/8` over the samples >= 0
 *     (side 0; key = bit pattern) or <= 0 (side 1; key = bit pattern of -x) whose key & mask == prefix:
 *     the building block of the exact radix select behind np.median(data[data >= 0]) (wav.py:145-146).
 * sushi_hip_load_normalise: in place clip to [lo, hi], subtract lo, divide by range (wav.py:148-151);
 *     if u8_dev != NULL also v * 255 + 0.5 truncated to uint8 (wav.py:153-156). */
SUSHI_HIP_API int sushi_hip_load_decode(const void* pcm_dev, int64_t n_frames, int32_t channels, int32_t sample_width,
                            float* mono_dev, void* hip_stream);
/* ---- weighted downmix: several mixes of a file's channels in one decode pass (13, additive) ----
 * sushi_hip_load_decode's decode with weights instead of the mean.  s_c: channel c's sample of a frame as sushi_hip_load_decode
 * takes it (the int16 value, for 24-bit samples the top two bytes, as float32).  Output row o of that frame, with the float32
 * weights w[o][0 .. channels):
 *     acc = w[o][0] * s_0                                  (float32 product, rounded)
 *     for c = 1 .. channels - 1:  acc = acc + w[o][c] * s_c    (the product rounded to float32, then the sum: no fused multiply-add)
 * Every channel takes part, in file order, zero weights included, so a NumPy float32 restatement (sushi_amd.downmix.mix_host)
 * equals the result bit for bit, signed zeros too.  Weights {0.5, 0.5} on 16-bit stereo give sushi_hip_load_decode's bits.
 * weights_host: n_out x channels float32, row-major, in HOST memory; it travels in the kernel's arguments: no device allocation,
 * no upload, no synchronisation.  Row o of frames [0, n_frames) goes to out_dev + o * out_stride; nothing else of out_dev is
 * touched.  pcm_dev may have any byte alignment; only its n_frames * channels * sample_width bytes are read.  One pass over the PCM
 * bytes serves all n_out rows.  Asynchronous; stateless.
 * Checked before any HIP call -- EINVAL: a null pointer, n_frames < 0, channels outside [1, SUSHI_HIP_MIX_MAX_CHANNELS], n_out
 * outside [1, SUSHI_HIP_MIX_MAX_OUTPUTS], sample_width not 2 or 3, out_stride < n_frames, a weight that is not finite; EALIGN:
 * out_dev not 4-byte aligned.  n_frames == 0 returns SUSHI_HIP_OK without a launch. */
#define SUSHI_HIP_MIX_MAX_CHANNELS 32
#define SUSHI_HIP_MIX_MAX_OUTPUTS 8
SUSHI_HIP_API int sushi_hip_load_decode_mix(const void* pcm_dev, int64_t n_frames, int32_t channels, int32_t sample_width,
                              const float* weights_host, int32_t n_out, float* out_dev, int64_t out_stride,
                              void* hip_stream);
/* ---- sample formats: the decode for 8-bit, 32-bit, float and double files (13, additive) ----
 * sushi_hip_load_decode and sushi_hip_load_decode_mix with a format code in place of the sample width.  A sample's value is a
 * float32 on the int16 scale of the rest of the pipeline, read little-endian, byte by byte, from its container:
 *     SUSHI_HIP_PCM_U8   1 byte    (float)(((int)b - 128) * 256)
 *     SUSHI_HIP_PCM_S16  2 bytes   the top two bytes as int16, as float32 (sushi_hip_load_decode's value; valid bits are
 *     SUSHI_HIP_PCM_S24  3 bytes   left-justified in their container, so 20-in-24 and 24-in-32 come out right)
 *     SUSHI_HIP_PCM_S32  4 bytes
 *     SUSHI_HIP_PCM_F32  4 bytes   s = v * 32768.0f: one float32 multiply.  A NaN or +-inf s becomes +0.0f.  A denormal v and
 *                                  -0.0f are values like any other: nothing is flushed and the sign is kept.
 *     SUSHI_HIP_PCM_F64  8 bytes   s = (float)(v * 32768.0): a float64 multiply, then one rounding to float32 (nearest-even).  A
 *                                  NaN or +-inf s becomes +0.0f, also where the cast overflows.
 * Nothing is clamped.  sushi_hip_load_decode_format: the mean of a frame's values -- the float32 sum left to right, divided by
 * float(channels), no division for one channel -- to mono_dev[0 .. n_frames).  sushi_hip_load_decode_mix_format: the weighted
 * rows of sushi_hip_load_decode_mix on those values, in its order (every product and every sum rounded to float32), to
 * out_dev + o * out_stride.  A NumPy restatement (sushi_amd.downmix.samples_from_bytes, then mean_host / mix_host) equals either
 * result bit for bit; S16 and S24 give the bits of sushi_hip_load_decode / sushi_hip_load_decode_mix at sample_width 2 and 3.
 * pcm_dev may have any byte alignment; only its n_frames * channels * container bytes are read.  weights_host is HOST memory and
 * travels in the kernel's arguments.  Asynchronous; stateless; nothing is allocated.
 * Checked before any HIP call, in this order -- sushi_hip_load_decode_format: EINVAL: a null pointer, n_frames < 0, channels < 1,
 * an unknown format; EALIGN: mono_dev not 4-byte aligned.  sushi_hip_load_decode_mix_format: EINVAL: a null pointer, n_frames < 0,
 * channels outside [1, SUSHI_HIP_MIX_MAX_CHANNELS], n_out outside [1, SUSHI_HIP_MIX_MAX_OUTPUTS], an unknown format, out_stride <
 * n_frames, a weight that is not finite; EALIGN: out_dev not 4-byte aligned.  n_frames == 0 returns SUSHI_HIP_OK without a launch. */
#define SUSHI_HIP_PCM_U8 1
#define SUSHI_HIP_PCM_S16 2
#define SUSHI_HIP_PCM_S24 3
#define SUSHI_HIP_PCM_S32 4
#define SUSHI_HIP_PCM_F32 5
#define SUSHI_HIP_PCM_F64 6
SUSHI_HIP_API int sushi_hip_load_decode_format(const void* pcm_dev, int64_t n_frames, int32_t channels, int32_t format,
                                 float* mono_dev, void* hip_stream);
SUSHI_HIP_API int sushi_hip_load_decode_mix_format(const void* pcm_dev, int64_t n_frames, int32_t channels, int32_t format,
                                     const float* weights_host, int32_t n_out, float* out_dev, int64_t out_stride,
                                     void* hip_stream);
SUSHI_HIP_API int sushi_hip_load_resample(const float* raw_dev, int64_t n_raw, int32_t chunk, int32_t nl_full, double scale_full,
                            int64_t n_full, int32_t rest, int32_t nl_rest, double scale_rest,
                            int64_t pad, int64_t total, float* data_dev, void* hip_stream);
/* ---- filtered decimation: a low-pass in front of the decimator (13, additive) ----
 * sushi_hip_load_resample's row with a zero-phase polyphase FIR filter in place of the nearest-neighbour read.  num / den: input
 * frames per output sample in lowest terms (frame rate / sample rate); table_dev: float64 [den][2 * half_width], row r the filter
 * for an output that lies r / den behind an input frame, every row summing to 1 (sushi_amd.resample.fir_table builds it on the
 * host; the library only applies it).  Body sample i, 0 <= i < n_body, W = half_width:
 *     t = i * num (int64);  j = t / den;  r = t % den;  acc = 0.0
 *     for c = 0 .. 2W - 1, in that order:  acc = acc + table[r][c] * (double)raw[clamp(j - W + 1 + c, 0, n_raw - 1)]
 *                                          (float64; the product rounded, then the sum: no fused multiply-add)
 *     data[pad + i] = (float)acc
 * so a NumPy float64 restatement (sushi_amd.resample.resample_host) equals the result bit for bit.  The rest of the row is what
 * sushi_hip_load_resample writes: zeros from pad + n_body to total - pad, data[0 .. pad) = data[pad], data[total - pad .. total)
 * = data[total - pad - 1].  All of [0, total) is written and nothing else.  Asynchronous; stateless.
 * Checked before any HIP call -- EINVAL: a null pointer, n_raw < 1, n_body < 1 or >= 2^40, num or den outside [1, 2^20],
 * half_width < 1, den * 2 * half_width > 65536, a last read (n_body - 1) * num / den > n_raw - 1, pad < 0,
 * pad + n_body > total - pad; EALIGN: table_dev not 8-byte aligned, raw_dev or data_dev not 4-byte aligned. */
SUSHI_HIP_API int sushi_hip_load_resample_fir(const float* raw_dev, int64_t n_raw, int32_t num, int32_t den,
                                const double* table_dev, int32_t half_width, int64_t n_body,
                                int64_t pad, int64_t total, float* data_dev, void* hip_stream);
SUSHI_HIP_API int sushi_hip_load_histogram(const float* data_dev, int64_t n, int side, uint32_t prefix, uint32_t mask, int shift,
                             uint64_t* hist_dev, void* hip_stream);
SUSHI_HIP_API int sushi_hip_load_normalise(float* data_dev, int64_t n, float lo, float hi, float range, uint8_t* u8_dev,
                             void* hip_stream);

/* Optional per-stage timing of the FFT path with HIP events recorded on the launch stream (bench.py's roofline
 * figures).  Between _begin and _end every sushi_hip_batch_run records its stage boundaries; _end waits for them and
 * writes, per run, the milliseconds spent in each stage (summed over the run's sub-batches) into
 * stage_ms[run][SUSHI_HIP_NSTAGES].  Not thread safe. */
#define SUSHI_HIP_NSTAGES 6
#define SUSHI_HIP_STAGE_TSPEC 0    /* pattern-segment DFTs                                          */
#define SUSHI_HIP_STAGE_MAC 1      /* frequency-domain multiply-accumulate                          */
#define SUSHI_HIP_STAGE_IFFT 2     /* inverse DFTs + scoring epilogue                               */
#define SUSHI_HIP_STAGE_REFINE 3   /* exact float64 evaluation of the listed candidates             */
#define SUSHI_HIP_STAGE_FINISH 4   /* candidate collection + exact tiles of flagged searches, unpack */
#define SUSHI_HIP_STAGE_BOUND 5    /* lower bounds of the block pairs' scores (three of the inverse transform's four passes)  */
SUSHI_HIP_API int sushi_hip_profile_begin(void);
SUSHI_HIP_API int sushi_hip_profile_end(float* stage_ms, int max_calls, int* n_calls);

#ifdef __cplusplus
}
#endif
#endif /* SUSHI_HIP_H */
