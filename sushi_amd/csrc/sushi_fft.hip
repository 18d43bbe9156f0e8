// sushi_amd/csrc/sushi_fft.hip -- overlap-save FFT form of Sushi's template match for gfx950 (MI355X),
// and the batch handle of the C ABI.
//
// For every (pattern, window) request the float32 result.argmin and result[argmin] of
//   wav.py:185  result = cv2.matchTemplate(search_source, pattern, cv2.TM_SQDIFF_NORMED)
//   wav.py:186  min_idx = result.argmin(axis=1)[0]
// cv2's crossCorr() computes the sliding dot product by block DFT; so does this path, which turns
// the O(P*M) FLOP-bound search into an O(P log N) HBM-bound one (DESIGN.md "FFT path").  With N-point
// complex transforms, pattern segments of B = FFT_SEG samples and H = N - B valid positions per real block:
//
//   spectra_kernel   once per destination stream, for every block j (hop B):
//                    Z_j = DFT_N( x[jB .. jB+N) + i * x[jB+H .. jB+H+N) )
//                    (+ the low band of Z_j once more and its norms outside the band: the band-split exclusion below)
//   tspec_real_kernel  per search, per pattern segment s (B samples, zero padded to N):
//                    Tt_s = conj(DFT_N(t_s)) / N                                  (+ its low band and its norm outside the band)
//                    -- t_s is real: packed into N/2 complex points, one N/2-point transform, unfolded (fft_core.hpp); its
//                    whole rows are conjugate-symmetric word for word and stored as HALF rows, which every reader expands;
//                    tspec_kernel (SUSHI_HIP_TSPEC=complex) is the N-point complex transform it replaced, kept for A/B
//   mac_kernel       per search, per frequency bin f, per pair I of the absolute pair grid (pair I starts at
//                    block FFT_STEP * I, FFT_STEP = 2H / B):
//                    Y_I(f) = sum_s Tt_s(f) * Z_{FFT_STEP*I+s}(f)       (a 1-D Toeplitz product along j)
//                    -- over every pair on the LOW rows (a quarter of the bins: the band-split form of the exclusion), or on whole
//                    rows (the whole-row form, no exclusion, the dense fall-back); mac_rows_kernel / mac_list_kernel form the
//                    whole rows of LISTED pairs only (search by search: each pilot with its search's audit pair, then what the
//                    bounds left)
//   bound_low_kernel / bound_kernel + slb_kernel, pilot_kernel, survivor_kernel
//                    a LOWER bound of every pair's scores without scoring it; the pair with the smallest bound of every search
//                    is transformed first, then only the pairs whose bound is not above what the search has found
//   ifft_kernel      y_I = IDFT_N(Y_I): Re y_I[r] / Im y_I[r] (r < H) are the cross terms of positions
//                    FFT_STEP*I*B + r and FFT_STEP*I*B + H + r.  Fused epilogue: window energies, normalised f32
//                    score, the pair's error bound, arg-min, and the list of positions that can still be the
//                    minimum (candidates); the pair's lower bound held to what it really scores (the exclusion's audit).
//   refine_kernel    (sushi_exact.hip) exact float64 re-evaluation of the candidates -> final (index, score);
//   collect + tiles  searches with more candidates than the lists hold: the inverse transforms of their pairs
//                    are redone with the search's final threshold, every candidate goes to a per-tile list
//                    (a tile = 1024 positions) and exact_tiles_kernel (sushi_exact.hip) evaluates those exactly.
//
// Pairing two real blocks as one complex block makes every N-point complex DFT produce 2H useful
// results and needs no real-FFT untangling pass: the pattern is real, so correlation is linear
// over the real and imaginary parts.
//
// gfx950 only: wave64, 160 KiB LDS/CU.  No CUDA compatibility paths.
//
// ONE translation unit, cut by stage (every part is included below, inside this file's anonymous namespace):
//   sushi_geometry.hpp     (a header: every unit's) the sizes and records host plan and device code agree on, and the one rule of
//                          what a request may be (request_fits)
//   stream_core.hpp        (a header: every unit's, host only, checked on the CPU by tests/host_stream_check.cpp) the stream handle and
//                          the table of a stream's parts: its buffer's size, the handle's pointers, sushi_hip_stream_view's answers
//                          (the curves' and the retime unit's host sides are checked there too: curve_core.hpp, retime_core.hpp)
//   plan_core.hpp          (a header: host only, checked on the CPU by tests/host_plan_check.cpp) the plan of a batch, its
//                          workspace and device-memory layouts, parse_bound_fault, ranking_key
//   batch_core.hpp         (a header: host only, checked on the CPU by tests/host_batch_check.cpp) what a handle holds about its
//                          requests and how it is staged: BatchPlanState, stage_batch, PlanCache, resolve_variant, the spans a run
//                          uploads and clears
//   run_policy.hpp         (a header: host only, checked on the CPU by tests/host_policy_check.cpp) what a run decides from the
//                          exclusion mode and from what earlier runs left: Learnt, LastRun, one function per rule
//   sushi_fft_store.inc    packed-half storage: scales, stored bin order, the low band of a row and the norms outside it
//   sushi_fft_spectra.inc  spectra_kernel, tspec_real_kernel / tspec_kernel, tspec_expand_kernel (half rows -> whole rows, for the workspace view)
//   sushi_fft_mac.inc      mac_kernel / mac_long_kernel / mac_list_kernel
//   sushi_fft_ifft.inc     ifft_kernel / ifft_list_kernel: transform, scoring epilogue, error model, candidates
//   sushi_fft_bound.inc    the pair exclusion: bound_kernel / bound_low_kernel / slb_kernel / pilot / survivor / second look / mac_rows_kernel;
//                          the rules every run kind shares: bound_excludes, is_audit_pair, append_pairs
//   sushi_fft_collect.inc  collect_kernel
//   sushi_fft_threshold.inc  the threshold run's own kernels: seed, audit, extension, output scan
//   sushi_fft_best.inc     the best-K run's own kernels: seed, escalation, audit, extension
//   sushi_fft_plan.inc     host: launches by method / sample type, stage timing, a sub-batch's view of the batch's memory (SubView)
//   (this file)            the batch handle and the HIP calls of its life (plan_and_upload: stage, wait, commit, upload), the skeleton
//                          of a run around its sub-batches (run_sub_batches) and the C ABI's entry points

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <float.h>
#include <limits.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <memory>
#include <mutex>
#include <new>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/sushi_hip.h"
#include "sushi_common.hpp"
#include "sushi_internal.hpp"
#include "fft_core.hpp"
#include "mac_core.hpp"
#include "plan_core.hpp"
#include "batch_core.hpp"
#include "run_policy.hpp"

namespace {

using namespace sushi;
using sushi_fft::cpx;

constexpr int FN = FFT_N;                              // complex points per transform
constexpr int FT = sushi_fft::Plan<FFT_LOGN>::NT;      // threads per transform workgroup
constexpr int FH = FFT_H;                              // result positions per half of a pair
constexpr int HPT = FH / FT;                           // result positions per thread and half
constexpr int RPB = FFT_SEG / FT;                      // of which per block
static_assert(FH % FT == 0 && FFT_SEG % FT == 0 && HPT == FFT_VB * RPB, "position layout");
static_assert(HPT <= sushi_fft::PER, "a thread's valid outputs are a prefix of its transform outputs");
constexpr int LDS_FLOATS = sushi_fft::lds_floats<FFT_LOGN>();

#include "sushi_fft_store.inc"
#include "sushi_fft_spectra.inc"
#include "sushi_fft_mac.inc"
#include "sushi_fft_ifft.inc"
#include "sushi_fft_bound.inc"
#include "sushi_fft_collect.inc"
#include "sushi_fft_threshold.inc"
#include "sushi_fft_best.inc"
#include "sushi_fft_plan.inc"

}  // namespace

// What a batch's FIRST run used to allocate -- 16 bytes of pinned host memory for the counts that come back behind an event, the
// lanes' HIP streams -- cost that run 9 - 13 ms of host time (hipHostMalloc maps into every device's page tables; a stream is a
// hardware queue): both now come from pools of the process's own, made once (tools/first_run_probe.py: the first run of a batch of
// BASELINE configs[2] spent 9.4 of its 21.6 ms inside sushi_hip_batch_run on the host).  Pool slots are handed out under a mutex; a handle is used by one host thread at a time.
struct HostSlots {
    static constexpr int SLOTS = 1024, WORDS = 2;
    std::mutex mu;
    unsigned long long* base = nullptr;
    std::vector<int> free_list;
    unsigned long long* take() {
        std::lock_guard<std::mutex> g(mu);
        if (!base) {
            if (hipHostMalloc((void**)&base, (size_t)SLOTS * WORDS * sizeof(unsigned long long), hipHostMallocPortable) != hipSuccess) { base = nullptr; return nullptr; }
            for (int k = SLOTS - 1; k >= 0; --k) free_list.push_back(k);
        }
        if (free_list.empty()) return nullptr;
        const int k = free_list.back(); free_list.pop_back();
        return base + (size_t)k * WORDS;
    }
    void give(unsigned long long* p) {
        if (!p) return;
        std::lock_guard<std::mutex> g(mu);
        free_list.push_back((int)((p - base) / WORDS));
    }
};
static HostSlots g_host_slots;

// The lanes' streams, per device: shared by every batch on that device (batches that run at the same time on different caller
// streams then share them too -- ordered by their own events, side by side no longer; one batch at a time is the product's use).
struct LanePool {
    static constexpr int MAX_DEVICES = 16;
    std::mutex mu;
    hipStream_t st[MAX_DEVICES][MAX_LANES] = {};
    hipStream_t get(int lane) {
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= MAX_DEVICES) return nullptr;
        std::lock_guard<std::mutex> g(mu);
        if (!st[dev][lane] && hipStreamCreateWithFlags(&st[dev][lane], hipStreamNonBlocking) != hipSuccess) st[dev][lane] = nullptr;
        return st[dev][lane];
    }
};
static LanePool g_lane_pool;

// The opaque batch handle of the C ABI.
struct SushiHipBatch {
    const SushiHipStream* dst = nullptr;
    const SushiHipStream* src = nullptr;
    int n = 0, path = 0, variant = 0, method = SUSHI_HIP_METHOD_SQDIFF_NORMED, exclusion = SUSHI_HIP_EXCLUDE_AUTO;
    Learnt learnt;                      // what the batch has learnt about its searches (run_policy.hpp; a new plan: about other searches now)
    LastRun last;                       // what its last run was
    unsigned run_seq = 0;               // runs so far: rotates which excluded pairs are audited
    int audit_every = 2;                // one search in this many has one excluded pair transformed as a check, per run
    int pilot_rows = PILOT_ROWS_BY_SEARCH;  // how the pilots' whole rows are formed (run_policy.hpp; SUSHI_HIP_PILOT_ROWS=list: pair by pair, for A/B)
    int rest_rows = REST_ROWS_BY_ITEM;      // the survivors' pass's unit of work (run_policy.hpp; SUSHI_HIP_REST_ROWS=search: a whole search, for A/B)
    int tspec = TSPEC_REAL;                 // the pattern segments' transform (run_policy.hpp; SUSHI_HIP_TSPEC=complex: the full-size complex one, for A/B)
    int slb = SLB_BY_GROUP;                 // lanes a pair in slb_kernel / slb_list_kernel (run_policy.hpp; SUSHI_HIP_SLB=wave: a wave a pair, for A/B)
    int second_look = SECOND_LOOK_AHEAD;    // the second look's transform kernel (run_policy.hpp; SUSHI_HIP_SECOND_LOOK=plain: the body before, for A/B)
    int bound_model = SUSHI_HIP_BOUND_WORST_CASE;   // (default) / SUSHI_HIP_BOUND_STATISTICAL: how the excluded side's roundings enter slb
    BoundArgs last_bounds;              // what the last bound pass of a run was launched with (sushi_hip_batch_bounds_again; valid: last_bounds_method >= 0)
    int last_bounds_method = -1;
    BoundFault fault;                   // the tests' seam (SUSHI_HIP_TEST_BOUND_FAULT; period 0, the default: none)
    // AUTO learns from its own runs (Learnt): the last run's counts come back through 16 bytes of pinned host memory behind an
    // event that is only ever QUERIED: a run never waits for an earlier one.
    unsigned long long* host_stats = nullptr;   // [2] pairs transformed, excluded pairs audited
    hipEvent_t stats_ready = nullptr;
    bool stats_pending = false;
    int32_t* packed_out = nullptr;      // NULL, or where every run ALSO leaves its results as 8-byte (index, score bits) records
    int32_t* early_out = nullptr;       // NULL, or sushi_hip_batch_set_early_output's 16-byte records (memory host and device both touch)
    // what it holds about its requests (batch_core.hpp): `now` is what runs; the next requests are staged into `spare`, and the two
    // change places once nothing can refuse them any more (plan_and_upload)
    BatchPlanState states[2];
    BatchPlanState *now = &states[0], *spare = &states[1];
    bool planned = false;               // false: a plan was taken but its upload failed -- no run until a reset succeeds
    size_t mem_bytes = 0, ws_cap = 0;   // what the caller gave: a re-plan (sushi_hip_batch_reset) must fit it
    char* mem = nullptr;
    hipStream_t last_stream = nullptr;
    hipEvent_t uploaded = nullptr;      // recorded on the create-time stream behind the descriptor / plan uploads
    // lanes (plan_core.hpp): lane 0 is the stream a run is given; the others are the batch's own, forked off it behind the
    // run's first launch and joined before its last
    hipStream_t lane_stream[MAX_LANES] = {};
    hipEvent_t lane_done[MAX_LANES] = {};
    hipEvent_t fork = nullptr;
    // sushi_hip_batch_workspace_view(WS_TSPEC) over half rows: the whole-row copy it hands out, made at the first request
    void* tspec_whole = nullptr;
    size_t tspec_whole_bytes = 0;
    void forget_learnt() { learnt.forget(); last = LastRun(); }
    ~SushiHipBatch() {
        for (int l = 1; l < MAX_LANES; ++l) {
            if (lane_stream[l]) (void)hipStreamSynchronize(lane_stream[l]);          // (the pool's: this batch's work on it has to be through)
            if (lane_done[l]) (void)hipEventDestroy(lane_done[l]);
        }
        if (fork) (void)hipEventDestroy(fork);
        if (uploaded) { (void)hipEventSynchronize(uploaded); (void)hipEventDestroy(uploaded); }    // (an upload may still read the handle's host buffers)
        if (stats_pending && stats_ready) (void)hipEventSynchronize(stats_ready);       // the last run's counts may still be on their way
        if (stats_ready) (void)hipEventDestroy(stats_ready);
        g_host_slots.give(host_stats);
        if (tspec_whole) (void)hipFree(tspec_whole);
    }
};

static SubView last_sub(const SushiHipBatch* b) {                // (of the last run)
    const std::vector<SubBatch>& subs = b->last.whole_cut ? b->now->plan.subs_whole : b->now->plan.subs;
    return SubView(b->mem, b->now->lay, b->now->plan.ws_lane, subs.back(), subs.size() - 1);
}

// What the stages of one run read besides their sub-batch: the batch, its streams and device memory, the run's own settings.
struct RunCtx {
    SushiHipBatch* b;
    const SushiHipStream *dst, *src;
    StreamRefs r;
    const SearchDesc* searches;         // every search of the batch
    unsigned long long *keys, *gkeys;   // [searches] each: result keys, running thresholds
    int *flags, *flag_list, *viol;
    RunCounters* counters;
    double delta;
    int method, lanes = 1;
    unsigned run_seq = 0;
    ProfCall* pc = nullptr;
    bool suspended = false, cand_filled = false, excluded_any = false;     // (cand_filled: the run's first launch cleared the candidate rows)
    RunCtx(SushiHipBatch* bb, double d) : b(bb), dst(bb->dst), src(bb->src), delta(d), method(bb->method) {
        r = StreamRefs{dst->xc, dst->s1, dst->s2, dst->n, src->xc, src->s1, src->s2, src->n, sushi_hip_centre(dst->dtype), dst->raw, src->raw,
                       dst->dtype};
        searches = (const SearchDesc*)(b->mem + b->now->lay.desc); keys = (unsigned long long*)(b->mem + b->now->lay.keys); gkeys = keys + b->n;
        flags = (int*)(b->mem + b->now->lay.flags); flag_list = (int*)(b->mem + b->now->lay.flag_list); viol = (int*)(b->mem + b->now->lay.viol);
        counters = (RunCounters*)(b->mem + b->now->lay.counters);
    }
};

// The lanes of one run: the batch's own streams start behind the run's first launches; join() puts the stream the run was given
// behind them again, and the destructor does so on every exit before that.
struct Lanes {
    SushiHipBatch* b;
    hipStream_t st[MAX_LANES];
    int forked = 1;                     // lanes 1 .. forked - 1 wait for the fork
    Lanes(SushiHipBatch* bb, hipStream_t st0) : b(bb) { for (hipStream_t& s : st) s = st0; }
    ~Lanes() { (void)join(); }
    int fork(int lanes) {
        if (lanes < 2) return SUSHI_HIP_OK;
        if ((!b->fork && hipEventCreateWithFlags(&b->fork, hipEventDisableTiming) != hipSuccess) || hipEventRecord(b->fork, st[0]) != hipSuccess)
            return SUSHI_HIP_ELAUNCH;
        for (int l = 1; l < lanes; ++l) {
            // (stream priorities for the lanes -- the batch's own below the caller's, above it, one of each -- and an occupancy cap on
            // mac_kernel<1024> were measured flat: 8.31 - 8.55 ms whatever the setting, tools/experiments/README.md)
            if (!b->lane_stream[l] && !(b->lane_stream[l] = g_lane_pool.get(l))) return SUSHI_HIP_ELAUNCH;
            if (!b->lane_done[l] && hipEventCreateWithFlags(&b->lane_done[l], hipEventDisableTiming) != hipSuccess) return SUSHI_HIP_ELAUNCH;
            if (hipStreamWaitEvent(b->lane_stream[l], b->fork, 0) != hipSuccess) return SUSHI_HIP_ELAUNCH;
            st[l] = b->lane_stream[l];
            forked = l + 1;
        }
        return SUSHI_HIP_OK;
    }
    int join() {
        int rc = SUSHI_HIP_OK;
        for (int l = 1; l < forked; ++l)
            if (hipEventRecord(b->lane_done[l], st[l]) != hipSuccess || hipStreamWaitEvent(st[0], b->lane_done[l], 0) != hipSuccess) rc = SUSHI_HIP_ELAUNCH;
        forked = 1;
        return rc;
    }
};

// How this run goes, from what the runs before it left: whether AUTO leaves the exclusion out, which cut of the plan it takes, on
// how many lanes.
struct RunForm { bool suspended; const std::vector<SubBatch>* subs; int lanes; };
static int run_form(SushiHipBatch* b, unsigned run_seq, hipStream_t st0, RunForm* f) {
    if (b->stats_pending && hipEventQuery(b->stats_ready) == hipSuccess) {
        b->stats_pending = false;
        absorb_counts(b->learnt, b->exclusion, run_seq, b->host_stats[0], b->host_stats[1], b->now->plan.pairs);
    }
    f->suspended = run_suspended(b->learnt, b->exclusion, run_seq);
    const bool whole_rows = whole_rows_throughout(b->learnt, b->exclusion, b->method, f->suspended);
    if (whole_rows && b->now->plan.whole_pending) {
        // the first run that wants the one-sub-batch cut makes it (host) and uploads its schedule and items behind the fill
        if (complete_whole_cut(b->now->descs, b->now->plan)) {
            for (const UploadSpan& u : whole_cut_upload(b->now->plan, b->now->lay))
                if (hipMemcpyAsync(b->mem + u.dev_off, u.host, u.bytes, hipMemcpyHostToDevice, st0) != hipSuccess) return SUSHI_HIP_ELAUNCH;
            // (the copies read the handle's own vectors: a re-plan and the destructor wait for this event before they touch them)
            if (hipEventRecord(b->uploaded, st0) != hipSuccess) return SUSHI_HIP_ELAUNCH;
        } else {
            b->now->plan.whole_pending = false;                       // (on no case of tests/host_plan_check.cpp: the room was sized for it; the parts run one after the other then)
        }
    }
    const bool whole_cut = takes_whole_cut(whole_rows, !b->now->plan.subs_whole.empty());
    f->subs = whole_cut ? &b->now->plan.subs_whole : &b->now->plan.subs;
    f->lanes = run_lanes(whole_rows, b->now->plan.lanes);
    b->last.suspended = f->suspended; b->last.whole_cut = whole_cut;
    return SUSHI_HIP_OK;
}

// One run of the FFT path around its sub-batches, whatever its kind: the handle notes what kind of run its last one was, the run's
// stream waits for the plan's upload, ONE launch clears what a run starts from (flags, violation marks, flag list, every sub-batch's
// small counters, the pattern rows' norm accumulators, the run's counters: one contiguous zero span of the batch's layout -- and
// the ranges `fa` arrives with), the run takes its sequence number, the lanes fork, every sub-batch goes through `per_sub` on its
// lane, the lanes join.  An argmin run asks run_form which cut of the plan it takes and on how many lanes; the other kinds take
// the plan's own.  Every return before the join still joins (Lanes' destructor).
static void fill_add(FillArgs& fa, void* p, size_t bytes, uint32_t v) { fa.p[fa.n] = (uint32_t*)p; fa.words[fa.n] = (uint32_t)(bytes / 4); fa.value[fa.n] = v; ++fa.n; }
// (the first two steps, which a direct-path run takes too)
static int begin_run(SushiHipBatch* b, const hipStream_t st0, const RunKind kind) {
    b->last_stream = st0;
    begin_run(b->last, kind);
    return hipStreamWaitEvent(st0, b->uploaded, 0) == hipSuccess ? SUSHI_HIP_OK : SUSHI_HIP_ELAUNCH;     // descriptors and plan have landed
}
template <class PerSub>
static int run_sub_batches(RunCtx& c, const hipStream_t st0, const RunKind kind, FillArgs fa, PerSub&& per_sub) {
    SushiHipBatch* b = c.b;
    int rc = begin_run(b, st0, kind);
    if (rc != SUSHI_HIP_OK) return rc;
    const MemSpan zeros = run_fill_span(b->now->lay);
    fill_add(fa, b->mem + zeros.off, zeros.bytes, 0u);
    if (launch_fill(fa, st0) != SUSHI_HIP_OK) return SUSHI_HIP_ELAUNCH;
    c.run_seq = b->run_seq++;
    RunForm form{false, &b->now->plan.subs, b->now->plan.lanes};
    if (kind == RUN_ARGMIN && (rc = run_form(b, c.run_seq, st0, &form)) != SUSHI_HIP_OK) return rc;
    c.suspended = form.suspended; c.lanes = form.lanes;
    Lanes lanes(b, st0);
    if ((rc = lanes.fork(form.lanes)) != SUSHI_HIP_OK) return rc;
    // Sub-batches of a plan on lanes run side by side (plan_core.hpp "Lanes"); the others one after the other.
    for (size_t si = 0; si < form.subs->size(); ++si) {
        const SubBatch& sb = (*form.subs)[si];
        if ((rc = per_sub(SubView(b->mem, b->now->lay, b->now->plan.ws_lane, sb, si), lanes.st[sb.lane])) != SUSHI_HIP_OK) return rc;
    }
    return lanes.join();
}

static int stage_tspec(const RunCtx& c, const SubView& v, hipStream_t st) {
    hipEvent_t t0 = prof_begin(c.pc, st);
    TspecArgs ta;
    ta.src_raw = c.src->raw; ta.searches = c.searches + v.sb.a0; ta.n_sub = v.n_sub; ta.sub_first_seg = v.sb.first_seg;
    ta.tspec = v.tspec; ta.sub_first_pair = v.sb.first_pair; ta.pairmap = v.pairmap; ta.tconst = v.tconst;
    ta.src_s1 = c.src->s1; ta.src_s2 = c.src->s2; ta.centre = c.r.centre; ta.dst_stats = c.dst->stats; ta.method = c.method;
    ta.tspec_low = v.tspec_low; ta.tnorm_rest = v.tnorm_rest;
    const bool real = tspec_real(c.b->tspec);
    if (launch_dtype(c.src->dtype, [&](auto t) {
            typedef std::remove_pointer_t<decltype(t)> S;
            if (real) hipLaunchKernelGGL(tspec_real_kernel<S>, dim3((unsigned)v.sb.segs), dim3(RT), 0, st, ta);
            else hipLaunchKernelGGL(tspec_kernel<S>, dim3((unsigned)v.sb.segs), dim3(FT), 0, st, ta); }) != SUSHI_HIP_OK)
        return SUSHI_HIP_ELAUNCH;
    prof_end(c.pc, t0, SUSHI_HIP_STAGE_TSPEC, st);
    return SUSHI_HIP_OK;
}

static BoundArgs bound_args(const RunCtx& c, const SubView& v) {
    const SushiHipStream* dst = c.dst;
    BoundArgs ba;
    memset(&ba, 0, sizeof(ba));
    ba.dst_stats = dst->stats; ba.searches = c.searches + v.sb.a0; ba.sub_first_pair = v.sb.first_pair; ba.first_search = v.sb.a0; ba.dst_len = dst->n;
    ba.pairmap = v.pairmap; ba.tconst = v.tconst; ba.ubase = dst->base; ba.sbase = dst->base1; ba.nb = dst->blocks;
    ba.coarse = dst->coarse; ba.nc = dst->nc; ba.slb = v.slb; ba.n_sub = v.n_sub; ba.n_pairs = (int)v.sb.pairs; ba.plist = v.plist;
    ba.slist = v.slist; ba.scount = v.n_slist; ba.order = v.order; ba.gkeys = c.gkeys; ba.pair_lb = v.pair_lb; ba.counters = c.counters; ba.acc = v.acc;
    ba.sub_first_seg = v.sb.first_seg; ba.tnorm_rest = v.tnorm_rest; ba.znorm_rest = dst->znorm_rest; ba.norm_stride = dst->norm_stride;
    ba.band_votes = v.votes; ba.audit_mark = v.audit_mark; ba.audit_seq = c.run_seq; ba.audit_every = c.b->audit_every;
    // What a packed-half transform output (bound_low_kernel / bound_kernel) may be off by, in units of the largest pass-1 value:
    // every output is a sum of 64 pass-1 values through ROUNDING LEVELS of 2^-11 each -- a level at which the partial sums hold m
    // terms each costs 2^-11 m per value and 64 / m values meet in an output: 2^-11 64 per level whatever m.  Worst path: pass 1's
    // own result 1, its half-precision matrix (2^-12 sqrt 2 per entry, sum |inputs| <= 4 max |output| by Parseval) 2.8, pass 2's
    // twiddle 2 + its radix-16 butterflies 1 + 1 + 2 + 3 (h_bfly_root32: q = 0 / 8 one rounding, 4 / 12 two, others three on the
    // e - w o side), pass 3's twiddle 2 + radix 4: 1 + 1, four levels of half-precision twiddle constants at 2^-12 each = 2:
    // 18.8 levels = 0.59.  (Round 5's 0.29 counted 9: about right for independent roundings, not a worst case.)
    ba.worst_case = c.b->bound_model == SUSHI_HIP_BOUND_WORST_CASE ? 1 : 0;
    ba.half_err = ba.worst_case ? 0.6f : 0.29f;
    return ba;
}

static int launch_slb(const RunCtx& c, const SubView& v, const BoundArgs& x, hipStream_t st) {
    // (a workgroup is four waves: of four pairs each, or of one)
    constexpr int per_group = 4 * (64 / SLB_GROUP);
    return launch_method(c.method, [&](auto m) {
        if (slb_by_wave(c.b->slb)) hipLaunchKernelGGL(slb_wave_kernel<decltype(m)::value>, dim3((unsigned)((v.sb.pairs + 3) / 4)), dim3(256), 0, st, x);
        else hipLaunchKernelGGL(slb_kernel<decltype(m)::value>, dim3((unsigned)((v.sb.pairs + per_group - 1) / per_group)), dim3(256), 0, st, x); });
}

// the tests' seam: the stored bounds of the batch's faulted pairs read +inf from here on (bound_fault_kernel); called behind every
// launch that writes slb, and only by a batch that carries a fault
static int launch_bound_fault(const RunCtx& c, const SubView& v, hipStream_t st) {
    BoundFaultArgs fa;
    fa.searches = c.searches + v.sb.a0; fa.pairmap = v.pairmap; fa.slb = v.slb; fa.first_search = v.sb.a0;
    fa.sub_first_pair = v.sb.first_pair; fa.n_pairs = (int)v.sb.pairs; fa.f = c.b->fault;
    hipLaunchKernelGGL(bound_fault_kernel, dim3((unsigned)((v.sb.pairs + 255) / 256)), dim3(256), 0, st, fa);
    return launch_ok();
}

// Which form of the exclusion: the band-split form multiplies, stores and transforms only the low band of
// every spectrum and bounds the rest by the rows' norms -- a quarter of the bytes and a third of the instructions, IF the
// streams keep most of their energy in the band (audio does; white noise does not).  Decided once per batch and method, on
// the device's own numbers: with nothing at all from the low band, does the rest alone leave the bound room to exclude?
// (One small kernel over the first excluded sub-batch's pairs and one 8 KB read-back, in the first run only: the one place a run
// waits for the device.)
static int decide_band(const RunCtx& c, const SubView& v, hipStream_t st, int* band) {
    SushiHipBatch* b = c.b;
    if (vote_due(b->learnt, b->exclusion, b->method)) {
        int slots[VOTE_SLOTS * VOTE_STRIDE];
        if (hipMemsetAsync(v.votes, 0, sizeof(slots), st) != hipSuccess) return SUSHI_HIP_ELAUNCH;
        BoundArgs bp = bound_args(c, v);
        bp.band = 2;
        if (launch_slb(c, v, bp, st) != SUSHI_HIP_OK) return SUSHI_HIP_ELAUNCH;
        if (hipMemcpyAsync(slots, v.votes, sizeof(slots), hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
            return SUSHI_HIP_ELAUNCH;
        int looked_at = 0, with_room = 0;
        for (int k = 0; k < VOTE_SLOTS; ++k) { looked_at += slots[k * VOTE_STRIDE]; with_room += slots[k * VOTE_STRIDE + 1]; }
        decide_form(b->learnt, b->method, looked_at, with_room);
    }
    *band = b->last.band = exclusion_form(b->learnt, b->exclusion);
    return SUSHI_HIP_OK;
}

// the multiply-accumulate over ALL pairs: of the low rows (band-split form) or of whole rows; `enable`: a device flag that
// may call the launch off (the whole-row launch queued behind the survivors' list, exclude_pairs)
static int launch_mac(const RunCtx& c, const SubView& v, hipStream_t st, const bool low, const int* enable, const int32_t* items_of_the_launch) {
    const SubBatch& sb = v.sb;
    MacArgs ma;
    ma.spec_blocks = c.dst->blocks; ma.searches = c.searches + sb.a0; ma.tconst = v.tconst; ma.sub_first_seg = sb.first_seg;
    ma.sub_first_pair = sb.first_pair; ma.dummy = v.dummy; ma.enable = enable;
    if (low) { ma.spec = (const uint4*)c.dst->spec_low; ma.tspec = v.tspec_low; ma.y = v.ylow; }
    else { ma.spec = (const uint4*)c.dst->spec; ma.tspec = (const uint4*)v.tspec; ma.y = v.y; }
    ma.tspec_half = !low && tspec_half_rows(c.b->tspec) ? 1 : 0;
    for (int kern = 0; kern < 2; ++kern) {
        if (sb.item_count[kern] == 0) continue;
        ma.items = items_of_the_launch + (size_t)(sb.item_first[kern] - sb.item_first[0]) * (1 + MAC_SPW);
        ma.n_items = sb.item_count[kern];
        const int chunks = (low ? LROWE : ROWE) / MAC_BW;
        ma.chunk_group = std::min(sb.chunk_group[kern], chunks / 8);
        const dim3 grid((unsigned)chunks * (unsigned)ma.n_items);
        auto go = [&](auto row) {
            if (kern == 0) hipLaunchKernelGGL(mac_kernel<decltype(row)::value>, grid, dim3(MAC_THREADS), 0, st, ma);
            else hipLaunchKernelGGL(mac_long_kernel<decltype(row)::value>, grid, dim3(MAC_THREADS), 0, st, ma);
        };
        if (low) go(std::integral_constant<int, LROWE>()); else go(std::integral_constant<int, ROWE>());
        if (launch_ok() != SUSHI_HIP_OK) return SUSHI_HIP_ELAUNCH;
    }
    return SUSHI_HIP_OK;
}

// the whole rows of LISTED pairs (band-split form: nothing but the low band exists until a pair is to be transformed)
static int launch_mac_list(const RunCtx& c, const SubView& v, hipStream_t st, const int* list, const int* count, int n_list,
                           const int* dense_search, int long_only) {
    MacListArgs la;
    la.dense_search = dense_search; la.long_only = long_only;
    la.spec = (const uint4*)c.dst->spec; la.spec_blocks = c.dst->blocks; la.tspec = (const uint4*)v.tspec; la.tspec_half = tspec_half_rows(c.b->tspec) ? 1 : 0; la.y = v.y;
    la.searches = c.searches + v.sb.a0; la.tconst = v.tconst; la.pairmap = v.pairmap; la.list = list; la.count = count;
    la.n_list = n_list; la.sub_first_seg = v.sb.first_seg; la.sub_first_pair = v.sb.first_pair;
    const int64_t want = (int64_t)n_list * MACL_PARTS;
    hipLaunchKernelGGL(mac_list_kernel, dim3((unsigned)std::min<int64_t>(want, 256 * 32)), dim3(MACL_THREADS), 0, st, la);
    return launch_ok();
}

// ... search by search, for the patterns of up to MAC_SMAX_LONG segments (header of MacRowsArgs; `mode`: which pairs of a search)
static int launch_mac_rows(const RunCtx& c, const SubView& v, hipStream_t st, const BoundArgs& ba, const int mode) {
    const SubBatch& sb = v.sb;
    MacRowsArgs ra;
    ra.spec = (const uint4*)c.dst->spec; ra.spec_blocks = c.dst->blocks; ra.tspec = (const uint4*)v.tspec; ra.tspec_half = tspec_half_rows(c.b->tspec) ? 1 : 0; ra.y = v.y;
    ra.searches = c.searches + sb.a0; ra.tconst = v.tconst; ra.mark = ba.audit_mark; ra.n_sub = v.n_sub;
    ra.sub_first_seg = sb.first_seg; ra.sub_first_pair = sb.first_pair; ra.dense_search = v.dense_search;
    ra.plist = ba.plist; ra.first_search = ba.first_search; ra.audit_seq = ba.audit_seq; ra.audit_every = ba.audit_every;
    ra.items = v.slist; ra.item_count = v.n_rest_items; ra.pairmap = v.pairmap; ra.n_pairs = (int)sb.pairs;
    // (ROWS_ITEMS: how many items there are only the device knows -- at most one per pair; a fixed grid strides over them)
    // (ROWS_FIRST over half rows: half as many workgroups a search, each forming two entries a thread)
    const int64_t rows_want = (int64_t)(mode == ROWS_ITEMS ? sb.pairs : v.n_sub) * (mode == ROWS_FIRST && ra.tspec_half ? MACL_PARTS / 2 : MACL_PARTS);
    const dim3 grid0((unsigned)std::min<int64_t>(rows_want, 256 * 32)), grid1((unsigned)std::min<int64_t>(rows_want, 256 * 16));
    auto go = [&](auto m) {
        if (sb.item_count[0] > 0) hipLaunchKernelGGL((mac_rows_kernel<0, decltype(m)::value>), grid0, dim3(MACL_THREADS), 0, st, ra);
        if (sb.item_count[1] > 0) hipLaunchKernelGGL((mac_rows_kernel<1, decltype(m)::value>), grid1, dim3(MACL_THREADS), 0, st, ra);
    };
    if (mode == ROWS_FIRST) go(std::integral_constant<int, ROWS_FIRST>());
    else if (mode == ROWS_REST) go(std::integral_constant<int, ROWS_REST>());
    else if (mode == ROWS_ITEMS) go(std::integral_constant<int, ROWS_ITEMS>());
    else go(std::integral_constant<int, ROWS_MARKED>());
    return launch_ok();
}

static int launch_ifft(const RunCtx& c, const IfftArgs& x, unsigned grid, hipStream_t st) {
    const bool strided = x.count && !x.list_direct;                   // a list whose length only the device knows: a fixed grid strides over its tail
    return launch_method(c.method, [&](auto m) {
        if (strided) hipLaunchKernelGGL(ifft_list_kernel<decltype(m)::value>, dim3(grid), dim3(FT), 0, st, x);
        else hipLaunchKernelGGL(ifft_kernel<decltype(m)::value>, dim3(grid), dim3(FT), 0, st, x);
    });
}

// the lower bound of every pair's scores (slb)
static int bound_pairs(const RunCtx& c, const SubView& v, hipStream_t st, const int band, BoundArgs& ba) {
    const SubBatch& sb = v.sb;
    ba = bound_args(c, v);
    ba.band = band;
    ba.y = band ? (const uint2*)v.ylow : (const uint2*)v.y;
    // (bound_kernel adds to the pairs' accumulators; bound_low_kernel -- a wave per pair -- stores them)
    if (!band && hipMemsetAsync(ba.acc, 0, (size_t)sb.pairs * 2 * sizeof(float), st) != hipSuccess) return SUSHI_HIP_ELAUNCH;
    // waves striding over the pairs: a small multiple of what is resident at the kernel's registers (four workgroups of four
    // waves per CU, three for bound_low_kernel), fewer for a small batch.  Exactly what is resident -- persistent waves --
    // leaves the hardware nothing to balance with: bound_low_kernel alone 2.41 - 2.44 ms at BASELINE configs[2] with 1 x,
    // 2.36 with 2 x, 2.30 - 2.32 with 4 x and 8 x; next to other lanes' kernels 2 x is as good as it gets (8 x and more:
    // the per-workgroup prologue shows)
    const int per_pair = band ? 1 : 16;                  // bound_low_kernel: a wave per pair
    const int64_t want = (sb.pairs * per_pair + BOUND_THREADS / 64 - 1) / (BOUND_THREADS / 64);
    const unsigned grid = (unsigned)std::min<int64_t>(want, 256 * (band ? 3 * (c.lanes > 1 ? 2 : 4) : 4));
    // (the row energies are the statistical model's: the worst case -- the default -- does without them)
    auto go = [&](auto energies) {
        if (band) hipLaunchKernelGGL(bound_low_kernel<decltype(energies)::value>, dim3(grid), dim3(BOUND_THREADS), 0, st, ba);
        else hipLaunchKernelGGL(bound_kernel<decltype(energies)::value>, dim3(grid), dim3(BOUND_THREADS), 0, st, ba);
    };
    if (ba.worst_case) go(std::false_type()); else go(std::true_type());
    if (launch_ok() != SUSHI_HIP_OK || launch_slb(c, v, ba, st) != SUSHI_HIP_OK) return SUSHI_HIP_ELAUNCH;
    c.b->last_bounds = ba; c.b->last_bounds_method = c.method;       // (host words only: sushi_hip_batch_bounds_again)
    if (c.b->fault.period > 0) return launch_bound_fault(c, v, st);
    return SUSHI_HIP_OK;
}

// the second look at what the band-split bound left (header of bound_low_exact_kernel): sharper bound, shorter list ->
// ba.list2 / ba.list2_count
static int second_look(const RunCtx& c, const SubView& v, hipStream_t st, BoundArgs& ba) {
    ba.list = ba.slist; ba.list_count = ba.scount;
    ba.list2 = v.slist2; ba.list2_count = v.n_slist2;
    if (second_look_plain(c.b->second_look)) hipLaunchKernelGGL(bound_low_exact_plain_kernel, dim3(256 * 4), dim3(BLE_T), 0, st, ba);
    else hipLaunchKernelGGL(bound_low_exact_kernel, dim3(256 * 4), dim3(BLE_T), 0, st, ba);
    if (launch_ok() != SUSHI_HIP_OK) return SUSHI_HIP_ELAUNCH;
    if (launch_method(c.method, [&](auto m) {
            if (slb_by_wave(c.b->slb)) hipLaunchKernelGGL(slb_list_wave_kernel<decltype(m)::value>, dim3(256 * 2), dim3(256), 0, st, ba);
            else hipLaunchKernelGGL(slb_list_kernel<decltype(m)::value>, dim3(256 * 2), dim3(256), 0, st, ba); }) != SUSHI_HIP_OK)
        return SUSHI_HIP_ELAUNCH;
    // (slb_list_kernel has just redone the listed pairs' bounds: a faulted audit pair's would be sound again, and the audit blind)
    if (c.b->fault.period > 0 && launch_bound_fault(c, v, st) != SUSHI_HIP_OK) return SUSHI_HIP_ELAUNCH;
    hipLaunchKernelGGL(survivor2_kernel, dim3(256), dim3(256), 0, st, ba);
    return launch_ok();
}

// The exclusion: a lower bound of every pair's scores first (three of the transform's four passes, no scoring); then the most
// promising pair of every search, which leaves the search's threshold; then whatever the bound could not exclude (header of
// bound_kernel).  `ip` leaves with the list of those pairs, to be transformed; `t0`: the bound's profile span, ended here.
static int exclude_pairs(const RunCtx& c, const SubView& v, hipStream_t st, const int band, IfftArgs& ip, hipEvent_t& t0) {
    const SubBatch& sb = v.sb;
    BoundArgs ba;
    if (bound_pairs(c, v, st, band, ba) != SUSHI_HIP_OK) return SUSHI_HIP_ELAUNCH;
    prof_end(c.pc, t0, SUSHI_HIP_STAGE_BOUND, st);
    t0 = prof_begin(c.pc, st);
    hipLaunchKernelGGL(pilot_kernel, dim3((unsigned)v.n_sub), dim3(64), 0, st, ba);
    if (launch_ok() != SUSHI_HIP_OK) return SUSHI_HIP_ELAUNCH;
    ip.slb = ba.slb; ip.audit_mark = nullptr;              // (the pairs transformed first are nobody's excluded pairs)
    ip.order = ba.plist; ip.count = nullptr;
    // the pilots' whole rows (band-split form): search by search, each audited search's audit row in the same read of its pattern's
    // spectra (run_policy.hpp pilot_rows_by_search), and pair by pair for the patterns beyond MAC_SMAX_LONG segments -- or every pilot
    // pair by pair.  (The pair-by-pair launch is made whether or not the sub-batch holds such a pattern: without one its workgroups
    // read a descriptor each and leave, a few microseconds, and the stage's kernels -- what the recorded traffic of every bench
    // workload lists, tests/test_bench_contract.py -- are the same for every batch.)
    const bool by_search = pilot_rows_by_search(c.b->pilot_rows);
    if (band && by_search && launch_mac_rows(c, v, st, ba, ROWS_FIRST) != SUSHI_HIP_OK) return SUSHI_HIP_ELAUNCH;
    if (band && launch_mac_list(c, v, st, ba.plist, nullptr, v.n_sub, nullptr, by_search ? 1 : 0) != SUSHI_HIP_OK) return SUSHI_HIP_ELAUNCH;
    if (launch_ifft(c, ip, (unsigned)v.n_sub, st) != SUSHI_HIP_OK) return SUSHI_HIP_ELAUNCH;
    hipLaunchKernelGGL(survivor_kernel, dim3((unsigned)((sb.pairs + SURVIVOR_THREADS - 1) / SURVIVOR_THREADS)), dim3(SURVIVOR_THREADS), 0, st, ba);
    if (launch_ok() != SUSHI_HIP_OK) return SUSHI_HIP_ELAUNCH;
    ip.order = ba.slist; ip.count = ba.scount; ip.audit_mark = ba.audit_mark;
    if (!band) return SUSHI_HIP_OK;
    // the second look at what the bound left
    if (second_look(c, v, st, ba) != SUSHI_HIP_OK) return SUSHI_HIP_ELAUNCH;
    ip.order = ba.list2; ip.count = ba.list2_count;
    // whole rows of what is left: pair by pair for the searches that left few (the usual case), by the dense
    // multiply-accumulate for the searches the bound could exclude little of (no match anywhere) -- decided per search and
    // regrouped into items of their own, on the device (dense_search_kernel, dense_repack_kernel)
    // (... and, for the survivors' pass by items, each search's pairs to form cut into that pass's work items: slist is dead behind
    // the second look, the count word zero since the run's first launch)
    const bool by_item = by_search && rest_rows_by_item(c.b->rest_rows);
    hipLaunchKernelGGL(dense_search_kernel, dim3((unsigned)v.n_sub), dim3(64), 0, st, ba, v.dense_search, v.n_dense_listed,
                       by_item ? v.slist : nullptr, v.n_rest_items);
    const size_t second = (size_t)(sb.item_first[1] - sb.item_first[0]) * (1 + MAC_SPW);
    hipLaunchKernelGGL(dense_repack_kernel, dim3(2), dim3(REPACK_THREADS), 0, st, v.items, sb.item_count[0], v.items + second,
                       sb.item_count[1], v.dense_search, v.n_sub, v.ditems, v.ditems + second, v.n_dense_listed, (int)(sb.pairs / 8),
                       v.any_dense);                             // (zero since the run's first launch)
    if (launch_ok() != SUSHI_HIP_OK) return SUSHI_HIP_ELAUNCH;
    // (what the pilots' pass formed beside the pilot is not formed again, and a search with nothing left is not read at all)
    if (launch_mac_rows(c, v, st, ba, by_item ? ROWS_ITEMS : by_search ? ROWS_REST : ROWS_MARKED) != SUSHI_HIP_OK) return SUSHI_HIP_ELAUNCH;
    if (sb.long_patterns && launch_mac_list(c, v, st, ba.list2, ba.list2_count, (int)sb.pairs, v.dense_search, 1) != SUSHI_HIP_OK) return SUSHI_HIP_ELAUNCH;
    return launch_mac(c, v, st, false, v.any_dense, v.ditems);
}

// the transform of the listed pairs
static int transform_listed(const RunCtx& c, const SubView& v, hipStream_t st, IfftArgs ip) {
    const SubBatch& sb = v.sb;
    const SushiHipBatch* b = c.b;
    // one workgroup per list slot up to `direct`, a fixed grid striding over whatever lies beyond (run_policy.hpp direct_slots)
    const unsigned direct = (unsigned)direct_slots(b->learnt.last_transformed, sb.pairs, b->now->plan.pairs);
    ip.list_first = 0; ip.list_direct = 1;
    if (launch_ifft(c, ip, direct, st) != SUSHI_HIP_OK) return SUSHI_HIP_ELAUNCH;
    if ((int64_t)direct >= sb.pairs) return SUSHI_HIP_OK;
    ip.list_first = (int)direct; ip.list_direct = 0;
    return launch_ifft(c, ip, (unsigned)std::min<int64_t>(sb.pairs - direct, 1024), st);
}

static int stage_refine(const RunCtx& c, const SubView& v, hipStream_t st) {
    hipEvent_t t0 = prof_begin(c.pc, st);
    RefineParams rp;
    rp.r = c.r; rp.searches = c.searches; rp.first_search = v.sb.a0; rp.n_sub = v.n_sub; rp.sub_first_pair = v.sb.first_pair;
    rp.cand = v.cand; rp.pair_lb = v.pair_lb; rp.gkeys = c.gkeys; rp.keys = c.keys; rp.flags = c.flags; rp.flag_list = c.flag_list + v.sb.a0;
    rp.sub = v.sub; rp.counters = c.counters; rp.delta = (float)c.delta; rp.method = c.method; rp.citems = v.citems; rp.n_citems = v.n_citems;
    rp.viol = c.viol; rp.early = reinterpret_cast<int4*>(c.b->early_out);
    const int rc = launch_refine(rp, st);
    if (rc == SUSHI_HIP_OK) prof_end(c.pc, t0, SUSHI_HIP_STAGE_REFINE, st);
    return rc;
}

// searches the lists could not finish: collect their candidates per tile, evaluate those exactly
// (both kernels leave after one load when nothing is flagged)
static int stage_collect(const RunCtx& c, const SubView& v, hipStream_t st, IfftArgs ia) {
    hipEvent_t t0 = prof_begin(c.pc, st);
    ia.citems = v.citems; ia.n_citems = v.n_citems;    // (refine_kernel's list: RefineParams::citems)
    if (launch_method(c.method, [&](auto m) { hipLaunchKernelGGL(collect_kernel<decltype(m)::value>, dim3(COLLECT_GRID), dim3(FT), 0, st, ia); }) !=
        SUSHI_HIP_OK)
        return SUSHI_HIP_ELAUNCH;
    TileParams tp;
    tp.r = c.r; tp.searches = c.searches; tp.tiles = v.tiles; tp.cand = v.candbuf; tp.keys = c.keys; tp.counters = c.counters; tp.sub = v.sub; tp.method = c.method;
    const int rc = launch_tiles(tp, st);
    if (rc == SUSHI_HIP_OK) prof_end(c.pc, t0, SUSHI_HIP_STAGE_FINISH, st);
    return rc;
}

// One sub-batch, its stages in order on stream `st` (the header of this file).
static int run_sub(RunCtx& c, const SubView& v, hipStream_t st) {
    SushiHipBatch* b = c.b;
    const SubBatch& sb = v.sb;
    int rc = stage_tspec(c, v, st);
    if (rc != SUSHI_HIP_OK) return rc;
    const bool exclude = sub_excludes(b->exclusion, c.suspended, sb.pairs, v.n_sub);
    c.excluded_any = c.excluded_any || exclude;
    int band = 0;
    if (exclude && (rc = decide_band(c, v, st, &band)) != SUSHI_HIP_OK) return rc;
    hipEvent_t t0 = prof_begin(c.pc, st);
    if (launch_mac(c, v, st, band != 0, nullptr, v.items) != SUSHI_HIP_OK) return SUSHI_HIP_ELAUNCH;
    prof_end(c.pc, t0, SUSHI_HIP_STAGE_MAC, st);
    t0 = prof_begin(c.pc, st);
    // the candidate rows start empty: ifft_kernel writes only the entries that exist
    if (!c.cand_filled && hipMemsetAsync(v.cand, 0xff, cand_rows_bytes(sb.pairs), st) != hipSuccess)
        return SUSHI_HIP_ELAUNCH;
    IfftArgs ia;
    memset(&ia, 0, sizeof(ia));
    ia.y = (const uint2*)v.y; ia.dst_stats = c.dst->stats; ia.searches = c.searches + sb.a0; ia.n_sub = v.n_sub; ia.first_search = sb.a0;
    ia.sub_first_pair = sb.first_pair; ia.dst_len = c.dst->n; ia.delta = (float)c.delta; ia.cand = v.cand; ia.pair_lb = v.pair_lb; ia.gkeys = c.gkeys;
    ia.pairmap = v.pairmap; ia.tconst = v.tconst; ia.order = v.order; ia.urel = c.dst->urel; ia.nb = c.dst->blocks; ia.ubase = c.dst->base;
    ia.usrel = c.dst->usrel; ia.sbase = c.dst->base1; ia.flags = c.flags; ia.flag_list = c.flag_list + sb.a0; ia.sub = v.sub;
    ia.tiles = v.tiles; ia.candbuf = v.candbuf; ia.cand_cap = (int)cand_capacity(sb.pairs); ia.counters = c.counters; ia.viol = c.viol;
    if (!exclude) {
        // every pair, in the L2-friendly schedule (what round 3 did for every batch)
        if (launch_ifft(c, ia, (unsigned)sb.pairs, st) != SUSHI_HIP_OK) return SUSHI_HIP_ELAUNCH;
        b->last.direct_pairs += sb.pairs;
    } else {
        IfftArgs ip = ia;
        if ((rc = exclude_pairs(c, v, st, band, ip, t0)) != SUSHI_HIP_OK || (rc = transform_listed(c, v, st, ip)) != SUSHI_HIP_OK) return rc;
    }
    prof_end(c.pc, t0, SUSHI_HIP_STAGE_IFFT, st);
    if ((rc = stage_refine(c, v, st)) != SUSHI_HIP_OK) return rc;
    return stage_collect(c, v, st, ia);
}

// ---- the listed-pair runs (threshold, best-K): what their sub-batches share ----
// what the tile kernels read (sushi_curve.hip): every pair of the sub-batch in the L2-friendly schedule, until a list replaces it
static ListedPairs listed_pairs(const RunCtx& c, const SubView& v) {
    ListedPairs lp;
    lp.r = c.r; lp.searches = c.searches + v.sb.a0; lp.pairmap = v.pairmap; lp.sub_first_pair = v.sb.first_pair; lp.first_search = v.sb.a0;
    lp.list = v.order; lp.list_count = nullptr; lp.list_max = (int)v.sb.pairs; lp.rows = (uint32_t*)v.y; lp.method = c.method;
    return lp;
}

// ... and the runs' own kernels (sushi_fft_threshold.inc, sushi_fft_best.inc): `a` arrives zeroed
static void pair_run_args(const RunCtx& c, const SubView& v, PairRunArgs& a) {
    a.searches = c.searches + v.sb.a0; a.first_search = v.sb.a0; a.sub_first_pair = v.sb.first_pair; a.n_sub = v.n_sub; a.n_pairs = (int)v.sb.pairs;
    a.pairmap = v.pairmap; a.rows = (const uint32_t*)v.y; a.slb = v.slb; a.audit_mark = v.audit_mark; a.viol = c.viol;
    a.counters = c.counters; a.method = c.method;
}

// the lower bound of every pair: the form of the exclusion, the multiply-accumulate that form needs, the bound (run_sub does the
// same between its profile spans)
static int mac_and_bound(const RunCtx& c, const SubView& v, hipStream_t st, int* band, BoundArgs& ba) {
    const int rc = decide_band(c, v, st, band);
    if (rc != SUSHI_HIP_OK) return rc;
    if (launch_mac(c, v, st, *band != 0, nullptr, v.items) != SUSHI_HIP_OK) return SUSHI_HIP_ELAUNCH;
    return bound_pairs(c, v, st, *band, ba);
}

// What one threshold run asks for: the threshold in ranking units as a search key (survivor_kernel reads U from it), and the output.
struct ThresholdRun { double threshold; unsigned long long ukey; int32_t capacity; SushiHipHit* hits; int64_t* counts; };

// One sub-batch of a threshold run (sushi_fft_threshold.inc): the bound, the survivors of U = the threshold, every
// position of those pairs exactly, the output.  SUSHI_HIP_EXCLUDE_NEVER: every pair, no bound.
static int run_sub_threshold(RunCtx& c, const SubView& v, hipStream_t st, const ThresholdRun& tr) {
    SushiHipBatch* b = c.b;
    const SubBatch& sb = v.sb;
    const bool exclude = listed_run_excludes(b->exclusion);
    ThresholdTileParams tp;
    tp.lp = listed_pairs(c, v);
    tp.threshold = tr.threshold; tp.pass = 0; tp.hits = tr.hits; tp.capacity = tr.capacity;
    ThrArgs ta;
    memset(&ta, 0, sizeof(ta));
    pair_run_args(c, v, ta);
    ta.rows_w = (uint32_t*)v.y; ta.counts_out = tr.counts;
    if (!exclude) ta.audit_mark = nullptr;                       // (every pair is evaluated)
    // (tspec_kernel also leaves the sub-batch's pair -> search map, which every stage below reads)
    int rc = stage_tspec(c, v, st);
    if (rc != SUSHI_HIP_OK) return rc;
    if (exclude) {
        hipLaunchKernelGGL(thr_seed_kernel, dim3((unsigned)((v.n_sub + 255) / 256)), dim3(256), 0, st, c.gkeys + sb.a0, v.n_sub, tr.ukey, v.plist);
        if (launch_ok() != SUSHI_HIP_OK) return SUSHI_HIP_ELAUNCH;
        int band = 0;
        BoundArgs ba;
        if ((rc = mac_and_bound(c, v, st, &band, ba)) != SUSHI_HIP_OK) return rc;
        // (no pilot pair: every pair is listed or excluded on its bound alone; the audit of the exclusion lists one excluded pair
        // of every audited search all the same)
        hipLaunchKernelGGL(survivor_kernel, dim3((unsigned)((sb.pairs + SURVIVOR_THREADS - 1) / SURVIVOR_THREADS)), dim3(SURVIVOR_THREADS), 0, st, ba);
        if (launch_ok() != SUSHI_HIP_OK) return SUSHI_HIP_ELAUNCH;
        tp.lp.list = ba.slist; tp.lp.list_count = ba.scount;
        if (band) {
            if (second_look(c, v, st, ba) != SUSHI_HIP_OK) return SUSHI_HIP_ELAUNCH;
            tp.lp.list = ba.list2; tp.lp.list_count = ba.list2_count;
        }
        ta.list = tp.lp.list; ta.list_count = tp.lp.list_count;
        // (the first list is free once the second look has read it; the whole-row form never used the second)
        ta.list3 = band ? v.slist : v.slist2; ta.list3_count = v.n_list3;
    } else {
        b->last.direct_pairs += sb.pairs;
    }
    if (launch_threshold_tiles(tp, st) != SUSHI_HIP_OK) return SUSHI_HIP_ELAUNCH;
    ThresholdTileParams t3 = tp;
    if (exclude) {
        hipLaunchKernelGGL(thr_check_kernel, dim3((unsigned)std::min<int64_t>((sb.pairs + 255) / 256, 256)), dim3(256), 0, st, ta);
        hipLaunchKernelGGL(thr_extend_kernel, dim3((unsigned)((sb.pairs + 255) / 256)), dim3(256), 0, st, ta);
        if (launch_ok() != SUSHI_HIP_OK) return SUSHI_HIP_ELAUNCH;
        t3.lp.list = ta.list3; t3.lp.list_count = ta.list3_count;
        if (launch_threshold_tiles(t3, st) != SUSHI_HIP_OK) return SUSHI_HIP_ELAUNCH;
    }
    hipLaunchKernelGGL(thr_scan_kernel, dim3((unsigned)v.n_sub), dim3(256), 0, st, ta);
    if (launch_ok() != SUSHI_HIP_OK) return SUSHI_HIP_ELAUNCH;
    if (tr.capacity == 0) return SUSHI_HIP_OK;                   // (counts only)
    tp.pass = 1; t3.pass = 1;
    if (launch_threshold_tiles(tp, st) != SUSHI_HIP_OK) return SUSHI_HIP_ELAUNCH;
    if (exclude && launch_threshold_tiles(t3, st) != SUSHI_HIP_OK) return SUSHI_HIP_ELAUNCH;
    return SUSHI_HIP_OK;
}

// What one best-K run asks for.
struct BestRun { int k, min_separation, has_threshold; double threshold; unsigned long long tkey; SushiHipHit* hits; int32_t* counts; };

// One sub-batch of a best-K run (sushi_fft_best.inc): the bound; the pairs of smallest bound evaluated exactly and
// the K picks made from them, which leave every search's U; rounds of (pairs U does not exclude, evaluated; picks again); the
// searches still unsettled then, and the audit's, at every pair.  SUSHI_HIP_EXCLUDE_NEVER: every pair, no bound, one selection.
static int run_sub_best(RunCtx& c, const SubView& v, hipStream_t st, const BestRun& br) {
    SushiHipBatch* b = c.b;
    const SubBatch& sb = v.sb;
    const bool exclude = listed_run_excludes(b->exclusion);
    BestParams bp;
    memset(&bp, 0, sizeof(bp));
    bp.lp = listed_pairs(c, v);
    bp.n_sub = v.n_sub; bp.has_threshold = br.has_threshold; bp.threshold = br.threshold; bp.tkey = br.tkey; bp.k = br.k;
    bp.min_separation = br.min_separation; bp.gkeys = c.gkeys; bp.hits = br.hits; bp.counts = br.counts;
    // (tspec_kernel also leaves the sub-batch's pair -> search map, which every stage below reads)
    int rc = stage_tspec(c, v, st);
    if (rc != SUSHI_HIP_OK) return rc;
    if (!exclude) {
        b->last.direct_pairs += sb.pairs;
        if (launch_best_tiles(bp, st) != SUSHI_HIP_OK) return SUSHI_HIP_ELAUNCH;
        return launch_best_select(bp, st);
    }
    // (the bounds depend on no threshold: made once)
    int band = 0;
    BoundArgs ba;
    if ((rc = mac_and_bound(c, v, st, &band, ba)) != SUSHI_HIP_OK) return rc;
    BestArgs a;
    memset(&a, 0, sizeof(a));
    pair_run_args(c, v, a);
    a.k = br.k; a.order = v.order; a.gkeys = c.gkeys; a.tkey = br.tkey; a.list = v.slist; a.list_count = v.n_slist; a.flags = c.flags;
    a.need = c.flag_list; a.audit_seq = c.run_seq; a.audit_every = b->audit_every;
    // the two lists and their lengths (zero since the run's first launch; every selection clears them for the round behind it)
    bp.audit_mark = v.audit_mark; bp.stamp_flags = c.flags; bp.reset0 = v.n_slist; bp.reset1 = v.n_slist2;
    const unsigned per_pair = (unsigned)((sb.pairs + 255) / 256);
    auto evaluate = [&](const int* list, const int* count) {
        bp.lp.list = list; bp.lp.list_count = count;
        return launch_best_tiles(bp, st);
    };
    int stamp = 1;
    a.stamp = bp.stamp = stamp;
    hipLaunchKernelGGL(best_seed_kernel, dim3((unsigned)v.n_sub), dim3(256), 0, st, a);
    if (launch_ok() != SUSHI_HIP_OK) return SUSHI_HIP_ELAUNCH;
    // (band-split form, with a threshold: the second look drops the seed pairs its sharper bound excludes under the threshold, as
    // it does in a threshold run; without one there is no U yet and every seed pair is evaluated)
    const bool seed_look = band && br.has_threshold;
    if (seed_look && second_look(c, v, st, ba) != SUSHI_HIP_OK) return SUSHI_HIP_ELAUNCH;
    if (evaluate(seed_look ? v.slist2 : v.slist, seed_look ? v.n_slist2 : v.n_slist) != SUSHI_HIP_OK || launch_best_select(bp, st) != SUSHI_HIP_OK) return SUSHI_HIP_ELAUNCH;
    for (int round = 0; round < BEST_ROUNDS; ++round) {
        a.stamp = bp.stamp = ++stamp;
        hipLaunchKernelGGL(best_survivor_kernel, dim3(per_pair), dim3(256), 0, st, a);
        if (launch_ok() != SUSHI_HIP_OK) return SUSHI_HIP_ELAUNCH;
        // (band-split form: the second look at what the bound left, as in every other run)
        if (band && second_look(c, v, st, ba) != SUSHI_HIP_OK) return SUSHI_HIP_ELAUNCH;
        if (evaluate(band ? v.slist2 : v.slist, band ? v.n_slist2 : v.n_slist) != SUSHI_HIP_OK || launch_best_select(bp, st) != SUSHI_HIP_OK) return SUSHI_HIP_ELAUNCH;
    }
    a.stamp = bp.stamp = ++stamp;
    hipLaunchKernelGGL(best_final_kernel, dim3(per_pair), dim3(256), 0, st, a);
    if (launch_ok() != SUSHI_HIP_OK || evaluate(v.slist, v.n_slist) != SUSHI_HIP_OK) return SUSHI_HIP_ELAUNCH;
    hipLaunchKernelGGL(best_check_kernel, dim3(per_pair), dim3(256), 0, st, a);
    a.list = v.slist2; a.list_count = v.n_slist2;
    hipLaunchKernelGGL(best_extend_kernel, dim3(per_pair), dim3(256), 0, st, a);
    if (launch_ok() != SUSHI_HIP_OK || evaluate(v.slist2, v.n_slist2) != SUSHI_HIP_OK) return SUSHI_HIP_ELAUNCH;
    return launch_best_select(bp, st);
}

// the plan sushi_hip_batch_bytes made, for the sushi_hip_batch_create behind it (batch_core.hpp PlanCache); SUSHI_HIP_LANES is
// read once per ABI call: the planner and the cache's key get the same value
static thread_local PlanCache g_plan_cache;

// (batch_core.hpp resolve_variant; -1: refused)
static int variant_of(int path, int variant, const SushiHipRequest* req, int n) {
    int tiles[DIRECT_CHOICES];
    for (int v = 0; v < DIRECT_CHOICES; ++v) tiles[v] = direct_variant_tile(v);
    return resolve_variant(path, variant, req, n, direct_variant_count(), tiles);
}

extern "C" {

int sushi_hip_device_prepare(void) {
    for (int l = 1; l < MAX_LANES; ++l)
        if (!g_lane_pool.get(l)) return SUSHI_HIP_ELAUNCH;
    unsigned long long* p = g_host_slots.take();
    if (!p) return SUSHI_HIP_ENOMEM;
    g_host_slots.give(p);
    return SUSHI_HIP_OK;
}

int sushi_hip_fft_size(void) { return FN; }

int sushi_hip_fft_block(void) { return FFT_SEG; }

int sushi_hip_fft_slot_of_bin(int bin) { return (bin < 0 || bin >= FN) ? -1 : sushi_fft::mslot_of_bin(bin); }

int sushi_hip_fft_low_slot_of_bin(int bin) { return sushi_fft::lslot_of_bin(bin); }

size_t sushi_hip_stream_spectra_bytes(int64_t n) { return n <= 0 ? 0 : spectra_layout(n).total; }

int sushi_hip_fft_layout(int64_t win_start, int32_t n_pos, int32_t tmpl_len, int32_t* n_pairs, int32_t* n_seg) {
    if (win_start < 0 || n_pos < 1 || tmpl_len < 1 || !n_pairs || !n_seg) return SUSHI_HIP_EINVAL;
    const FftLayout l = fft_layout(win_start, n_pos, tmpl_len);
    *n_pairs = l.n_pairs;
    *n_seg = l.n_seg;
    return SUSHI_HIP_OK;
}

int sushi_hip_stream_add_spectra(SushiHipStream* s, void* mem_dev, size_t mem_bytes, void* hip_stream) {
    if (!s || !mem_dev) return SUSHI_HIP_EINVAL;
    if ((uintptr_t)mem_dev & 255) return SUSHI_HIP_EALIGN;
    const size_t need = sushi_hip_stream_spectra_bytes(s->n);
    if (mem_bytes < need) return SUSHI_HIP_ENOSPACE;
    if (s->blocks >= 0x7fffffff) return SUSHI_HIP_EINVAL;
    SushiHipStream with = *s;                                    // (the handle gets its spectra when they are on their way)
    fill_spectra(with, mem_dev, stream_layout(s->n, 0));
    if (launch_dtype(s->dtype, [&](auto t) {
            using T = std::remove_pointer_t<decltype(t)>;
            hipLaunchKernelGGL(spectra_kernel<T>, dim3((unsigned)s->blocks + 1), dim3(FT), 0, (hipStream_t)hip_stream, (const T*)s->raw, s->n,
                               (uint32_t*)with.spec, (const double*)s->stats, (uint4*)with.spec_low, with.znorm_rest, with.norm_stride); }) != SUSHI_HIP_OK)
        return SUSHI_HIP_ELAUNCH;
    *s = with;
    return SUSHI_HIP_OK;
}

size_t sushi_hip_batch_bytes(const SushiHipRequest* req_host, int n, int path, int variant, size_t workspace_cap_bytes) { return c_boundary([&]() -> size_t {
    if (!req_host || n <= 0 || (path != SUSHI_HIP_PATH_FFT && path != SUSHI_HIP_PATH_DIRECT)) return 0;
    if ((variant = variant_of(path, variant, req_host, n)) < 0) return 0;
    std::vector<SearchDesc> descs;
    int64_t tiles;
    if (make_descs(req_host, n, direct_variant_tile(variant), descs, &tiles) != SUSHI_HIP_OK) return 0;
    if (path == SUSHI_HIP_PATH_DIRECT) return batch_layout(n, path, 0, 0, 0, 0, 0).total;
    Plan plan;
    const char* lanes = getenv("SUSHI_HIP_LANES");
    if (make_plan(descs, workspace_cap_bytes, lanes, plan) != SUSHI_HIP_OK) return 0;
    const size_t total = batch_layout(n, path, plan.order.size(), plan.items.size(), plan.ws_bytes, plan.subs.size(), plan.segs).total;
    g_plan_cache.remember(req_host, n, workspace_cap_bytes, lanes, std::move(plan));
    return total;
}, 0, 0); }

// requests -> the handle's descriptors, plan, layout and upload image, uploaded on `st`.  Staged into the spare state first: every
// refusal up to the commit -- EINVAL, ENOSPACE, a plan's own, an event that cannot be made or waited for -- leaves the handle as
// it was.  Behind the commit only the copy's enqueue and the event's record are left; should one fail, the handle is not planned.
static int plan_and_upload(SushiHipBatch* b, const SushiHipRequest* req_host, int n, hipStream_t st) {
    const BatchSpec spec{b->path, direct_variant_tile(b->variant), b->ws_cap, b->mem_bytes, b->dst->n, b->src->n, b->dst->dtype == SUSHI_HIP_F32 ? 4.0 : 1.0};
    const int rc = stage_batch(req_host, n, spec, getenv("SUSHI_HIP_LANES"), g_plan_cache, *b->spare);
    if (rc != SUSHI_HIP_OK) return rc;
    // a run may be launched on another stream than `st`: it waits for this event first; and an earlier plan's upload (a run's, of
    // the whole cut) reads the handle's host buffers until the event has passed
    if (b->uploaded ? hipEventSynchronize(b->uploaded) != hipSuccess : hipEventCreateWithFlags(&b->uploaded, hipEventDisableTiming) != hipSuccess)
        return SUSHI_HIP_ELAUNCH;
    std::swap(b->now, b->spare);
    b->forget_learnt();
    b->last_bounds_method = -1;
    // (the host buffer lives in the handle: the copy may still be in flight when this returns)
    b->planned = hipMemcpyAsync(b->mem + b->now->lay.desc, b->now->upload.data(), b->now->upload.size(), hipMemcpyHostToDevice, st) == hipSuccess &&
                 hipEventRecord(b->uploaded, st) == hipSuccess;
    return b->planned ? SUSHI_HIP_OK : SUSHI_HIP_ELAUNCH;
}

int sushi_hip_batch_create(const SushiHipStream* dst, const SushiHipStream* src, const SushiHipRequest* req_host, int n,
                           int path, int variant, size_t workspace_cap_bytes, void* mem_dev, size_t mem_bytes,
                           void* hip_stream, SushiHipBatch** out) { return c_boundary([&]() -> int {
    if (!dst || !src || !req_host || !mem_dev || !out || n <= 0) return SUSHI_HIP_EINVAL;
    if (path != SUSHI_HIP_PATH_FFT && path != SUSHI_HIP_PATH_DIRECT) return SUSHI_HIP_EINVAL;
    if (dst->dtype != src->dtype) return SUSHI_HIP_EINVAL;       // cv2.matchTemplate asserts equal types
    if ((uintptr_t)mem_dev & 255) return SUSHI_HIP_EALIGN;
    if (path == SUSHI_HIP_PATH_FFT && !dst->spec) return SUSHI_HIP_EINVAL;     // not searchable: sushi_hip_stream_add_spectra first
    if ((variant = variant_of(path, variant, req_host, n)) < 0) return SUSHI_HIP_EINVAL;
    SushiHipBatch* b = new (std::nothrow) SushiHipBatch();
    if (!b) return SUSHI_HIP_ENOMEM;
    std::unique_ptr<SushiHipBatch> guard(b);                     // freed on every early return and on an exception
    b->dst = dst; b->src = src; b->n = n; b->path = path; b->variant = variant;
    b->mem = (char*)mem_dev; b->mem_bytes = mem_bytes; b->ws_cap = workspace_cap_bytes;
    // (measurements only, read once per batch: 0 = no excluded pair is audited; "statistical" = round 5's error model)
    const char* e = getenv("SUSHI_HIP_AUDIT_EVERY");
    if (e && *e) { const int v = atoi(e); b->audit_every = v < 0 ? 0 : v; }
    // (a value that is neither route is refused: a typo must not turn an A/B measurement into an A/A one)
    if ((b->pilot_rows = pilot_rows_route(getenv("SUSHI_HIP_PILOT_ROWS"))) < 0) return SUSHI_HIP_EINVAL;
    if ((b->rest_rows = rest_rows_route(getenv("SUSHI_HIP_REST_ROWS"))) < 0) return SUSHI_HIP_EINVAL;
    if ((b->tspec = tspec_route(getenv("SUSHI_HIP_TSPEC"))) < 0) return SUSHI_HIP_EINVAL;
    if ((b->slb = slb_route(getenv("SUSHI_HIP_SLB"))) < 0) return SUSHI_HIP_EINVAL;
    if ((b->second_look = second_look_route(getenv("SUSHI_HIP_SECOND_LOOK"))) < 0) return SUSHI_HIP_EINVAL;
    const char* m = getenv("SUSHI_HIP_BOUND_MODEL");
    if (m && !strcmp(m, "statistical")) b->bound_model = SUSHI_HIP_BOUND_STATISTICAL;
    // (the tests' seam, DESIGN.md 3.2: a value that does not parse is refused -- a typo must not turn a fault test into a no-fault test)
    const char* f = getenv("SUSHI_HIP_TEST_BOUND_FAULT");
    if (f && *f && !parse_bound_fault(f, &b->fault)) return SUSHI_HIP_EINVAL;
    const int rc = plan_and_upload(b, req_host, n, (hipStream_t)hip_stream);
    if (rc != SUSHI_HIP_OK) return rc;
    *out = guard.release();
    return SUSHI_HIP_OK;
}); }

int sushi_hip_batch_reset(SushiHipBatch* b, const SushiHipRequest* req_host, int n, void* hip_stream) { return c_boundary([&]() -> int {
    if (!b || !req_host || n != b->n) return SUSHI_HIP_EINVAL;
    // the last run's counts may still be on their way into the handle's pinned words
    if (b->stats_pending && b->stats_ready) { (void)hipEventSynchronize(b->stats_ready); b->stats_pending = false; }
    return plan_and_upload(b, req_host, n, (hipStream_t)hip_stream);
}); }

int sushi_hip_batch_info(const SushiHipBatch* b, SushiHipBatchInfo* info) {
    if (!b || !info) return SUSHI_HIP_EINVAL;
    memset(info, 0, sizeof(*info));
    info->n_search = b->n; info->path = b->path; info->variant = b->variant;
    info->sub_batches = b->path == SUSHI_HIP_PATH_FFT ? (int32_t)b->now->plan.subs.size() : 1;
    info->direct_tiles = b->now->n_tiles;
    info->fft_pairs = b->now->plan.pairs; info->fft_segments = b->now->plan.segs;
    info->workspace_bytes = b->now->plan.ws_bytes; info->mem_bytes = b->now->lay.total;
    info->flops = b->now->flops; info->algorithmic_bytes = b->now->algorithmic_bytes;
    info->lanes = b->path == SUSHI_HIP_PATH_FFT ? b->now->plan.lanes : 1;
    return SUSHI_HIP_OK;
}

void sushi_hip_batch_destroy(SushiHipBatch* b) { delete b; }

int sushi_hip_batch_set_method(SushiHipBatch* b, int method) {
    if (!b) return SUSHI_HIP_EINVAL;
    if (!method_known(method)) return SUSHI_HIP_EINVAL;
    b->method = method;                                          // both paths compute both methods
    return SUSHI_HIP_OK;
}

int sushi_hip_batch_set_packed_output(SushiHipBatch* b, int32_t* out_packed_dev) {
    if (!b) return SUSHI_HIP_EINVAL;
    if ((uintptr_t)out_packed_dev & 7) return SUSHI_HIP_EALIGN;
    b->packed_out = out_packed_dev;
    return SUSHI_HIP_OK;
}

int sushi_hip_batch_set_early_output(SushiHipBatch* b, int32_t* early) {
    if (!b) return SUSHI_HIP_EINVAL;
    if ((uintptr_t)early & 15) return SUSHI_HIP_EALIGN;
    b->early_out = early;
    return SUSHI_HIP_OK;
}

int sushi_hip_batch_set_exclusion(SushiHipBatch* b, int mode) {
    if (!b || mode < SUSHI_HIP_EXCLUDE_AUTO || mode > SUSHI_HIP_EXCLUDE_WHOLE) return SUSHI_HIP_EINVAL;
    b->exclusion = mode;
    return SUSHI_HIP_OK;
}

int sushi_hip_batch_set_bound_model(SushiHipBatch* b, int model) {
    if (!b || (model != SUSHI_HIP_BOUND_WORST_CASE && model != SUSHI_HIP_BOUND_STATISTICAL)) return SUSHI_HIP_EINVAL;
    b->bound_model = model;
    return SUSHI_HIP_OK;
}

int sushi_hip_batch_run(SushiHipBatch* b, double delta, int32_t* out_idx_dev, float* out_score_dev, void* hip_stream) { return c_boundary([&]() -> int {
    if (!b || !out_idx_dev || !out_score_dev || !b->planned) return SUSHI_HIP_EINVAL;
    const hipStream_t st0 = (hipStream_t)hip_stream;
    RunCtx c(b, delta);
    if (b->path == SUSHI_HIP_PATH_DIRECT) {
        if (begin_run(b, st0, RUN_ARGMIN) != SUSHI_HIP_OK) return SUSHI_HIP_ELAUNCH;
        return launch_direct(c.r, c.searches, b->n, (int)b->now->n_tiles, b->variant, b->method, c.keys, out_idx_dev, out_score_dev, b->packed_out, st0);
    }
    if (!(delta >= 3.8e-6) || delta > 1.0) return SUSHI_HIP_EINVAL;      // the floor covers the scoring arithmetic's own rounding
    if (g_prof_on) { g_prof.emplace_back(); c.pc = &g_prof.back(); }
    // What an argmin run clears besides: the result keys (all ones) and -- a batch of one sub-batch, while they are small -- its
    // candidate rows.
    FillArgs fa{};
    fill_add(fa, c.keys, (size_t)2 * b->n * sizeof(uint64_t), 0xffffffffu);
    if ((c.cand_filled = fills_candidate_rows(b->now->plan))) {
        const SubView v0(b->mem, b->now->lay, b->now->plan.ws_lane, b->now->plan.subs[0], 0);
        fill_add(fa, v0.cand, cand_rows_bytes(v0.sb.pairs), 0xffffffffu);
    }
    int rc = run_sub_batches(c, st0, RUN_ARGMIN, fa, [&](const SubView& v, hipStream_t st) { return run_sub(c, v, st); });
    if (rc != SUSHI_HIP_OK) return rc;
    hipEvent_t t0 = prof_begin(c.pc, st0);
    rc = launch_unpack(c.keys, b->n, b->method, out_idx_dev, out_score_dev, b->packed_out, st0);
    prof_end(c.pc, t0, SUSHI_HIP_STAGE_FINISH, st0);
    if (rc == SUSHI_HIP_OK && c.excluded_any && !b->stats_pending) {
        // what this run's exclusion left, for the runs after it (never waited for: the event is queried)
        if (!b->host_stats) b->host_stats = g_host_slots.take();                 // (none left: this batch's AUTO does not learn)
        if (b->host_stats && !b->stats_ready && hipEventCreateWithFlags(&b->stats_ready, hipEventDisableTiming) != hipSuccess) b->stats_ready = nullptr;
        if (b->host_stats && b->stats_ready &&
            hipMemcpyAsync(b->host_stats, &c.counters->pairs_transformed, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, st0) == hipSuccess &&
            hipEventRecord(b->stats_ready, st0) == hipSuccess)
            b->stats_pending = true;
    }
    return rc;
}); }

int sushi_hip_batch_run_threshold(SushiHipBatch* b, double threshold, int32_t capacity, SushiHipHit* out_hits_dev, int64_t* out_counts_dev,
                                  void* hip_stream) { return c_boundary([&]() -> int {
    if (!b || !out_hits_dev || !out_counts_dev || capacity < 0 || !std::isfinite(threshold) || b->path != SUSHI_HIP_PATH_FFT || !b->planned)
        return SUSHI_HIP_EINVAL;
    if (((uintptr_t)out_hits_dev & 3) || ((uintptr_t)out_counts_dev & 7)) return SUSHI_HIP_EALIGN;
    const ThresholdRun tr{threshold, ranking_key(b->method, threshold, false), capacity, out_hits_dev, out_counts_dev};
    RunCtx c(b, 0.0);
    return run_sub_batches(c, (hipStream_t)hip_stream, RUN_THRESHOLD, FillArgs{},
                           [&](const SubView& v, hipStream_t st) { return run_sub_threshold(c, v, st, tr); });
}); }

int sushi_hip_batch_run_best(SushiHipBatch* b, int32_t k, int32_t min_separation, const double* threshold, SushiHipHit* out_hits_dev,
                             int32_t* out_counts_dev, void* hip_stream) { return c_boundary([&]() -> int {
    if (!b || !out_hits_dev || !out_counts_dev || k < 1 || k > SUSHI_HIP_BEST_MAX_K || min_separation < 0 ||
        (threshold && !std::isfinite(*threshold)) || b->path != SUSHI_HIP_PATH_FFT || !b->planned)
        return SUSHI_HIP_EINVAL;
    if (((uintptr_t)out_hits_dev & 3) || ((uintptr_t)out_counts_dev & 3)) return SUSHI_HIP_EALIGN;
    // (the threshold's key never below 0, unlike a threshold run's: ranking_key)
    const BestRun br{k, min_separation, threshold ? 1 : 0, threshold ? *threshold : 0.0,
                     threshold ? ranking_key(b->method, *threshold, true) : NO_KEY, out_hits_dev, out_counts_dev};
    RunCtx c(b, 0.0);
    return run_sub_batches(c, (hipStream_t)hip_stream, RUN_BEST, FillArgs{},
                           [&](const SubView& v, hipStream_t st) { return run_sub_best(c, v, st, br); });
}); }

int sushi_hip_batch_diagnostics(SushiHipBatch* b, SushiHipBatchDiag* diag, float* ranking_err_host, int32_t* flagged_host) { return c_boundary([&]() -> int {
    if (!b || !diag) return SUSHI_HIP_EINVAL;
    memset(diag, 0, sizeof(*diag));
    if (!b->last.ran || b->path != SUSHI_HIP_PATH_FFT) {
        if (ranking_err_host) memset(ranking_err_host, 0, (size_t)b->n * sizeof(float));
        if (flagged_host) memset(flagged_host, 0, (size_t)b->n * sizeof(int32_t));
        return SUSHI_HIP_OK;
    }
    if (hipStreamSynchronize(b->last_stream) != hipSuccess) return SUSHI_HIP_ELAUNCH;
    RunCounters c;
    if (hipMemcpy(&c, b->mem + b->now->lay.counters, sizeof(c), hipMemcpyDeviceToHost) != hipSuccess) return SUSHI_HIP_ELAUNCH;
    diag->flagged = c.n_flagged; diag->all_positions = c.n_all_positions;
    diag->tiles_dense = (int64_t)c.tiles_dense; diag->tiles_sparse = (int64_t)c.tiles_sparse;
    diag->candidates = (int64_t)c.candidates;
    memcpy(&diag->max_bound_ratio, &c.max_ratio_bits, sizeof(float));
    memcpy(&diag->max_bound_ratio_noncandidate, &c.max_ratio_audit_bits, sizeof(float));
    diag->audited = (int64_t)c.audited;
    diag->excluded_audited = (int64_t)c.excluded_audited;
    memcpy(&diag->max_slb_ratio_excluded, &c.max_slb_ratio_bits, sizeof(float));
    diag->slb_violations = c.slb_violations;
    report_last_run(b->last, b->learnt, c, diag);
    if (b->last.kind != RUN_ARGMIN) {
        // (a threshold or best-K run: the bound's figures only -- its exact stage is not the search's)
        if (ranking_err_host) memset(ranking_err_host, 0, (size_t)b->n * sizeof(float));
        if (flagged_host) memset(flagged_host, 0, (size_t)b->n * sizeof(int32_t));
        // (a best-K run: the last round that evaluated a pair of each search -- 1 the seed, 2 .. the escalation rounds, BEST_ROUNDS + 2
        // the last stage; 0 without the exclusion)
        if (b->last.kind == RUN_BEST && flagged_host &&
            hipMemcpy(flagged_host, b->mem + b->now->lay.flags, (size_t)b->n * sizeof(int32_t), hipMemcpyDeviceToHost) != hipSuccess)
            return SUSHI_HIP_ELAUNCH;
        return SUSHI_HIP_OK;
    }
    std::vector<int32_t> fl((size_t)b->n);
    if (hipMemcpy(fl.data(), b->mem + b->now->lay.flags, (size_t)b->n * sizeof(int32_t), hipMemcpyDeviceToHost) != hipSuccess)
        return SUSHI_HIP_ELAUNCH;
    if (flagged_host) memcpy(flagged_host, fl.data(), (size_t)b->n * sizeof(int32_t));
    if (ranking_err_host) {
        std::vector<unsigned long long> g((size_t)b->n);
        if (hipMemcpy(g.data(), b->mem + b->now->lay.keys + (size_t)b->n * sizeof(unsigned long long),
                      (size_t)b->n * sizeof(unsigned long long), hipMemcpyDeviceToHost) != hipSuccess)
            return SUSHI_HIP_ELAUNCH;
        for (int k = 0; k < b->n; ++k) {
            const uint32_t bits = fl[k] ? 0u : (uint32_t)(g[k] & 0xffffffffull);     // flagged searches keep their threshold there
            memcpy(&ranking_err_host[k], &bits, sizeof(float));
        }
    }
    return SUSHI_HIP_OK;
}); }

int sushi_hip_batch_pair_bounds(SushiHipBatch* b, float* slb_host, float* acc_host, int64_t* n_pairs) { return c_boundary([&]() -> int {
    if (!b || !n_pairs) return SUSHI_HIP_EINVAL;
    if (!b->last.ran || b->path != SUSHI_HIP_PATH_FFT || b->now->plan.subs.empty()) { *n_pairs = 0; return SUSHI_HIP_OK; }
    if (hipStreamSynchronize(b->last_stream) != hipSuccess) return SUSHI_HIP_ELAUNCH;
    const SubView v = last_sub(b);
    const int64_t cap = *n_pairs;
    *n_pairs = v.sb.pairs;
    if (cap < v.sb.pairs) return SUSHI_HIP_ENOSPACE;
    if (slb_host && hipMemcpy(slb_host, v.slb, (size_t)v.sb.pairs * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess) return SUSHI_HIP_ELAUNCH;
    if (acc_host && hipMemcpy(acc_host, v.acc, (size_t)v.sb.pairs * 2 * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess) return SUSHI_HIP_ELAUNCH;
    return SUSHI_HIP_OK;
}); }

int sushi_hip_batch_bounds_again(SushiHipBatch* b, int by_wave, int pass, float* slb_host, int32_t* votes_host, int64_t* n_pairs) {
    return c_boundary([&]() -> int {
    if (!b || !n_pairs || pass < 0 || pass > 2 || (by_wave != 0 && by_wave != 1)) return SUSHI_HIP_EINVAL;
    if (!b->last.ran || b->path != SUSHI_HIP_PATH_FFT || b->last_bounds_method < 0) { *n_pairs = 0; return SUSHI_HIP_OK; }
    hipStream_t st = b->last_stream;
    if (hipStreamSynchronize(st) != hipSuccess) return SUSHI_HIP_ELAUNCH;
    BoundArgs ba = b->last_bounds;
    const int64_t cap = *n_pairs;
    *n_pairs = ba.n_pairs;
    if (slb_host && cap < ba.n_pairs) return SUSHI_HIP_ENOSPACE;
    int votes[VOTE_SLOTS * VOTE_STRIDE];
    if (pass == 2) {
        ba.band = 2;
        if (hipMemsetAsync(ba.band_votes, 0, sizeof(votes), st) != hipSuccess) return SUSHI_HIP_ELAUNCH;
    }
    if (pass == 1) {
        // (the list the transforms took: the second look's in the band-split form, which is never overwritten)
        if (ba.band != 1) return SUSHI_HIP_EINVAL;
        const SubView v = last_sub(b);
        ba.list = v.slist2; ba.list_count = v.n_slist2;
    }
    constexpr int per_group = 4 * (64 / SLB_GROUP);
    const int rc = launch_method(b->last_bounds_method, [&](auto m) {
        constexpr int M = decltype(m)::value;
        if (pass == 1 && by_wave) hipLaunchKernelGGL(slb_list_wave_kernel<M>, dim3(256 * 2), dim3(256), 0, st, ba);
        else if (pass == 1) hipLaunchKernelGGL(slb_list_kernel<M>, dim3(256 * 2), dim3(256), 0, st, ba);
        else if (by_wave) hipLaunchKernelGGL(slb_wave_kernel<M>, dim3((unsigned)((ba.n_pairs + 3) / 4)), dim3(256), 0, st, ba);
        else hipLaunchKernelGGL(slb_kernel<M>, dim3((unsigned)((ba.n_pairs + per_group - 1) / per_group)), dim3(256), 0, st, ba); });
    if (rc != SUSHI_HIP_OK) return rc;
    if (pass == 2 && hipMemcpyAsync(votes, ba.band_votes, sizeof(votes), hipMemcpyDeviceToHost, st) != hipSuccess) return SUSHI_HIP_ELAUNCH;
    if (slb_host && hipMemcpyAsync(slb_host, ba.slb, (size_t)ba.n_pairs * sizeof(float), hipMemcpyDeviceToHost, st) != hipSuccess)
        return SUSHI_HIP_ELAUNCH;
    if (hipStreamSynchronize(st) != hipSuccess) return SUSHI_HIP_ELAUNCH;
    if (pass == 2 && votes_host) {
        votes_host[0] = votes_host[1] = 0;
        for (int k = 0; k < VOTE_SLOTS; ++k) { votes_host[0] += votes[k * VOTE_STRIDE]; votes_host[1] += votes[k * VOTE_STRIDE + 1]; }
    }
    return SUSHI_HIP_OK;
}); }

int sushi_hip_batch_workspace_view(SushiHipBatch* b, int which, void** ptr_dev, size_t* bytes) {
    if (!b || !ptr_dev || !bytes) return SUSHI_HIP_EINVAL;
    *ptr_dev = nullptr; *bytes = 0;
    if (!b->last.ran || b->path != SUSHI_HIP_PATH_FFT || b->now->plan.subs.empty()) return SUSHI_HIP_OK;
    if (hipStreamSynchronize(b->last_stream) != hipSuccess) return SUSHI_HIP_ELAUNCH;
    const SubView v = last_sub(b);
    switch (which) {
        case SUSHI_HIP_WS_TSPEC: {
            const size_t need = (size_t)v.sb.segs * ROW_BYTES;
            if (!tspec_half_rows(b->tspec)) { *ptr_dev = v.tspec; *bytes = need; break; }
            // the view means whole rows: expanded from the half rows into a buffer of the batch's own
            if (b->tspec_whole_bytes < need) {
                if (b->tspec_whole) (void)hipFree(b->tspec_whole);
                b->tspec_whole = nullptr; b->tspec_whole_bytes = 0;
                if (hipMalloc(&b->tspec_whole, need) != hipSuccess) { b->tspec_whole = nullptr; return SUSHI_HIP_ENOMEM; }
                b->tspec_whole_bytes = need;
            }
            const long long n_entries = (long long)v.sb.segs * ROWE;
            hipLaunchKernelGGL(tspec_expand_kernel, dim3((unsigned)std::min<long long>((n_entries + 255) / 256, 256 * 32)), dim3(256), 0, b->last_stream,
                               (const uint4*)v.tspec, (uint4*)b->tspec_whole, n_entries);
            if (launch_ok() != SUSHI_HIP_OK || hipStreamSynchronize(b->last_stream) != hipSuccess) return SUSHI_HIP_ELAUNCH;
            *ptr_dev = b->tspec_whole; *bytes = need;
            break;
        }
        case SUSHI_HIP_WS_TSPEC_HALF:
            if (!tspec_half_rows(b->tspec)) return SUSHI_HIP_EINVAL;
            *ptr_dev = v.tspec; *bytes = (size_t)v.sb.segs * HROW_BYTES;
            break;
        case SUSHI_HIP_WS_Y: *ptr_dev = v.y; *bytes = (size_t)v.sb.pairs * ROW_BYTES; break;
        case SUSHI_HIP_WS_TSPEC_LOW: *ptr_dev = v.tspec_low; *bytes = (size_t)v.sb.segs * LROW_BYTES; break;
        case SUSHI_HIP_WS_Y_LOW: *ptr_dev = v.ylow; *bytes = (size_t)v.sb.pairs * LROW_BYTES; break;
        case SUSHI_HIP_WS_TNORM_REST: *ptr_dev = v.tnorm_rest; *bytes = (size_t)v.sb.segs * sizeof(float); break;
        case SUSHI_HIP_WS_SLIST: *ptr_dev = v.slist; *bytes = (size_t)v.sb.pairs * sizeof(int); break;
        case SUSHI_HIP_WS_SLIST2: *ptr_dev = v.slist2; *bytes = (size_t)v.sb.pairs * sizeof(int); break;
        case SUSHI_HIP_WS_SCOUNT: *ptr_dev = v.n_slist; *bytes = (size_t)SC_WORDS * sizeof(int); break;
        case SUSHI_HIP_WS_MARKS: *ptr_dev = v.audit_mark; *bytes = (size_t)v.sb.pairs; break;
        case SUSHI_HIP_WS_PAIR_LB: *ptr_dev = v.pair_lb; *bytes = (size_t)v.sb.pairs * sizeof(float); break;
        default: return SUSHI_HIP_EINVAL;
    }
    return SUSHI_HIP_OK;
}

int sushi_hip_profile_begin(void) {
    for (ProfCall& c : g_prof)
        for (ProfSpan& sp : c.spans) { (void)hipEventDestroy(sp.t0); (void)hipEventDestroy(sp.t1); }
    g_prof.clear();
    g_prof_on = true;
    return SUSHI_HIP_OK;
}

int sushi_hip_profile_end(float* stage_ms, int max_calls, int* n_calls) { return c_boundary([&]() -> int {
    g_prof_on = false;
    if (!stage_ms || !n_calls || max_calls < 0) return SUSHI_HIP_EINVAL;
    int out = 0;
    int rc = SUSHI_HIP_OK;
    for (ProfCall& c : g_prof) {
        if (out < max_calls && !c.spans.empty()) {
            float* row = stage_ms + (size_t)out * SUSHI_HIP_NSTAGES;
            for (int k = 0; k < SUSHI_HIP_NSTAGES; ++k) row[k] = 0.f;
            for (ProfSpan& sp : c.spans) {
                float ms = 0.f;
                if (hipEventSynchronize(sp.t1) != hipSuccess || hipEventElapsedTime(&ms, sp.t0, sp.t1) != hipSuccess) {
                    rc = SUSHI_HIP_ELAUNCH;
                    break;
                }
                if (sp.stage >= 0 && sp.stage < SUSHI_HIP_NSTAGES) row[sp.stage] += ms;
            }
            ++out;
        }
        for (ProfSpan& sp : c.spans) { (void)hipEventDestroy(sp.t0); (void)hipEventDestroy(sp.t1); }
    }
    g_prof.clear();
    *n_calls = out;
    return rc;
}); }

}  // extern "C"
