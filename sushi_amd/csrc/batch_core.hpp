// sushi_amd/csrc/batch_core.hpp -- what a batch handle holds about its requests and how that is made, host only: no HIP header, no
// environment, no globals (the caller passes in what getenv returned).  Everything in a handle's life that needs no HIP call;
// sushi_fft.hip makes the HIP calls around it (the events, the copies, the fill).  Built with plain g++ by tests/host_batch_check.cpp,
// which states what a staged batch must be and checks it on the CPU; sushi_fft.hip includes the same file.
//   BatchPlanState                what a handle holds about its current requests: descriptors, plan, layout, accounting, and the
//                                 upload image; a handle has two, the current one and a spare that the next requests are staged into
//   PlanCache                     the plan made when a batch was sized, kept for its creation: remember / take, one key
//   choose_direct_variant, resolve_variant    which kernel variant of the direct path a batch is made with
//   BatchSpec, stage_batch        requests -> a BatchPlanState, or a refusal that has written nothing but the state it was given
//   whole_cut_upload              what a run uploads after complete_whole_cut
//   run_fill_span, fills_candidate_rows       what a run's one fill clears
#ifndef SUSHI_BATCH_CORE_HPP
#define SUSHI_BATCH_CORE_HPP

#include <array>
#include <string>
#include <utility>

#include "sushi_geometry.hpp"
#include "plan_core.hpp"

namespace sushi {

struct BatchPlanState {
    std::vector<SearchDesc> descs;
    Plan plan;
    BatchLayout lay = {};
    int64_t n_tiles = 0;                // (of the direct path)
    double flops = 0.0, algorithmic_bytes = 0.0;
    std::vector<char> upload;           // descriptors | schedule | work items as they lie in device memory from lay.desc on: one copy per (re)plan
};

// A caller sizes a batch (sushi_hip_batch_bytes) and then creates it from the same requests: the plan made for the first call is
// kept for the second (per host thread; compared request by request, so a changed request list simply plans again).  The key:
// the requests' bytes, the workspace cap and SUSHI_HIP_LANES as it read when the plan was made.
struct PlanCache {
    bool valid = false;
    size_t cap = 0;
    std::string lanes_env;
    std::vector<SushiHipRequest> req;
    Plan plan;
    void remember(const SushiHipRequest* r, int n, size_t cap_, const char* lanes, Plan&& p) {
        valid = true; cap = cap_; lanes_env = lanes ? lanes : "";
        req.assign(r, r + n);
        plan = std::move(p);
    }
    // true: `out` is the plan remembered for this very key (once: the cache is empty then)
    bool take(const SushiHipRequest* r, int n, size_t cap_, const char* lanes, Plan& out) {
        if (!valid || cap != cap_ || (int)req.size() != n || memcmp(req.data(), r, (size_t)n * sizeof(SushiHipRequest)) != 0 || lanes_env != (lanes ? lanes : ""))
            return false;                // (a plan that is not taken stays)
        out = std::move(plan);
        valid = false;
        return true;
    }
};

// largest tile variant whose grid still gives the chip (256 CUs x 4 SIMDs) a few waves per SIMD; `tiles`: positions per tile of
// the direct path's first min(n_variants, DIRECT_CHOICES) variants (the table is sushi_direct.hip's)
constexpr int DIRECT_CHOICES = 3;
inline int choose_direct_variant(const SushiHipRequest* req, int n, int n_variants, const int* tiles) {
    const int waves[DIRECT_CHOICES] = {1, 4, 4};
    int best = 0;
    for (int v = 0; v < n_variants && v < DIRECT_CHOICES; ++v) {
        int64_t nt = 0;
        for (int k = 0; k < n; ++k) nt += (req[k].n_pos + tiles[v] - 1) / tiles[v];
        if (nt * waves[v] >= 4096) best = v;
    }
    return best;
}

// The variant a batch of `path` is made with: the FFT path's descriptors count tiles of the largest; the direct path takes the
// one asked for, or (< 0) chooses.  -1: there is no such variant.
inline int resolve_variant(int path, int variant, const SushiHipRequest* req, int n, int n_variants, const int* tiles) {
    if (path == SUSHI_HIP_PATH_FFT) return n_variants - 1;
    if (variant < 0) variant = choose_direct_variant(req, n, n_variants, tiles);
    return variant < n_variants ? variant : -1;
}

// What a batch was created with: a re-plan must fit it.
struct BatchSpec {
    int path, tile;                     // (tile: positions per tile of its direct-path variant)
    size_t ws_cap, mem_bytes;
    int64_t dst_len, src_len;           // the two streams' samples
    double width;                       // bytes per sample
};

// requests -> descriptors, accounting, plan (the cache's, or made), layout and upload image of `out`, which may hold anything
// before and keeps its vectors' room (a re-plan allocates nothing for them).  EINVAL: a malformed request, or one outside its
// stream; ENOSPACE: they do not fit spec.mem_bytes; make_plan's own.  A refusal leaves `out` half written: it is the SPARE state.
inline int stage_batch(const SushiHipRequest* req, int n, const BatchSpec& spec, const char* lanes_env, PlanCache& cache, BatchPlanState& out) {
    int rc = make_descs(req, n, spec.tile, out.descs, &out.n_tiles, spec.dst_len, spec.src_len);
    if (rc != SUSHI_HIP_OK) return rc;
    out.flops = out.algorithmic_bytes = 0.0;
    for (int k = 0; k < n; ++k) {
        const SushiHipRequest& r = req[k];
        out.flops += 2.0 * (double)r.n_pos * (double)r.tmpl_len;
        out.algorithmic_bytes += spec.width * ((double)r.n_pos + r.tmpl_len - 1) + spec.width * r.tmpl_len + 8.0;
    }
    Plan& plan = out.plan;
    Plan fresh;                         // (an empty plan in the old one's vectors)
    fresh.subs.swap(plan.subs); fresh.subs_whole.swap(plan.subs_whole); fresh.order.swap(plan.order); fresh.items.swap(plan.items);
    fresh.subs.clear(); fresh.subs_whole.clear(); fresh.order.clear(); fresh.items.clear();
    plan = std::move(fresh);
    const bool fft = spec.path == SUSHI_HIP_PATH_FFT;
    if (fft && !cache.take(req, n, spec.ws_cap, lanes_env, plan) && (rc = make_plan(out.descs, spec.ws_cap, lanes_env, plan)) != SUSHI_HIP_OK) return rc;
    const BatchLayout& lay = out.lay;
    out.lay = batch_layout(n, spec.path, plan.order.size(), plan.items.size(), plan.ws_bytes, plan.subs.size(), plan.segs);
    if (spec.mem_bytes < lay.total) return SUSHI_HIP_ENOSPACE;
    const size_t desc_bytes = (size_t)n * sizeof(SearchDesc), order_bytes = plan.order.size() * sizeof(int32_t), items_bytes = plan.items.size() * sizeof(int32_t);
    out.upload.assign(fft ? lay.items + align_up(items_bytes, 256) - lay.desc : align_up(desc_bytes, 256), 0);
    memcpy(out.upload.data(), out.descs.data(), desc_bytes);
    if (order_bytes) memcpy(out.upload.data() + (lay.order - lay.desc), plan.order.data(), order_bytes);
    if (items_bytes) memcpy(out.upload.data() + (lay.items - lay.desc), plan.items.data(), items_bytes);
    return SUSHI_HIP_OK;
}

// A stretch of the batch's device memory (offset from its start) and the host bytes that go there.
struct UploadSpan { size_t dev_off; const void* host; size_t bytes; };

// What the run that made the one-sub-batch cut (complete_whole_cut) uploads: the tails of the schedule and of the items that were
// kept free for it.
inline std::array<UploadSpan, 2> whole_cut_upload(const Plan& plan, const BatchLayout& lay) {
    const size_t o0 = plan.whole_order_first, i0 = plan.whole_items_first;
    return {{{lay.order + o0 * sizeof(int32_t), plan.order.data() + o0, (plan.order.size() - o0) * sizeof(int32_t)},
             {lay.items + i0 * sizeof(int32_t), plan.items.data() + i0, (plan.items.size() - i0) * sizeof(int32_t)}}};
}

// What every run clears in one fill before its first kernel: flags .. counters, one span of the layout without a gap.
struct MemSpan { size_t off, bytes; };
inline MemSpan run_fill_span(const BatchLayout& lay) { return {lay.flags, lay.counters + align_up(sizeof(RunCounters), 256) - lay.flags}; }

// An argmin run's fill also sets the candidate rows (to all ones) where the batch is one sub-batch and they are small; the
// sub-batches of every other batch set their own.
inline size_t cand_rows_bytes(int64_t pairs) { return (size_t)pairs * FFT_ROW * sizeof(unsigned long long); }
constexpr size_t CAND_FILL_MAX = (size_t)8 << 20;
inline bool fills_candidate_rows(const Plan& plan) { return plan.subs.size() == 1 && cand_rows_bytes(plan.subs[0].pairs) <= CAND_FILL_MAX; }

}  // namespace sushi
#endif
