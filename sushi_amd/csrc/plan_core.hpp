// sushi_amd/csrc/plan_core.hpp -- the plan of a batch, host only: no HIP header, no environment, no globals.  Built with plain g++
// by tests/host_plan_check.cpp, which states what a plan must be and checks it on the CPU; sushi_fft.hip includes the same file.
//   ws_layout / batch_layout      the workspace of one sub-batch, the device memory of a batch
//   choose_lanes                  into how many sub-batches on how many lanes a batch is cut
//   make_descs, make_plan         requests -> descriptors -> sub-batches, their pair schedules and multiply-accumulate items
//   complete_whole_cut            the one-sub-batch cut of a plan on lanes, made when a run first wants it
//   parse_bound_fault, ranking_key    the two pure helpers of a run
#ifndef SUSHI_PLAN_CORE_HPP
#define SUSHI_PLAN_CORE_HPP

#include <limits.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "sushi_geometry.hpp"

namespace sushi {

inline int64_t cand_capacity(int64_t pairs) {
    const int64_t want = pairs * 64;
    return want < (1 << 16) ? (1 << 16) : (want > (1 << 24) ? (1 << 24) : want);
}

// bytes of workspace for one sub-batch of `pairs` block pairs, `segs` pattern segments and `searches` searches
struct WsLayout { size_t tspec, y, cand, pair_lb, pairmap, tconst, tiles, candbuf, dummy, slb, acc, plist, slist, citems,
                  tspec_low, ylow, audit_mark, slist2, dense_search, ditems, votes, total; };
inline WsLayout ws_layout(int64_t pairs, int64_t segs, int64_t searches) {
    WsLayout w;
    size_t o = 0;
    w.tspec = o; o += align_up((size_t)segs * ROW_BYTES, 256);                   // packed halves: 4 bytes per bin
    w.y = o; o += align_up((size_t)pairs * FFT_N * 2 * sizeof(uint16_t), 256);      // packed halves: 4 bytes per bin
    w.cand = o; o += align_up((size_t)pairs * FFT_ROW * sizeof(unsigned long long), 256);
    w.pair_lb = o; o += align_up((size_t)pairs * sizeof(float), 256);
    w.pairmap = o; o += align_up((size_t)pairs * sizeof(int), 256);
    w.tconst = o; o += align_up((size_t)searches * sizeof(TemplConsts), 256);
    w.tiles = o; o += align_up(((size_t)pairs * TILES_PER_PAIR + (size_t)cand_capacity(pairs) / SPARSE_UNIT + 1) * sizeof(TileDesc), 256);
    w.candbuf = o; o += align_up((size_t)cand_capacity(pairs) * sizeof(int32_t), 256);
    w.dummy = o; o += align_up((size_t)MAC_DUMMY_LINES * MAC_THREADS * 16, 256);          // (a 16-byte store per thread and line)
    w.slb = o; o += align_up((size_t)pairs * sizeof(float), 256);
    w.acc = o; o += align_up((size_t)pairs * 2 * sizeof(float), 256);
    w.plist = o; o += align_up((size_t)searches * sizeof(int), 256);
    w.slist = o; o += align_up((size_t)pairs * sizeof(int), 256);
    w.citems = o; o += align_up((size_t)pairs * sizeof(int), 256);
    // band-split exclusion: low-band rows of the pattern spectra and of the products (the pattern rows' norms outside the band
    // and every small counter live in the batch's own layout, per segment / per sub-batch: one launch clears them all)
    w.tspec_low = o; o += align_up((size_t)segs * LROW_BYTES, 256);
    w.ylow = o; o += align_up((size_t)pairs * LROW_BYTES, 256);
    w.audit_mark = o; o += align_up((size_t)pairs, 256);
    w.slist2 = o; o += align_up((size_t)pairs * sizeof(int), 256);
    w.dense_search = o; o += align_up((size_t)searches * sizeof(int), 256);
    // the dense searches' own items (dense_repack_kernel): at most one partly filled item per class more than searches / MAC_SPW
    w.ditems = o; o += align_up(((size_t)searches / MAC_SPW + MAC_CLASSES + 2) * (1 + MAC_SPW) * sizeof(int), 256);
    w.votes = o; o += VOTE_SLOTS * VOTE_STRIDE * sizeof(int);                      // the form prediction's counters
    w.total = o;
    return w;
}

// ---- host-side plan of a batch: sub-batches that fit the workspace, the inverse-transform schedule, the
// multiply-accumulate work items ------------------------------------------------------------------------
struct SubBatch {
    int a0, b0;                         // searches [a0, b0)
    int64_t pairs, segs;
    int first_pair, first_seg;
    int item_first[2];                  // [mac_kernel, mac_long_kernel]: into the item array (items of 1 + MAC_SPW ints)
    int item_count[2];
    int chunk_group[2];                 // bin chunks an XCD works on at a time
    int long_patterns;                  // searches whose pattern has more than MAC_SMAX_LONG segments
    int lane;                           // which HIP stream and which workspace of the plan's `lanes` it runs on / in
    int order_first;                    // its schedule inside Plan::order
};

struct Plan {
    std::vector<SubBatch> subs;
    // A plan on lanes also holds the cut it would have without them -- the whole batch as ONE sub-batch in lane 0's place (as few
    // as fit the workspace cap where one does not) --, for
    // the runs that form whole rows for every pair (the whole-row form of the exclusion, no exclusion at all): HBM traffic from the
    // first kernel to the last, which side by side only contends (unrelated audio at BASELINE configs[2]: 24.9 ms as one sub-batch,
    // 26.8 as nine on three lanes, 30.5 as nine one after the other).  Which cut a run takes is decided when it starts.
    std::vector<SubBatch> subs_whole;   // (made by the first run that wants it: complete_whole_cut; room for its schedule and items is kept from the start)
    bool whole_pending = false;
    size_t whole_order_first = 0, whole_items_first = 0, whole_items_room = 0, ws_whole = 0;
    std::vector<int32_t> order;         // per sub-batch (of either cut): workgroup -> pair
    std::vector<int32_t> items;         // [total items][1 + MAC_SPW]: class, then search indices inside the sub-batch or -1
    int64_t pairs = 0, segs = 0;
    size_t ws_bytes = 0;                // workspace the plan was cut for: lanes x ws_lane
    size_t ws_lane = 0;                 // workspace of one lane (sub-batches of a lane run one after the other in it)
    int lanes = 1;                      // sub-batches run side by side on this many HIP streams (1: all on the caller's)
};

// every search's overlap-save layout: computed once per plan, read by everything below
inline std::vector<FftLayout> search_layouts(const std::vector<SearchDesc>& s) {
    std::vector<FftLayout> lay;
    lay.reserve(s.size());
    for (const SearchDesc& d : s) lay.push_back(fft_layout(d.win_start, d.n_pos, d.tmpl_len));
    return lay;
}

// workspace of the most demanding single search / of the whole batch as one sub-batch
inline void ws_extremes(const std::vector<FftLayout>& lay, size_t* need_one, size_t* need_all) {
    size_t one = 0;
    int64_t pairs = 0, segs = 0;
    for (const FftLayout& l : lay) {
        one = std::max(one, ws_layout(l.n_pairs, l.n_seg, 1).total);
        pairs += l.n_pairs; segs += l.n_seg;
    }
    *need_one = one;
    *need_all = ws_layout(pairs, segs, (int64_t)lay.size()).total;
}

// Lanes (round 6): the stages of the path are bound by different things -- the low rows' multiply-accumulate by its stores, the
// bound by instruction issue, the transforms by the LDS, the row kernels by HBM reads -- and every stage ends in a tail that leaves
// most of the chip idle.  A batch that is large enough is therefore cut into SUBS sub-batches of equal pair counts that run side by
// side on LANES HIP streams (lane 0 is the caller's), each lane in its own workspace: the hardware co-schedules one sub-batch's
// store-bound kernel with another's issue-bound one.  Measured at BASELINE configs[2] inside one run (forked behind its first launch,
// joined before its last; ms per step, two sweeps on one box): 1:1 8.94 / 8.99; 2:2 8.44 / 8.50; 3:3 8.52 / 8.52; 4:2 8.52 / 8.52;
// 6:2 8.33 / 8.62; 6:3 8.47 / 8.43; 9:3 8.29 / 8.38; 12:3 8.35 / 8.27; 8:4 8.29 / 8.40; 12:4 8.26 / 8.39.  (Separate batches on
// separate streams with no join between steps -- tools/overlap_probe.py -- read 7.81 for 6 on 3: the streams then also overlap one
// step's tail with the next one's head, which one run cannot.)  What a sub-batch must keep is enough searches for its own grids:
// the 1500-event shard of a two-rank run takes 4.48 ms as one, 4.32 as 2:2, 4.48 as 4:2, 4.89 as 6:3, 5.41 as 9:3; 750 events
// 2.40 / 2.26 (2:2) / 3.02 (6:3); 375 events 1.31 / 1.25 (2:2) / 1.49 (4:2).  Hence: two halves on two lanes from 128 searches
// and 24 k pairs on; three lanes (four from twelve parts on) only where every part keeps ~330 searches.
// `e`, "subs:lanes" or NULL (the caller's SUSHI_HIP_LANES, read where a plan is made, never in a run), overrides the choice for measurements.
constexpr int MAX_LANES = 4;
constexpr int64_t LANES_MIN_PAIRS = 24 * 1024;     // below: one sub-batch (a lane's fixed cost -- two dozen launches, small grids -- outweighs the overlap)
constexpr int LANES_MIN_SEARCHES = 128;
constexpr int LANES_PART_SEARCHES = 330;           // searches a part keeps where there are more than two parts
struct LaneChoice { int subs, lanes; };
inline LaneChoice choose_lanes(int64_t pairs, int n_search, const char* e) {
    LaneChoice c{1, 1};
    if (pairs >= LANES_MIN_PAIRS && n_search >= LANES_MIN_SEARCHES) {
        const int parts = std::min(12, n_search / LANES_PART_SEARCHES);
        c = parts >= 9 ? LaneChoice{parts, parts >= 12 ? 4 : 3} : LaneChoice{2, 2};
    }
    if (e && *e) {
        int k = 0, l = 0;
        if (sscanf(e, "%d:%d", &k, &l) == 2 && k >= 1 && l >= 1 && l <= MAX_LANES && k <= 64) c = LaneChoice{std::min(k, std::max(1, n_search)), std::min(l, k)};
    }
    if (c.subs < c.lanes) c.lanes = c.subs;
    return c;
}

// The inverse transforms' schedule of searches [a0, b0), `pairs` pairs in all, appended to `order`: workgroup -> pair of the sub-batch.
// Every pair is keyed by the region of the destination stream it scores (its absolute pair index); workgroup b runs on XCD b % 8
// (observed; speed only), so the pairs of a region go to the queue of one XCD and share its L2.
// (a counting sort by region, stable in pair order, then one pass that deals the sorted pairs to the queue of their region's
// XCD: what eight std::stable_sort calls over vectors of (region, pair) did at four times the host time -- a plan of
// BASELINE configs[2] took 10 ms, most of it here)
inline void schedule_pairs(const std::vector<FftLayout>& lay, int a0, int b0, int64_t pairs, std::vector<int32_t>& order) {
    int64_t rmin = INT64_MAX, rmax = INT64_MIN;
    for (int k = a0; k < b0; ++k) { rmin = std::min<int64_t>(rmin, lay[k].pair0); rmax = std::max<int64_t>(rmax, lay[k].pair0 + lay[k].n_pairs - 1); }
    const size_t n_regions = (size_t)(rmax - rmin + 1);
    std::vector<int32_t> start(n_regions + 1, 0);
    for (int k = a0; k < b0; ++k) {
        const FftLayout l = lay[k];                                     // (a copy: the stores below may alias the vector's ints)
        for (int i = 0; i < l.n_pairs; ++i) ++start[(size_t)(l.pair0 + i - rmin) + 1];
    }
    size_t qsize[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (size_t r = 0; r < n_regions; ++r) { qsize[(size_t)((int64_t)r + rmin) & 7] += (size_t)start[r + 1]; start[r + 1] += start[r]; }
    std::vector<int32_t> sorted((size_t)pairs);                     // pair indices by (region, pair)
    {
        std::vector<int32_t> fill(start.begin(), start.end() - 1);
        int pair = 0;
        for (int k = a0; k < b0; ++k) {
            const FftLayout l = lay[k];
            for (int i = 0; i < l.n_pairs; ++i, ++pair) sorted[(size_t)fill[(size_t)(l.pair0 + i - rmin)]++] = pair;
        }
    }
    std::vector<int32_t> lists[8];
    for (int x = 0; x < 8; ++x) lists[x].reserve(qsize[x]);
    for (size_t r = 0; r < n_regions; ++r) {
        std::vector<int32_t>& q = lists[(size_t)((int64_t)r + rmin) & 7];
        q.insert(q.end(), sorted.begin() + start[r], sorted.begin() + start[r + 1]);
    }
    size_t head[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    const size_t o0 = order.size();
    order.resize(o0 + (size_t)pairs);
    int32_t* __restrict__ out = order.data() + o0;
    for (int64_t b = 0; b < pairs; ++b) {
        int x = (int)(b & 7);
        if (head[x] >= lists[x].size()) {               // that XCD's queue is exhausted: take from the fullest one
            size_t best = 0;
            for (int y = 0; y < 8; ++y) {
                const size_t left = lists[y].size() - head[y];
                if (left > best) { best = left; x = y; }
            }
        }
        out[b] = lists[x][head[x]++];
    }
}

// The multiply-accumulate items of one kernel -- 0: mac_kernel, classes below MAC_SHORT_CLASSES; 1: mac_long_kernel, the others --
// for searches [a0, b0), appended to `items`; returns how many, and the kernel's chunk_group.
// An item is MAC_SPW searches of one segment-count class whose windows START next to each other
// (a wave walks the union of its searches' block ranges with every lane computing, so an item costs
// union x class size whatever its members need: sorted by window start, eight neighbours of a class differ by as
// little as that class allows -- in request order the windows of neighbouring events can be a whole window
// apart, which cost 18 % more rows at BASELINE configs[2]); the items themselves in stream order whatever
// their class.
inline int mac_items(const std::vector<SearchDesc>& s, const std::vector<FftLayout>& lay, int a0, int b0, int kern, std::vector<int32_t>& items,
                     int* chunk_group) {
    struct Item { int64_t first; int cls; std::vector<int> members; };
    std::vector<Item> its;
    std::vector<int> of_class[MAC_CLASSES];
    int n_members = 0;
    double win_blocks = 0.0;
    int64_t ws_lo = INT64_MAX, ws_hi = INT64_MIN;
    for (int k = a0; k < b0; ++k) {
        const int c = mac_class(lay[k].n_seg);
        if ((c >= MAC_SHORT_CLASSES) != (kern == 1)) continue;
        of_class[c].push_back(k);
        ++n_members; win_blocks += (double)s[k].n_pos / FFT_SEG;
        ws_lo = std::min(ws_lo, s[k].win_start); ws_hi = std::max(ws_hi, s[k].win_start);
    }
    for (int c = 0; c < MAC_CLASSES; ++c) {
        std::vector<int>& v = of_class[c];
        std::stable_sort(v.begin(), v.end(), [&](int p, int q) { return s[p].win_start < s[q].win_start; });
        for (size_t i = 0; i < v.size(); i += MAC_SPW) {
            Item it{s[v[i]].win_start, c, {}};
            for (size_t g = i; g < v.size() && g < i + MAC_SPW; ++g) it.members.push_back(v[g] - a0);
            its.push_back(it);
        }
    }
    std::stable_sort(its.begin(), its.end(), [](const Item& p, const Item& q) { return p.first < q.first; });
    for (const Item& it : its) {
        items.push_back(it.cls);
        for (int g = 0; g < MAC_SPW; ++g) items.push_back(g < (int)it.members.size() ? it.members[g] : -1);
    }
    // how many items overlap a row of block spectra: window length / spacing of the items' windows.  An XCD keeps
    // 32 CUs x (3 | 2) workgroups in flight; with chunk_group = that / overlap the items in flight per chunk are
    // the ones that share rows (mac_kernel's comment).
    int cg = 1;
    if (n_members > 0) {
        win_blocks /= n_members;
        const double span_blocks = (double)(ws_hi - ws_lo) / FFT_SEG;
        const double spacing = its.size() > 1 ? std::max(span_blocks / (double)(its.size() - 1), 1e-3) : win_blocks;
        const double overlap = std::max(win_blocks / spacing, 1.0);
        const double in_flight = kern == 0 ? 96.0 : 64.0;
        while (cg < MAC_CHUNKS / 8 && in_flight / overlap >= 1.5 * cg) cg *= 2;
    }
    *chunk_group = cg;
    return (int)its.size();
}

// One cut of a batch into sub-batches, appended to `subs`, their schedules and work items to plan.order / plan.items.
// `cuts`: NULL = as many searches per sub-batch as `ws_bytes` holds (greedy); else the sub-batches' ends (b0 of each), on `lanes` lanes
inline int build_plan(const std::vector<SearchDesc>& s, const std::vector<FftLayout>& lay, size_t ws_bytes, Plan& plan, std::vector<SubBatch>& subs,
                      const std::vector<int>* cuts = nullptr, int lanes = 1) {
    const int n = (int)s.size();
    size_t cut_i = 0;
    for (int a0 = 0; a0 < n; ++cut_i) {
        SubBatch sb;
        sb.a0 = a0; sb.pairs = 0; sb.segs = 0; sb.long_patterns = 0;
        int b0 = a0;
        for (; b0 < n; ++b0) {
            const FftLayout& l = lay[b0];
            if (cuts ? b0 >= (*cuts)[cut_i] : ws_layout(sb.pairs + l.n_pairs, sb.segs + l.n_seg, b0 - a0 + 1).total > ws_bytes) break;
            sb.pairs += l.n_pairs; sb.segs += l.n_seg;
            if (l.n_seg > mac_class_smax(MAC_CLASSES - 1)) ++sb.long_patterns;
        }
        if (b0 == a0 || ws_layout(sb.pairs, sb.segs, b0 - a0).total > ws_bytes) return SUSHI_HIP_ENOSPACE;
        sb.b0 = b0;
        sb.first_pair = s[a0].first_pair; sb.first_seg = s[a0].first_seg;
        sb.lane = (int)(subs.size() % (size_t)lanes);
        sb.order_first = (int)plan.order.size();
        schedule_pairs(lay, a0, b0, sb.pairs, plan.order);
        for (int kern = 0; kern < 2; ++kern) {
            sb.item_first[kern] = (int)(plan.items.size() / (1 + MAC_SPW));
            sb.item_count[kern] = mac_items(s, lay, a0, b0, kern, plan.items, &sb.chunk_group[kern]);
        }
        subs.push_back(sb);
        a0 = b0;
    }
    return SUSHI_HIP_OK;
}

// The one-sub-batch cut of a plan on lanes, made when a run first wants it (a job whose every run takes the band-split form never
// pays for it: 9 ms of host time at BASELINE configs[2]): schedule and items into the room kept for them.  false: it does not fit
// that room, or has more sub-batches than the plan has (tests/host_plan_check.cpp: on none of its cases) -- the run then takes the
// plan's own sub-batches one after the other.
inline bool complete_whole_cut(const std::vector<SearchDesc>& descs, Plan& plan) {
    Plan tmp;
    std::vector<SubBatch> subs;
    if (build_plan(descs, search_layouts(descs), plan.ws_whole, tmp, subs) != SUSHI_HIP_OK || subs.empty()) return false;
    // (batch_layout kept a block of counters per sub-batch of plan.subs; a run of this cut indexes them by ITS sub-batches)
    if (subs.size() > plan.subs.size()) return false;
    if (tmp.order.size() > plan.order.size() - plan.whole_order_first || tmp.items.size() > plan.whole_items_room) return false;
    std::copy(tmp.order.begin(), tmp.order.end(), plan.order.begin() + (ptrdiff_t)plan.whole_order_first);
    std::copy(tmp.items.begin(), tmp.items.end(), plan.items.begin() + (ptrdiff_t)plan.whole_items_first);
    for (SubBatch& sb : subs) {
        sb.order_first += (int)plan.whole_order_first;
        for (int kern = 0; kern < 2; ++kern) sb.item_first[kern] += (int)(plan.whole_items_first / (1 + MAC_SPW));
    }
    plan.subs_whole.swap(subs);
    plan.whole_pending = false;
    return true;
}

// device-memory layout of a batch
struct BatchLayout { size_t desc, keys, flags, viol, flag_list, subc, tnorm, counters, order, items, ws, total; };

// (flags .. counters is ONE span of zeros at the start of a run: flags, violation marks, flag list, every sub-batch's small counters
// (SUBC_BYTES each: SubCounters, then the `scount` words), the pattern rows' norm accumulators of the whole batch, the run's counters)
constexpr size_t SUBC_BYTES = 256;
constexpr int SUBC_SCOUNT = 8;          // int index inside a sub-batch's block of its first `scount` word
static_assert(sizeof(SubCounters) <= SUBC_SCOUNT * sizeof(int), "the scount words lie behind the SubCounters");
// The `scount` words of a sub-batch: list lengths and marks the kernels of a run count with (SubView names a pointer to each).
enum ScountSlot {
    SC_SLIST = 0,           // survivors: entries of slist
    SC_CITEMS = 1,          // collect items: entries of citems (refine_kernel's list for collect_kernel)
    SC_REST_ITEMS = 2,      // work items of the survivors' pass (dense_search_kernel): entries of slist, which is dead by then
    // 3: free
    SC_ANY_DENSE = 4,       // dense whole rows: 1 where some search takes the dense form (dense_repack_kernel; enables that launch)
    SC_SLIST2 = 5,          // pairs left after the second look: entries of slist2
    SC_DENSE_LISTED = 6,    // listed pairs of the searches that would take the dense form
    SC_LIST3 = 7,           // the threshold run's extension list
    SC_WORDS = 8
};
static_assert((SUBC_SCOUNT + SC_WORDS) * sizeof(int) <= SUBC_BYTES, "the scount words fit the sub-batch's block");
inline BatchLayout batch_layout(int n, int path, size_t n_order_ints, size_t n_item_ints, size_t ws_bytes, size_t n_subs, int64_t total_segs) {
    BatchLayout b;
    size_t o = 0;
    // (descriptors, schedule and work items first and next to each other: ONE upload per batch, from one host buffer)
    b.desc = o; o += align_up((size_t)n * sizeof(SearchDesc), 256);
    b.order = o; o += path == SUSHI_HIP_PATH_FFT ? align_up(n_order_ints * sizeof(int32_t), 256) : 0;
    b.items = o; o += path == SUSHI_HIP_PATH_FFT ? align_up(n_item_ints * sizeof(int32_t), 256) : 0;
    b.keys = o; o += align_up((size_t)2 * n * sizeof(unsigned long long), 256);
    b.flags = o; o += align_up((size_t)n * sizeof(int), 256);
    b.viol = o; o += align_up((size_t)n * sizeof(int), 256);
    b.flag_list = o; o += align_up((size_t)n * sizeof(int), 256);
    b.subc = o; o += std::max<size_t>(n_subs, 1) * SUBC_BYTES;
    b.tnorm = o; o += align_up((size_t)total_segs * sizeof(float), 256);
    b.counters = o; o += align_up(sizeof(RunCounters), 256);
    b.ws = o; o += path == SUSHI_HIP_PATH_FFT ? align_up(ws_bytes, 256) : 0;
    b.total = o;
    return b;
}

// requests -> descriptors with their running sums; EINVAL for a request that request_fits refuses -- malformed, or outside streams
// of `dst_n` / `src_n` samples (the default: no streams yet, a batch that is only sized)
// (`tp`: positions per tile of the direct path's kernel variant)
inline int make_descs(const SushiHipRequest* req, int n, int tp, std::vector<SearchDesc>& out, int64_t* n_tiles,
                      int64_t dst_n = INT64_MAX, int64_t src_n = INT64_MAX) {
    out.resize(n);
    int64_t tiles = 0, pairs = 0, segs = 0;
    for (int k = 0; k < n; ++k) {
        const SushiHipRequest& r = req[k];
        if (!request_fits(r, dst_n, src_n)) return SUSHI_HIP_EINVAL;
        SearchDesc d;
        d.tmpl_off = r.tmpl_off; d.win_start = r.win_start; d.tmpl_len = r.tmpl_len; d.n_pos = r.n_pos;
        if (tiles > 0x7fffffff || pairs > 0x7fffffff || segs > 0x7fffffff) return SUSHI_HIP_EINVAL;
        d.first_tile = (int32_t)tiles; d.first_pair = (int32_t)pairs; d.first_seg = (int32_t)segs; d.reserved = 0;
        const FftLayout l = fft_layout(r.win_start, r.n_pos, r.tmpl_len);
        tiles += (r.n_pos + tp - 1) / tp;
        pairs += l.n_pairs;
        segs += l.n_seg;
        out[k] = d;
    }
    if (tiles > 0x7fffffff || pairs > 0x7fffffff || segs > 0x7fffffff) return SUSHI_HIP_EINVAL;
    *n_tiles = tiles;
    return SUSHI_HIP_OK;
}

// The plan of a batch under a workspace cap (0: whatever one sub-batch for everything needs): on lanes when the batch is large
// enough and the lanes' workspaces fit the cap, else one sub-batch after the other in one workspace.
inline int make_plan(const std::vector<SearchDesc>& descs, size_t cap, const char* lanes_override, Plan& plan) {
    const std::vector<FftLayout> lay = search_layouts(descs);
    size_t need_one, need_all;
    ws_extremes(lay, &need_one, &need_all);
    const size_t ws1 = cap == 0 ? need_all : std::max(need_one, std::min(need_all, cap));
    const int n = (int)descs.size();
    std::vector<int64_t> pairs_upto((size_t)n + 1, 0), segs_upto((size_t)n + 1, 0);
    for (int k = 0; k < n; ++k) {
        pairs_upto[(size_t)k + 1] = pairs_upto[(size_t)k] + lay[k].n_pairs;
        segs_upto[(size_t)k + 1] = segs_upto[(size_t)k] + lay[k].n_seg;
    }
    const int64_t total = pairs_upto[(size_t)n];
    if (total > 0x7fffffff / 2) return SUSHI_HIP_EINVAL;               // (schedules of two cuts are indexed by int)
    plan.pairs = total; plan.segs = segs_upto[(size_t)n];
    const LaneChoice lc = choose_lanes(total, n, lanes_override);
    if (lc.subs > 1) {
        // ends of the sub-batches where the running pair count crosses k / subs of the total; a lane's workspace holds the largest
        std::vector<int> cuts;
        size_t ws_lane = 0;
        for (int k = 1, a0 = 0; k <= lc.subs && a0 < n; ++k) {
            const int64_t want = total * k / lc.subs;
            int b0 = (int)(std::lower_bound(pairs_upto.begin(), pairs_upto.end(), want) - pairs_upto.begin());
            b0 = k == lc.subs ? n : std::min(n, std::max(b0, a0 + 1));
            ws_lane = std::max(ws_lane, ws_layout(pairs_upto[(size_t)b0] - pairs_upto[(size_t)a0], segs_upto[(size_t)b0] - segs_upto[(size_t)a0], b0 - a0).total);
            cuts.push_back(b0);
            a0 = b0;
        }
        ws_lane = align_up(ws_lane, 256);
        const int lanes = std::min<int>(lc.lanes, (int)cuts.size());
        if (cuts.size() > 1 && (cap == 0 || ws_lane * (size_t)lanes <= cap)) {
            plan.lanes = lanes; plan.ws_lane = ws_lane;
            plan.ws_bytes = std::max(ws_lane * (size_t)lanes, ws1);                  // (ws1 <= cap)
            const int rc = build_plan(descs, lay, ws_lane, plan, plan.subs, &cuts, lanes);
            if (rc != SUSHI_HIP_OK) return rc;
            // room for the cut without lanes (the whole batch as one sub-batch where the cap allows, else as few as fit it): a
            // schedule entry per pair; of items at most one partly filled per class, kernel and sub-batch
            plan.whole_pending = true; plan.ws_whole = ws1;
            plan.whole_order_first = plan.order.size(); plan.whole_items_first = plan.items.size();
            const size_t whole_subs = need_all / ws1 + 2;
            plan.whole_items_room = ((size_t)n / MAC_SPW + (2 * MAC_CLASSES + 2) * whole_subs) * (1 + MAC_SPW);
            plan.order.resize(plan.order.size() + (size_t)total, 0);
            plan.items.resize(plan.items.size() + plan.whole_items_room, -1);
            return SUSHI_HIP_OK;
        }
    }
    plan.lanes = 1; plan.ws_lane = ws1; plan.ws_bytes = ws1;
    return build_plan(descs, lay, ws1, plan, plan.subs);
}

// the tests' seam (sushi_fft_bound.inc bound_fault_kernel): which pairs' stored bounds are made wrong
struct BoundFault { int period = 0, phase = 0, pair = -1; };

// SUSHI_HIP_TEST_BOUND_FAULT=<period>:<phase>[:<pair>] -- decimal digits only, period >= 1, 0 <= phase < period, pair >= 0, nothing
// behind the last field; false: malformed
inline bool parse_bound_fault(const char* s, BoundFault* out) {
    long field[3] = {0, 0, -1};
    int n = 0;
    for (;;) {
        if (n == 3 || *s < '0' || *s > '9') return false;
        char* end = nullptr;
        field[n] = strtol(s, &end, 10);
        if (field[n] > INT_MAX) return false;                     // (no sign was read: never negative; LONG_MAX on overflow)
        ++n;
        if (!*end) break;
        if (*end != ':') return false;
        s = end + 1;
    }
    if (n < 2 || field[0] < 1 || field[1] >= field[0]) return false;
    out->period = (int)field[0]; out->phase = (int)field[1]; out->pair = n == 3 ? (int)field[2] : -1;
    return true;
}

// a threshold in ranking units (what the bound is a lower bound of: the score, 1 - the coefficient), rounded UP to a float, as a
// search key: a pair is excluded only if its bound is above it (bound_excludes, with its slack).  `clamp_at_zero`: never below 0 --
// no ranking score is, and the best-K run orders these keys as unsigned numbers.
inline unsigned long long ranking_key(const int method, const double threshold, const bool clamp_at_zero) {
    double u = method == SUSHI_HIP_METHOD_CCOEFF_NORMED ? 1.0 - threshold : threshold;
    if (clamp_at_zero) u = std::max(0.0, u);
    float uf = (float)u;
    if (std::isfinite(uf) && (double)uf < u) uf = std::nextafter(uf, INFINITY);
    uint32_t ubits;
    memcpy(&ubits, &uf, sizeof(ubits));
    return ((unsigned long long)ubits << 32) | 0xffffffffull;
}

}  // namespace sushi
#endif
