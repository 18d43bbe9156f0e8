// The plan of a batch (sushi_amd/csrc/plan_core.hpp) on the CPU: what a plan must be, stated as checks, over a fixed table of cases
// (tests/batch_cases.hpp, which tests/host_batch_check.cpp goes through as well).
// usage: host_plan_check                  checks every case that plans, ranking_key and parse_bound_fault; exit 1 with a message
//                                         on the first violation
//        host_plan_check --dump           one JSON record per case and line: return code, totals, every SubBatch field of both cuts,
//                                         FNV-1a digests of every sub-batch's schedule and items, every BatchLayout offset
//                                         (tests/golden/plan_cases.json is this output)
//        host_plan_check --requests DIR   writes every case's requests (SushiHipRequest records) to DIR/<case name>.req: what
//                                         tests/test_plan_host.py hands to the library's sushi_hip_batch_bytes
// Built by tests/test_plan_host.py with g++ -O2 -std=c++17, and once more with -O1 -g -fsanitize=address,undefined.
#include "../sushi_amd/csrc/sushi_geometry.hpp"
#include "../sushi_amd/csrc/plan_core.hpp"
#include "../sushi_amd/csrc/batch_core.hpp"
#include "batch_cases.hpp"

#include <cinttypes>
#include <random>

using namespace sushi;
using namespace batch_cases;

namespace {

// ---- a case, planned ----
struct Planned {
    int rc = SUSHI_HIP_OK;
    size_t cap = 0;
    std::vector<SearchDesc> descs;
    Plan plan;
    BatchLayout lay = {};
    bool whole_wanted = false, whole_ok = false;
};

// what sushi_hip_batch_bytes does, then what the first run that wants the one-sub-batch cut does
Planned plan_case(const Case& c) {
    Planned p;
    int64_t tiles = 0;
    p.rc = make_descs(c.req.data(), (int)c.req.size(), FFT_PATH_TILE, p.descs, &tiles);
    if (p.rc != SUSHI_HIP_OK) return p;
    p.cap = case_cap(c, p.descs);
    p.rc = make_plan(p.descs, p.cap, c.lanes.c_str(), p.plan);
    if (p.rc != SUSHI_HIP_OK) return p;
    p.lay = batch_layout((int)c.req.size(), SUSHI_HIP_PATH_FFT, p.plan.order.size(), p.plan.items.size(), p.plan.ws_bytes, p.plan.subs.size(), p.plan.segs);
    p.whole_wanted = p.plan.whole_pending;
    if (p.whole_wanted) p.whole_ok = complete_whole_cut(p.descs, p.plan);
    return p;
}

// ---- --dump ----
uint64_t fnv1a(const int32_t* p, size_t n) {
    uint64_t h = 0xcbf29ce484222325ull;
    const unsigned char* b = (const unsigned char*)p;
    for (size_t i = 0; i < n * sizeof(int32_t); ++i) { h ^= b[i]; h *= 0x100000001b3ull; }
    return h;
}

void dump_subs(const char* key, const Plan& plan, const std::vector<SubBatch>& subs) {
    printf(",\"%s\":[", key);
    for (size_t i = 0; i < subs.size(); ++i) {
        const SubBatch& s = subs[i];
        const size_t n_items = (size_t)(s.item_count[0] + s.item_count[1]) * (1 + MAC_SPW);
        printf("%s{\"a0\":%d,\"b0\":%d,\"pairs\":%" PRId64 ",\"segs\":%" PRId64 ",\"first_pair\":%d,\"first_seg\":%d,\"item_first\":[%d,%d],"
               "\"item_count\":[%d,%d],\"chunk_group\":[%d,%d],\"long_patterns\":%d,\"lane\":%d,\"order_first\":%d,"
               "\"order_fnv\":\"%016" PRIx64 "\",\"items_fnv\":\"%016" PRIx64 "\"}",
               i ? "," : "", s.a0, s.b0, s.pairs, s.segs, s.first_pair, s.first_seg, s.item_first[0], s.item_first[1], s.item_count[0],
               s.item_count[1], s.chunk_group[0], s.chunk_group[1], s.long_patterns, s.lane, s.order_first,
               fnv1a(plan.order.data() + s.order_first, (size_t)s.pairs),
               fnv1a(plan.items.data() + (size_t)s.item_first[0] * (1 + MAC_SPW), n_items));
    }
    printf("]");
}

void dump(const Case& c, const Planned& p) {
    printf("{\"name\":\"%s\",\"n\":%zu,\"cap\":%zu,\"lanes_override\":\"%s\",\"rc\":%d", c.name.c_str(), c.req.size(), p.cap, c.lanes.c_str(), p.rc);
    if (p.rc == SUSHI_HIP_OK) {
        const Plan& q = p.plan;
        printf(",\"pairs\":%" PRId64 ",\"segs\":%" PRId64 ",\"lanes\":%d,\"ws_lane\":%zu,\"ws_bytes\":%zu,\"ws_whole\":%zu", q.pairs, q.segs, q.lanes,
               q.ws_lane, q.ws_bytes, q.ws_whole);
        printf(",\"whole_order_first\":%zu,\"whole_items_first\":%zu,\"whole_items_room\":%zu,\"whole_wanted\":%d,\"whole_ok\":%d",
               q.whole_order_first, q.whole_items_first, q.whole_items_room, p.whole_wanted ? 1 : 0, p.whole_ok ? 1 : 0);
        dump_subs("subs", q, q.subs);
        dump_subs("subs_whole", q, q.subs_whole);
        const BatchLayout& b = p.lay;
        printf(",\"layout\":{\"desc\":%zu,\"order\":%zu,\"items\":%zu,\"keys\":%zu,\"flags\":%zu,\"viol\":%zu,\"flag_list\":%zu,\"subc\":%zu,"
               "\"tnorm\":%zu,\"counters\":%zu,\"ws\":%zu}", b.desc, b.order, b.items, b.keys, b.flags, b.viol, b.flag_list, b.subc, b.tnorm,
               b.counters, b.ws);
    }
    printf(",\"total\":%zu}\n", p.rc == SUSHI_HIP_OK ? p.lay.total : (size_t)0);
}

// ---- the checks ----
std::string g_case;
#define REQUIRE(cond, ...) do { if (!(cond)) { fprintf(stderr, "%s: %s -- ", g_case.c_str(), #cond); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); exit(1); } } while (0)

// offsets in memory order, `end` behind the last part: 256-aligned and increasing
void check_offsets(const char* what, const std::vector<size_t>& o) {
    for (size_t i = 0; i < o.size(); ++i) {
        REQUIRE(o[i] % 256 == 0, "%s offset %zu = %zu", what, i, o[i]);
        REQUIRE(i == 0 || o[i] > o[i - 1], "%s offset %zu = %zu after %zu", what, i, o[i], o[i - 1]);
    }
}

// one cut of the plan: `ws_room` bytes of workspace per sub-batch, on `lanes` lanes; its schedules inside plan.order[order_lo, order_hi),
// its items inside plan.items[items_lo, items_hi)
void check_cut(const Planned& p, const std::vector<SubBatch>& subs, size_t ws_room, int lanes, size_t order_lo, size_t order_hi, size_t items_lo,
               size_t items_hi) {
    const Plan& plan = p.plan;
    const int n = (int)p.descs.size();
    REQUIRE(!subs.empty() && subs.front().a0 == 0 && subs.back().b0 == n, "the sub-batches tile [0, %d)", n);
    int64_t run_pairs = 0, run_segs = 0;
    for (size_t si = 0; si < subs.size(); ++si) {
        const SubBatch& sb = subs[si];
        REQUIRE(sb.a0 < sb.b0 && (si == 0 || sb.a0 == subs[si - 1].b0), "sub-batch %zu is [%d, %d)", si, sb.a0, sb.b0);
        REQUIRE(sb.first_pair == run_pairs && sb.first_seg == run_segs, "sub-batch %zu starts at pair %d, segment %d", si, sb.first_pair, sb.first_seg);
        REQUIRE(sb.first_pair == p.descs[sb.a0].first_pair && sb.first_seg == p.descs[sb.a0].first_seg, "sub-batch %zu against its first search", si);
        int64_t pairs = 0, segs = 0;
        int long_patterns = 0;
        for (int k = sb.a0; k < sb.b0; ++k) {
            const FftLayout l = fft_layout(p.descs[k].win_start, p.descs[k].n_pos, p.descs[k].tmpl_len);
            pairs += l.n_pairs; segs += l.n_seg;
            if (l.n_seg > mac_class_smax(MAC_CLASSES - 1)) ++long_patterns;
        }
        REQUIRE(sb.pairs == pairs && sb.segs == segs, "sub-batch %zu: %" PRId64 " pairs, %" PRId64 " segments", si, sb.pairs, sb.segs);
        REQUIRE(sb.long_patterns == long_patterns, "sub-batch %zu: %d long patterns", si, sb.long_patterns);
        run_pairs += pairs; run_segs += segs;
        const WsLayout w = ws_layout(sb.pairs, sb.segs, sb.b0 - sb.a0);
        REQUIRE(w.total <= ws_room, "sub-batch %zu needs %zu of %zu bytes", si, w.total, ws_room);
        check_offsets("workspace", {w.tspec, w.y, w.cand, w.pair_lb, w.pairmap, w.tconst, w.tiles, w.candbuf, w.dummy, w.slb, w.acc, w.plist, w.slist,
                                    w.citems, w.tspec_low, w.ylow, w.audit_mark, w.slist2, w.dense_search, w.ditems, w.votes, w.total});
        REQUIRE(sb.lane >= 0 && sb.lane < lanes, "sub-batch %zu on lane %d of %d", si, sb.lane, lanes);
        // its schedule: a permutation of its pairs
        REQUIRE(sb.order_first >= 0 && (size_t)sb.order_first >= order_lo && (size_t)sb.order_first + (size_t)sb.pairs <= order_hi,
                "sub-batch %zu: schedule at %d", si, sb.order_first);
        std::vector<char> seen((size_t)sb.pairs, 0);
        for (int64_t i = 0; i < sb.pairs; ++i) {
            const int32_t pr = plan.order[(size_t)sb.order_first + (size_t)i];
            REQUIRE(pr >= 0 && pr < sb.pairs && !seen[(size_t)pr], "sub-batch %zu: schedule entry %" PRId64 " is %d", si, i, pr);
            seen[(size_t)pr] = 1;
        }
        // its items: every search in exactly one, of its own class and in its class's list; padded at the tail only
        REQUIRE(sb.item_first[1] == sb.item_first[0] + sb.item_count[0], "sub-batch %zu: its two item lists lie next to each other", si);
        std::vector<char> placed((size_t)(sb.b0 - sb.a0), 0);
        for (int kern = 0; kern < 2; ++kern) {
            const int cg = sb.chunk_group[kern];
            REQUIRE(cg >= 1 && (cg & (cg - 1)) == 0 && cg <= MAC_CHUNKS / 8, "sub-batch %zu: chunk_group %d", si, cg);
            REQUIRE(sb.item_first[kern] >= 0 && sb.item_count[kern] >= 0 && (size_t)sb.item_first[kern] * (1 + MAC_SPW) >= items_lo &&
                    (size_t)(sb.item_first[kern] + sb.item_count[kern]) * (1 + MAC_SPW) <= items_hi, "sub-batch %zu: items at %d", si, sb.item_first[kern]);
            for (int it = 0; it < sb.item_count[kern]; ++it) {
                const int32_t* item = plan.items.data() + (size_t)(sb.item_first[kern] + it) * (1 + MAC_SPW);
                const int cls = item[0];
                REQUIRE(cls >= 0 && cls < MAC_CLASSES && (cls < MAC_SHORT_CLASSES) == (kern == 0), "sub-batch %zu: class %d in list %d", si, cls, kern);
                REQUIRE(item[1] >= 0, "sub-batch %zu: an empty item", si);
                bool tail = false;
                for (int g = 0; g < MAC_SPW; ++g) {
                    const int32_t m = item[1 + g];
                    if (m == -1) { tail = true; continue; }
                    REQUIRE(!tail, "sub-batch %zu: a member behind the padding", si);
                    REQUIRE(m >= 0 && m < sb.b0 - sb.a0 && !placed[(size_t)m], "sub-batch %zu: member %d", si, m);
                    placed[(size_t)m] = 1;
                    const SearchDesc& d = p.descs[(size_t)(sb.a0 + m)];
                    REQUIRE(mac_class(fft_layout(d.win_start, d.n_pos, d.tmpl_len).n_seg) == cls, "sub-batch %zu: member %d in class %d", si, m, cls);
                }
            }
        }
        for (size_t m = 0; m < placed.size(); ++m) REQUIRE(placed[m], "sub-batch %zu: search %zu is in no item", si, m);
    }
    REQUIRE(run_pairs == plan.pairs && run_segs == plan.segs, "the plan's totals");
}

void check_case(const Case& c, const Planned& p) {
    const Plan& plan = p.plan;
    const int n = (int)c.req.size();
    REQUIRE(plan.lanes >= 1 && plan.lanes <= MAX_LANES && plan.ws_lane * (size_t)plan.lanes <= plan.ws_bytes, "%d lanes of %zu bytes in %zu",
            plan.lanes, plan.ws_lane, plan.ws_bytes);
    REQUIRE(plan.lanes == 1 || p.cap == 0 || plan.ws_lane * (size_t)plan.lanes <= p.cap, "lanes' workspaces %zu x %d under a cap of %zu", plan.ws_lane, plan.lanes, p.cap);
    const size_t order_end = p.whole_wanted ? plan.whole_order_first : plan.order.size();
    const size_t items_end = p.whole_wanted ? plan.whole_items_first : plan.items.size();
    check_cut(p, plan.subs, plan.ws_lane, plan.lanes, 0, order_end, 0, items_end);
    if (p.whole_wanted) {
        REQUIRE(plan.subs.size() > 1, "a pending whole cut belongs to a plan cut into parts");
        REQUIRE(p.whole_ok && !plan.whole_pending, "complete_whole_cut");
        REQUIRE(plan.ws_whole <= plan.ws_bytes, "the whole cut's workspace %zu in %zu", plan.ws_whole, plan.ws_bytes);
        REQUIRE(plan.whole_items_first + plan.whole_items_room == plan.items.size() && plan.whole_order_first + (size_t)plan.pairs == plan.order.size(),
                "the room kept for the whole cut");
        check_cut(p, plan.subs_whole, plan.ws_whole, 1, plan.whole_order_first, plan.order.size(), plan.whole_items_first, plan.items.size());
        // (batch_layout sizes the sub-batches' counter blocks for plan.subs; a whole-cut run indexes them by subs_whole)
        REQUIRE(plan.subs_whole.size() <= plan.subs.size(), "%zu sub-batches in the whole cut, %zu in the plan", plan.subs_whole.size(), plan.subs.size());
    } else {
        REQUIRE(plan.subs_whole.empty(), "a whole cut nobody asked for");
    }
    const BatchLayout& b = p.lay;
    check_offsets("batch", {b.desc, b.order, b.items, b.keys, b.flags, b.viol, b.flag_list, b.subc, b.tnorm, b.counters, b.ws, b.total});
    // flags .. counters: one span without a gap, which run_sub_batches clears in one fill
    const MemSpan fill = run_fill_span(b);
    REQUIRE(fill.off == b.flags && fill.off + fill.bytes == b.ws, "the run's fill ends where the workspace begins");
    const size_t per_search = align_up((size_t)n * sizeof(int), 256);
    REQUIRE(b.viol == b.flags + per_search && b.flag_list == b.viol + per_search && b.subc == b.flag_list + per_search, "flags, marks, flag list");
    const size_t blocks = std::max(plan.subs.size(), plan.subs_whole.size());
    REQUIRE(b.tnorm == b.subc + plan.subs.size() * SUBC_BYTES && b.tnorm - b.subc >= blocks * SUBC_BYTES, "the sub-batches' counter blocks");
    REQUIRE(b.counters == b.tnorm + align_up((size_t)plan.segs * sizeof(float), 256) && b.ws == b.counters + align_up(sizeof(RunCounters), 256),
            "norm accumulators, run counters");
    REQUIRE(b.total >= b.ws + plan.ws_bytes, "the workspace");
    REQUIRE(b.order + plan.order.size() * sizeof(int32_t) <= b.items && b.items + plan.items.size() * sizeof(int32_t) <= b.keys, "schedule and items");
}

void check_scount_words() {
    g_case = "scount";
    REQUIRE(sizeof(SubCounters) <= SUBC_SCOUNT * sizeof(int) && (SUBC_SCOUNT + SC_WORDS) * sizeof(int) <= SUBC_BYTES, "the scount words fit SUBC_BYTES");
    const int slots[] = {SC_SLIST, SC_CITEMS, SC_ANY_DENSE, SC_SLIST2, SC_DENSE_LISTED, SC_LIST3};
    for (size_t i = 0; i < sizeof(slots) / sizeof(slots[0]); ++i) {
        REQUIRE(slots[i] >= 0 && slots[i] < SC_WORDS, "slot %d", slots[i]);
        for (size_t j = 0; j < i; ++j) REQUIRE(slots[i] != slots[j], "slot %d twice", slots[i]);
    }
}

// the key's float is the smallest float >= the ranking value (the score; 1 - the coefficient), its low word all ones
void check_ranking_key() {
    g_case = "ranking_key";
    std::mt19937_64 rng(20261018);
    std::vector<double> thresholds = {0.0, -0.0, 1.0, -1.0, 0.5, 2.0, 1e-30, -1e-30, 1e-46, 1.0 + 1e-12, 1.0 - 1e-12, 0.1, (double)0.1f, 3.0e38, -3.0e38};
    for (int i = 0; i < 4000; ++i) {
        const double m = (double)(rng() >> 11) * (1.0 / 9007199254740992.0) * 4.0 - 2.0;       // [-2, 2)
        thresholds.push_back(i % 4 == 3 ? ldexp(m, -(int)(rng() % 60)) : i % 4 == 2 ? (double)(float)m : m);
    }
    const int methods[2] = {SUSHI_HIP_METHOD_SQDIFF_NORMED, SUSHI_HIP_METHOD_CCOEFF_NORMED};
    for (const double t : thresholds)
        for (const int method : methods)
            for (int clamp = 0; clamp < 2; ++clamp) {
                double u = method == SUSHI_HIP_METHOD_CCOEFF_NORMED ? 1.0 - t : t;
                if (clamp && u < 0.0) u = 0.0;
                const unsigned long long key = ranking_key(method, t, clamp != 0);
                REQUIRE((key & 0xffffffffull) == 0xffffffffull, "low word of %016llx", key);
                const uint32_t bits = (uint32_t)(key >> 32);
                float f;
                memcpy(&f, &bits, sizeof(f));
                REQUIRE((double)f >= u, "threshold %.17g, method %d: key %.9g below %.17g", t, method, f, u);
                REQUIRE((double)nextafterf(f, -INFINITY) < u, "threshold %.17g, method %d: key %.9g is not the smallest float >= %.17g", t, method, f, u);
                REQUIRE(!clamp || (f >= 0.0f && !(bits >> 31)), "threshold %.17g, method %d: key %.9g below 0", t, method, f);
            }
}

void check_parse_bound_fault() {
    g_case = "parse_bound_fault";
    const struct { const char* s; int period, phase, pair; } good[] = {{"1:0", 1, 0, -1}, {"3:1:2", 3, 1, 2}, {"2147483647:0", 2147483647, 0, -1}};
    for (const auto& g : good) {
        BoundFault f;
        REQUIRE(parse_bound_fault(g.s, &f), "\"%s\" refused", g.s);
        REQUIRE(f.period == g.period && f.phase == g.phase && f.pair == g.pair, "\"%s\" read as %d:%d:%d", g.s, f.period, f.phase, f.pair);
    }
    const char* bad[] = {"", "3", "3:3", "0:0", "3:1:", "3:1:2:4", "-3:1", " 3:1", "3:1x", "99999999999:0"};
    for (const char* s : bad) {
        BoundFault f;
        REQUIRE(!parse_bound_fault(s, &f), "\"%s\" accepted", s);
        REQUIRE(f.period == 0 && f.phase == 0 && f.pair == -1, "\"%s\" refused but written", s);
    }
}

}  // namespace

int main(int argc, char** argv) {
    const bool dumping = argc == 2 && !strcmp(argv[1], "--dump");
    const bool requests = argc == 3 && !strcmp(argv[1], "--requests");
    if (argc != 1 && !dumping && !requests) { fprintf(stderr, "usage: %s [--dump | --requests DIR]\n", argv[0]); return 2; }
    for (const Case& c : cases()) {
        if (requests) {
            const std::string path = std::string(argv[2]) + "/" + c.name + ".req";
            FILE* f = fopen(path.c_str(), "wb");
            if (!f || fwrite(c.req.data(), sizeof(SushiHipRequest), c.req.size(), f) != c.req.size() || fclose(f) != 0) {
                fprintf(stderr, "cannot write %s\n", path.c_str());
                return 2;
            }
            continue;
        }
        g_case = c.name;
        const Planned p = plan_case(c);
        if (dumping) dump(c, p);
        else if (p.rc == SUSHI_HIP_OK) check_case(c, p);
    }
    if (argc == 1) {
        check_scount_words();
        check_ranking_key();
        check_parse_bound_fault();
    }
    return 0;
}
