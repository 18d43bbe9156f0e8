// What a batch handle holds about its requests (sushi_amd/csrc/batch_core.hpp) on the CPU: what a staged batch must be, stated as
// checks, over the table of cases of tests/batch_cases.hpp (FFT path, float32 streams just long enough for the case's requests).
// usage: host_batch_check                   checks every case -- the upload image, refusals, the plan cache, the life of a handle as
//                                           two states, the whole-cut spans, the variant; exit 1 with a message on the first violation
//        host_batch_check --dump            one JSON record per case and line: return code, accounting, size and FNV-1a digest of the
//                                           image, and (a plan with a whole cut, after complete_whole_cut) of each of the two spans
//                                           a run uploads, with its device offset (tests/golden/batch_stage.json is this output)
//        host_batch_check --image DIR       writes every staged case's requests (SushiHipRequest records) to DIR/<case>.req, its
//                                           image to DIR/<case>.img and its whole-cut spans to DIR/<case>.whole0 / .whole1: what
//                                           tests/test_batch_host.py hands to the library and compares device memory with
//        host_batch_check --stage REQ CAP LANES OUT    stages the SushiHipRequest records of the file REQ under the workspace cap
//                                           CAP (bytes) and the lanes override LANES ("" for none), writes the image to OUT
// Built by tests/test_batch_host.py with g++ -O2 -std=c++17, and once more with -O1 -g -fsanitize=address,undefined.
#include "../sushi_amd/csrc/sushi_geometry.hpp"
#include "../sushi_amd/csrc/plan_core.hpp"
#include "../sushi_amd/csrc/batch_core.hpp"
#include "batch_cases.hpp"

#include <cinttypes>

using namespace sushi;
using namespace batch_cases;

namespace {

std::string g_case;
#define REQUIRE(cond, ...) do { if (!(cond)) { fprintf(stderr, "%s: %s -- ", g_case.c_str(), #cond); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); exit(1); } } while (0)

// ---- digests ----
struct Fnv {
    uint64_t h = 0xcbf29ce484222325ull;
    void bytes(const void* p, size_t n) { for (size_t i = 0; i < n; ++i) { h ^= ((const unsigned char*)p)[i]; h *= 0x100000001b3ull; } }
    template <class T> void value(const T& v) { bytes(&v, sizeof(v)); }
    template <class T> void values(const std::vector<T>& v) { value(v.size()); if (!v.empty()) bytes(v.data(), v.size() * sizeof(T)); }
};
uint64_t fnv1a(const void* p, size_t n) { Fnv f; f.bytes(p, n); return f.h; }

// (field by field: a SubBatch has padding)
void digest_subs(Fnv& f, const std::vector<SubBatch>& subs) {
    f.value(subs.size());
    for (const SubBatch& s : subs) {
        f.value(s.a0); f.value(s.b0); f.value(s.pairs); f.value(s.segs); f.value(s.first_pair); f.value(s.first_seg); f.value(s.item_first);
        f.value(s.item_count); f.value(s.chunk_group); f.value(s.long_patterns); f.value(s.lane); f.value(s.order_first);
    }
}
uint64_t digest(const Plan& p) {
    Fnv f;
    digest_subs(f, p.subs); digest_subs(f, p.subs_whole);
    f.value(p.whole_pending); f.value(p.whole_order_first); f.value(p.whole_items_first); f.value(p.whole_items_room); f.value(p.ws_whole);
    f.values(p.order); f.values(p.items);
    f.value(p.pairs); f.value(p.segs); f.value(p.ws_bytes); f.value(p.ws_lane); f.value(p.lanes);
    return f.h;
}
// everything a state holds
uint64_t digest(const BatchPlanState& s) {
    Fnv f;
    f.values(s.descs); f.value(digest(s.plan));
    const BatchLayout& l = s.lay;
    const size_t offsets[] = {l.desc, l.keys, l.flags, l.viol, l.flag_list, l.subc, l.tnorm, l.counters, l.order, l.items, l.ws, l.total};
    f.value(offsets);
    f.value(s.n_tiles); f.value(s.flops); f.value(s.algorithmic_bytes); f.values(s.upload);
    return f.h;
}

// ---- a case, staged ----
BatchSpec spec_of(const std::vector<SushiHipRequest>& req, size_t cap, int path = SUSHI_HIP_PATH_FFT, int tile = FFT_PATH_TILE) {
    BatchSpec s{path, tile, cap, SIZE_MAX, 0, 0, 4.0};
    for (const SushiHipRequest& r : req) {
        s.src_len = std::max<int64_t>(s.src_len, r.tmpl_off + r.tmpl_len);
        s.dst_len = std::max<int64_t>(s.dst_len, r.win_start + (int64_t)r.n_pos + r.tmpl_len - 1);
    }
    return s;
}
BatchSpec spec_of(const Case& c) {
    std::vector<SearchDesc> descs;
    int64_t tiles = 0;
    const bool ok = make_descs(c.req.data(), (int)c.req.size(), FFT_PATH_TILE, descs, &tiles) == SUSHI_HIP_OK;
    return spec_of(c.req, ok ? case_cap(c, descs) : c.cap);
}
int stage(const Case& c, const BatchSpec& spec, BatchPlanState& out) {
    PlanCache none;
    return stage_batch(c.req.data(), (int)c.req.size(), spec, c.lanes.c_str(), none, out);
}

// ---- the checks ----
// the image: descriptors at 0, the schedule and the items at their layout offsets, zeros elsewhere; its size; the accounting
void check_image(const Case& c, const BatchPlanState& s) {
    const size_t n = c.req.size();
    const BatchLayout& l = s.lay;
    const Plan& p = s.plan;
    REQUIRE(l.desc == 0, "the image starts the batch's memory");
    REQUIRE(s.upload.size() == l.items + align_up(p.items.size() * sizeof(int32_t), 256) - l.desc && s.upload.size() == l.keys, "image of %zu bytes", s.upload.size());
    std::vector<char> want(s.upload.size(), 0);
    memcpy(want.data(), s.descs.data(), n * sizeof(SearchDesc));
    for (size_t i = 0; i < p.order.size(); ++i) memcpy(want.data() + (l.order - l.desc) + i * sizeof(int32_t), &p.order[i], sizeof(int32_t));
    for (size_t i = 0; i < p.items.size(); ++i) memcpy(want.data() + (l.items - l.desc) + i * sizeof(int32_t), &p.items[i], sizeof(int32_t));
    REQUIRE(n * sizeof(SearchDesc) <= l.order - l.desc && l.order + p.order.size() * sizeof(int32_t) <= l.items, "the parts do not overlap");
    REQUIRE(want == s.upload, "the image's contents");
    double flops = 0.0, bytes = 0.0;
    for (const SushiHipRequest& r : c.req) {
        flops += 2.0 * (double)r.n_pos * (double)r.tmpl_len;
        bytes += 4.0 * ((double)r.n_pos + r.tmpl_len - 1) + 4.0 * r.tmpl_len + 8.0;
    }
    REQUIRE(s.flops == flops && s.algorithmic_bytes == bytes, "accounting %.17g flop, %.17g bytes", s.flops, s.algorithmic_bytes);
    // the direct path: the descriptors alone
    BatchPlanState d;
    REQUIRE(stage(c, spec_of(c.req, 0, SUSHI_HIP_PATH_DIRECT, 1024), d) == SUSHI_HIP_OK, "the direct path refuses");
    REQUIRE(d.upload.size() == align_up(n * sizeof(SearchDesc), 256) && d.lay.total == batch_layout((int)n, SUSHI_HIP_PATH_DIRECT, 0, 0, 0, 0, 0).total &&
            d.plan.subs.empty() && d.plan.order.empty(), "the direct path's image and layout");
    REQUIRE(memcmp(d.upload.data(), d.descs.data(), n * sizeof(SearchDesc)) == 0, "the direct path's descriptors");
    for (size_t i = n * sizeof(SearchDesc); i < d.upload.size(); ++i) REQUIRE(d.upload[i] == 0, "byte %zu behind the direct path's descriptors", i);
    int64_t tiles = 0;
    for (const SushiHipRequest& r : c.req) tiles += (r.n_pos + 1023) / 1024;
    REQUIRE(d.n_tiles == tiles, "%" PRId64 " tiles of 1024", d.n_tiles);
}

// a stage that is refused has written nothing but the state it was given: `held` (what the handle runs) stays byte for byte
void check_refusals(const std::vector<Case>& all, const Case& held_case) {
    BatchPlanState held, spare;
    g_case = held_case.name;
    const BatchSpec held_spec = spec_of(held_case);
    REQUIRE(stage(held_case, held_spec, held) == SUSHI_HIP_OK, "the held case");
    const uint64_t before = digest(held);
    for (const Case& c : all) {
        g_case = c.name + " (refusals)";
        BatchSpec spec = spec_of(c);
        BatchPlanState first;
        const int rc = stage(c, spec, first);
        if (rc != SUSHI_HIP_OK) {
            REQUIRE(c.name[0] == 'g' && rc == SUSHI_HIP_EINVAL, "rc %d", rc);
            REQUIRE(stage(c, spec, spare) == rc && digest(held) == before, "a refused stage");
            continue;
        }
        REQUIRE(c.name[0] != 'g', "a refusing case was staged");
        // memory one byte short; exactly enough; a stream one sample short
        spec.mem_bytes = first.lay.total - 1;
        REQUIRE(stage(c, spec, spare) == SUSHI_HIP_ENOSPACE && digest(held) == before, "one byte short");
        spec.mem_bytes = first.lay.total;
        REQUIRE(stage(c, spec, spare) == SUSHI_HIP_OK && digest(spare) == digest(first), "exactly enough memory, into a state a refusal left");
        --spec.dst_len;
        REQUIRE(stage(c, spec, spare) == SUSHI_HIP_EINVAL && digest(held) == before, "a window past the destination");
        ++spec.dst_len; --spec.src_len;
        REQUIRE(stage(c, spec, spare) == SUSHI_HIP_EINVAL && digest(held) == before, "a pattern past the source");
    }
}

// the plan sushi_hip_batch_bytes remembers is taken once, for its own key only, and is the plan make_plan makes
void check_cache(const Case& c) {
    g_case = c.name + " (cache)";
    const BatchSpec spec = spec_of(c);
    const int n = (int)c.req.size();
    BatchPlanState fresh;
    REQUIRE(stage(c, spec, fresh) == SUSHI_HIP_OK, "the case");
    PlanCache cache;
    auto remember = [&] {
        std::vector<SearchDesc> descs;
        int64_t tiles = 0;
        Plan plan;
        REQUIRE(make_descs(c.req.data(), n, FFT_PATH_TILE, descs, &tiles) == SUSHI_HIP_OK && make_plan(descs, spec.ws_cap, c.lanes.c_str(), plan) == SUSHI_HIP_OK, "a plan");
        cache.remember(c.req.data(), n, spec.ws_cap, c.lanes.c_str(), std::move(plan));
    };
    remember();
    Plan got;
    for (size_t byte = 0; byte < c.req.size() * sizeof(SushiHipRequest); byte += 7) {
        std::vector<SushiHipRequest> other = c.req;
        ((unsigned char*)other.data())[byte] ^= 1;
        REQUIRE(!cache.take(other.data(), n, spec.ws_cap, c.lanes.c_str(), got), "taken with byte %zu of the requests changed", byte);
    }
    REQUIRE(!cache.take(c.req.data(), n - 1, spec.ws_cap, c.lanes.c_str(), got), "taken for fewer requests");
    REQUIRE(!cache.take(c.req.data(), n, spec.ws_cap + 1, c.lanes.c_str(), got), "taken under another cap");
    REQUIRE(!cache.take(c.req.data(), n, spec.ws_cap, (c.lanes + "0").c_str(), got), "taken under another lanes override");
    REQUIRE(c.lanes.empty() == cache.take(c.req.data(), n, spec.ws_cap, nullptr, got), "no override and an empty one are one key");
    if (c.lanes.empty()) remember();
    REQUIRE(cache.valid && cache.take(c.req.data(), n, spec.ws_cap, c.lanes.c_str(), got) && !cache.valid, "not taken for its own key");
    REQUIRE(digest(got) == digest(fresh.plan) && got.order == fresh.plan.order && got.items == fresh.plan.items, "the remembered plan is not the fresh one");
    REQUIRE(!cache.take(c.req.data(), n, spec.ws_cap, c.lanes.c_str(), got), "taken twice");
    // ... and through stage_batch: the same state as without a cache, and the cache empty behind it
    remember();
    BatchPlanState staged;
    REQUIRE(stage_batch(c.req.data(), n, spec, c.lanes.c_str(), cache, staged) == SUSHI_HIP_OK && !cache.valid, "stage_batch leaves the cache full");
    REQUIRE(digest(staged) == digest(fresh), "a state staged from the cache");
}

// The life of a handle as sushi_fft.hip leads it: two states; requests are staged into the spare, and the two change places only
// when the stage was not refused.
void check_life(const Case& a, const Case& b, const Case& refused, bool short_of_memory) {
    g_case = "life: " + a.name + ", " + b.name + ", " + refused.name + (short_of_memory ? " one byte short" : "");
    BatchPlanState states[2], *now = &states[0], *spare = &states[1];
    REQUIRE(stage(a, spec_of(a), *spare) == SUSHI_HIP_OK, "A");
    std::swap(now, spare);
    const uint64_t first_a = digest(*now);
    REQUIRE(stage(b, spec_of(b), *spare) == SUSHI_HIP_OK, "B");
    std::swap(now, spare);
    const uint64_t is_b = digest(*now);
    BatchSpec spec = spec_of(refused);
    if (short_of_memory) {
        BatchPlanState whole;
        REQUIRE(stage(refused, spec, whole) == SUSHI_HIP_OK, "C with memory");
        spec.mem_bytes = whole.lay.total - 1;
    }
    REQUIRE(stage(refused, spec, *spare) != SUSHI_HIP_OK, "C was not refused");
    REQUIRE(digest(*now) == is_b, "the current state after a refused C");
    const size_t room[] = {spare->descs.capacity(), spare->upload.capacity(), spare->plan.subs.capacity(), spare->plan.subs_whole.capacity(),
                           spare->plan.order.capacity(), spare->plan.items.capacity()};
    const void* const at[] = {spare->descs.data(), spare->upload.data(), spare->plan.subs.data(), spare->plan.order.data(), spare->plan.items.data()};
    REQUIRE(stage(a, spec_of(a), *spare) == SUSHI_HIP_OK, "A again");
    std::swap(now, spare);
    REQUIRE(digest(*now) == first_a, "A again is not the first A");
    REQUIRE(digest(*spare) == is_b, "B, now the spare");
    const size_t room_now[] = {now->descs.capacity(), now->upload.capacity(), now->plan.subs.capacity(), now->plan.subs_whole.capacity(),
                               now->plan.order.capacity(), now->plan.items.capacity()};
    const void* const at_now[] = {now->descs.data(), now->upload.data(), now->plan.subs.data(), now->plan.order.data(), now->plan.items.data()};
    for (size_t i = 0; i < sizeof(room) / sizeof(room[0]); ++i) REQUIRE(room[i] == room_now[i], "vector %zu of the spare: room %zu, now %zu", i, room[i], room_now[i]);
    for (size_t i = 0; i < sizeof(at) / sizeof(at[0]); ++i) REQUIRE(at[i] == at_now[i], "vector %zu of the spare was reallocated", i);
}

// the two spans a run uploads after complete_whole_cut: exactly the tails kept for the whole cut, inside the image's room for them
void check_whole_cut(const BatchPlanState& s, const std::array<UploadSpan, 2>& up) {
    const Plan& p = s.plan;
    const BatchLayout& l = s.lay;
    const struct { size_t base, first, size, end; const int32_t* data; } part[2] = {{l.order, p.whole_order_first, p.order.size(), l.items, p.order.data()},
                                                                                     {l.items, p.whole_items_first, p.items.size(), l.keys, p.items.data()}};
    for (int k = 0; k < 2; ++k) {
        const UploadSpan& u = up[k];
        REQUIRE(u.dev_off >= part[k].base && (u.dev_off - part[k].base) % sizeof(int32_t) == 0 && u.bytes % sizeof(int32_t) == 0, "span %d at %zu, %zu bytes", k, u.dev_off, u.bytes);
        const size_t first = (u.dev_off - part[k].base) / sizeof(int32_t), count = u.bytes / sizeof(int32_t);
        REQUIRE(first == part[k].first && first + count == part[k].size && count > 0, "span %d is ints [%zu, %zu)", k, first, first + count);
        REQUIRE(u.host == part[k].data + first, "span %d reads from elsewhere", k);
        REQUIRE(u.dev_off + u.bytes <= part[k].end && u.dev_off + u.bytes <= l.desc + s.upload.size(), "span %d leaves its room", k);
    }
}

// resolve_variant against what the two entry points did, each for itself, before it existed
void check_variant(const Case& c) {
    const int tiles[3] = {1024, 4096, 16384}, n = (int)c.req.size();
    auto old_choice = [&] {
        const int waves[3] = {1, 4, 4};
        int best = 0;
        for (int v = 0; v < 3; ++v) {
            int64_t nt = 0;
            for (int k = 0; k < n; ++k) nt += (c.req[k].n_pos + tiles[v] - 1) / tiles[v];
            if (nt * waves[v] >= 4096) best = v;
        }
        return best;
    };
    auto old_answer = [&](int path, int variant) {
        if (path == SUSHI_HIP_PATH_FFT) variant = 3 - 1;
        else if (variant < 0) variant = old_choice();
        return variant >= 3 ? -1 : variant;
    };
    for (int variant = -1; variant <= 3; ++variant) {
        const int paths[2] = {SUSHI_HIP_PATH_FFT, SUSHI_HIP_PATH_DIRECT};
        for (const int path : paths)
            REQUIRE(resolve_variant(path, variant, c.req.data(), n, 3, tiles) == old_answer(path, variant), "path %d, variant %d", path, variant);
    }
    REQUIRE(resolve_variant(SUSHI_HIP_PATH_DIRECT, 3, c.req.data(), n, 3, tiles) == -1 && resolve_variant(SUSHI_HIP_PATH_DIRECT, 2, c.req.data(), n, 3, tiles) == 2, "one past the last");
}

bool write_file(const std::string& path, const void* p, size_t bytes) {
    FILE* f = fopen(path.c_str(), "wb");
    const bool ok = f && fwrite(p, 1, bytes, f) == bytes;
    if (!(f && fclose(f) == 0 && ok)) fprintf(stderr, "cannot write %s\n", path.c_str());
    return ok;
}

}  // namespace

int main(int argc, char** argv) {
    const bool checking = argc == 1, dumping = argc == 2 && !strcmp(argv[1], "--dump"), images = argc == 3 && !strcmp(argv[1], "--image");
    if (argc == 6 && !strcmp(argv[1], "--stage")) {
        Case c{"staged", {}, CAP_GIVEN, (size_t)strtoull(argv[3], nullptr, 10), argv[4]};
        FILE* f = fopen(argv[2], "rb");
        SushiHipRequest r;
        while (f && fread(&r, sizeof(r), 1, f) == 1) c.req.push_back(r);
        if (f) fclose(f);
        BatchPlanState s;
        const int rc = c.req.empty() ? SUSHI_HIP_EINVAL : stage(c, spec_of(c), s);
        if (rc != SUSHI_HIP_OK) { fprintf(stderr, "%s: rc %d\n", argv[2], rc); return 1; }
        return write_file(argv[5], s.upload.data(), s.upload.size()) ? 0 : 2;
    }
    if (!checking && !dumping && !images) { fprintf(stderr, "usage: %s [--dump | --image DIR | --stage REQ CAP LANES OUT]\n", argv[0]); return 2; }
    const std::vector<Case> all = cases();
    for (const Case& c : all) {
        g_case = c.name;
        BatchPlanState s;
        const int rc = stage(c, spec_of(c), s);
        if (dumping) printf("{\"name\":\"%s\",\"rc\":%d", c.name.c_str(), rc);
        if (rc == SUSHI_HIP_OK) {
            if (checking) { check_image(c, s); check_variant(c); }
            if (dumping)
                printf(",\"n_tiles\":%" PRId64 ",\"flops\":%.17g,\"algorithmic_bytes\":%.17g,\"total\":%zu,\"image_bytes\":%zu,\"image_fnv\":\"%016" PRIx64 "\",\"whole\":",
                       s.n_tiles, s.flops, s.algorithmic_bytes, s.lay.total, s.upload.size(), fnv1a(s.upload.data(), s.upload.size()));
            if (images && !(write_file(std::string(argv[2]) + "/" + c.name + ".req", c.req.data(), c.req.size() * sizeof(SushiHipRequest)) &&
                            write_file(std::string(argv[2]) + "/" + c.name + ".img", s.upload.data(), s.upload.size()))) return 2;
            const bool whole = s.plan.whole_pending;
            if (whole) {
                REQUIRE(complete_whole_cut(s.descs, s.plan), "complete_whole_cut");
                const std::array<UploadSpan, 2> up = whole_cut_upload(s.plan, s.lay);
                if (checking) check_whole_cut(s, up);
                for (int k = 0; k < 2; ++k) {
                    if (dumping) printf("%s[%zu,%zu,\"%016" PRIx64 "\"]", k ? "," : "[", up[k].dev_off, up[k].bytes, fnv1a(up[k].host, up[k].bytes));
                    if (images && !write_file(std::string(argv[2]) + "/" + c.name + ".whole" + (k ? "1" : "0"), up[k].host, up[k].bytes)) return 2;
                }
            }
            if (dumping) printf(whole ? "]" : "null");
        }
        if (dumping) printf("}\n");
    }
    if (checking) {
        auto named = [&](const char* name) -> const Case& {
            for (const Case& c : all) if (c.name == name) return c;
            fprintf(stderr, "no case %s\n", name);
            exit(2);
        };
        check_refusals(all, named("b_four_4x2_cap0"));
        for (const char* name : {"a_one", "b_four_cap0", "b_four_4x2_cap1", "d_mixed_halfway", "e_130_8x2_halfway"}) check_cache(named(name));
        check_life(named("b_four_4x2_cap0"), named("d_mixed_halfway"), named("g_n_pos_0"), false);
        check_life(named("b_four_4x2_cap0"), named("b_four_cap0"), named("g_pairs_past_int"), false);
        check_life(named("d_mixed_halfway"), named("b_four_4x2_cap0"), named("e_130_8x2_halfway"), true);
        check_life(named("b_four_cap0"), named("a_one"), named("b_four_cap0"), true);
    }
    return 0;
}
