// The host side of a prepared stream, of a curve call and of a retime call on the CPU: sushi_amd/csrc/stream_core.hpp (the table of
// a stream's parts), curve_core.hpp (stage_curves) and the host part of retime_core.hpp (stage_retime), with the request rule they
// share with a batch (sushi_geometry.hpp request_fits).  What each must give is stated here, independently of the code under test.
// usage: host_stream_check                  checks every case; exit 1 with a message on the first violation
//        host_stream_check --dump           one JSON record per case and line (tests/golden/stream_stage.json is this output):
//                                           stream: total bytes and (offset from the stream's buffer, bytes) of every SUSHI_HIP_VIEW_*,
//                                           offset -1 for a part that does not exist; curves / retime: the launch facts, size and
//                                           FNV-1a digest of the upload image
//        host_stream_check --stage-curves REQ DTYPE DST_N SRC_N OUT      stages the SushiHipRequest records of the file REQ, writes the
//                                           image to OUT
//        host_stream_check --stage-retime SEG DTYPE N_IN N_OUT OUT_ADDR OUT    the same for SushiHipRetimeSegment records and an
//                                           output at the device address OUT_ADDR (decimal)
// Built by tests/test_stream_host.py with g++ -O2 -std=c++17, and once more with -O1 -g -fsanitize=address,undefined.
#include "../sushi_amd/csrc/sushi_geometry.hpp"
#include "../sushi_amd/csrc/stream_core.hpp"
#include "../sushi_amd/csrc/curve_core.hpp"
#include "../sushi_amd/csrc/retime_core.hpp"
#include "batch_cases.hpp"

#include <cinttypes>

using namespace sushi;
using batch_cases::request;

namespace {

std::string g_case;
#define REQUIRE(cond, ...) do { if (!(cond)) { fprintf(stderr, "%s: %s -- ", g_case.c_str(), #cond); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); exit(1); } } while (0)

uint64_t fnv1a(const void* p, size_t n) {
    uint64_t h = 0xcbf29ce484222325ull;
    for (size_t i = 0; i < n; ++i) { h ^= ((const unsigned char*)p)[i]; h *= 0x100000001b3ull; }
    return h;
}

size_t up256(size_t x) { return (x + 255) / 256 * 256; }
const int DTYPES[2] = {SUSHI_HIP_U8, SUSHI_HIP_F32};

// =========================================================================================================================== streams
const int64_t STREAM_N[] = {1, PB - 1, PB, PB + 1, 3 * COARSE_G + 1, 2 * FFT_N + 7, 347000000};
constexpr int N_VIEWS = 11;

// What the library gave before there was a table (commit e6d26e5: stream_layout and the pointer fill of sushi_hip_stream_create in
// sushi_stream.hip, sushi_hip_stream_add_spectra in sushi_fft.hip, the switch of sushi_hip_stream_view), written out once.
struct Old {
    size_t xc, s1, s2, urel, srel, base, coarse, spec, total;     // the eight parts of the stream's buffer, in this order
    size_t spec_low, znorm;                                       // (from the spectra buffer's start)
    size_t part_bytes[8];
    size_t view_off[N_VIEWS], view_bytes[N_VIEWS];                // offsets from the buffer that holds the part
    int64_t nb, nc, norm_stride;
};
Old old_stream(int64_t n, bool searchable) {
    Old o;
    o.nb = (n + 4096 - 1) / 4096;
    o.nc = n / 256 + 2;
    const size_t rows = (size_t)((n + 4096 - 1) / 4096 + 1), norm_bytes = up256(rows * 4);
    const size_t whole = rows * 16384 * 4, low = rows * 16384, spectra_total = whole + low + 3 * norm_bytes;
    o.norm_stride = (int64_t)(norm_bytes / 4);
    const size_t bytes[8] = {(size_t)n * 4, (size_t)(n + 1) * 8, (size_t)(n + 1) * 8, (size_t)(n + 1) * 4, (size_t)(n + 1) * 2 * 4,
                             (size_t)(2 * (o.nb + 1) + 2) * 8, (size_t)2 * (size_t)(n / 256 + 2) * 8, searchable ? spectra_total : 0};
    size_t* const at[8] = {&o.xc, &o.s1, &o.s2, &o.urel, &o.srel, &o.base, &o.coarse, &o.spec};
    size_t off = 0;
    for (int p = 0; p < 8; ++p) { *at[p] = off; o.part_bytes[p] = bytes[p]; off += up256(bytes[p]); }
    o.total = off;
    o.spec_low = whole; o.znorm = whole + low;
    const size_t nb1 = (size_t)(o.nb + 1) * 8;
    const struct { int view; size_t off, bytes; } views[N_VIEWS] = {
        {SUSHI_HIP_VIEW_XC, o.xc, (size_t)n * 4}, {SUSHI_HIP_VIEW_S1, o.s1, (size_t)(n + 1) * 8}, {SUSHI_HIP_VIEW_S2, o.s2, (size_t)(n + 1) * 8},
        {SUSHI_HIP_VIEW_UREL, o.urel, (size_t)(n + 1) * 4}, {SUSHI_HIP_VIEW_BASE, o.base, nb1}, {SUSHI_HIP_VIEW_SPECTRA, 0, whole},
        {SUSHI_HIP_VIEW_SPECTRA_LOW, o.spec_low, whole / 4}, {SUSHI_HIP_VIEW_ZNORM_REST, o.znorm, (size_t)3 * (size_t)o.norm_stride * 4},
        {SUSHI_HIP_VIEW_USREL, o.srel, (size_t)(n + 1) * 2 * 4}, {SUSHI_HIP_VIEW_BASE1, o.base + nb1, nb1},
        {SUSHI_HIP_VIEW_COARSE, o.coarse, (size_t)2 * (size_t)o.nc * 8}};
    for (const auto& v : views) { o.view_off[v.view] = v.off; o.view_bytes[v.view] = v.bytes; }
    return o;
}
bool spectra_view(int v) { return v == SUSHI_HIP_VIEW_SPECTRA || v == SUSHI_HIP_VIEW_SPECTRA_LOW || v == SUSHI_HIP_VIEW_ZNORM_REST; }

// a handle as sushi_hip_stream_create fills it, in a buffer at `mem` (an address only: nothing is read through it)
SushiHipStream handle_of(int64_t n, int dtype, bool searchable, char* mem, const void* raw) {
    const StreamLayout l = stream_layout(n, searchable);
    SushiHipStream s;
    fill_stream(s, raw, dtype, n, mem, l);
    if (searchable) fill_spectra(s, mem + l.spec, l);
    return s;
}
char* const FAKE_MEM = reinterpret_cast<char*>((uintptr_t)1 << 44);

void check_stream(int64_t n, int dtype, bool searchable) {
    g_case = "stream n=" + std::to_string(n) + (dtype == SUSHI_HIP_U8 ? " u8" : " f32") + (searchable ? " searchable" : "");
    const Old o = old_stream(n, searchable);
    const StreamLayout l = stream_layout(n, searchable);
    REQUIRE(stream_bytes(n, dtype, searchable) == o.total && l.total == o.total, "total %zu, was %zu", l.total, o.total);
    REQUIRE(l.nb == o.nb && l.nc == o.nc && l.spec == o.spec, "nb %" PRId64 ", nc %" PRId64 ", spectra at %zu", l.nb, l.nc, l.spec);
    // The parts of each buffer lie in the table's order without overlap; each begins on a multiple of 256 bytes -- but the block
    // bases of s1 and the stats, which are the tail of the part that begins with the block bases of s2 -- and the buffer ends
    // where its last part does, rounded up.
    size_t end[2] = {0, 0};
    for (int p = 0; p < STREAM_PARTS; ++p) {
        const StreamPart& q = l.part[p];
        size_t& e = end[q.in_spectra];
        REQUIRE(q.in_spectra == (p >= PART_SPECTRA) && q.bytes > 0, "part %d", p);
        REQUIRE(q.offset >= e, "part %d at %zu begins inside the one before it, which ends at %zu", p, q.offset, e);
        if (p == PART_BASE1 || p == PART_STATS) REQUIRE(q.offset == e, "part %d at %zu is not right behind the one before it", p, q.offset);
        else REQUIRE(q.offset % 256 == 0 && q.offset == up256(e), "part %d at %zu", p, q.offset);
        e = q.offset + q.bytes;
    }
    REQUIRE(l.spec == up256(end[0]) && l.total == l.spec + (searchable ? up256(end[1]) : 0), "the buffer ends at %zu", l.total);
    REQUIRE(end[1] == spectra_layout(n).total && end[1] % 256 == 0, "the spectra buffer ends at %zu", end[1]);
    // the parts where they were
    const size_t was[STREAM_PARTS] = {o.xc, o.s1, o.s2, o.urel, o.srel, o.base, o.base + (size_t)(o.nb + 1) * 8, o.base + (size_t)(2 * (o.nb + 1)) * 8,
                                      o.coarse, 0, o.spec_low, o.znorm};
    for (int p = 0; p < STREAM_PARTS; ++p) REQUIRE(l.part[p].offset == was[p], "part %d at %zu, was at %zu", p, l.part[p].offset, was[p]);
    REQUIRE(l.part[PART_STATS].offset + l.part[PART_STATS].bytes - l.part[PART_BASE].offset == o.part_bytes[5], "block bases and stats");
    // the handle
    const char raw = 0;
    const SushiHipStream s = handle_of(n, dtype, searchable, FAKE_MEM, &raw);
    char* const m = FAKE_MEM;
    REQUIRE(s.raw == &raw && s.dtype == dtype && s.n == n && s.blocks == o.nb && s.nc == o.nc, "the handle's scalars");
    REQUIRE((char*)s.xc == m + o.xc && (char*)s.s1 == m + o.s1 && (char*)s.s2 == m + o.s2 && (char*)s.urel == m + o.urel && (char*)s.usrel == m + o.srel, "the handle's arrays");
    REQUIRE((char*)s.base == m + o.base && s.base1 == s.base + (o.nb + 1) && s.stats == s.base + 2 * (o.nb + 1) && (char*)s.coarse == m + o.coarse, "the handle's tables");
    if (searchable)
        REQUIRE((char*)s.spec == m + o.spec && (char*)s.spec_low == m + o.spec + o.spec_low && (char*)s.znorm_rest == m + o.spec + o.znorm && s.norm_stride == o.norm_stride, "the handle's spectra");
    else
        REQUIRE(!s.spec && !s.spec_low && !s.znorm_rest && s.norm_stride == 0, "spectra that were not attached");
    // every view
    for (int v = 0; v < N_VIEWS; ++v) {
        const void* p = &raw;
        size_t bytes = 1;
        REQUIRE(stream_view(s, v, &p, &bytes) == SUSHI_HIP_OK, "view %d", v);
        if (spectra_view(v) && !searchable) { REQUIRE(p == nullptr && bytes == 0, "view %d of spectra that do not exist", v); continue; }
        const char* buf = spectra_view(v) ? m + o.spec : m;
        REQUIRE(p == buf + o.view_off[v] && bytes == o.view_bytes[v], "view %d: %zu bytes at %td, were %zu at %zu", v, bytes, (const char*)p - buf, o.view_bytes[v], o.view_off[v]);
    }
    const void* p = nullptr;
    size_t bytes = 0;
    REQUIRE(stream_view(s, N_VIEWS, &p, &bytes) == SUSHI_HIP_EINVAL && stream_view(s, NO_VIEW, &p, &bytes) == SUSHI_HIP_EINVAL && !p, "a view that does not exist");
    // spectra attached later, in a buffer of their own (what a DeviceStream does)
    if (!searchable) {
        SushiHipStream later = s;
        char* const sm = FAKE_MEM + ((size_t)1 << 40);
        fill_spectra(later, sm, l);
        REQUIRE((char*)later.spec == sm && (char*)later.spec_low == sm + o.spec_low && (char*)later.znorm_rest == sm + o.znorm && later.norm_stride == o.norm_stride && later.xc == s.xc, "spectra attached later");
        for (int v = 0; v < N_VIEWS; ++v)
            if (spectra_view(v)) REQUIRE(stream_view(later, v, &p, &bytes) == SUSHI_HIP_OK && p == sm + o.view_off[v] && bytes == o.view_bytes[v], "view %d of spectra attached later", v);
    }
}

void dump_stream(int64_t n, int dtype, bool searchable) {
    const SushiHipStream s = handle_of(n, dtype, searchable, FAKE_MEM, nullptr);
    printf("{\"kind\":\"stream\",\"n\":%" PRId64 ",\"dtype\":%d,\"searchable\":%d,\"total\":%zu,\"views\":[", n, dtype, (int)searchable, stream_bytes(n, dtype, searchable));
    for (int v = 0; v < N_VIEWS; ++v) {
        const void* p = nullptr;
        size_t bytes = 0;
        if (stream_view(s, v, &p, &bytes) != SUSHI_HIP_OK) exit(1);
        printf("%s[%" PRId64 ",%zu]", v ? "," : "", p ? (int64_t)((const char*)p - FAKE_MEM) : (int64_t)-1, bytes);
    }
    printf("]}\n");
}

// ============================================================================================================================ curves
struct CurveCase { std::string name; std::vector<SushiHipRequest> req; };
std::vector<CurveCase> curve_cases() {
    std::vector<CurveCase> c;
    c.push_back({"one", {request(0, 0, 1, 1)}});
    c.push_back({"three", {request(5, 3, 100, 1), request(0, 700, 36000, 256), request(40000, 11, 77, 1025)}});
    // float32: items of 1024 positions from 2048 of them on
    c.push_back({"below_the_switch", {request(0, 0, 9, 2047 * 1024)}});
    c.push_back({"at_the_switch", {request(0, 0, 9, 2047 * 1024 + 1)}});
    c.push_back({"below_the_switch_many", std::vector<SushiHipRequest>(2047, request(3, 1, 50, 1024))});
    c.push_back({"at_the_switch_many", std::vector<SushiHipRequest>(2047, request(3, 1, 50, 1024))});
    c.back().req.push_back(request(0, 0, 1, 1));
    return c;
}
void lengths_for(const std::vector<SushiHipRequest>& req, int64_t* dst_n, int64_t* src_n) {
    *dst_n = *src_n = 1;
    for (const SushiHipRequest& r : req) {
        *src_n = std::max<int64_t>(*src_n, r.tmpl_off + r.tmpl_len);
        *dst_n = std::max<int64_t>(*dst_n, r.win_start + (int64_t)r.n_pos + r.tmpl_len - 1);
    }
}

void check_staged_curves(const std::vector<SushiHipRequest>& req, int dtype, int64_t dst_n, int64_t src_n) {
    const int n = (int)req.size();
    CurveStage s;
    REQUIRE(stage_curves(req.data(), n, dtype, dst_n, src_n, s) == SUSHI_HIP_OK, "refused");
    // the tile: what sushi_hip_match_curves chose at commit e6d26e5
    int64_t items1024 = 0;
    for (const SushiHipRequest& r : req) items1024 += (r.n_pos + 1023) / 1024;
    const int per_item = dtype == SUSHI_HIP_U8 ? 1024 : (items1024 >= 2048 ? 1024 : 256);
    REQUIRE(s.per_item == per_item, "%d positions per item, %" PRId64 " items of 1024", s.per_item, items1024);
    // the image: zeros but for the descriptors from byte 256 on, 40 bytes each
    REQUIRE(s.image.size() == 256 + up256((size_t)n * 40) && s.image.size() == curve_layout_bytes(n), "image of %zu bytes", s.image.size());
    std::vector<char> want(s.image.size(), 0);
    int64_t out_off = 0, items = 0;
    for (int k = 0; k < n; ++k) {
        char* d = want.data() + 256 + (size_t)k * 40;
        memcpy(d, &req[k].tmpl_off, 8); memcpy(d + 8, &req[k].win_start, 8); memcpy(d + 16, &out_off, 8); memcpy(d + 24, &items, 8);
        memcpy(d + 32, &req[k].tmpl_len, 4); memcpy(d + 36, &req[k].n_pos, 4);
        out_off += req[k].n_pos;
        items += (req[k].n_pos + per_item - 1) / per_item;
    }
    REQUIRE(want == s.image, "the image's contents");
    REQUIRE(s.n_items == items && s.grid == (unsigned)std::min<int64_t>(items, 2048) && s.grid >= 1, "%" PRId64 " items on a grid of %u", s.n_items, s.grid);
    // one sample short on either side
    CurveStage spare;
    REQUIRE(stage_curves(req.data(), n, dtype, dst_n - 1, src_n, spare) == SUSHI_HIP_EINVAL, "a window past the destination");
    REQUIRE(stage_curves(req.data(), n, dtype, dst_n, src_n - 1, spare) == SUSHI_HIP_EINVAL, "a pattern past the source");
}

void check_curves() {
    for (const CurveCase& c : curve_cases())
        for (const int dtype : DTYPES) {
            g_case = "curves " + c.name + (dtype == SUSHI_HIP_U8 ? " u8" : " f32");
            int64_t dst_n, src_n;
            lengths_for(c.req, &dst_n, &src_n);
            check_staged_curves(c.req, dtype, dst_n, src_n);
        }
    // the request rule is the batch's: over the batches of tests/batch_cases.hpp, on streams that hold every request, a curve call
    // is refused exactly where make_descs refuses, and each of the table's malformed requests is
    int refused = 0;
    for (const batch_cases::Case& c : batch_cases::cases()) {
        g_case = "curves of " + c.name;
        std::vector<SearchDesc> descs;
        int64_t tiles = 0, dst_n, src_n;
        const int rc = make_descs(c.req.data(), (int)c.req.size(), batch_cases::FFT_PATH_TILE, descs, &tiles);
        bool fits = true;
        for (const SushiHipRequest& r : c.req) fits = fits && request_fits(r, INT64_MAX, INT64_MAX);
        REQUIRE((rc == SUSHI_HIP_OK) == fits, "make_descs %d", rc);
        if (fits) lengths_for(c.req, &dst_n, &src_n); else dst_n = src_n = INT64_MAX;
        for (const int dtype : DTYPES) {
            CurveStage s;
            if (fits) check_staged_curves(c.req, dtype, dst_n, src_n);
            else REQUIRE(stage_curves(c.req.data(), (int)c.req.size(), dtype, dst_n, src_n, s) == SUSHI_HIP_EINVAL, "staged");
        }
        refused += !fits;
    }
    g_case = "curves";
    REQUIRE(refused == 3, "%d cases of the table break the request rule", refused);
    // the rule's own edges
    const int32_t big = 0x7fffffff - 65536;
    REQUIRE(request_fits(request(0, 0, big, big), INT64_MAX, INT64_MAX) && !request_fits(request(0, 0, big + 1, 1), INT64_MAX, INT64_MAX) &&
            !request_fits(request(0, 0, 1, big + 1), INT64_MAX, INT64_MAX), "the largest terms");
    REQUIRE(!request_fits(request(0, -1, 1, 1), 10, 10) && !request_fits(request(-1, 0, 1, 1), 10, 10) && !request_fits(request(0, 0, 0, 1), 10, 10) &&
            !request_fits(request(0, 0, 1, 0), 10, 10), "negative or empty");
    REQUIRE(request_fits(request(7, 4, 3, 4), 10, 10) && !request_fits(request(8, 4, 3, 4), 10, 10) && !request_fits(request(7, 5, 3, 4), 10, 10), "the streams' ends");
    REQUIRE(!request_fits(request(INT64_MAX, 0, 1, 1), INT64_MAX, INT64_MAX) && !request_fits(request(0, INT64_MAX, 1, 2), INT64_MAX, INT64_MAX) &&
            request_fits(request(INT64_MAX - 1, INT64_MAX - 1, 1, 1), INT64_MAX, INT64_MAX), "offsets at the end of 64 bits");
}

void dump_curves() {
    for (const CurveCase& c : curve_cases())
        for (const int dtype : DTYPES) {
            int64_t dst_n, src_n;
            lengths_for(c.req, &dst_n, &src_n);
            CurveStage s;
            const int rc = stage_curves(c.req.data(), (int)c.req.size(), dtype, dst_n, src_n, s);
            printf("{\"kind\":\"curves\",\"name\":\"%s\",\"dtype\":%d,\"rc\":%d,\"per_item\":%d,\"n_items\":%" PRId64 ",\"grid\":%u,\"image_bytes\":%zu,\"image_fnv\":\"%016" PRIx64 "\"}\n",
                   c.name.c_str(), dtype, rc, s.per_item, s.n_items, s.grid, s.image.size(), fnv1a(s.image.data(), s.image.size()));
        }
}

// ============================================================================================================================ retime
SushiHipRetimeSegment segment(int64_t in_start, int64_t out_off, int64_t out_len, int32_t num, int32_t den) {
    SushiHipRetimeSegment s;
    memset(&s, 0, sizeof(s));
    s.in_start = in_start; s.out_off = out_off; s.out_len = out_len; s.num = num; s.den = den;
    return s;
}
struct RetimeCase { std::string name; std::vector<SushiHipRetimeSegment> seg; int64_t n_in, n_out; };
std::vector<RetimeCase> retime_cases() {
    std::vector<RetimeCase> c;
    c.push_back({"one", {segment(10, 0, 5000, 25, 24)}, 6000, 5000});
    // outputs that begin 0, 3 and 21 samples behind the buffer's start; the last of several tiles
    c.push_back({"three", {segment(0, 0, 3, 1, 1), segment(100, 3, 18, 24, 25), segment(7, 21, 20000, 1001, 960)}, 30000, 20021});
    return c;
}
const uintptr_t RETIME_ADDR[] = {(uintptr_t)1 << 40, ((uintptr_t)1 << 40) + 4, ((uintptr_t)1 << 40) + 12};     // 16-byte aligned; 4 and 12 bytes behind

void check_staged_retime(const RetimeCase& c, int dtype, uintptr_t addr) {
    const int n = (int)c.seg.size();
    RetimeStage s;
    REQUIRE(stage_retime(c.seg.data(), n, dtype, c.n_in, c.n_out, addr, s) == SUSHI_HIP_OK, "refused");
    // sushi_hip_retime at commit e6d26e5: chunks of 16 bytes' worth of samples on the grid of 16-byte addresses, 256 to a tile
    const int size = dtype == SUSHI_HIP_U8 ? 1 : 4, per = dtype == SUSHI_HIP_U8 ? 16 : 8;
    REQUIRE(s.image.size() == (size_t)n && sizeof(RetimeSeg) == 48 && retime_layout_bytes(n) == up256((size_t)n * 48), "a table of %zu", s.image.size());
    std::vector<char> want((size_t)n * 48, 0);
    int64_t tiles = 0;
    for (int k = 0; k < n; ++k) {
        const SushiHipRetimeSegment& g = c.seg[k];
        const int32_t phase = (int32_t)(((addr + (uint64_t)g.out_off * size) % 16) / size);
        char* d = want.data() + (size_t)k * 48;
        memcpy(d, &g.in_start, 8); memcpy(d + 8, &g.out_off, 8); memcpy(d + 16, &g.out_len, 8); memcpy(d + 24, &tiles, 8);
        memcpy(d + 32, &g.num, 4); memcpy(d + 36, &g.den, 4); memcpy(d + 40, &phase, 4);
        REQUIRE(s.image[k].phase == phase && phase >= 0 && phase < per && ((addr + (uint64_t)(g.out_off - phase) * size) % 16) == 0, "segment %d: phase %d", k, s.image[k].phase);
        const int64_t chunks = (g.out_len + phase + per - 1) / per;
        tiles += (chunks + 255) / 256;
    }
    REQUIRE(memcmp(want.data(), s.image.data(), want.size()) == 0, "the table's contents");
    REQUIRE(s.n_tiles == tiles && s.grid == (unsigned)std::min<int64_t>(tiles, 2048) && s.grid >= 1, "%" PRId64 " tiles on a grid of %u", s.n_tiles, s.grid);
}

void check_retime() {
    bool zero_phase = false, other_phase = false, several_tiles = false;
    for (const RetimeCase& c : retime_cases())
        for (const int dtype : DTYPES)
            for (const uintptr_t addr : RETIME_ADDR) {
                g_case = "retime " + c.name + (dtype == SUSHI_HIP_U8 ? " u8 at +" : " f32 at +") + std::to_string(addr % 16);
                check_staged_retime(c, dtype, addr);
                RetimeStage s;
                stage_retime(c.seg.data(), (int)c.seg.size(), dtype, c.n_in, c.n_out, addr, s);
                for (const RetimeSeg& g : s.image) { zero_phase |= g.phase == 0; other_phase |= g.phase != 0; }
                several_tiles |= s.n_tiles > (int64_t)s.image.size();
            }
    g_case = "retime";
    REQUIRE(zero_phase && other_phase && several_tiles, "the cases reach phase 0, another phase and a segment of several tiles");
    // every refusal: a good segment with one thing wrong
    const int64_t n_in = (int64_t)1 << 42, n_out = (int64_t)1 << 42;
    const SushiHipRetimeSegment good = segment(100, 50, 1000, 25, 24);
    RetimeStage s;
    REQUIRE(stage_retime(&good, 1, SUSHI_HIP_F32, n_in, n_out, 0, s) == SUSHI_HIP_OK, "the good segment");
    auto refused = [&](const char* what, SushiHipRetimeSegment seg, int64_t in = (int64_t)1 << 42, int64_t out = (int64_t)1 << 42) {
        g_case = std::string("retime refusal: ") + what;
        REQUIRE(!segment_ok(seg, in, out) && stage_retime(&seg, 1, SUSHI_HIP_F32, in, out, 0, s) == SUSHI_HIP_EINVAL, "accepted");
        const SushiHipRetimeSegment both[2] = {good, seg};
        REQUIRE(stage_retime(both, 2, SUSHI_HIP_U8, in, out, 0, s) == SUSHI_HIP_EINVAL, "accepted behind a good one");
    };
    SushiHipRetimeSegment b;
    b = good; b.num = 0; refused("num < 1", b);
    b = good; b.num = (1 << 20) + 1; b.den = 1 << 20; refused("num > 2^20", b);
    b = good; b.den = 0; refused("den < 1", b);
    b = good; b.den = (1 << 20) + 1; b.num = 1 << 20; refused("den > 2^20", b);
    b = good; b.num = 17; b.den = 2; refused("num > 8 den", b);
    b = good; b.num = 2; b.den = 17; refused("den > 8 num", b);
    b = good; b.out_len = 0; refused("out_len < 1", b);
    b = good; b.out_len = (int64_t)1 << 40; b.num = 1; b.den = 8; refused("out_len >= 2^40", b);
    b = good; b.in_start = -1; refused("in_start < 0", b);
    b = good; b.in_start = 5000; refused("in_start > n_in - 1", b, 5000);
    b = good; refused("a last read past the input", b, 100 + 999 * 25 / 24);
    b = good; b.out_off = -1; refused("out_off < 0", b);
    b = good; b.out_off = 2001; refused("out_off > n_out", b, n_in, 2000);
    b = good; refused("outputs past the end", b, n_in, 1049);
    // ... and each of them just inside
    g_case = "retime: just inside";
    b = good; b.num = 1 << 20; b.den = 1 << 20; REQUIRE(segment_ok(b, n_in, n_out), "num = den = 2^20");
    b = good; b.num = 16; b.den = 2; REQUIRE(segment_ok(b, n_in, n_out), "num = 8 den");
    b = good; b.num = 2; b.den = 16; REQUIRE(segment_ok(b, n_in, n_out), "den = 8 num");
    b = good; b.out_len = ((int64_t)1 << 40) - 1; b.num = 1; b.den = 8; REQUIRE(segment_ok(b, n_in, n_out), "out_len = 2^40 - 1");
    REQUIRE(segment_ok(good, 100 + 999 * 25 / 24 + 1, n_out) && segment_ok(good, n_in, 1050), "the last read and the last output at the ends");
    // the call's own arguments
    REQUIRE(stage_retime(&good, 1, 2, n_in, n_out, 0, s) == SUSHI_HIP_EINVAL && stage_retime(&good, 0, SUSHI_HIP_U8, n_in, n_out, 0, s) == SUSHI_HIP_EINVAL &&
            stage_retime(&good, 1, SUSHI_HIP_U8, 0, n_out, 0, s) == SUSHI_HIP_EINVAL && stage_retime(&good, 1, SUSHI_HIP_U8, n_in, 0, 0, s) == SUSHI_HIP_EINVAL, "dtype and counts");
}

void dump_retime() {
    for (const RetimeCase& c : retime_cases())
        for (const int dtype : DTYPES)
            for (const uintptr_t addr : RETIME_ADDR) {
                RetimeStage s;
                const int rc = stage_retime(c.seg.data(), (int)c.seg.size(), dtype, c.n_in, c.n_out, addr, s);
                printf("{\"kind\":\"retime\",\"name\":\"%s\",\"dtype\":%d,\"addr_mod_16\":%d,\"rc\":%d,\"n_tiles\":%" PRId64 ",\"grid\":%u,\"image_bytes\":%zu,\"image_fnv\":\"%016" PRIx64 "\"}\n",
                       c.name.c_str(), dtype, (int)(addr % 16), rc, s.n_tiles, s.grid, s.image.size() * sizeof(RetimeSeg), fnv1a(s.image.data(), s.image.size() * sizeof(RetimeSeg)));
            }
}

// ============================================================================================================================= files
template <class T> std::vector<T> read_records(const char* path) {
    std::vector<T> v;
    FILE* f = fopen(path, "rb");
    T r;
    while (f && fread(&r, sizeof(r), 1, f) == 1) v.push_back(r);
    if (f) fclose(f);
    return v;
}
int write_file(const char* path, const void* p, size_t bytes) {
    FILE* f = fopen(path, "wb");
    const bool ok = f && fwrite(p, 1, bytes, f) == bytes;
    if (!(f && fclose(f) == 0 && ok)) { fprintf(stderr, "cannot write %s\n", path); return 2; }
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc == 7 && !strcmp(argv[1], "--stage-curves")) {
        const std::vector<SushiHipRequest> req = read_records<SushiHipRequest>(argv[2]);
        CurveStage s;
        const int rc = req.empty() ? SUSHI_HIP_EINVAL : stage_curves(req.data(), (int)req.size(), atoi(argv[3]), atoll(argv[4]), atoll(argv[5]), s);
        if (rc != SUSHI_HIP_OK) { fprintf(stderr, "%s: rc %d\n", argv[2], rc); return 1; }
        return write_file(argv[6], s.image.data(), s.image.size());
    }
    if (argc == 8 && !strcmp(argv[1], "--stage-retime")) {
        const std::vector<SushiHipRetimeSegment> seg = read_records<SushiHipRetimeSegment>(argv[2]);
        RetimeStage s;
        const int rc = stage_retime(seg.data(), (int)seg.size(), atoi(argv[3]), atoll(argv[4]), atoll(argv[5]), (uintptr_t)strtoull(argv[6], nullptr, 10), s);
        if (rc != SUSHI_HIP_OK) { fprintf(stderr, "%s: rc %d\n", argv[2], rc); return 1; }
        return write_file(argv[7], s.image.data(), s.image.size() * sizeof(RetimeSeg));
    }
    const bool checking = argc == 1, dumping = argc == 2 && !strcmp(argv[1], "--dump");
    if (!checking && !dumping) { fprintf(stderr, "usage: %s [--dump | --stage-curves REQ DTYPE DST_N SRC_N OUT | --stage-retime SEG DTYPE N_IN N_OUT OUT_ADDR OUT]\n", argv[0]); return 2; }
    for (const int64_t n : STREAM_N)
        for (const int dtype : DTYPES)
            for (const bool searchable : {false, true}) {
                if (checking) check_stream(n, dtype, searchable); else dump_stream(n, dtype, searchable);
            }
    if (checking) {
        g_case = "stream sizes";
        REQUIRE(stream_bytes(0, SUSHI_HIP_F32, 0) == 0 && stream_bytes(-1, SUSHI_HIP_U8, 1) == 0 && stream_bytes(10, 7, 0) == 0, "no bytes for no stream");
        check_curves();
        check_retime();
    } else {
        dump_curves();
        dump_retime();
    }
    return 0;
}
