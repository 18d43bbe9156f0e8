// tests/host_tspec_real_check.cpp -- the real-input forward transform of a pattern segment (sushi_amd/csrc/fft_core.hpp "Forward
// transform of a REAL, zero-padded pattern segment"; tspec_real_kernel) on the CPU, one emulated thread at a time, barriers as
// loop boundaries.  Built with g++ and run as a program by tests/test_tspec_real_host.py.
//
// usage: host_tspec_real_check          the index functions: who stores which bin where, and the switch's rule; exit 1 with a message on the first violation
//        host_tspec_real_check errors   the float32 route (pack / 8192-point transform / unfold, fft_core.hpp's own functions) against a
//                                       float64 DFT of the padded segment: one line "<case> <relative 2-norm error>" per segment
#include <cmath>
#include <complex>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "../include/sushi_hip.h"
#include "../sushi_amd/csrc/fft_core.hpp"
#include "../sushi_amd/csrc/run_policy.hpp"

using namespace sushi_fft;
typedef std::complex<double> cd;

#define REQUIRE(cond, ...) \
    do { \
        if (!(cond)) { fprintf(stderr, "tspec_real: [%s] ", #cond); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); return 1; } \
    } while (0)

constexpr int SEG = 4096;                       // FFT_SEG: samples of a segment
constexpr unsigned REAL_CONJ = 0x80000000u;     // a word's bit that real_conj_word flips: the sign of the imaginary half
constexpr unsigned TAG = 0x00010000u;           // makes a tag's "imaginary half" non-zero: a mirror of it shows

// What tspec_real_kernel stores, restated with any word type W (conj: the mirror of a word): every thread its row a (entries 0, 1
// as computed, 2, 3 mirrored), every thread but 0 its row b, the tail's lanes the words of row 512.  `put(word index, word)`.
template <class Put>
static void store_thread(int t, const unsigned* wa, const unsigned* wb, Put put) {
    unsigned ma[8], mb[8];
    real_mirror_words(wa, wb, t, ma, mb);
    const int ra = real_row(t, 0), rb = real_row(t, 1);
    for (int j = 0; j < 4; ++j) {
        put(4 * real_entry(ra, 0) + j, wa[j]); put(4 * real_entry(ra, 1) + j, wa[4 + j]);
        put(4 * real_entry(ra, 2) + j, ma[j]); put(4 * real_entry(ra, 3) + j, ma[4 + j]);
        if (t != 0) {
            put(4 * real_entry(rb, 0) + j, wb[j]); put(4 * real_entry(rb, 1) + j, wb[4 + j]);
            put(4 * real_entry(rb, 2) + j, mb[j]); put(4 * real_entry(rb, 3) + j, mb[4 + j]);
        }
    }
}
template <class Put>
static void store_tail(int l, unsigned wlo, unsigned whi, Put put) {
    put(real_tail_word(l), wlo); put(real_tail_word(7 - l), whi);
    put(real_tail_word(8 + l), real_conj_word(whi)); put(real_tail_word(15 - l), real_conj_word(wlo));
}

// Words are TAGS here: the bin a computed value is, with TAG (bit 31: conjugated).
static int check_indices() {
    std::vector<int> writes(RN, 0);
    std::vector<unsigned> stored(RN, 0xffffffffu);
    bool outside = false;
    auto put = [&](int word, unsigned tag) { if (word >= 0 && word < RN) { ++writes[word]; stored[word] = tag; } else outside = true; };
    std::vector<int> z_reads(RN / 2, 0);
    for (int t = 0; t < RNT; ++t) {
        const int a = real_row(t, 0), b = real_row(t, 1);
        REQUIRE(a >= 0 && a < 512 && b == 1024 - a, "thread %d rows %d %d", t, a, b);
        REQUIRE((t == 0) == (a == 0), "thread 0 and no other owns row 0 (thread %d)", t);
        unsigned wa[8], wb[8];
        for (int d = 0; d < 8; ++d) {
            // the butterfly of za[d] = Z[a + 1024 d] and zb[7 - d] = Z[(b + 1024 (7 - d)) mod RN/2]: partners RN/2 - k of each other
            const int k = a + 1024 * d, p = (b + 1024 * (7 - d)) % (RN / 2);
            REQUIRE((k + p) % (RN / 2) == 0, "thread %d butterfly %d pairs Z[%d] with Z[%d]", t, d, k, p);
            ++z_reads[k]; ++z_reads[p];
            wa[d] = (unsigned)(a + 1024 * d) | TAG;             // lo = X[k]
            wb[d] = (unsigned)(b + 1024 * d) | TAG;             // hi of butterfly 7 - d = X[RN/2 - (a + 1024 (7 - d))] = X[b + 1024 d]
            REQUIRE(RN / 2 - (a + 1024 * (7 - d)) == b + 1024 * d, "thread %d bin %d of row b", t, d);
        }
        store_thread(t, wa, wb, put);
        // the hand-over's places stay inside the buffer and a thread's are its own
        REQUIRE(real_zpos(t + RNT * 15) < lds_floats<RLOGN>() && real_zpos(t + RNT * 3) == real_zpos(t) + (RNT + 2 * (RNT >> 6)) * 3, "store places of thread %d", t);
        REQUIRE(real_zpos(a + 1024 * 7) == real_zpos(a) + REAL_ZSTEP * 7 && real_zpos(1023 + 1024 * 7) < lds_floats<RLOGN>(), "load places of thread %d", t);
        // the samples of the packed input: registers 0, 1, 8, 9 inside the segment, every other one behind it
        for (int r = 0; r < PER; ++r) {
            REQUIRE(real_in_sample(t, r) == 2 * in_index<RLOGN>(t, r), "input register %d of thread %d", r, t);
            REQUIRE((real_in_sample(t, r) + 1 < SEG) == ((r % R1) < 2) && (real_in_sample(t, r) < SEG) == ((r % R1) < 2), "input register %d of thread %d", r, t);
        }
    }
    for (int l = 0; l < REAL_TAIL_LANES; ++l) {
        const int k = real_tail_z(l, 0), p = real_tail_z(l, 1);
        REQUIRE(k + p == RN / 2 && k == REAL_TAIL_ROW + 1024 * l, "the tail's lane %d pairs Z[%d] with Z[%d]", l, k, p);
        ++z_reads[k]; ++z_reads[p];
        store_tail(l, (unsigned)k | TAG, (unsigned)p | TAG, put);
    }
    REQUIRE(!outside, "a store outside the row");
    // every Z is read: once by its row's owner (thread 0's rows: bins 1024 d, d = 1 .. 7 twice, Z[0] twice -- with itself)
    for (int e = 0; e < RN / 2; ++e)
        REQUIRE(z_reads[e] == ((e % 1024) == 0 ? 2 : 1), "Z[%d] is read %d times", e, z_reads[e]);
    // every stored word is written exactly once, holds its bin -- the order is mslot_of_bin's, the one the inverse transform loads --
    // and is a mirror exactly where it is the conjugate of a word that is not
    for (int f = 0; f < RN; ++f) {
        const int word = mslot_of_bin(f);
        REQUIRE(writes[word] == 1, "bin %d (word %d) is written %d times", f, word, writes[word]);
        const unsigned tag = stored[word];
        const int src = (int)(tag & 0xffffu), conj = (tag & REAL_CONJ) != 0;
        REQUIRE(src == (conj ? (RN - f) % RN : f), "bin %d holds the value of bin %d%s", f, src, conj ? " conjugated" : "");
        REQUIRE(conj == (f > RN / 2), "bin %d: computed bins are 0 .. N/2, mirrors the others", f);
        const unsigned partner = stored[mslot_of_bin((RN - f) % RN)];
        if (f != 0 && f != RN / 2) REQUIRE(partner == (tag ^ REAL_CONJ), "bin %d and its mirror hold %08x %08x", f, tag, partner);
    }
    for (int f = 0; f < RN; ++f)
        REQUIRE(4 * real_entry(f % 1024, f >> 12) + ((f >> 10) & 3) == mslot_of_bin(f), "real_entry(%d, %d)", f % 1024, f >> 12);
    // what the inverse transform's thread tid loads as sub-position j of its entry g (mbin) is that bin
    for (int tid = 0; tid < WNT; ++tid)
        for (int g = 0; g < 4; ++g)
            for (int j = 0; j < 4; ++j) {
                const int f = mbin(tid, g, j);
                REQUIRE((int)(stored[mslot_of_bin(f)] & 0xffffu) == (f > RN / 2 ? RN - f : f), "entry %d of loading thread %d", g, tid);
            }
    // sixteen consecutive lanes store sixteen consecutive entries: whole 128-byte lines
    for (int t = 0; t < RNT; t += 16)
        for (int l = 0; l < 16; ++l)
            for (int u = 0; u < 4; ++u) {
                REQUIRE(real_entry(real_row(t + l, 0), u) == real_entry(real_row(t, 0), u) + l && (real_entry(real_row(t, 0), u) & 15) == 0, "row a of lanes %d ..", t);
                // (rows b of the first 32 threads, the partners of a & 15 == 0, run with a borrow: not in one piece)
                if (t >= 32) REQUIRE(real_entry(real_row(t + l, 1), u) == real_entry(real_row(t, 1), u) - l, "row b of lanes %d ..", t);
            }
    // the rows whose mirrors are special: 0 (thread 0: bins 0 and 8 real and their own mirrors, bin 16 - d of d) and 512 (the tail)
    REQUIRE(stored[mslot_of_bin(0)] == TAG && stored[mslot_of_bin(RN / 2)] == ((unsigned)(RN / 2) | TAG), "bins 0 and N/2");
    for (int r = 1; r < 16; ++r) {
        const unsigned tag = stored[mslot_of_bin(1024 * r)];
        REQUIRE(tag == (TAG | (r <= 8 ? (unsigned)(1024 * r) : ((unsigned)(1024 * (16 - r)) | REAL_CONJ))), "bin 1024 * %d", r);
    }
    // the low entries: row r's bins 0, 1, 14, 15 are the entry lslot_of_thread(r) of a low row
    for (int r = 0; r < 1024; ++r)
        for (int j = 0; j < 4; ++j) {
            const int f = r + 1024 * (j < 2 ? j : 12 + j);
            REQUIRE(lslot_of_bin(f) == 4 * lslot_of_thread(r) + j, "low entry of row %d, word %d", r, j);
        }
    // a mirror's word: the imaginary half's sign flipped, a zero one (either sign) kept
    for (unsigned w : {0x3c003c00u, 0xbc00bc00u, 0x00010000u, 0x80010000u, 0x7bff0001u})
        REQUIRE(real_conj_word(w) == (w ^ REAL_CONJ) && real_conj_word(real_conj_word(w)) == w, "the mirror of %08x", w);
    for (unsigned w : {0u, 0x80000000u, 0x00003c00u, 0x8000bc00u})
        REQUIRE(real_conj_word(w) == w, "the mirror of %08x, whose imaginary half is zero", w);
    // the switch (run_policy.hpp tspec_route: SUSHI_HIP_TSPEC)
    using namespace sushi;
    REQUIRE(tspec_route(nullptr) == TSPEC_REAL && tspec_route("") == TSPEC_REAL && tspec_route("real") == TSPEC_REAL, "the default route");
    REQUIRE(tspec_route("complex") == TSPEC_COMPLEX, "the earlier route");
    for (const char* bad : {"Real", "complex ", "cplx", "0", "1", "real,complex"}) REQUIRE(tspec_route(bad) < 0, "'%s' is no route", bad);
    REQUIRE(tspec_real(TSPEC_REAL) && !tspec_real(TSPEC_COMPLEX) && TSPEC_REAL == 0, "a zeroed handle takes the default");
    return 0;
}

static void ref_fft(std::vector<cd>& a, int dir) {   // iterative radix-2, float64
    const int n = (int)a.size();
    for (int i = 1, j = 0; i < n; ++i) {
        int bit = n >> 1;
        for (; j & bit; bit >>= 1) j ^= bit;
        j ^= bit;
        if (i < j) std::swap(a[i], a[j]);
    }
    for (int len = 2; len <= n; len <<= 1) {
        const double ang = dir * 2.0 * M_PI / len;
        for (int i = 0; i < n; i += len)
            for (int k = 0; k < len / 2; ++k) {
                const cd w(std::cos(ang * k), std::sin(ang * k));
                const cd u = a[i + k], v = a[i + k + len / 2] * w;
                a[i + k] = u + v;
                a[i + k + len / 2] = u - v;
            }
    }
}

// the route in float32 on a segment of `len` samples -> relative 2-norm error of its RN bins (as stored: mslot_of_bin) against float64
static double route_error(const std::vector<float>& seg, const std::vector<cpx>& tw) {
    typedef Plan<RLOGN> P;
    const int len = (int)seg.size();
    std::vector<cd> ref(RN, cd(0, 0));
    for (int n = 0; n < len; ++n) ref[n] = cd(seg[n], 0);
    ref_fft(ref, -1);
    std::vector<cpx> regs((size_t)RNT * PER);
    for (int t = 0; t < RNT; ++t)
        for (int r = 0; r < PER; ++r) {
            const int e = real_in_sample(t, r);
            regs[(size_t)t * PER + r] = cpx{e < len ? seg[e] : 0.f, e + 1 < len ? seg[e + 1] : 0.f};
        }
    std::vector<float> fl(lds_floats<RLOGN>(), 1e30f);
#define ALL(stmt) for (int tid = 0; tid < RNT; ++tid) { cpx* v = &regs[(size_t)tid * PER]; \
        const Twiddles t = load_twiddles<RLOGN, -1>(tid, tw.data()); (void)t; stmt; }
#define XCHG(EX) \
        ALL((split_store<RLOGN, EX, 0>(v, tid, fl.data()))) \
        ALL((split_load<RLOGN, EX, 0>(v, tid, fl.data()))) \
        ALL((split_store<RLOGN, EX, 1>(v, tid, fl.data()))) \
        ALL((split_load<RLOGN, EX, 1>(v, tid, fl.data())))
    ALL((pass_compute<R1, 1, -1>(v, cpx{1.f, 0.f})))
    XCHG(1)
    ALL((pass_compute<R2, R1, -1>(v, t.p2)))
    XCHG(2)
    ALL((pass_compute<P::R3, R1 * R2, -1>(v, t.p3)))
    XCHG(3)
    ALL((pass_compute<R4, P::NT, -1>(v, t.p4)))
#undef XCHG
    // the hand-over, as the kernel's barriers order it
    std::vector<cpx> za((size_t)RNT * 8), zb((size_t)RNT * 8), tz(REAL_TAIL_LANES), tp(REAL_TAIL_LANES);
    std::fill(fl.begin(), fl.end(), 1e30f);
    ALL((real_z_store<0>(v, tid, fl.data())))
    ALL((real_z_load<0>(&za[(size_t)tid * 8], &zb[(size_t)tid * 8], tid, fl.data())))
    for (int l = 0; l < REAL_TAIL_LANES; ++l) real_tail_load<0>(tz[l], tp[l], l, fl.data());
    ALL((real_z_store<1>(v, tid, fl.data())))
    ALL((real_z_load<1>(&za[(size_t)tid * 8], &zb[(size_t)tid * 8], tid, fl.data())))
    for (int l = 0; l < REAL_TAIL_LANES; ++l) real_tail_load<1>(tz[l], tp[l], l, fl.data());
#undef ALL
    // unfold; the "words" are indices into the values a thread computed, placed where the kernel stores them
    std::vector<cpx> out(RN, cpx{1e30f, 1e30f});
    for (int t = 0; t < RNT; ++t) {
        cpx x[16];
        real_unfold(&za[(size_t)t * 8], &zb[(size_t)t * 8], t, tw[real_row(t, 0)], x, x + 8);
        unsigned wa[8], wb[8];
        for (int d = 0; d < 8; ++d) { wa[d] = (unsigned)d | TAG; wb[d] = (unsigned)(8 + d) | TAG; }
        store_thread(t, wa, wb, [&](int word, unsigned tag) {
            const cpx c = x[tag & 15u];
            out[word] = (tag & REAL_CONJ) ? cconj(c) : c;
        });
    }
    for (int l = 0; l < REAL_TAIL_LANES; ++l) {
        cpx x[2];
        real_tail_bfly(tz[l], tp[l], tw[real_tail_z(l, 0)], x[0], x[1]);
        store_tail(l, 0u | TAG, 1u | TAG, [&](int word, unsigned tag) {
            const cpx c = x[tag & 1u];
            out[word] = (tag & REAL_CONJ) ? cconj(c) : c;
        });
    }
    double err2 = 0, ref2 = 0;
    for (int f = 0; f < RN; ++f) {
        const cpx g = out[mslot_of_bin(f)];
        err2 += std::norm(cd(0.5 * g.x, 0.5 * g.y) - ref[f]);       // (the unfold leaves twice the bins)
        ref2 += std::norm(ref[f]);
    }
    return std::sqrt(err2 / ref2);
}

static int print_errors() {
    std::vector<cpx> tw(TWIDDLE_N);
    for (int n = 0; n < TWIDDLE_N; ++n) {
        tw[n].x = (float)std::cos(2.0 * M_PI * n / TWIDDLE_N);
        tw[n].y = (float)-std::sin(2.0 * M_PI * n / TWIDDLE_N);
    }
    srand(20240607);
    auto noise = [](int len) {
        std::vector<float> s(len);
        for (int n = 0; n < len; ++n) s[n] = (float)rand() / (float)RAND_MAX - 0.5f;
        return s;
    };
    std::vector<std::pair<std::string, std::vector<float>>> cases;
    for (int len : {1, 2, 3, 4095, 4096}) cases.push_back({"length_" + std::to_string(len), noise(len)});
    std::vector<float> s(SEG, 0.f);
    s[SEG - 1] = 1.f;
    cases.push_back({"impulse_last", s});
    cases.push_back({"constant", std::vector<float>(SEG, 0.75f)});
    for (int n = 0; n < SEG; ++n) s[n] = (n & 1) ? -1.f : 1.f;
    cases.push_back({"alternating", s});
    cases.push_back({"random", noise(SEG)});
    for (int n = 0; n < SEG; ++n) s[n] = 200.f + 55.f * ((float)rand() / (float)RAND_MAX);     // (uint8-like: a level well above the spread)
    cases.push_back({"random_offset", s});
    for (const auto& c : cases) printf("%s %.6e\n", c.first.c_str(), route_error(c.second, tw));
    return 0;
}

int main(int argc, char** argv) {
    if (argc > 1 && !strcmp(argv[1], "errors")) return print_errors();
    return check_indices();
}
