// sushi_amd/csrc/track_wide_core.hpp -- the arithmetic of the wide tracking pass (include/sushi_hip.h "wide tracking"; DESIGN.md
// 3.23): near_e[j] for a reach above TRACK_MAX_REACH and a step_cost of +-0.0, in a time that does not grow with the reach.  Plain
// C++: sushi_track.hip and sushi_track_order.hip run it on the device, tests/host_track_wide_check.cpp on the CPU (g++).  Both are
// compiled with -ffp-contract=off, as every track unit is.  The tile's size, the workspace's layout and a wide call's staging are
// track_core.hpp's (stage_track(..., wide) and the stages built on it); stage_track_wide and stage_margins_wide, at the end, are
// one-line forwards to them.
//
// With a free move the order of track_replaces -- (value, |d|, d > 0) -- decomposes: the minimum of X[j - r .. j - 1] with ties to
// the LARGEST index, the minimum of X[j + 1 .. j + r] with ties to the SMALLEST index, and X[j] itself, combined by track_replaces.
// Adding +-0.0 changes no order, so the selection runs on X and the price is added once, to the winner.  The axis is cut into window
// tiles of WIDE_TILE values.  Per element a tile pass leaves the minimum of its tile's values up to it (the prefix) and from it on
// (the suffix), each as a value and the first and the last index that attain it; a window that spans a tile boundary is then one
// suffix record, the whole tiles between (their record: the prefix at the tile's last element) and one prefix record.  A reach >=
// WIDE_TILE always spans a boundary unless the axis's end cuts the window, and then one record is the whole window.
#ifndef SUSHI_TRACK_WIDE_CORE_HPP
#define SUSHI_TRACK_WIDE_CORE_HPP

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/sushi_hip.h"
#include "track_core.hpp"
#include "track_margin_core.hpp"

namespace sushi {

constexpr int WIDE_PER = WIDE_TILE / TRACK_THREADS;         // consecutive values a thread of the tile pass holds

// ---- the records ----
// The minimum of a run of consecutive values: its value (of equal values any one's: 0.0 and -0.0 are equal, so the sign of a zero
// is not the winner's -- wide_near reads the winner itself where that matters) and the first and the last index inside the tile
// that attain it.  first < 0: the run is empty.
struct WideRec { double v; int32_t first, last; };
SUSHI_GEOM_HD inline WideRec wide_empty() { return WideRec{INFINITY, -1, -1}; }
SUSHI_GEOM_HD inline WideRec wide_one(double v, int32_t at) { return WideRec{v, at, at}; }
// run a followed by run b (b's indices are the higher ones).  Associative; no order of combining changes the result.
SUSHI_GEOM_HD inline WideRec wide_combine(const WideRec& a, const WideRec& b) {
    const bool a_none = a.first < 0, b_none = b.first < 0;
    const bool take_b = (int)a_none | ((int)!b_none & (int)(b.v < a.v));          // b alone
    const bool take_a = (int)b_none | ((int)!a_none & (int)(a.v < b.v));          // a alone (both empty: a, which is empty)
    WideRec r;
    r.v = take_b ? b.v : a.v;
    r.first = take_b ? b.first : a.first;
    r.last = take_a ? a.last : b.last;
    return r;
}
// a record's two indices as they are stored: one 32-bit word
SUSHI_GEOM_HD inline uint32_t wide_pack(const WideRec& r) { return (uint32_t)r.first | ((uint32_t)r.last << 16); }
SUSHI_GEOM_HD inline int32_t wide_first(uint32_t w) { return (int32_t)(w & 0xffffu); }
SUSHI_GEOM_HD inline int32_t wide_last(uint32_t w) { return (int32_t)(w >> 16); }

// what the tile pass leaves of one row X, per element i: pv / pi the record of X[tile's first index .. i], sv / si that of X[i ..
// tile's last index] (the axis's last index in its last tile)
struct WideRecords {
    double* pv; double* sv;
    uint32_t* pi; uint32_t* si;
};

// One window tile on the CPU, one element after the other (the device scans it in a workgroup: sushi_track_wide_tile.inc).
inline void wide_tile_scan(const double* X, int32_t n_shift, int64_t tile, const WideRecords& w) {
    const int64_t lo = tile << WIDE_TILE_BITS, hi = lo + WIDE_TILE < n_shift ? lo + WIDE_TILE : n_shift;
    WideRec run = wide_empty();
    for (int64_t i = lo; i < hi; ++i) {
        run = wide_combine(run, wide_one(X[i], (int32_t)(i - lo)));
        w.pv[i] = run.v; w.pi[i] = wide_pack(run);
    }
    run = wide_empty();
    for (int64_t i = hi - 1; i >= lo; --i) {
        run = wide_combine(wide_one(X[i], (int32_t)(i - lo)), run);
        w.sv[i] = run.v; w.si[i] = wide_pack(run);
    }
}

// ---- near_e[j] ----
// The whole tiles t_lo .. t_hi a work item of `span` indices from `base` on may ask for, at reach r: at most WIDE_ITEM_TILES.
constexpr int WIDE_ITEM_TILES = (AXIS_PER_LARGE * AXIS_THREADS - 1 + 2 * TRACK_WIDE_MAX_REACH) / WIDE_TILE + 2;
SUSHI_GEOM_HD inline int64_t wide_item_first_tile(int64_t base, int32_t r) { return (base < r ? 0 : base - r) >> WIDE_TILE_BITS; }
SUSHI_GEOM_HD inline int64_t wide_item_last_tile(int64_t base, int64_t span, int32_t r, int32_t n_shift) {
    const int64_t to = base + span - 1 + r;
    return (to < n_shift ? to : (int64_t)n_shift - 1) >> WIDE_TILE_BITS;
}
// the element whose prefix record is tile t's whole record
SUSHI_GEOM_HD inline int64_t wide_tile_end(int64_t t, int32_t n_shift) {
    const int64_t end = ((t + 1) << WIDE_TILE_BITS) - 1;
    return end < n_shift ? end : (int64_t)n_shift - 1;
}

struct WideTileRec { double v; uint32_t idx; };

// near_e[j] of row X for WIDE_TILE <= r <= TRACK_WIDE_MAX_REACH and mu = +-0.0; *d: the winning move.  tiles(t): tile t's whole
// record (read from the records on the CPU, staged in LDS once per work item on the device); 0 <= j < n_shift.  Every index read
// lies inside the axis.
template <typename Tiles>
SUSHI_GEOM_HD inline double wide_near(const double* X, const double* pv, const double* sv, const uint32_t* pi, const uint32_t* si,
                                      const Tiles& tiles, int64_t j, int32_t n_shift, int32_t r, double mu, int32_t* d) {
    double best = X[j];
    int32_t bd = 0;
    if (j >= 1) {                           // the left side: X[a .. b], ties to the largest index
        const int64_t a = j < r ? 0 : j - r, b = j - 1;
        const int64_t ta = a >> WIDE_TILE_BITS, tb = b >> WIDE_TILE_BITS;
        double v = pv[b];
        int64_t at = (tb << WIDE_TILE_BITS) + wide_last(pi[b]);
        // (ta == tb: the axis's start cut the window, a is its tile's first index and the prefix record is the whole window)
        for (int64_t t = tb - 1; t > ta; --t) {
            const WideTileRec rec = tiles(t);
            const bool take = rec.v < v;    // walking down, an equal value lies at a smaller index: it does not replace
            v = take ? rec.v : v; at = take ? (t << WIDE_TILE_BITS) + wide_last(rec.idx) : at;
        }
        if (ta != tb) {
            const double s = sv[a];
            const bool take = s < v;
            v = take ? s : v; at = take ? (ta << WIDE_TILE_BITS) + wide_last(si[a]) : at;
        }
        const int32_t dl = (int32_t)(at - j);
        if (track_replaces(v, dl, best, bd)) { best = v; bd = dl; }
    }
    if (j + 1 < n_shift) {                  // the right side: X[a .. b], ties to the smallest index
        const int64_t a = j + 1, b = j + r < n_shift ? j + r : (int64_t)n_shift - 1;
        const int64_t ta = a >> WIDE_TILE_BITS, tb = b >> WIDE_TILE_BITS;
        double v = sv[a];
        int64_t at = (ta << WIDE_TILE_BITS) + wide_first(si[a]);
        // (ta == tb: the axis's end cut the window, b is its tile's last index and the suffix record is the whole window)
        for (int64_t t = ta + 1; t < tb; ++t) {
            const WideTileRec rec = tiles(t);
            const bool take = rec.v < v;    // walking up, an equal value lies at a larger index: it does not replace
            v = take ? rec.v : v; at = take ? (t << WIDE_TILE_BITS) + wide_first(rec.idx) : at;
        }
        if (ta != tb) {
            const double p = pv[b];
            const bool take = p < v;
            v = take ? p : v; at = take ? (tb << WIDE_TILE_BITS) + wide_first(pi[b]) : at;
        }
        const int32_t dr = (int32_t)(at - j);
        if (track_replaces(v, dr, best, bd)) { best = v; bd = dr; }
    }
    *d = bd;
    if (bd == 0) return best;               // cand(0): the value itself, nothing added
    // a record's zero may carry another element's sign: the winner's own bits (any other value is its bits already)
    if (best == 0.0) best = X[path_clamp((int32_t)(j + bd), n_shift)];
    return track_cand(best, track_price(mu, bd < 0 ? -bd : bd));
}

// a wide call's record arrays in its workspace (the layout: track_core.hpp)
inline WideRecords wide_records(char* mem, const WideLayout& l) {
    return WideRecords{(double*)(mem + l.pv), (double*)(mem + l.sv), (uint32_t*)(mem + l.pi), (uint32_t*)(mem + l.si)};
}

// ---- a wide call's stage by a name of its own ----
// The stage functions with `wide` set, in the shape the CPU checks of the wide calls read (tests/host_track_wide_check.cpp,
// tests/host_track_order_wide_check.cpp): the walk's own stage as `plain`, the wide facts beside it.  One-line forwards: the
// checking body is the walk's.
template <typename Stage>
struct WideStageOf : TrackCall {
    Stage plain;
};
using TrackWideStage = WideStageOf<TrackStage>;
using MarginWideStage = WideStageOf<MarginStage>;

inline int stage_track_wide(const SushiHipJointRow* rows, const int32_t* reach, int n_rows, int32_t n_shift, int64_t n_curve, int method,
                            double penalty, double step_cost, int row0, int n_total, const void* mem, size_t mem_bytes,
                            TrackWideStage& out) {
    const int rc = stage_track(rows, reach, n_rows, n_shift, n_curve, method, penalty, step_cost, row0, n_total, mem, mem_bytes, out.plain, true);
    static_cast<TrackCall&>(out) = out.plain;
    return rc;
}
inline int stage_margins_wide(const SushiHipJointRow* rows, const int32_t* reach, const int32_t* guard, int n_rows, int32_t n_shift,
                              int64_t n_curve, int method, double penalty, double step_cost, int row0, int n_total, const void* mem,
                              size_t mem_bytes, MarginWideStage& out) {
    const int rc = stage_margins(rows, reach, guard, n_rows, n_shift, n_curve, method, penalty, step_cost, row0, n_total, mem, mem_bytes,
                                 out.plain, true);
    static_cast<TrackCall&>(out) = out.plain;
    return rc;
}

}  // namespace sushi
#endif
