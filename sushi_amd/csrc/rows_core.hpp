// sushi_amd/csrc/rows_core.hpp -- score rows clamped at a threshold (include/sushi_hip.h "rows"): the rule by which
// a value passes or is replaced, how a row is cut into tiles, the search for a tile's hits in a threshold run's sorted list, and the
// checks of such a list.  Plain C++: sushi_rows.hip runs it on the device, tests/host_rows_check.cpp on the CPU (g++).
// Behind it, host only: the record the kernels read, the workspace's layout, and stage_rows -- a table -> a refusal, or the image
// that is uploaded and the facts of the launch.
#ifndef SUSHI_ROWS_CORE_HPP
#define SUSHI_ROWS_CORE_HPP

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "../../include/sushi_hip.h"
#include "sushi_geometry.hpp"      // SUSHI_GEOM_HD, method_known, align_up

namespace sushi {

// A row is cut into tiles of ROWS_TILE consecutive floats (the last one shorter), one work item each; a workgroup of ROWS_THREADS
// threads takes an item, and a grid of at most ROWS_MAX_GRID workgroups (256 CUs, eight each) strides over the items of all rows.
constexpr int ROWS_THREADS = 256;
constexpr int32_t ROWS_TILE = 4096;
constexpr int64_t ROWS_MAX_GRID = 2048;

// ---- the rule ----
// Whether the score v passes f: v <= f (SQDIFF_NORMED) or v >= f (CCOEFF_NORMED).  Two floats compare as their doubles do, so this
// is the threshold run's comparison with (double)f; -0.0 passes 0.0 both ways, a NaN passes nothing.
SUSHI_GEOM_HD inline bool rows_passes(int method, float v, float f) {
    return method == SUSHI_HIP_METHOD_CCOEFF_NORMED ? v >= f : v <= f;
}
// The clamped value: v itself (its bits) where it passes, else f.
SUSHI_GEOM_HD inline float rows_clamped(int method, float v, float f) { return rows_passes(method, v, f) ? v : f; }

// ---- tiles ----
SUSHI_GEOM_HD inline int32_t rows_tiles(int32_t n_pos) { return (int32_t)(((int64_t)n_pos + ROWS_TILE - 1) / ROWS_TILE); }
// tile t of a row of n_pos floats is [t0, t0 + len)
SUSHI_GEOM_HD inline int32_t rows_tile_first(int32_t tile) { return tile * ROWS_TILE; }
SUSHI_GEOM_HD inline int32_t rows_tile_len(int32_t tile, int32_t n_pos) {
    const int32_t left = n_pos - rows_tile_first(tile);
    return left < ROWS_TILE ? left : ROWS_TILE;
}

// ---- a request's hit list ----
// How many records of a request's list are read: all `count` of them, or none -- with a flag -- where the list overflowed its
// `capacity` (the row is then all f) or the count is negative.
SUSHI_GEOM_HD inline int64_t rows_kept(int64_t count, int32_t capacity, int* flag) {
    *flag = 0;
    if (count < 0) { *flag = SUSHI_HIP_ROWS_BAD_HITS; return 0; }
    if (count > (int64_t)capacity) { *flag = SUSHI_HIP_ROWS_OVERFLOW; return 0; }
    return count;
}

// The first j in [0, count] whose hits[j].index >= x (count where there is none): bisection of a list in ascending index order.
// On any other list it still ends, inside [0, count].
SUSHI_GEOM_HD inline int64_t rows_lower_bound(const SushiHipHit* hits, int64_t count, int64_t x) {
    int64_t lo = 0, hi = count;
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if ((int64_t)hits[mid].index < x) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// The records [lo, hi) of a sorted list whose indices lie in the tile [t0, t1).
struct RowsRange { int64_t lo, hi; };
SUSHI_GEOM_HD inline RowsRange rows_tile_range(const SushiHipHit* hits, int64_t count, int32_t t0, int32_t t1) {
    RowsRange r;
    r.lo = rows_lower_bound(hits, count, t0);
    r.hi = rows_lower_bound(hits, count, t1);
    if (r.hi < r.lo) r.hi = r.lo;               // (a list that is not sorted)
    return r;
}

// Whether record j of a list is what a threshold run leaves: its index inside the row, and above the index of the record before it.
SUSHI_GEOM_HD inline bool rows_hit_ok(const SushiHipHit* hits, int64_t j, int32_t n_pos) {
    const int32_t at = hits[j].index;
    return at >= 0 && at < n_pos && (j == 0 || hits[j - 1].index < at);
}

// Which records tile `tile` of a row of n_tiles checks: the list is shared out evenly among the row's tiles, [*j0, *j1).
SUSHI_GEOM_HD inline void rows_check_slice(int64_t count, int32_t n_tiles, int32_t tile, int64_t* j0, int64_t* j1) {
    const int64_t per = (count + n_tiles - 1) / n_tiles;
    const int64_t a = per * tile, b = a + per;
    *j0 = a < count ? a : count;
    *j1 = b < count ? b : count;
}

// One tile of sushi_hip_rows_from_hits, as the definition: the tile filled with f, then the records of its range written where
// their index lies in the tile; returns the flags its slice of the checks gives.  out: the row's first float.
inline int rows_form_tile(const SushiHipHit* hits, int64_t count, int32_t capacity, int32_t n_pos, int32_t tile, float f, float* out) {
    const int32_t t0 = rows_tile_first(tile), t1 = t0 + rows_tile_len(tile, n_pos);
    for (int32_t p = t0; p < t1; ++p) out[p] = f;
    int flag;
    const int64_t kept = rows_kept(count, capacity, &flag);
    int64_t j0, j1;
    rows_check_slice(kept, rows_tiles(n_pos), tile, &j0, &j1);
    for (int64_t j = j0; j < j1; ++j)
        if (!rows_hit_ok(hits, j, n_pos)) flag |= SUSHI_HIP_ROWS_BAD_HITS;
    const RowsRange r = rows_tile_range(hits, kept, t0, t1);
    for (int64_t j = r.lo; j < r.hi; ++j)
        if (hits[j].index >= t0 && hits[j].index < t1) out[hits[j].index] = hits[j].score;
    return flag;
}

// ---- the host side of a call ----
// a row on the device
struct RowsRowDev {
    int64_t out_off, in_off;
    int64_t first_item;     // work items of the rows before this one
    int32_t n_pos, n_tiles;
};
static_assert(sizeof(RowsRowDev) == 32, "RowsRowDev layout");

// workspace: [RowsRowDev x n], padded to 256 bytes, uploaded in one copy
inline size_t rows_layout_bytes(int n) { return n < 1 ? 0 : align_up((size_t)n * sizeof(RowsRowDev), 256); }

struct RowsStage {
    std::vector<char> image;    // the workspace as uploaded
    int64_t n_items;
    unsigned grid;
};

// a row of n_pos floats from `off` on stays inside a buffer of n_buf floats (without forming the sum)
inline bool rows_inside(int64_t off, int32_t n_pos, int64_t n_buf) { return off >= 0 && off <= n_buf - (int64_t)n_pos; }

// EINVAL: n < 1, n_out < 1, an f that is not finite, n_pos < 1, a row that leaves out_dev -- or, with_in (sushi_hip_rows_clamp),
// n_in < 1 or a row that leaves in_dev.  `out` is then unspecified.
inline int stage_rows(const SushiHipRowsRow* rows, int n, int64_t n_out, bool with_in, int64_t n_in, float f, RowsStage& out) {
    if (n < 1 || n_out < 1 || (with_in && n_in < 1) || !isfinite(f)) return SUSHI_HIP_EINVAL;
    for (int k = 0; k < n; ++k) {
        if (rows[k].n_pos < 1 || !rows_inside(rows[k].out_off, rows[k].n_pos, n_out)) return SUSHI_HIP_EINVAL;
        if (with_in && !rows_inside(rows[k].in_off, rows[k].n_pos, n_in)) return SUSHI_HIP_EINVAL;
    }
    out.image.assign(rows_layout_bytes(n), 0);
    RowsRowDev* rd = reinterpret_cast<RowsRowDev*>(out.image.data());
    int64_t items = 0;
    for (int k = 0; k < n; ++k) {
        rd[k].out_off = rows[k].out_off; rd[k].in_off = with_in ? rows[k].in_off : 0;
        rd[k].first_item = items;
        rd[k].n_pos = rows[k].n_pos; rd[k].n_tiles = rows_tiles(rows[k].n_pos);
        items += rd[k].n_tiles;
    }
    out.n_items = items;
    out.grid = (unsigned)(items < ROWS_MAX_GRID ? items : ROWS_MAX_GRID);
    return SUSHI_HIP_OK;
}

// Buffers of n_in and n_out floats that share bytes are taken only in place: the same first float, and every row at the same
// offset in both.
inline bool rows_overlap_ok(const float* in, int64_t n_in, const float* out, int64_t n_out, const SushiHipRowsRow* rows, int n) {
    const uintptr_t a = (uintptr_t)in, b = (uintptr_t)out;
    const bool apart = a + (uint64_t)n_in * 4 <= b || b + (uint64_t)n_out * 4 <= a;
    if (apart) return true;
    if (a != b) return false;
    for (int k = 0; k < n; ++k)
        if (rows[k].in_off != rows[k].out_off) return false;
    return true;
}

// the row of work item `item`: the last row whose first item is not behind it
SUSHI_GEOM_HD inline int rows_row_of(const RowsRowDev* rows, int n, int64_t item) {
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (rows[mid].first_item <= item) lo = mid; else hi = mid - 1;
    }
    return lo;
}

}  // namespace sushi
#endif
