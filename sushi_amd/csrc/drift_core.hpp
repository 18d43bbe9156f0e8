// sushi_amd/csrc/drift_core.hpp -- the arithmetic of sushi_hip_drift_reduce (include/sushi_hip.h "drift search"), one
// (candidate, index) at a time.  Plain C++: sushi_drift.hip runs it on the device, tests/host_drift_check.cpp on the CPU (g++).  Both
// are compiled with -ffp-contract=off: it is joint_accumulate unchanged, the product and the sum of a weighted row round separately.
// Behind it, host only: the workspace's layout and stage_drift -- tables -> a refusal, or the image that is uploaded and the facts of
// the launch.
#ifndef SUSHI_DRIFT_CORE_HPP
#define SUSHI_DRIFT_CORE_HPP

#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../include/sushi_hip.h"
#include "joint_core.hpp"          // joint_accumulate; through it axis_core.hpp: the first-extremum rule, the row check, the work split

namespace sushi {

// Candidates are taken DRIFT_DB at a time: a thread holds DRIFT_DB x PER sums, and the DRIFT_DB loads of one row, a few floats
// apart, are what the vector cache serves from one fetch.  (Measured at 2, 4 and 8, the macros for that: profiles/drift/README.md.)
#ifndef SUSHI_DRIFT_DB
#define SUSHI_DRIFT_DB 2
#endif
#ifndef SUSHI_DRIFT_FILL
#define SUSHI_DRIFT_FILL 2048
#endif
constexpr int DRIFT_DB = SUSHI_DRIFT_DB;
constexpr int DRIFT_MAX_DRIFTS = 65535;
constexpr int64_t DRIFT_FILL = SUSHI_DRIFT_FILL;    // work items of AXIS_PER_LARGE from which on they are taken

// The uploaded offset table is cut into blocks of DRIFT_DB candidates, [block][row][DRIFT_DB]: the DRIFT_DB offsets of one row lie
// together.  Candidates past the last (the last block's padding) repeat the last one's offsets and have an empty range.
SUSHI_GEOM_HD inline int64_t drift_offset_at(int n_rows, int d, int e) {
    return ((int64_t)(d / DRIFT_DB) * n_rows + e) * DRIFT_DB + d % DRIFT_DB;
}

// line[d][j] for a valid j of candidate d (lo_d <= j < hi_d: every row is addressed inside itself), in row order.
SUSHI_GEOM_HD inline float drift_value(const float* curves, const SushiHipJointRow* rows, int n_rows, const int32_t* offs, int d,
                                       int64_t j) {
    double acc = 0.0;
    for (int e = 0; e < n_rows; ++e)
        acc = joint_accumulate(acc, rows[e].weight, curves[rows[e].curve_off + j + offs[drift_offset_at(n_rows, d, e)]]);
    return (float)acc;
}

// ---- the host side of a call ----
struct DriftRange { int32_t lo, hi; };           // candidate d is valid on [lo, hi)
static_assert(sizeof(DriftRange) == 8, "DriftRange layout");

// workspace: [SushiHipJointRow x n_rows][int32 offsets x blocks x n_rows x DRIFT_DB][DriftRange x blocks x DRIFT_DB]
// [candidate keys (u64) x blocks x DRIFT_DB][the answer's key (u64)], each part padded to 256 bytes, uploaded in one copy (the keys
// as NO_KEY: all bits set)
struct DriftLayout {
    size_t rows, offs, ranges, keys, best_key, bytes;
};
inline int64_t drift_blocks(int n_drifts) { return ((int64_t)n_drifts + DRIFT_DB - 1) / DRIFT_DB; }
inline DriftLayout drift_layout(int n_rows, int n_drifts) {
    const size_t slots = (size_t)drift_blocks(n_drifts) * DRIFT_DB;
    DriftLayout l;
    l.rows = 0;
    l.offs = l.rows + align_up((size_t)n_rows * sizeof(SushiHipJointRow), 256);
    l.ranges = l.offs + align_up(slots * (size_t)n_rows * 4, 256);
    l.keys = l.ranges + align_up(slots * sizeof(DriftRange), 256);
    l.best_key = l.keys + align_up(slots * 8, 256);
    l.bytes = l.best_key + 256;
    return l;
}
inline size_t drift_layout_bytes(int n_rows, int n_drifts) {
    return n_rows < 1 || n_drifts < 1 || n_drifts > DRIFT_MAX_DRIFTS ? 0 : drift_layout(n_rows, n_drifts).bytes;
}

struct DriftStage {
    std::vector<char> image;    // the workspace as uploaded
    DriftLayout lay;
    int per;                    // AXIS_PER_LARGE or AXIS_PER_SMALL
    int64_t n_jitems;           // items of PER * AXIS_THREADS indices the axis is cut into
    int64_t n_items;            // n_jitems x blocks
    unsigned grid;
};

// EINVAL: a null table; an unknown method; n_rows < 1; n_drifts outside 1 .. DRIFT_MAX_DRIFTS; n_shift < 1; a row that leaves the
// curve buffer (axis_row_ok: without forming the sum); a weight that is not finite or is negative; a candidate whose valid range
// [max(0, max_e -o), n_shift - max(0, max_e o)) is empty -- any |o| >= n_shift is one; decided in 64 bits, INT32_MIN included.
// `out` is then unspecified.
inline int stage_drift(const SushiHipJointRow* rows, int n_rows, int32_t n_shift, const int32_t* offsets, int n_drifts,
                       int64_t n_curve, int method, DriftStage& out) {
    if (!rows || !offsets || !method_known(method)) return SUSHI_HIP_EINVAL;
    if (n_rows < 1 || n_drifts < 1 || n_drifts > DRIFT_MAX_DRIFTS || n_shift < 1) return SUSHI_HIP_EINVAL;
    for (int e = 0; e < n_rows; ++e)
        if (!axis_row_ok(rows[e], n_curve, n_shift)) return SUSHI_HIP_EINVAL;
    const int64_t blocks = drift_blocks(n_drifts);
    out.lay = drift_layout(n_rows, n_drifts);
    out.image.assign(out.lay.bytes, 0);
    memcpy(out.image.data() + out.lay.rows, rows, (size_t)n_rows * sizeof(SushiHipJointRow));
    int32_t* offs = reinterpret_cast<int32_t*>(out.image.data() + out.lay.offs);
    DriftRange* ranges = reinterpret_cast<DriftRange*>(out.image.data() + out.lay.ranges);
    for (int64_t d = 0; d < blocks * DRIFT_DB; ++d) {
        const int32_t* o = offsets + (size_t)(d < n_drifts ? d : n_drifts - 1) * (size_t)n_rows;
        int64_t below = 0, above = 0;               // max(0, max_e -o), max(0, max_e o)
        for (int e = 0; e < n_rows; ++e) {
            offs[drift_offset_at(n_rows, (int)d, e)] = o[e];
            if (-(int64_t)o[e] > below) below = -(int64_t)o[e];
            if ((int64_t)o[e] > above) above = o[e];
        }
        if (d >= n_drifts) { ranges[d].lo = ranges[d].hi = 0; continue; }
        if ((int64_t)n_shift - above <= below) return SUSHI_HIP_EINVAL;
        ranges[d].lo = (int32_t)below;
        ranges[d].hi = (int32_t)((int64_t)n_shift - above);
    }
    memset(out.image.data() + out.lay.keys, 0xff, out.lay.bytes - out.lay.keys);
    out.per = axis_per(axis_items(n_shift, AXIS_PER_LARGE) * blocks, DRIFT_FILL);
    out.n_jitems = axis_items(n_shift, out.per);
    out.n_items = out.n_jitems * blocks;
    out.grid = axis_grid(out.n_items);
    return SUSHI_HIP_OK;
}

}  // namespace sushi
#endif
