// sushi_amd/csrc/joint_core.hpp -- the arithmetic of sushi_hip_joint_reduce (include/sushi_hip.h "joint search"), one
// joint index at a time.  Plain C++: sushi_joint.hip runs it on the device, tests/host_joint_check.cpp on the CPU (g++).  Both are
// compiled with -ffp-contract=off: the product and the sum of a weighted row round separately, as NumPy's do.
// Behind it, host only: the records the kernels read, the workspace's layout, and stage_joint -- tables -> a refusal, or the image
// that is uploaded and the facts of the launch.
#ifndef SUSHI_JOINT_CORE_HPP
#define SUSHI_JOINT_CORE_HPP

#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../include/sushi_hip.h"
#include "axis_core.hpp"           // the first-extremum rule, the row check, the work split

namespace sushi {

// One row's share of a joint value: acc + w * (double)v, the product rounded before the sum.
SUSHI_GEOM_HD inline double joint_accumulate(double acc, double w, float v) {
    const double p = w * (double)v;
    return acc + p;
}

// joint[j] of a group: rows first_row .. first_row + n_rows - 1 of `rows` (any record with curve_off and weight), in row order.
template <class Row>
SUSHI_GEOM_HD inline float joint_value(const float* curves, const Row* rows, int first_row, int n_rows, int64_t j) {
    double acc = 0.0;
    for (int i = 0; i < n_rows; ++i) acc = joint_accumulate(acc, rows[first_row + i].weight, curves[rows[first_row + i].curve_off + j]);
    return (float)acc;
}

// the first extremum of n >= 1 values (axis_better's rule)
inline int32_t joint_first_extremum(const float* v, int32_t n, int method) {
    int32_t at = 0;
    for (int32_t j = 1; j < n; ++j)
        if (axis_better(method, v[j], v[at])) at = j;
    return at;
}

// ---- the host side of a call ----
// a group on the device
struct JointGroupDev {
    int64_t first_item;     // work items of the groups before this one
    int64_t joint_off;      // first float of its joint row in out_joint_dev: sum of n_shift of the groups before it
    int32_t first_row, n_rows, n_shift;
    int32_t reserved;
};
static_assert(sizeof(JointGroupDev) == 32, "JointGroupDev layout");
// a row on the device
struct JointRowDev {
    int64_t curve_off;
    double weight;
    int32_t group;
    int32_t reserved;
};
static_assert(sizeof(JointRowDev) == 24, "JointRowDev layout");

// Every group's joint indices are cut into work items of their own (axis_core.hpp), and one grid strides over the items of all groups.
constexpr int64_t JOINT_FILL = 2048;            // items of AXIS_PER_LARGE, over all groups, from which on they are taken

// workspace: [JointGroupDev x n_groups][JointRowDev x n_rows][group keys (u64) x n_groups][row keys (u64) x n_rows], each part
// padded to 256 bytes, uploaded in one copy (the keys as NO_KEY: all bits set)
struct JointLayout {
    size_t groups, rows, group_keys, row_keys, bytes;
};
inline JointLayout joint_layout(int n_groups, int n_rows) {
    JointLayout l;
    l.groups = 0;
    l.rows = l.groups + align_up((size_t)n_groups * sizeof(JointGroupDev), 256);
    l.group_keys = l.rows + align_up((size_t)n_rows * sizeof(JointRowDev), 256);
    l.row_keys = l.group_keys + align_up((size_t)n_groups * 8, 256);
    l.bytes = l.row_keys + align_up((size_t)n_rows * 8, 256);
    return l;
}
inline size_t joint_layout_bytes(int n_groups, int n_rows) {
    return n_groups < 1 || n_rows < n_groups ? 0 : joint_layout(n_groups, n_rows).bytes;
}

struct JointStage {
    std::vector<char> image;    // the workspace as uploaded
    JointLayout lay;
    int per;                    // AXIS_PER_LARGE or AXIS_PER_SMALL
    int64_t n_items;
    int64_t n_joint;            // floats of out_joint_dev
    unsigned grid;
};

// EINVAL: an unknown method; no group, no row, fewer rows than groups, an empty curve buffer; groups that do not tile the rows in
// order (first_row is not the sum of the n_rows before it, n_rows < 1, or the last group does not end at n_rows); n_shift < 1; a row
// that leaves the curve buffer (curve_off < 0 or curve_off + n_shift > n_curve, without forming the sum); a weight that is not
// finite or is negative.  `out` is then unspecified.
inline int stage_joint(const SushiHipJointRow* rows, int n_rows, const SushiHipJointGroup* groups, int n_groups, int64_t n_curve,
                       int method, JointStage& out) {
    if (!method_known(method)) return SUSHI_HIP_EINVAL;
    if (n_groups < 1 || n_rows < n_groups || n_curve < 1) return SUSHI_HIP_EINVAL;
    int64_t next_row = 0, items_large = 0;
    for (int g = 0; g < n_groups; ++g) {
        const SushiHipJointGroup& G = groups[g];
        if (G.first_row != next_row || G.n_rows < 1 || G.n_rows > n_rows - next_row) return SUSHI_HIP_EINVAL;
        if (G.n_shift < 1 || G.n_shift > n_curve) return SUSHI_HIP_EINVAL;
        for (int i = 0; i < G.n_rows; ++i)
            if (!axis_row_ok(rows[G.first_row + i], n_curve, G.n_shift)) return SUSHI_HIP_EINVAL;
        next_row += G.n_rows;
        items_large += axis_items(G.n_shift, AXIS_PER_LARGE);
    }
    if (next_row != n_rows) return SUSHI_HIP_EINVAL;
    out.per = axis_per(items_large, JOINT_FILL);
    out.lay = joint_layout(n_groups, n_rows);
    out.image.assign(out.lay.bytes, 0);
    JointGroupDev* gd = reinterpret_cast<JointGroupDev*>(out.image.data() + out.lay.groups);
    JointRowDev* rd = reinterpret_cast<JointRowDev*>(out.image.data() + out.lay.rows);
    int64_t items = 0, joint_off = 0;
    for (int g = 0; g < n_groups; ++g) {
        const SushiHipJointGroup& G = groups[g];
        gd[g].first_item = items; gd[g].joint_off = joint_off;
        gd[g].first_row = G.first_row; gd[g].n_rows = G.n_rows; gd[g].n_shift = G.n_shift; gd[g].reserved = 0;
        for (int i = 0; i < G.n_rows; ++i) {
            JointRowDev& r = rd[G.first_row + i];
            r.curve_off = rows[G.first_row + i].curve_off; r.weight = rows[G.first_row + i].weight; r.group = g; r.reserved = 0;
        }
        items += axis_items(G.n_shift, out.per);
        joint_off += G.n_shift;
    }
    memset(out.image.data() + out.lay.group_keys, 0xff, out.lay.bytes - out.lay.group_keys);
    out.n_items = items;
    out.n_joint = joint_off;
    out.grid = axis_grid(items);
    return SUSHI_HIP_OK;
}

}  // namespace sushi
#endif
