// sushi_amd/csrc/curve_core.hpp -- what sushi_hip_match_curves decides on the host, host only: no HIP header.  The records its
// kernels read (sushi_curve.hip), the workspace's layout, and stage_curves: requests -> a refusal, or the image that is uploaded and
// the facts of the launch.  tests/host_stream_check.cpp (plain g++) states what a staged call must be.
#ifndef SUSHI_CURVE_CORE_HPP
#define SUSHI_CURVE_CORE_HPP

#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "../../include/sushi_hip.h"
#include "sushi_geometry.hpp"

namespace sushi {

// One request on the device: where its pattern and window are, where its curve goes, its first work item.
struct CurveDesc {
    int64_t tmpl_off;
    int64_t win_start;
    int64_t out_off;        // first float of its curve in out_dev: sum of n_pos of the requests before it
    int64_t first_item;     // work items of the requests before it
    int32_t tmpl_len;
    int32_t n_pos;
};
static_assert(sizeof(CurveDesc) == 40, "CurveDesc layout");

// workspace: [queue head (u64) | padding to 256 B][CurveDesc x n], uploaded in one copy
constexpr size_t CURVE_HEAD = 256;
inline size_t curve_layout_bytes(int n) { return n <= 0 ? 0 : CURVE_HEAD + align_up((size_t)n * sizeof(CurveDesc), 256); }

// Positions per work item.  uint8: a tile of the matrix pipe; float32: 1024 where there are enough such items to fill the GPU,
// else 256 (a quarter of the chains' length each, four times the items).
constexpr int CURVE_U8_ITEM = TILE, CURVE_F32_ITEM = 1024, CURVE_F32_SMALL_ITEM = 256;
constexpr int64_t CURVE_F32_FILL = 2048;        // items of 1024 from which on they are taken
constexpr int64_t CURVE_MAX_GRID = 2048;        // a fixed grid that takes the items off the queue: 256 CUs, a few workgroups each

struct CurveStage {
    std::vector<char> image;    // the workspace as uploaded: queue head 0, then the descriptors
    int per_item;               // positions per work item
    int64_t n_items;
    unsigned grid;
};

// `n` >= 1 requests on streams of `dst_n` / `src_n` samples of `dtype`.  EINVAL: a request that request_fits refuses (`out` is
// then unspecified).
inline int stage_curves(const SushiHipRequest* req, int n, int dtype, int64_t dst_n, int64_t src_n, CurveStage& out) {
    int64_t items1024 = 0;
    for (int k = 0; k < n; ++k) {
        if (!request_fits(req[k], dst_n, src_n)) return SUSHI_HIP_EINVAL;
        items1024 += (req[k].n_pos + CURVE_F32_ITEM - 1) / CURVE_F32_ITEM;
    }
    out.per_item = dtype == SUSHI_HIP_U8 ? CURVE_U8_ITEM : (items1024 >= CURVE_F32_FILL ? CURVE_F32_ITEM : CURVE_F32_SMALL_ITEM);
    out.image.assign(curve_layout_bytes(n), 0);
    CurveDesc* d = reinterpret_cast<CurveDesc*>(out.image.data() + CURVE_HEAD);
    int64_t out_off = 0, items = 0;
    for (int k = 0; k < n; ++k) {
        const SushiHipRequest& r = req[k];
        d[k].tmpl_off = r.tmpl_off; d[k].win_start = r.win_start; d[k].tmpl_len = r.tmpl_len; d[k].n_pos = r.n_pos;
        d[k].out_off = out_off; d[k].first_item = items;
        out_off += r.n_pos;
        items += (r.n_pos + out.per_item - 1) / out.per_item;
    }
    out.n_items = items;
    out.grid = (unsigned)(items < CURVE_MAX_GRID ? items : CURVE_MAX_GRID);
    return SUSHI_HIP_OK;
}

}  // namespace sushi
#endif
