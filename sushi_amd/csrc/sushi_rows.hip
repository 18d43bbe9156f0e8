// sushi_amd/csrc/sushi_rows.hip -- sushi_hip_rows_from_hits, sushi_hip_rows_clamp: score rows clamped at a threshold (gfx950).
//
// A clamped row holds every score that passes a float32 value f and f everywhere else (include/sushi_hip.h "rows"; the rule, the
// tiles and the search are rows_core.hpp's).  sushi_hip_rows_from_hits forms it from what a threshold run left -- every passing
// position with the bits of its score, in ascending index order -- without forming a score: a streaming write, bound by HBM.
//
// One launch serves all rows: a row is cut into work items of ROWS_TILE consecutive floats, a workgroup finds its item's row by
// bisection of the items' running count.  It fills its tile with f -- the floats up to the first 16-byte boundary one by one, then
// whole 16-byte stores, lane <-> consecutive address, then the rest one by one: rows start at any float --, and while those stores
// drain it finds the records of its tile by two bisections of the request's list and checks its share of the list.  After a barrier
// it writes those records' scores.  No other workgroup writes to the tile, so the rows need no atomics and the result does not
// depend on the grid; the flags are OR-ed into words a memset cleared, which no order changes.
// sushi_hip_rows_clamp is the dense route for the requests whose lists overflowed: the same tiles, every float read, put through the
// rule and written by one thread (so in place is allowed), lane <-> consecutive float on both sides.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/sushi_hip.h"
#include "sushi_internal.hpp"
#include "rows_core.hpp"

namespace {

using namespace sushi;

struct RowsArgs {
    const RowsRowDev* rows;
    int n;
    int64_t n_items;
    const SushiHipHit* hits;        // from_hits: [n][capacity]
    const int64_t* counts;          // from_hits: [n]
    int32_t capacity;
    int32_t* flags;                 // from_hits: [n], cleared before the launch
    const float* in;                // clamp
    float* out;
    float f;
    int method;                     // clamp
};

__global__ __launch_bounds__(ROWS_THREADS)
void rows_from_hits_kernel(RowsArgs a) {
    const int tid = threadIdx.x;
    for (int64_t item = blockIdx.x; item < a.n_items; item += gridDim.x) {
        const int k = rows_row_of(a.rows, a.n, item);
        const RowsRowDev r = a.rows[k];
        const int32_t tile = (int32_t)(item - r.first_item);
        const int32_t t0 = rows_tile_first(tile), len = rows_tile_len(tile, r.n_pos);
        float* p = a.out + r.out_off + t0;
        // the fill: [0, head) up to a 16-byte boundary, nv whole 16-byte stores, the rest
        int32_t head = (int32_t)((4 - (((uintptr_t)p >> 2) & 3)) & 3);
        head = head < len ? head : len;
        const int32_t nv = (len - head) >> 2, rest0 = head + 4 * nv;
        if (tid < head) p[tid] = a.f;
        float4* q = reinterpret_cast<float4*>(p + head);
        const float4 f4 = make_float4(a.f, a.f, a.f, a.f);
        for (int32_t v = tid; v < nv; v += ROWS_THREADS) q[v] = f4;
        if (tid < len - rest0) p[rest0 + tid] = a.f;
        // the tile's records, and this tile's share of the checks
        int flag;
        const int64_t kept = rows_kept(a.counts[k], a.capacity, &flag);
        const SushiHipHit* h = a.hits + (int64_t)k * a.capacity;
        const RowsRange g = rows_tile_range(h, kept, t0, t0 + len);
        int64_t j0, j1;
        rows_check_slice(kept, r.n_tiles, tile, &j0, &j1);
        bool bad = false;
        for (int64_t j = j0 + tid; j < j1; j += ROWS_THREADS) bad = bad || !rows_hit_ok(h, j, r.n_pos);
        if (bad) flag |= SUSHI_HIP_ROWS_BAD_HITS;
        if (tid != 0 || tile != 0) flag &= ~SUSHI_HIP_ROWS_OVERFLOW;        // (what the count alone says: one thread of the row says it)
        if (flag) atomicOr(a.flags + k, flag);
        __syncthreads();            // the fill lies before the scores in every thread's view of the tile
        for (int64_t j = g.lo + tid; j < g.hi; j += ROWS_THREADS) {
            const SushiHipHit hit = h[j];
            if (hit.index >= t0 && hit.index < t0 + len) p[hit.index - t0] = hit.score;
        }
    }
}

__global__ __launch_bounds__(ROWS_THREADS)
void rows_clamp_kernel(RowsArgs a) {
    const int tid = threadIdx.x;
    for (int64_t item = blockIdx.x; item < a.n_items; item += gridDim.x) {
        const int k = rows_row_of(a.rows, a.n, item);
        const RowsRowDev r = a.rows[k];
        const int32_t tile = (int32_t)(item - r.first_item);
        const int32_t t0 = rows_tile_first(tile), len = rows_tile_len(tile, r.n_pos);
        const float* s = a.in + r.in_off + t0;      // (may be p: no __restrict__)
        float* p = a.out + r.out_off + t0;
#pragma unroll 4
        for (int32_t i = tid; i < len; i += ROWS_THREADS) p[i] = rows_clamped(a.method, s[i], a.f);
    }
}

// the table into the workspace; what both calls do before their launch
int upload_rows(const RowsStage& staged, void* mem_dev, size_t mem_bytes, hipStream_t st) {
    if ((uintptr_t)mem_dev & 255) return SUSHI_HIP_EALIGN;
    if (mem_bytes < staged.image.size()) return SUSHI_HIP_ENOSPACE;
    // (The source is pageable host memory that dies with the call.  ASSUMED: the runtime has taken its copy of such a source when
    // hipMemcpyAsync returns.)
    if (hipMemcpyAsync(mem_dev, staged.image.data(), staged.image.size(), hipMemcpyHostToDevice, st) != hipSuccess)
        return SUSHI_HIP_ELAUNCH;
    return SUSHI_HIP_OK;
}

}  // namespace

extern "C" {

int sushi_hip_rows_tile(void) { return ROWS_TILE; }

size_t sushi_hip_rows_bytes(int n) { return rows_layout_bytes(n); }

int sushi_hip_rows_from_hits(const SushiHipHit* hits_dev, const int64_t* counts_dev, int n, int32_t capacity,
                             const SushiHipRowsRow* rows_host, float f, float* out_dev, int64_t n_out, int32_t* flags_dev,
                             void* mem_dev, size_t mem_bytes, void* hip_stream) { return c_boundary([&]() -> int {
    if (!hits_dev || !counts_dev || !rows_host || !out_dev || !flags_dev || !mem_dev || capacity < 0) return SUSHI_HIP_EINVAL;
    RowsStage staged;
    int rc = stage_rows(rows_host, n, n_out, false, 0, f, staged);
    if (rc != SUSHI_HIP_OK) return rc;
    if (((uintptr_t)counts_dev & 7) || (((uintptr_t)hits_dev | (uintptr_t)out_dev | (uintptr_t)flags_dev) & 3)) return SUSHI_HIP_EALIGN;
    hipStream_t st = (hipStream_t)hip_stream;
    rc = upload_rows(staged, mem_dev, mem_bytes, st);
    if (rc != SUSHI_HIP_OK) return rc;
    if (hipMemsetAsync(flags_dev, 0, (size_t)n * sizeof(int32_t), st) != hipSuccess) return SUSHI_HIP_ELAUNCH;
    RowsArgs a = {};
    a.rows = (const RowsRowDev*)mem_dev; a.n = n; a.n_items = staged.n_items;
    a.hits = hits_dev; a.counts = counts_dev; a.capacity = capacity; a.flags = flags_dev;
    a.out = out_dev; a.f = f;
    hipLaunchKernelGGL(rows_from_hits_kernel, dim3(staged.grid), dim3(ROWS_THREADS), 0, st, a);
    return launch_ok();
}); }

int sushi_hip_rows_clamp(const float* in_dev, int64_t n_in, float* out_dev, int64_t n_out, const SushiHipRowsRow* rows_host, int n,
                         int method, float f, void* mem_dev, size_t mem_bytes, void* hip_stream) { return c_boundary([&]() -> int {
    if (!in_dev || !out_dev || !rows_host || !mem_dev || !method_known(method)) return SUSHI_HIP_EINVAL;
    RowsStage staged;
    int rc = stage_rows(rows_host, n, n_out, true, n_in, f, staged);
    if (rc != SUSHI_HIP_OK) return rc;
    if (!rows_overlap_ok(in_dev, n_in, out_dev, n_out, rows_host, n)) return SUSHI_HIP_EINVAL;
    if (((uintptr_t)in_dev | (uintptr_t)out_dev) & 3) return SUSHI_HIP_EALIGN;
    hipStream_t st = (hipStream_t)hip_stream;
    rc = upload_rows(staged, mem_dev, mem_bytes, st);
    if (rc != SUSHI_HIP_OK) return rc;
    RowsArgs a = {};
    a.rows = (const RowsRowDev*)mem_dev; a.n = n; a.n_items = staged.n_items;
    a.in = in_dev; a.out = out_dev; a.f = f; a.method = method;
    hipLaunchKernelGGL(rows_clamp_kernel, dim3(staged.grid), dim3(ROWS_THREADS), 0, st, a);
    return launch_ok();
}); }

}  // extern "C"
