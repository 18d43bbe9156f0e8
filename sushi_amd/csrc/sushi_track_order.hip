// sushi_amd/csrc/sushi_track_order.hip -- sushi_hip_track_forward_ordered / sushi_hip_track_backtrack_ordered: the tracking pass
// (sushi_track.hip) with events kept in order -- a jump into (e, j) comes from an index of row e - 1 no further than back_e above j,
// at a penalty of row e's own (gfx950).
//
// D_e[j] = u_e[j] + min(near_e[j], P_{e-1}[t_e(j)] + penalty_e), P the prefix minimum of D_{e-1} and t_e(j) = min(j + back_e,
// n_shift - 1), in the arithmetic include/sushi_hip.h "ordered tracking" states and track_core.hpp / track_order_core.hpp implement
// (float64, -ffp-contract=off).  The output is bit-identical to the NumPy restatement (sushi_amd/track.py track_ordered_host); with
// every back unlimited and one penalty it is sushi_track.hip's, bit for bit.
//
// Per row the all-to-all is no longer one scalar but a whole row, P_{e-1}, and with it A_{e-1}, the index that attains it.  Three
// plain launches per row, stream-ordered; the launch boundary is the only synchronisation, and no workgroup waits on another:
//   step   sushi_track.hip's step kernel -- the window minimum over an LDS tile, the <PER, MAX, HALO> dispatch, the partial records
//          -- with jump read per index from P at t_e(j): lane <-> consecutive index still, so a wave reads 64 consecutive doubles
//          shifted by back_e.  It also leaves one (min, first index) record per work item.
//   scan   one workgroup: the exclusive scan of the work items' records -- what lies before every item -- and the row's outputs
//          from the partial records (so no launch closes a call).
//   apply  a work item re-reads its PER x 256 values of D_e, scans them (a wave's shuffles, the four waves through LDS, PER rounds
//          in index order) onto what lies before it, and writes P_e and A_e.
// P is one buffer: row e's step reads P_{e-1} before row e's apply writes P_e.  A call that ends before the sequence's last row
// leaves P and A of its last row in the state, and the next call's first step reads them: chunks have the bits of one call.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/sushi_hip.h"
#include "sushi_internal.hpp"
#include "track_order_core.hpp"
#include "path_device.hpp"

namespace {

using namespace sushi;

struct OrderArgs {
    const float* row;                       // R_e: curves + curve_off
    double weight, penalty, step_cost;      // penalty: row e's
    const double* D_in;                     // [n_shift] D_{e-1}: half (e - 1) & 1
    double* D_out;                          // [n_shift] D_e: half e & 1
    int16_t* move;                          // [n_shift] row e's moves
    double* P;                              // [n_shift]: P_{e-1} for the step, P_e after the apply
    int32_t* from;                          // [n_shift] row e's A
    int32_t* back_dev;                      // [n_total]
    int32_t n_shift;
    int32_t reach;                          // reach_e (0 for e = 0)
    int32_t back;                           // back_e
    int64_t n_items;
    int e;                                  // the row of the sequence
    int n_partials;                         // records of `partials`
    PathPartials partials;                  // the step's, one per workgroup
    double* item_min; int32_t* item_arg;    // [n_items] the step's, one per work item
    double* before_min; int32_t* before_arg;    // [n_items] the scan's: (min, first index) over the items before this one
    double* row_min; int32_t* row_arg; int32_t* row_own_index; float* row_own_score;    // the whole sequence's
};

__device__ __forceinline__ OrderMin shfl_up_min(OrderMin a, int d) {
    return OrderMin{__shfl_up(a.v, d, 64), __shfl_up(a.i, d, 64)};
}
// the inclusive scan of a wave's 64 elements in lane order
__device__ __forceinline__ OrderMin wave_scan_min(OrderMin x) {
    const int lane = (int)threadIdx.x & 63;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const OrderMin o = shfl_up_min(x, d);
        const OrderMin c = order_combine(o, x);
        x = lane >= d ? c : x;
    }
    return x;
}
struct ScanLds { double v[4]; int32_t i[4]; };
// A workgroup's 256 elements in thread order, scanned onto `carry` (what lies before them): the inclusive result of this thread's
// element, and `carry` moved past all 256.  *before_mine: what lies before this thread's element.  Two barriers, the first of which
// lets the readers of an earlier round through: every thread calls it.
__device__ __forceinline__ OrderMin block_scan_min(OrderMin x, OrderMin& carry, ScanLds& s, OrderMin* before_mine) {
    const int lane = (int)threadIdx.x & 63, w = (int)threadIdx.x >> 6;
    const OrderMin incl = wave_scan_min(x);
    __syncthreads();
    if (lane == 63) { s.v[w] = incl.v; s.i[w] = incl.i; }
    __syncthreads();
    OrderMin pref = carry;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const OrderMin c = order_combine(carry, OrderMin{s.v[k], s.i[k]});
        pref = k < w ? c : pref;
        carry = c;
    }
    const OrderMin left = shfl_up_min(incl, 1);
    const OrderMin upto = order_combine(pref, left);
    *before_mine = lane == 0 ? pref : upto;
    return order_combine(pref, incl);
}

// HALO: the rounds of 256 halo values a launch loads (track_halo_rounds(reach): 0 at reach 0, where nothing is staged)
template <int PER, bool MAX, int HALO>
__global__ __launch_bounds__(TRACK_THREADS)
void order_step_kernel(OrderArgs a) {
    constexpr int METHOD = MAX ? SUSHI_HIP_METHOD_CCOEFF_NORMED : SUSHI_HIP_METHOD_SQDIFF_NORMED;
    constexpr int SPAN = PER * TRACK_THREADS;
    __shared__ PathLds lds;
    extern __shared__ double tile[];        // [reach + SPAN + reach]: entry l is D_{e-1}[item's first index - reach + l]
    const float* __restrict__ row = a.row;
    const double* __restrict__ Din = a.D_in;
    const double* __restrict__ Pin = a.P;
    double* __restrict__ Dout = a.D_out;
    int16_t* __restrict__ move = a.move;
    const int32_t n_shift = a.n_shift;
    const int32_t reach = HALO == 0 ? 0 : a.reach;
    const bool first = a.e == 0;

    MinD best = {INFINITY, PATH_NO_INDEX};
    OwnF own = {own_worst<METHOD>(), PATH_NO_INDEX};
    for (int64_t item = blockIdx.x; item < a.n_items; item += gridDim.x) {
        // (an item's first index is below n_shift < 2^31; the indices behind it may pass 2^31 only where they are not used: 64 bits)
        const int64_t base = item * SPAN;
        const int64_t j0 = base + threadIdx.x;
        // every load is always made, the indices outside the axis moved onto an element inside it (axis_at; t_e(j) lies inside the
        // axis for every j >= 0): the tile, the halo, P and the row are all asked for before the first value is used
        int32_t at[PER];
        float r[PER];
        double d[PER], pt[PER];
        double hv[HALO > 0 ? HALO : 1];
        int32_t hl[HALO > 0 ? HALO : 1];    // where a halo value goes in the tile; -1: this thread has none in that round
#pragma unroll
        for (int p = 0; p < PER; ++p) at[p] = axis_at(j0 + p * TRACK_THREADS, n_shift);
#pragma unroll
        for (int p = 0; p < PER; ++p) d[p] = Din[at[p]];
        if (HALO > 0) {
#pragma unroll
            for (int k = 0; k < HALO; ++k) {
                // halo entry h of 2 * reach: the left side's h < reach at index base - reach + h, the right side's at base + SPAN + h - reach
                const int32_t h = (int32_t)threadIdx.x + k * TRACK_THREADS;
                const bool left = h < reach;
                int64_t g = left ? base - reach + h : base + SPAN + (h - reach);
                g = g < 0 ? 0 : g;
                hl[k] = h < 2 * reach ? (left ? h : SPAN + h) : -1;
                hv[k] = Din[axis_at(g, n_shift)];
            }
        }
        // P_{e-1} at t_e(j): consecutive lanes read consecutive doubles, back_e further up, the last ones all the row's last
#pragma unroll
        for (int p = 0; p < PER; ++p) pt[p] = Pin[order_reach_back(at[p], a.back, n_shift)];
#pragma unroll
        for (int p = 0; p < PER; ++p) r[p] = row[at[p]];
        // (nothing is scheduled across this line: the loads above are all in flight before the first is waited for)
        __builtin_amdgcn_sched_barrier(0);
        if (HALO > 0) {
            __syncthreads();                // the readers of the item before this one are through
#pragma unroll
            for (int p = 0; p < PER; ++p) tile[reach + (int32_t)threadIdx.x + p * TRACK_THREADS] = d[p];
#pragma unroll
            for (int k = 0; k < HALO; ++k)
                if (hl[k] >= 0) tile[hl[k]] = hv[k];
            __syncthreads();
        }
        // near_e[j], as in sushi_track.hip: the thread's own value is cand(0); the others come from the tile in the order -1, +1,
        // -2, +2, ..., in which track_replaces is the strict comparison
        double near[PER];
        int32_t nd[PER], room_lo[PER], room_hi[PER];
#pragma unroll
        for (int p = 0; p < PER; ++p) {
            const int64_t j = j0 + p * TRACK_THREADS, up = (int64_t)n_shift - 1 - j;
            near[p] = d[p]; nd[p] = 0;
            room_lo[p] = (int32_t)(j < reach ? j : reach);
            room_hi[p] = (int32_t)(up < 0 ? -1 : (up < reach ? up : reach));
        }
        if (HALO > 0) {
            for (int32_t s = 1; s <= reach; ++s) {
                const double price = track_price(a.step_cost, s);
#pragma unroll
                for (int p = 0; p < PER; ++p) {
                    const int32_t l = reach + (int32_t)threadIdx.x + p * TRACK_THREADS;
                    const double lo = track_cand(tile[l - s], price), hi = track_cand(tile[l + s], price);
                    const bool take_lo = (int)(s <= room_lo[p]) & (int)track_replaces_in_order(lo, near[p]);
                    near[p] = take_lo ? lo : near[p]; nd[p] = take_lo ? -s : nd[p];
                    const bool take_hi = (int)(s <= room_hi[p]) & (int)track_replaces_in_order(hi, near[p]);
                    near[p] = take_hi ? hi : near[p]; nd[p] = take_hi ? s : nd[p];
                }
            }
        }
        MinD mine = {INFINITY, PATH_NO_INDEX};
#pragma unroll
        for (int p = 0; p < PER; ++p) {
            const int64_t j = j0 + p * TRACK_THREADS;
            const bool valid = j < n_shift;
            const double u = path_cost(METHOD, a.weight, r[p]);
            int16_t mv = 0;
            const double stepped = track_step(near[p], nd[p], u, order_jump(pt[p], a.penalty), &mv);
            const double dn = first ? u : stepped;
            mv = first ? (int16_t)0 : mv;
            const bool take = (int)valid & (int)path_min_replaces(dn, (int32_t)j, mine.v, mine.i);
            mine.v = take ? dn : mine.v; mine.i = take ? (int32_t)j : mine.i;
            const bool take_own = (int)valid & (int)path_own_replaces(METHOD, r[p], (int32_t)j, own.v, own.i);
            own.v = take_own ? r[p] : own.v; own.i = take_own ? (int32_t)j : own.i;
            if (valid) {
                Dout[j] = dn;
                move[j] = mv;
            }
        }
        // the item's record (valid in every thread), and the workgroup's over its items
        mine = block_first_min(mine, lds);
        if (threadIdx.x == 0) { a.item_min[item] = mine.v; a.item_arg[item] = mine.i; }
        const bool take = path_min_replaces(mine.v, mine.i, best.v, best.i);
        best.v = take ? mine.v : best.v; best.i = take ? mine.i : best.i;
    }
    own = block_first_own<METHOD>(own, lds);
    if (threadIdx.x == 0) {
        a.partials.d_min[blockIdx.x] = best.v; a.partials.d_arg[blockIdx.x] = best.i;
        a.partials.own_idx[blockIdx.x] = own.i; a.partials.own_val[blockIdx.x] = own.v;
    }
}

// one workgroup: what lies before every work item of row e, the row's outputs, and its back for the backtrack
template <bool MAX>
__global__ __launch_bounds__(TRACK_THREADS)
void order_scan_kernel(OrderArgs a) {
    constexpr int METHOD = MAX ? SUSHI_HIP_METHOD_CCOEFF_NORMED : SUSHI_HIP_METHOD_SQDIFF_NORMED;
    __shared__ PathLds lds;
    __shared__ ScanLds scan;
    OrderMin carry = order_none();
    for (int64_t k0 = 0; k0 < a.n_items; k0 += TRACK_THREADS) {
        const int64_t k = k0 + threadIdx.x;
        const bool valid = k < a.n_items;
        const int64_t at = valid ? k : a.n_items - 1;
        const double v = a.item_min[at];
        const int32_t i = a.item_arg[at];
        OrderMin before;
        block_scan_min(valid ? OrderMin{v, i} : order_none(), carry, scan, &before);
        if (valid) { a.before_min[k] = before.v; a.before_arg[k] = before.i; }
    }
    reduce_partials<METHOD>(a.partials, a.n_partials, true, a.e, a, lds);
    if (threadIdx.x == 0) a.back_dev[a.e] = a.back;
}

// P_e and A_e of one work item's indices: its values of D_e scanned, PER rounds of 256 in index order, onto what lies before it
template <int PER>
__global__ __launch_bounds__(TRACK_THREADS)
void order_apply_kernel(OrderArgs a) {
    constexpr int SPAN = PER * TRACK_THREADS;
    __shared__ ScanLds scan;
    const double* __restrict__ D = a.D_out;
    const int32_t n_shift = a.n_shift;
    for (int64_t item = blockIdx.x; item < a.n_items; item += gridDim.x) {
        const int64_t j0 = item * SPAN + threadIdx.x;
        double d[PER];
#pragma unroll
        for (int p = 0; p < PER; ++p) d[p] = D[axis_at(j0 + p * TRACK_THREADS, n_shift)];
        OrderMin carry = {a.before_min[item], a.before_arg[item]};
#pragma unroll
        for (int p = 0; p < PER; ++p) {
            const int64_t j = j0 + p * TRACK_THREADS;
            const bool valid = j < n_shift;
            OrderMin before;
            const OrderMin upto = block_scan_min(valid ? OrderMin{d[p], (int32_t)j} : order_none(), carry, scan, &before);
            if (valid) {
                a.P[j] = upto.v;
                a.from[j] = upto.i;
            }
        }
    }
}

// one wave; lane 0 walks the rows backwards: every step reads the move the step before it chose
__global__ __launch_bounds__(64)
void order_backtrack_kernel(const int16_t* move, const int32_t* from, const int32_t* back, const int32_t* row_arg, int n_total,
                            int32_t n_shift, int32_t* out_shift) {
    if (threadIdx.x == 0 && blockIdx.x == 0) order_backtrack(move, from, back, row_arg, n_total, n_shift, out_shift);
}

template <int PER, bool MAX>
void launch_step(int halo, dim3 grid, size_t tile_bytes, hipStream_t st, const OrderArgs& a) {
    const dim3 block(TRACK_THREADS);
    if (halo == 0) hipLaunchKernelGGL((order_step_kernel<PER, MAX, 0>), grid, block, 0, st, a);
    else if (halo == TRACK_HALO_SMALL) hipLaunchKernelGGL((order_step_kernel<PER, MAX, TRACK_HALO_SMALL>), grid, block, tile_bytes, st, a);
    else hipLaunchKernelGGL((order_step_kernel<PER, MAX, TRACK_HALO_LARGE>), grid, block, tile_bytes, st, a);
}

}  // namespace

extern "C" {

size_t sushi_hip_track_order_bytes(int n_rows, int32_t n_shift) { return order_layout_bytes(n_rows, n_shift); }

// sushi_hip_track_forward_ordered and sushi_hip_track_forward_ordered_keep: one body.  keep: D_dev holds every row ([n_total][n_shift]:
// row e reads row e - 1 and writes row e) instead of two halves used by turns; the launches, and so the bits, are the same.
static int track_forward_ordered(bool keep, const float* curves_dev, int64_t n_curve, const SushiHipJointRow* rows_host,
                                 const int32_t* reach_host, const int32_t* back_host, int n_rows, int32_t n_shift, int method,
                                 const double* penalty_host, double step_cost, int row0, int n_total, double* D_dev, int16_t* move_dev,
                                 double* P_dev, int32_t* from_dev, int32_t* back_dev, double* row_min_dev, int32_t* row_arg_dev,
                                 int32_t* row_own_index_dev, float* row_own_score_dev, void* mem_dev, size_t mem_bytes,
                                 void* hip_stream) {
    if (!curves_dev || !rows_host || !reach_host || !back_host || !penalty_host || !D_dev || !move_dev || !P_dev || !from_dev ||
        !back_dev || !row_min_dev || !row_arg_dev || !row_own_index_dev || !row_own_score_dev || !mem_dev) return SUSHI_HIP_EINVAL;
    OrderStage staged;
    const int rc = stage_track_ordered(rows_host, reach_host, back_host, penalty_host, n_rows, n_shift, n_curve, method, step_cost, row0,
                                       n_total, mem_dev, mem_bytes, staged);
    if (rc != SUSHI_HIP_OK) return rc;
    if ((((uintptr_t)D_dev | (uintptr_t)P_dev | (uintptr_t)row_min_dev) & 7) ||
        (((uintptr_t)curves_dev | (uintptr_t)from_dev | (uintptr_t)back_dev | (uintptr_t)row_arg_dev | (uintptr_t)row_own_index_dev |
          (uintptr_t)row_own_score_dev) & 3) ||
        ((uintptr_t)move_dev & 1))
        return SUSHI_HIP_EALIGN;

    hipStream_t st = (hipStream_t)hip_stream;
    char* mem = (char*)mem_dev;
    OrderArgs a;
    a.step_cost = step_cost;
    a.P = P_dev;
    a.back_dev = back_dev;
    a.n_shift = n_shift;
    a.n_items = staged.split.n_items;
    a.n_partials = (int)staged.split.grid;
    a.partials = partial_set(mem, staged.lay.partials, 0);
    a.item_min = (double*)(mem + staged.lay.item_min); a.item_arg = (int32_t*)(mem + staged.lay.item_arg);
    a.before_min = (double*)(mem + staged.lay.before_min); a.before_arg = (int32_t*)(mem + staged.lay.before_arg);
    a.row_min = row_min_dev; a.row_arg = row_arg_dev; a.row_own_index = row_own_index_dev; a.row_own_score = row_own_score_dev;
    const bool mx = method == SUSHI_HIP_METHOD_CCOEFF_NORMED;
    const dim3 grid(staged.split.grid), block(TRACK_THREADS);
    for (int i = 0; i < n_rows; ++i) {
        a.e = row0 + i;
        a.row = curves_dev + rows_host[i].curve_off;
        a.weight = rows_host[i].weight;
        a.penalty = a.e == 0 ? 0.0 : penalty_host[i];
        a.reach = a.e == 0 ? 0 : reach_host[i];
        a.back = back_host[i];
        // (row 0 has no row before it: its launch's loads of D_in and P, which are always made and never used, go to its own
        // half -- keep: its own row -- and to P as it stands)
        a.D_in = D_dev + (keep ? (int64_t)(a.e == 0 ? 0 : a.e - 1) : (int64_t)((a.e + 1) & 1)) * n_shift;
        a.D_out = D_dev + (keep ? (int64_t)a.e : (int64_t)(a.e & 1)) * n_shift;
        a.move = move_dev + (int64_t)a.e * n_shift;
        a.from = from_dev + (int64_t)a.e * n_shift;
        const int halo = track_halo_rounds(a.reach);
        const size_t tile_bytes = track_tile_bytes(staged.split.per, a.reach);
        axis_dispatch(staged.split.per, mx, [&](auto per, auto is_max) {
            launch_step<per.value, is_max.value>(halo, grid, tile_bytes, st, a);
            hipLaunchKernelGGL(order_scan_kernel<is_max.value>, dim3(1), block, 0, st, a);
            hipLaunchKernelGGL(order_apply_kernel<per.value>, grid, block, 0, st, a);
        });
        if (hipGetLastError() != hipSuccess) return SUSHI_HIP_ELAUNCH;
    }
    return launch_ok();
}

int sushi_hip_track_forward_ordered(const float* curves_dev, int64_t n_curve, const SushiHipJointRow* rows_host, const int32_t* reach_host,
                                    const int32_t* back_host, int n_rows, int32_t n_shift, int method, const double* penalty_host,
                                    double step_cost, int row0, int n_total, double* D_dev, int16_t* move_dev, double* P_dev,
                                    int32_t* from_dev, int32_t* back_dev, double* row_min_dev, int32_t* row_arg_dev,
                                    int32_t* row_own_index_dev, float* row_own_score_dev, void* mem_dev, size_t mem_bytes,
                                    void* hip_stream) { return c_boundary([&]() -> int {
    return track_forward_ordered(false, curves_dev, n_curve, rows_host, reach_host, back_host, n_rows, n_shift, method, penalty_host,
                                 step_cost, row0, n_total, D_dev, move_dev, P_dev, from_dev, back_dev, row_min_dev, row_arg_dev,
                                 row_own_index_dev, row_own_score_dev, mem_dev, mem_bytes, hip_stream);
}); }

int sushi_hip_track_forward_ordered_keep(const float* curves_dev, int64_t n_curve, const SushiHipJointRow* rows_host,
                                         const int32_t* reach_host, const int32_t* back_host, int n_rows, int32_t n_shift, int method,
                                         const double* penalty_host, double step_cost, int row0, int n_total, double* D_all_dev,
                                         int16_t* move_dev, double* P_dev, int32_t* from_dev, int32_t* back_dev, double* row_min_dev,
                                         int32_t* row_arg_dev, int32_t* row_own_index_dev, float* row_own_score_dev, void* mem_dev,
                                         size_t mem_bytes, void* hip_stream) { return c_boundary([&]() -> int {
    return track_forward_ordered(true, curves_dev, n_curve, rows_host, reach_host, back_host, n_rows, n_shift, method, penalty_host,
                                 step_cost, row0, n_total, D_all_dev, move_dev, P_dev, from_dev, back_dev, row_min_dev, row_arg_dev,
                                 row_own_index_dev, row_own_score_dev, mem_dev, mem_bytes, hip_stream);
}); }

int sushi_hip_track_backtrack_ordered(const int16_t* move_dev, const int32_t* from_dev, const int32_t* back_dev, const int32_t* row_arg_dev,
                                      int n_total, int32_t n_shift, int32_t* out_shift_dev, void* hip_stream) {
    return c_boundary([&]() -> int {
    if (!move_dev || !from_dev || !back_dev || !row_arg_dev || !out_shift_dev || n_total < 1 || n_shift < 1) return SUSHI_HIP_EINVAL;
    if (((uintptr_t)move_dev & 1) || (((uintptr_t)from_dev | (uintptr_t)back_dev | (uintptr_t)row_arg_dev | (uintptr_t)out_shift_dev) & 3))
        return SUSHI_HIP_EALIGN;
    hipLaunchKernelGGL(order_backtrack_kernel, dim3(1), dim3(64), 0, (hipStream_t)hip_stream, move_dev, from_dev, back_dev, row_arg_dev,
                       n_total, n_shift, out_shift_dev);
    return launch_ok();
}); }

}  // extern "C"
