// sushi_amd/csrc/sushi_track_margins_step.inc -- the margins pass's step and close kernels and their launcher: a part of
// sushi_track.hip, which describes them; a wide call sends its rows of a reach up to TRACK_MAX_REACH through the same code.
// Included once, inside the unit's anonymous namespace, after sushi_internal.hpp, track_margin_core.hpp,
// path_device.hpp and track_margin_device.hpp and a `using namespace sushi`.
struct MarginArgs {
    const float* row;                       // R_e: curves + curve_off
    double weight, penalty, step_cost;
    const double* C_in;                     // [n_shift] C_{e+1}: half (e + 1) & 1
    double* C_out;                          // [n_shift] C_e: half e & 1
    const double* D_row;                    // [n_shift] D_e
    double* M_row;                          // [n_shift] M_e, or null
    const int32_t* shift;                   // [n_total] s_e
    int32_t n_shift;
    int32_t reach;                          // reach_{e+1} (0 for the sequence's last row)
    int32_t guard;                          // guard_e
    int64_t n_items;
    int e;                                  // the row of the sequence
    int prev;                               // where n_{e+1} comes from (path_device.hpp PREV_*; PREV_ROW_MIN: c_min[e + 1])
    int n_partials;                         // records of `in`
    MarginPartials in, out;
    double* through; double* best; int32_t* best_arg; double* alt; int32_t* alt_arg; double* c_min;    // the whole sequence's
};

// HALO: the rounds of 256 halo values a launch loads (track_halo_rounds(reach): 0 at reach 0, where nothing is staged)
template <int PER, bool MAX, int HALO>
__global__ __launch_bounds__(TRACK_THREADS)
void margin_step_kernel(MarginArgs a) {
    constexpr int METHOD = MAX ? SUSHI_HIP_METHOD_CCOEFF_NORMED : SUSHI_HIP_METHOD_SQDIFF_NORMED;
    constexpr int SPAN = PER * TRACK_THREADS;
    __shared__ PathLds lds;
    extern __shared__ double tile[];        // [reach + SPAN + reach]: entry l is C_{e+1}[item's first index - reach + l]
    const float* __restrict__ row = a.row;
    const double* __restrict__ Cin = a.C_in;
    const double* __restrict__ Drow = a.D_row;
    double* __restrict__ Cout = a.C_out;
    double* __restrict__ Mrow = a.M_row;
    const int32_t n_shift = a.n_shift;
    const int32_t reach = HALO == 0 ? 0 : a.reach;
    const bool last = a.prev == PREV_NONE;  // the sequence's last row: there is no B
    const int32_t s_e = path_clamp(a.shift[a.e], n_shift);
    const int32_t guard = a.guard;
    double jump = 0.0;
    if (a.prev == PREV_PARTIALS) jump = reduce_margin_partials(a, blockIdx.x == 0, a.e + 1, lds) + a.penalty;
    else if (a.prev == PREV_ROW_MIN) jump = a.c_min[a.e + 1] + a.penalty;

    MinD best_c = {INFINITY, PATH_NO_INDEX}, best_m = {INFINITY, PATH_NO_INDEX}, best_a = {INFINITY, PATH_NO_INDEX};
    for (int64_t item = blockIdx.x; item < a.n_items; item += gridDim.x) {
        // (an item's first index is below n_shift < 2^31; the indices behind it may pass 2^31 only where they are not used: 64 bits)
        const int64_t base = item * SPAN;
        const int64_t j0 = base + threadIdx.x;
        // every load is always made, the indices outside the axis moved onto an element inside it (axis_at): the tile, the halo,
        // the row and D_e are all asked for before the first value is used
        int32_t at[PER];
        float r[PER];
        double c[PER], dd[PER];
        double hv[HALO > 0 ? HALO : 1];
        int32_t hl[HALO > 0 ? HALO : 1];    // where a halo value goes in the tile; -1: this thread has none in that round
#pragma unroll
        for (int p = 0; p < PER; ++p) at[p] = axis_at(j0 + p * TRACK_THREADS, n_shift);
#pragma unroll
        for (int p = 0; p < PER; ++p) c[p] = Cin[at[p]];
        if (HALO > 0) {
#pragma unroll
            for (int k = 0; k < HALO; ++k) {
                // halo entry h of 2 * reach: the left side's h < reach at index base - reach + h, the right side's at base + SPAN + h - reach
                const int32_t h = (int32_t)threadIdx.x + k * TRACK_THREADS;
                const bool left = h < reach;
                int64_t g = left ? base - reach + h : base + SPAN + (h - reach);
                g = g < 0 ? 0 : g;
                hl[k] = h < 2 * reach ? (left ? h : SPAN + h) : -1;
                hv[k] = Cin[axis_at(g, n_shift)];
            }
        }
#pragma unroll
        for (int p = 0; p < PER; ++p) dd[p] = Drow[at[p]];
#pragma unroll
        for (int p = 0; p < PER; ++p) r[p] = row[at[p]];
        // (nothing is scheduled across this line: the loads above are all in flight before the first is waited for)
        __builtin_amdgcn_sched_barrier(0);
        if (HALO > 0) {
            __syncthreads();                // the readers of the item before this one are through
#pragma unroll
            for (int p = 0; p < PER; ++p) tile[reach + (int32_t)threadIdx.x + p * TRACK_THREADS] = c[p];
#pragma unroll
            for (int k = 0; k < HALO; ++k)
                if (hl[k] >= 0) tile[hl[k]] = hv[k];
            __syncthreads();
        }
        // nearB[j]: the thread's own value is cand(0); the others come from the tile in the order -1, +1, -2, +2, ..., in which
        // track_replaces is the strict comparison (the value only: no move word).  room: how far index j may move down / up inside
        // the axis and the reach
        double near[PER];
        int32_t room_lo[PER], room_hi[PER];
#pragma unroll
        for (int p = 0; p < PER; ++p) {
            const int64_t j = j0 + p * TRACK_THREADS, up = (int64_t)n_shift - 1 - j;
            near[p] = c[p];
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
                    // (selects: a candidate outside the axis was loaded from an element inside it, and is left out here)
                    const bool take_lo = (int)(s <= room_lo[p]) & (int)track_replaces_in_order(lo, near[p]);
                    near[p] = take_lo ? lo : near[p];
                    const bool take_hi = (int)(s <= room_hi[p]) & (int)track_replaces_in_order(hi, near[p]);
                    near[p] = take_hi ? hi : near[p];
                }
            }
        }
#pragma unroll
        for (int p = 0; p < PER; ++p) {
            const int64_t j = j0 + p * TRACK_THREADS;
            const bool valid = j < n_shift;
            const double u = path_cost(METHOD, a.weight, r[p]);
            const double b = margin_back(near[p], jump);
            const double m = margin_through(dd[p], b, last);
            const double cn = margin_suffix(u, b, last);
            const bool take_c = (int)valid & (int)path_min_replaces(cn, (int32_t)j, best_c.v, best_c.i);
            best_c.v = take_c ? cn : best_c.v; best_c.i = take_c ? (int32_t)j : best_c.i;
            const bool take_m = (int)valid & (int)path_min_replaces(m, (int32_t)j, best_m.v, best_m.i);
            best_m.v = take_m ? m : best_m.v; best_m.i = take_m ? (int32_t)j : best_m.i;
            const bool take_a = (int)valid & (int)margin_outside(j, s_e, guard) & (int)path_min_replaces(m, (int32_t)j, best_a.v, best_a.i);
            best_a.v = take_a ? m : best_a.v; best_a.i = take_a ? (int32_t)j : best_a.i;
            if (valid) {
                Cout[j] = cn;
                if (Mrow) Mrow[j] = m;
                if (j == s_e) a.through[a.e] = m;
            }
        }
    }
    best_c = block_first_min(best_c, lds);
    best_m = block_first_min(best_m, lds);
    best_a = block_first_min(best_a, lds);
    if (threadIdx.x == 0) {
        a.out.c_min[blockIdx.x] = best_c.v; a.out.c_arg[blockIdx.x] = best_c.i;
        a.out.m_min[blockIdx.x] = best_m.v; a.out.m_arg[blockIdx.x] = best_m.i;
        a.out.a_min[blockIdx.x] = best_a.v; a.out.a_arg[blockIdx.x] = best_a.i;
    }
}

// closes a call's last launch (row row0): one workgroup turns its partial records into the row's outputs
__global__ __launch_bounds__(TRACK_THREADS)
void margin_close_kernel(MarginArgs a) {
    __shared__ PathLds lds;
    reduce_margin_partials(a, true, a.e, lds);
}

template <int PER, bool MAX>
void launch_margin_step(int halo, dim3 grid, size_t tile_bytes, hipStream_t st, const MarginArgs& a) {
    const dim3 block(TRACK_THREADS);
    if (halo == 0) hipLaunchKernelGGL((margin_step_kernel<PER, MAX, 0>), grid, block, 0, st, a);
    else if (halo == TRACK_HALO_SMALL) hipLaunchKernelGGL((margin_step_kernel<PER, MAX, TRACK_HALO_SMALL>), grid, block, tile_bytes, st, a);
    else hipLaunchKernelGGL((margin_step_kernel<PER, MAX, TRACK_HALO_LARGE>), grid, block, tile_bytes, st, a);
}
