// sushi_amd/csrc/sushi_track_step.inc -- the tracking pass's step and close kernels and their launcher: a part of sushi_track.hip,
// which describes them; a wide call sends its rows of a reach up to TRACK_MAX_REACH through the same code.  Included once, inside
// the unit's anonymous namespace, after sushi_internal.hpp, track_core.hpp and path_device.hpp and a `using
// namespace sushi`.
struct TrackArgs {
    const float* row;                       // R_e: curves + curve_off
    double weight, penalty, step_cost;
    const double* D_in;                     // [n_shift] D_{e-1}: half (e - 1) & 1
    double* D_out;                          // [n_shift] D_e: half e & 1
    int16_t* move;                          // [n_shift] row e's moves
    int32_t n_shift;
    int32_t reach;                          // reach_e (0 for e = 0)
    int64_t n_items;
    int e;                                  // the row of the sequence
    int prev;                               // where m_{e-1} comes from (path_device.hpp PREV_*)
    int n_partials;                         // records of `in`
    PathPartials in, out;
    double* row_min; int32_t* row_arg; int32_t* row_own_index; float* row_own_score;    // the whole sequence's
};

// HALO: the rounds of 256 halo values a launch loads (track_halo_rounds(reach): 0 at reach 0, where nothing is staged)
template <int PER, bool MAX, int HALO>
__global__ __launch_bounds__(TRACK_THREADS)
void track_step_kernel(TrackArgs a) {
    constexpr int METHOD = MAX ? SUSHI_HIP_METHOD_CCOEFF_NORMED : SUSHI_HIP_METHOD_SQDIFF_NORMED;
    constexpr int SPAN = PER * TRACK_THREADS;
    __shared__ PathLds lds;
    extern __shared__ double tile[];        // [reach + SPAN + reach]: entry l is D_{e-1}[item's first index - reach + l]
    const float* __restrict__ row = a.row;
    const double* __restrict__ Din = a.D_in;
    double* __restrict__ Dout = a.D_out;
    int16_t* __restrict__ move = a.move;
    const int32_t n_shift = a.n_shift;
    const int32_t reach = HALO == 0 ? 0 : a.reach;
    const bool first = a.prev == PREV_NONE;
    double jump = 0.0;
    if (a.prev == PREV_PARTIALS) jump = reduce_partials<METHOD>(a.in, a.n_partials, blockIdx.x == 0, a.e - 1, a, lds) + a.penalty;
    else if (a.prev == PREV_ROW_MIN) jump = a.row_min[a.e - 1] + a.penalty;

    MinD best = {INFINITY, PATH_NO_INDEX};
    OwnF own = {own_worst<METHOD>(), PATH_NO_INDEX};
    for (int64_t item = blockIdx.x; item < a.n_items; item += gridDim.x) {
        // (an item's first index is below n_shift < 2^31; the indices behind it may pass 2^31 only where they are not used: 64 bits)
        const int64_t base = item * SPAN;
        const int64_t j0 = base + threadIdx.x;
        // every load is always made, the indices outside the axis moved onto an element inside it (axis_at): the tile, the halo and
        // the row are all asked for before the first value is used
        int32_t at[PER];
        float r[PER];
        double d[PER];
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
        // near_e[j]: the thread's own value is cand(0); the others come from the tile in the order -1, +1, -2, +2, ..., in which
        // track_replaces is the strict comparison.  room: how far index j may move down / up inside the axis and the reach
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
                    // (selects: a candidate outside the axis was loaded from an element inside it, and is left out here)
                    const bool take_lo = (int)(s <= room_lo[p]) & (int)track_replaces_in_order(lo, near[p]);
                    near[p] = take_lo ? lo : near[p]; nd[p] = take_lo ? -s : nd[p];
                    const bool take_hi = (int)(s <= room_hi[p]) & (int)track_replaces_in_order(hi, near[p]);
                    near[p] = take_hi ? hi : near[p]; nd[p] = take_hi ? s : nd[p];
                }
            }
        }
#pragma unroll
        for (int p = 0; p < PER; ++p) {
            const int64_t j = j0 + p * TRACK_THREADS;
            const bool valid = j < n_shift;
            const double u = path_cost(METHOD, a.weight, r[p]);
            int16_t mv = 0;
            const double stepped = track_step(near[p], nd[p], u, jump, &mv);
            const double dn = first ? u : stepped;
            mv = first ? (int16_t)0 : mv;
            const bool take = (int)valid & (int)path_min_replaces(dn, (int32_t)j, best.v, best.i);
            best.v = take ? dn : best.v; best.i = take ? (int32_t)j : best.i;
            const bool take_own = (int)valid & (int)path_own_replaces(METHOD, r[p], (int32_t)j, own.v, own.i);
            own.v = take_own ? r[p] : own.v; own.i = take_own ? (int32_t)j : own.i;
            if (valid) {
                Dout[j] = dn;
                move[j] = mv;
            }
        }
    }
    best = block_first_min(best, lds);
    own = block_first_own<METHOD>(own, lds);
    if (threadIdx.x == 0) {
        a.out.d_min[blockIdx.x] = best.v; a.out.d_arg[blockIdx.x] = best.i;
        a.out.own_idx[blockIdx.x] = own.i; a.out.own_val[blockIdx.x] = own.v;
    }
}

// closes a call's last row: one workgroup turns its partial records into the row's outputs
template <bool MAX>
__global__ __launch_bounds__(TRACK_THREADS)
void track_close_kernel(TrackArgs a) {
    constexpr int METHOD = MAX ? SUSHI_HIP_METHOD_CCOEFF_NORMED : SUSHI_HIP_METHOD_SQDIFF_NORMED;
    __shared__ PathLds lds;
    reduce_partials<METHOD>(a.in, a.n_partials, true, a.e, a, lds);
}

template <int PER, bool MAX>
void launch_step(int halo, dim3 grid, size_t tile_bytes, hipStream_t st, const TrackArgs& a) {
    const dim3 block(TRACK_THREADS);
    if (halo == 0) hipLaunchKernelGGL((track_step_kernel<PER, MAX, 0>), grid, block, 0, st, a);
    else if (halo == TRACK_HALO_SMALL) hipLaunchKernelGGL((track_step_kernel<PER, MAX, TRACK_HALO_SMALL>), grid, block, tile_bytes, st, a);
    else hipLaunchKernelGGL((track_step_kernel<PER, MAX, TRACK_HALO_LARGE>), grid, block, tile_bytes, st, a);
}
