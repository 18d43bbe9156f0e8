// sushi_amd/csrc/sushi_track_order_step.inc -- the ordered tracking pass's step, scan and apply kernels and the step's launcher,
// included once, inside the anonymous namespace of sushi_track_order.hip, which describes them; a wide call sends its rows of a
// reach up to TRACK_MAX_REACH through them, and every row through the scan and the apply.
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

template <int PER, bool MAX>
void launch_step(int halo, dim3 grid, size_t tile_bytes, hipStream_t st, const OrderArgs& a) {
    const dim3 block(TRACK_THREADS);
    if (halo == 0) hipLaunchKernelGGL((order_step_kernel<PER, MAX, 0>), grid, block, 0, st, a);
    else if (halo == TRACK_HALO_SMALL) hipLaunchKernelGGL((order_step_kernel<PER, MAX, TRACK_HALO_SMALL>), grid, block, tile_bytes, st, a);
    else hipLaunchKernelGGL((order_step_kernel<PER, MAX, TRACK_HALO_LARGE>), grid, block, tile_bytes, st, a);
}
