// sushi_amd/csrc/sushi_track_order_margins_step.inc -- the ordered margins' step, scan and apply kernels and the step's launcher,
// included once, inside the anonymous namespace of sushi_track_order.hip, which describes them; a wide call sends its rows of a
// reach up to TRACK_MAX_REACH through them, and every row through the scan and the apply.
struct OrderMarginArgs {
    const float* row;                       // R_e: curves + curve_off
    double weight, penalty, step_cost;      // penalty: row e + 1's
    const double* C_in;                     // [n_shift] C_{e+1}: half (e + 1) & 1
    double* C_out;                          // [n_shift] C_e: half e & 1
    const double* D_row;                    // [n_shift] D_e
    double* M_row;                          // [n_shift] M_e, or null
    double* S;                              // [n_shift]: S_{e+1} for the step, S_e after the apply
    const int32_t* shift;                   // [n_total] s_e
    int32_t n_shift;
    int32_t reach;                          // reach_{e+1} (0 for the sequence's last row)
    int32_t back;                           // back_{e+1}
    int32_t guard;                          // guard_e
    int64_t n_items;
    int e;                                  // the row of the sequence
    int last;                               // the sequence's last row: there is no B
    int n_partials;                         // records of `in`
    MarginPartials in;                      // the step's, one per workgroup
    double* item_min; int32_t* item_arg;    // [n_items] the step's, one per work item
    double* after_min;                      // [n_items] the scan's: the minimum of C_e over the items after this one
    double* through; double* best; int32_t* best_arg; double* alt; int32_t* alt_arg; double* c_min;    // the whole sequence's
};

// HALO: the rounds of 256 halo values a launch loads (track_halo_rounds(reach): 0 at reach 0, where nothing is staged)
template <int PER, bool MAX, int HALO>
__global__ __launch_bounds__(TRACK_THREADS)
void order_margin_step_kernel(OrderMarginArgs a) {
    constexpr int METHOD = MAX ? SUSHI_HIP_METHOD_CCOEFF_NORMED : SUSHI_HIP_METHOD_SQDIFF_NORMED;
    constexpr int SPAN = PER * TRACK_THREADS;
    __shared__ PathLds lds;
    extern __shared__ double tile[];        // [reach + SPAN + reach]: entry l is C_{e+1}[item's first index - reach + l]
    const float* __restrict__ row = a.row;
    const double* __restrict__ Cin = a.C_in;
    const double* __restrict__ Drow = a.D_row;
    const double* __restrict__ Sin = a.S;
    double* __restrict__ Cout = a.C_out;
    double* __restrict__ Mrow = a.M_row;
    const int32_t n_shift = a.n_shift;
    const int32_t reach = HALO == 0 ? 0 : a.reach;
    const bool last = a.last != 0;
    const int32_t s_e = path_clamp(a.shift[a.e], n_shift);
    const int32_t guard = a.guard;

    MinD best_c = {INFINITY, PATH_NO_INDEX}, best_m = {INFINITY, PATH_NO_INDEX}, best_a = {INFINITY, PATH_NO_INDEX};
    for (int64_t item = blockIdx.x; item < a.n_items; item += gridDim.x) {
        // (an item's first index is below n_shift < 2^31; the indices behind it may pass 2^31 only where they are not used: 64 bits)
        const int64_t base = item * SPAN;
        const int64_t j0 = base + threadIdx.x;
        // every load is always made, the indices outside the axis moved onto an element inside it (axis_at; t'_e(j) lies inside the
        // axis for every j inside it): the tile, the halo, S, D_e and the row are all asked for before the first value is used
        int32_t at[PER];
        float r[PER];
        double c[PER], dd[PER], st[PER];
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
        // S_{e+1} at t'_e(j): consecutive lanes read consecutive doubles, the back further down, the first ones all the row's first
#pragma unroll
        for (int p = 0; p < PER; ++p) st[p] = Sin[order_margin_from(at[p], a.back)];
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
        // nearB[j], as in sushi_track_margins.hip: the thread's own value is cand(0); the others come from the tile in the order -1,
        // +1, -2, +2, ..., in which track_replaces is the strict comparison (the value only: no move word)
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
        MinD mine = {INFINITY, PATH_NO_INDEX};
#pragma unroll
        for (int p = 0; p < PER; ++p) {
            const int64_t j = j0 + p * TRACK_THREADS;
            const bool valid = j < n_shift;
            const double u = path_cost(METHOD, a.weight, r[p]);
            const double b = margin_back(near[p], order_margin_jump(st[p], a.penalty));
            const double m = margin_through(dd[p], b, last);
            const double cn = margin_suffix(u, b, last);
            const bool take_c = (int)valid & (int)path_min_replaces(cn, (int32_t)j, mine.v, mine.i);
            mine.v = take_c ? cn : mine.v; mine.i = take_c ? (int32_t)j : mine.i;
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
        // the item's record of C_e (valid in every thread), and the workgroup's over its items
        mine = block_first_min(mine, lds);
        if (threadIdx.x == 0) { a.item_min[item] = mine.v; a.item_arg[item] = mine.i; }
        const bool take = path_min_replaces(mine.v, mine.i, best_c.v, best_c.i);
        best_c.v = take ? mine.v : best_c.v; best_c.i = take ? mine.i : best_c.i;
    }
    best_m = block_first_min(best_m, lds);
    best_a = block_first_min(best_a, lds);
    if (threadIdx.x == 0) {
        a.in.c_min[blockIdx.x] = best_c.v; a.in.c_arg[blockIdx.x] = best_c.i;
        a.in.m_min[blockIdx.x] = best_m.v; a.in.m_arg[blockIdx.x] = best_m.i;
        a.in.a_min[blockIdx.x] = best_a.v; a.in.a_arg[blockIdx.x] = best_a.i;
    }
}

struct ItemScanLds { double v[4]; int32_t i[4]; };

// one workgroup: what lies after every work item of row e, and the row's outputs.  The items are taken 256 at a time from the last
// one down, thread t the t-th from the top of its round, so that `carry` is what lies after the round.
__global__ __launch_bounds__(TRACK_THREADS)
void order_margin_scan_kernel(OrderMarginArgs a) {
    __shared__ PathLds lds;
    __shared__ ItemScanLds scan;
    const int lane = (int)threadIdx.x & 63, w = (int)threadIdx.x >> 6;
    OrderMin carry = order_none();
    for (int64_t k0 = 0; k0 < a.n_items; k0 += TRACK_THREADS) {
        const int64_t k = a.n_items - 1 - k0 - threadIdx.x;
        const bool valid = k >= 0;
        const int64_t at = valid ? k : 0;
        const double v = a.item_min[at];
        const int32_t i = a.item_arg[at];
        // the inclusive scan of a wave's 64 records in lane order: lane l's covers the items of the lanes 0 .. l, those above item k
        OrderMin x = valid ? OrderMin{v, i} : order_none();
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const OrderMin o = OrderMin{__shfl_up(x.v, d, 64), __shfl_up(x.i, d, 64)};
            const OrderMin c = order_combine(x, o);
            x = lane >= d ? c : x;
        }
        __syncthreads();                    // the readers of the round before this one are through
        if (lane == 63) { scan.v[w] = x.v; scan.i[w] = x.i; }
        __syncthreads();
        OrderMin pref = carry;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const OrderMin c = order_combine(OrderMin{scan.v[q], scan.i[q]}, carry);
            pref = q < w ? c : pref;
            carry = c;
        }
        // what lies after item k: the waves before this one (and the rounds before this one), and the lanes below this one
        const OrderMin upto = OrderMin{__shfl_up(x.v, 1, 64), __shfl_up(x.i, 1, 64)};
        const OrderMin after = lane == 0 ? pref : order_combine(upto, pref);
        if (valid) a.after_min[k] = after.v;
    }
    reduce_margin_partials(a, true, a.e, lds);
}

// the inclusive suffix scan of a wave's 64 values in lane order: lane l's covers the lanes l .. 63
__device__ __forceinline__ double wave_suffix_min(double x) {
    const int lane = (int)threadIdx.x & 63;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const double o = __shfl_down(x, d, 64);
        const double c = order_suffix_combine(x, o);
        x = lane + d < 64 ? c : x;
    }
    return x;
}

// S_e of one work item's indices: its values of C_e scanned downwards onto what lies after the item
template <int PER>
__global__ __launch_bounds__(TRACK_THREADS)
void order_margin_apply_kernel(OrderMarginArgs a) {
    constexpr int SPAN = PER * TRACK_THREADS;
    __shared__ double total[2][PER * 4];    // [turn][round p, wave w]: the minimum of that wave's 64 values, in index order
    const double* __restrict__ C = a.C_out;
    double* __restrict__ S = a.S;
    const int32_t n_shift = a.n_shift;
    const int lane = (int)threadIdx.x & 63, w = (int)threadIdx.x >> 6;
    int turn = 0;
    for (int64_t item = blockIdx.x; item < a.n_items; item += gridDim.x, turn ^= 1) {
        const int64_t j0 = item * SPAN + threadIdx.x;
        double x[PER];
#pragma unroll
        for (int p = 0; p < PER; ++p) {
            const int64_t j = j0 + p * TRACK_THREADS;
            const double v = C[axis_at(j, n_shift)];
            x[p] = j < n_shift ? v : INFINITY;
        }
        const double after = a.after_min[item];
#pragma unroll
        for (int p = 0; p < PER; ++p) x[p] = wave_suffix_min(x[p]);
        if (lane == 0) {
#pragma unroll
            for (int p = 0; p < PER; ++p) total[turn][p * 4 + w] = x[p];
        }
        // (one barrier an item: the totals of the item before this one lie in the other half, and its readers are through before any
        // thread passes this item's barrier and comes to write that half again)
        __syncthreads();
        // behind[q]: the minimum of everything after span q = (round, wave) -- the spans q + 1 .. and what lies after the item
        double behind = after;
#pragma unroll
        for (int q = PER * 4 - 1; q >= 0; --q) {
            const double t = total[turn][q];
            if ((q & 3) == w) {             // (wave-uniform)
                const int p = q >> 2;
                const int64_t j = j0 + p * TRACK_THREADS;
                if (j < n_shift) S[j] = order_suffix_combine(x[p], behind);
            }
            behind = order_suffix_combine(t, behind);
        }
    }
}

template <int PER, bool MAX>
void launch_order_margin_step(int halo, dim3 grid, size_t tile_bytes, hipStream_t st, const OrderMarginArgs& a) {
    const dim3 block(TRACK_THREADS);
    if (halo == 0) hipLaunchKernelGGL((order_margin_step_kernel<PER, MAX, 0>), grid, block, 0, st, a);
    else if (halo == TRACK_HALO_SMALL) hipLaunchKernelGGL((order_margin_step_kernel<PER, MAX, TRACK_HALO_SMALL>), grid, block, tile_bytes, st, a);
    else hipLaunchKernelGGL((order_margin_step_kernel<PER, MAX, TRACK_HALO_LARGE>), grid, block, tile_bytes, st, a);
}
