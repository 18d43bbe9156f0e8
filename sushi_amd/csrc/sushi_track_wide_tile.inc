// sushi_amd/csrc/sushi_track_wide_tile.inc -- the wide pass's tile kernel and its launcher, and how a work item of a wide step
// stages its whole tiles' records in LDS; included inside the anonymous namespace of sushi_track.hip and of sushi_track_order.hip:
// one text, the same code in both units.

// ---- the tile pass ----
__device__ __forceinline__ WideRec wide_shfl_up(const WideRec& r, int off) {
    return WideRec{__shfl_up(r.v, off, 64), __shfl_up(r.first, off, 64), __shfl_up(r.last, off, 64)};
}
__device__ __forceinline__ WideRec wide_shfl_down(const WideRec& r, int off) {
    return WideRec{__shfl_down(r.v, off, 64), __shfl_down(r.first, off, 64), __shfl_down(r.last, off, 64)};
}

__global__ __launch_bounds__(TRACK_THREADS)
void wide_tile_kernel(const double* __restrict__ X, int32_t n_shift, int64_t n_tiles, WideRecords w) {
    __shared__ WideRec totals[TRACK_THREADS / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int32_t k0 = (int32_t)threadIdx.x * WIDE_PER;
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int64_t base = (tile << WIDE_TILE_BITS) + k0;
        // every load is always made (axis_at); an element past the axis's end is an empty run
        WideRec pl[WIDE_PER], sl[WIDE_PER];
#pragma unroll
        for (int k = 0; k < WIDE_PER; ++k) {
            const double x = X[axis_at(base + k, n_shift)];
            pl[k] = base + k < n_shift ? wide_one(x, k0 + k) : wide_empty();
            sl[k] = pl[k];
        }
        // the thread's four values: prefix records upwards, suffix records downwards
#pragma unroll
        for (int k = 1; k < WIDE_PER; ++k) pl[k] = wide_combine(pl[k - 1], pl[k]);
#pragma unroll
        for (int k = WIDE_PER - 2; k >= 0; --k) sl[k] = wide_combine(sl[k], sl[k + 1]);
        // the wave: inclusive scans of the threads' totals, upwards and downwards (every lane takes part in every shuffle)
        WideRec up = pl[WIDE_PER - 1], down = sl[0];
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const WideRec o = wide_shfl_up(up, off);
            if (lane >= off) up = wide_combine(o, up);
        }
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const WideRec o = wide_shfl_down(down, off);
            if (lane + off < 64) down = wide_combine(down, o);
        }
        __syncthreads();                    // the readers of the tile before this one are through
        if (lane == 63) totals[wave] = up;  // the wave's whole record
        __syncthreads();
        WideRec before = wide_empty(), after = wide_empty();
#pragma unroll
        for (int q = 0; q < TRACK_THREADS / 64; ++q)
            if (q < wave) before = wide_combine(before, totals[q]);
#pragma unroll
        for (int q = TRACK_THREADS / 64 - 1; q >= 0; --q)
            if (q > wave) after = wide_combine(totals[q], after);
        // what lies in front of / behind the thread's values: the other waves' totals and the wave's lanes below / above it
        WideRec ex_up = wide_shfl_up(up, 1), ex_down = wide_shfl_down(down, 1);
        if (lane == 0) ex_up = wide_empty();
        if (lane == 63) ex_down = wide_empty();
        const WideRec carry_up = wide_combine(before, ex_up), carry_down = wide_combine(ex_down, after);
#pragma unroll
        for (int k = 0; k < WIDE_PER; ++k) {
            if (base + k < n_shift) {
                const WideRec p = wide_combine(carry_up, pl[k]), s = wide_combine(sl[k], carry_down);
                w.pv[base + k] = p.v; w.pi[base + k] = wide_pack(p);
                w.sv[base + k] = s.v; w.si[base + k] = wide_pack(s);
            }
        }
    }
}

// ---- what a step stages ----
// the whole tiles' records a work item staged: tile t's is entry t - first
struct WideItemTiles { double v[WIDE_ITEM_TILES]; uint32_t idx[WIDE_ITEM_TILES]; };
struct StagedTiles {
    const WideItemTiles* s;
    int64_t first;
    __device__ __forceinline__ WideTileRec operator()(int64_t t) const { return WideTileRec{s->v[t - first], s->idx[t - first]}; }
};

// Every thread of the workgroup: stages the records of the tiles the item's windows may hold whole.  Two barriers, the first of
// which lets the readers of the item before through.
__device__ __forceinline__ StagedTiles stage_item_tiles(const WideRecords& w, int64_t base, int64_t span, int32_t reach, int32_t n_shift,
                                                        WideItemTiles& s) {
    const int64_t t_lo = wide_item_first_tile(base, reach), t_hi = wide_item_last_tile(base, span, reach, n_shift);
    __syncthreads();
    if ((int64_t)threadIdx.x <= t_hi - t_lo && threadIdx.x < WIDE_ITEM_TILES) {
        const int64_t end = wide_tile_end(t_lo + threadIdx.x, n_shift);
        s.v[threadIdx.x] = w.pv[end]; s.idx[threadIdx.x] = w.pi[end];
    }
    __syncthreads();
    return StagedTiles{&s, t_lo};
}

void launch_wide_tiles(const double* X, int32_t n_shift, unsigned tile_grid, const WideRecords& w, hipStream_t st) {
    hipLaunchKernelGGL(wide_tile_kernel, dim3(tile_grid), dim3(TRACK_THREADS), 0, st, X, n_shift, wide_tiles(n_shift), w);
}
