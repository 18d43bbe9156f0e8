// sushi_amd/csrc/sushi_fft_mac.inc -- part of sushi_fft.hip (included there, inside its anonymous namespace; not a header of its own):
// the frequency-domain multiply-accumulate: mac_kernel / mac_long_kernel over all pairs, mac_list_kernel for listed pairs.

// ------------------------------------------------------------------------------------------
// Frequency-domain multiply-accumulate.  A wave = MAC_SPW searches of one segment-count class, neighbours in the stream (window starts),
// x MAC_BPW entries of four adjacent bins: lane = (search slot, entry).  All searches sit on the same absolute block grid,
// so the lanes of a wave walk the union of their block ranges together (mac_core.hpp): the row piece Z_j(32 bins) is one
// 128-byte line that the eight search slots read at the same address -- one L2 request serves eight searches x 32 bins --
// and every output Y_I(32 bins) of a search is a full 128-byte line written by eight neighbouring lanes.  Pattern spectra
// live in registers (per lane: its own search's, one 32-bit word per bin), a ring of SMAX / FFT_STEP float32 outputs is
// live per lane.  No barriers.
// What bounds the kernel is the bytes a CU's L1 passes (~10 B per clock): with every operand a packed half a byte through
// the L1 feeds twice the multiply-adds it fed as float32, and they are two to an instruction.
// ------------------------------------------------------------------------------------------
struct MacArgs {
    const uint4* spec;                // destination spectra, as 4-bin entries of packed halves
    int64_t spec_blocks;              // blocks of the stream; block `spec_blocks` is all zero
    const uint4* tspec;
    int tspec_half;                   // whole rows only: `tspec` holds half rows (TspecLane)
    uint4* y;                         // [pairs of the sub-batch][ROWE]
    const SearchDesc* searches;       // the sub-batch's searches
    const TemplConsts* tconst;        // [searches of the sub-batch]: mac_scale
    const int* items;                 // [n_items][1 + MAC_SPW]: segment-count class, then search indices inside the sub-batch (-1 = none)
    int n_items;
    int sub_first_seg;
    int sub_first_pair;
    int chunk_group;                  // bin chunks an XCD works on at a time (a power of two dividing its share)
    uint4* dummy;                     // [MAC_DUMMY_LINES][MAC_THREADS] where the stores of lanes without a valid output go
    const int* enable;                // NULL, or a device flag: 0 = this launch is not needed (every workgroup leaves at once)
};

// Where a lane finds entry `e` of a pattern's whole rows, segment after segment.  Whole rows as they are; of HALF rows (the real
// route's format, fft_core.hpp "HALF ROWS") the one function every reader goes through: the place in the half row and whether
// the words there are the entry's conj-reversal.  Every entry comes back with the words a whole row holds.
struct TspecLane { const uint4* __restrict__ p; size_t stride; bool conjrev; };
__device__ __forceinline__ TspecLane tspec_lane(const uint4* __restrict__ tspec, const int half_rows, const size_t first_seg, const int e) {
    if (!half_rows) return TspecLane{tspec + first_seg * ROWE + e, (size_t)ROWE, false};
    const sushi_fft::HalfSource s = sushi_fft::half_source(e);
    return TspecLane{tspec + first_seg * HROWE + s.index, (size_t)HROWE, s.conjrev};
}
__device__ __forceinline__ uint4 tspec_entry(const TspecLane& t, const size_t s) {
    const uint4 v = t.p[s * t.stride];
    return t.conjrev ? sushi_fft::real_conjrev(v) : v;
}

constexpr int MAC_ZR = 6;                        // rows per load instruction: divides every SMAX

__device__ __forceinline__ int wave_min_i32(int v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) { const int o = __shfl_xor(v, d, 64); v = o < v ? o : v; }
    return v;
}
__device__ __forceinline__ int wave_max_i32(int v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) { const int o = __shfl_xor(v, d, 64); v = o > v ? o : v; }
    return v;
}

constexpr int MAC_SMAX_SHORT = mac_class_smax(MAC_SHORT_CLASSES - 1);   // 18: mac_kernel
constexpr int MAC_SMAX_LONG = mac_class_smax(MAC_CLASSES - 1);           // 30: mac_long_kernel
constexpr int MAC_CH = MAC_ZR;                   // rows one load instruction brings (lane = row x entry)
static_assert(MAC_CH <= MAC_SPW, "a load's rows are spread over the search slots");
constexpr int MAC_AHEAD_ROWS = 36;               // rows in flight per wave (mac_kernel: a multiple of each of its SMAX; mac_long_kernel: one group): 4.5 KB

__device__ __forceinline__ sushi_mac::h8 as_h8(const uint4 v) { return sushi_mac::h8{{v.x, v.y, v.z, v.w}}; }
__device__ __forceinline__ uint4 as_uint4(const sushi_mac::h8 v) { return uint4{v.w[0], v.w[1], v.w[2], v.w[3]}; }

// The walk of one wave (MAC_SPW searches x MAC_BPW entries) for its segment-count class.  Rows reach the lanes in
// two hops: a load instruction fetches MAC_CH consecutive rows at once (lane = (row, entry): 128 distinct bytes per
// row), LA = MAC_AHEAD_ROWS / SMAX groups ahead of their use into a register ring; one group ahead they are dropped
// into the wave's private LDS buffer -- the piece itself and its rotation by -i, which the imaginary parts' dot products
// take (mac_core.hpp): made once here instead of once per search slot -- from where every search slot reads the same row
// (a broadcast read).  The wave's own LDS operations are ordered, so none of this needs a barrier.
// Every memory operation of the loop body is unconditional -- lanes without a row to fetch re-fetch a neighbour's,
// lanes without a valid output store to a dummy line: the compiler then knows how many operations are in flight at every
// point and waits for exactly the load it needs (a conditional one makes it drain everything, every group).
template <int SMAX, bool ACCUM, int ZROWS, int RE>
__device__ __forceinline__ void mac_chunk(const MacArgs& a, const int c0, const int wv_first, const int wv_last,
                                          const long long pair_lo, const long long pair_hi, const bool lane_chunk,
                                          const sushi_mac::h8 (&tt)[SMAX], const uint4* __restrict__ zsp, const int z_zero,
                                          uint4* __restrict__ yout, uint4* __restrict__ dummy, const float sy, const int slot,
                                          const int fb, uint4 (*zw)[ZROWS + 1][2][MAC_BPW]) {
    using sushi_mac::acc4;
    using sushi_mac::zrow;
    constexpr int STEP = FFT_STEP;
    constexpr int AHEAD = SMAX < MAC_SMAX_SHORT ? MAC_AHEAD_ROWS : SMAX;    // rows in flight (the largest class of each kernel: what its registers allow)
    constexpr int NC = SMAX / MAC_CH;                           // load instructions per group
    constexpr int LA = AHEAD / SMAX;                            // groups between a load and its use
    constexpr int NQ = LA * NC;                                 // register ring, in loads
    constexpr int UNROLL = (LA % 2) ? 2 * LA : LA;              // ring slot and LDS buffer of a group are compile-time
    static_assert(SMAX % MAC_CH == 0 && AHEAD % SMAX == 0 && SMAX <= ZROWS, "ring geometry");
    const int lrow = slot % MAC_CH;                              // the row of a load this lane fetches
    const bool loader = slot < MAC_CH;                           // ... and whether its copy is the one that goes to LDS
    // rows jrow + lrow of one load; blocks past the stream are the all-zero block
    auto load_rows = [&](const int jrow) {
        const int jj = jrow + lrow;
        return zsp[(size_t)(jj < z_zero ? jj : z_zero) * RE];
    };
    // a loaded piece into an LDS buffer: the row as it is and rotated
    auto drop = [&](const int buf, const int c, const uint4 piece) {
        const int row = loader ? MAC_CH * c + slot : ZROWS;
        zw[buf][row][0][fb] = piece;
        zw[buf][row][1][fb] = as_uint4(sushi_mac::rot_mi(as_h8(piece)));
    };
    acc4 acc[SMAX / STEP];
#pragma unroll
    for (int r = 0; r < SMAX / STEP; ++r) acc[r] = sushi_mac::zero_acc();
    uint4 rq[NQ];
    // prologue: group 0 straight into LDS buffer 0, groups 1 .. LA into the register ring
    {
        uint4 first[NC];
#pragma unroll
        for (int c = 0; c < NC; ++c) first[c] = load_rows(wv_first + c0 + MAC_CH * c);
#pragma unroll
        for (int g = 1; g <= LA; ++g) {
#pragma unroll
            for (int c = 0; c < NC; ++c) rq[(g % LA) * NC + c] = load_rows(wv_first + c0 + SMAX * g + MAC_CH * c);
        }
#pragma unroll
        for (int c = 0; c < NC; ++c) drop(0, c, first[c]);
    }
    for (int jb = wv_first; jb <= wv_last; jb += SMAX * UNROLL) {
#pragma unroll
        for (int t = 0; t < UNROLL; ++t) {
            const int jg = jb + SMAX * t;                      // group t of this round (groups past wv_last: dummy work)
            // the next group leaves the register ring for the other LDS buffer (this wave read that buffer one group
            // ago: its LDS operations are in order) ...
#pragma unroll
            for (int c = 0; c < NC; ++c) drop((t + 1) & 1, c, rq[((t + 1) % LA) * NC + c]);
            // ... and its ring slots take the loads of the group LA further on
#pragma unroll
            for (int c = 0; c < NC; ++c) rq[((t + 1) % LA) * NC + c] = load_rows(jg + c0 + SMAX * (1 + LA) + MAC_CH * c);
            auto get_z = [&](const int u) { return zrow{as_h8(zw[t & 1][u][0][fb]), as_h8(zw[t & 1][u][1][fb])}; };
            auto store = [&](const int i, const bool valid, const acc4& v) {
                typedef unsigned u4 __attribute__((ext_vector_type(4)));
                typedef _Float16 h2 __attribute__((ext_vector_type(2)));
                // (a lane-predicated store instead of the dummy line was tried: the compiler branches around it and
                // falls back to draining the load queue, tools/experiments/README.md)
                const bool ok = valid && lane_chunk && jg <= wv_last;
                u4* __restrict__ dst = reinterpret_cast<u4*>(ok ? yout + (size_t)i * RE : dummy);
                float re[sushi_mac::BINS], im[sushi_mac::BINS];
#pragma unroll
                for (int k = 0; k < sushi_mac::BINS; ++k) { re[k] = v.re[k] * sy; im[k] = v.im[k] * sy; }   // to the scale of Y
                if (ACCUM) {                                    // patterns beyond one pass: the row accumulates (in halves)
                    // (the entry as EIGHT halves, not `bit_cast<half2>(prev[k])`: hipcc 7.2 reads the first word four times -- add_abs2_entry)
                    typedef _Float16 h8 __attribute__((ext_vector_type(8)));
                    static_assert(sushi_mac::BINS == 4, "an entry is four bins");
                    const h8 pv = __builtin_bit_cast(h8, *dst);
#pragma unroll
                    for (int k = 0; k < sushi_mac::BINS; ++k) { re[k] += (float)pv[2 * k]; im[k] += (float)pv[2 * k + 1]; }
                }
                u4 o;
#pragma unroll
                for (int k = 0; k < sushi_mac::BINS; ++k) {
                    const h2 q = {(_Float16)re[k], (_Float16)im[k]};                 // v_cvt_pk_f16_f32: round to nearest even
                    o[k] = __builtin_bit_cast(unsigned, q);
                }
                // Y is streamed once and read back once by another kernel: non-temporal stores keep the block spectra in
                // L2.  A store with dummy lanes in it goes the write-back way instead (one store instruction on either
                // path): the dummy lines are overwritten in L2 again and again and never reach HBM, whereas non-temporal
                // stores to them would all be written through (measured: 68 GB of writes per launch for 46 GB of Y).
                if (__ballot(ok) == ~0ull) __builtin_nontemporal_store(o, dst);
                else *dst = o;
            };
            // (a row of the large classes meets three or more segments: one row of look-ahead covers the LDS latency, and
            // their registers do not hold two)
            sushi_mac::mac_group<SMAX, STEP, (SMAX >= MAC_SMAX_SHORT ? 2 : 3)>((long long)jg, pair_lo, pair_hi, tt, acc, get_z, store);
        }
    }
}

template <int SMAX, int ZROWS, int RE>
__device__ __forceinline__ void mac_item(const MacArgs& a, const int* __restrict__ item, const int e0, const int slot,
                                         uint4 (*zw)[ZROWS + 1][2][MAC_BPW]) {
    using sushi_mac::h8;
    constexpr int STEP = FFT_STEP;
    const int fb = threadIdx.x % MAC_BPW;
    const int k = item[1 + slot];                               // this lane's search
    long long pair_lo = 0, pair_hi = 0;
    int jb0 = 0x7fffffff, jb1 = -0x7fffffff, n_seg = 0, first_seg = 0, first_pair = 0;
    float sy = 0.f;
    if (k >= 0) {
        const SearchDesc sd = a.searches[k];
        const FftLayout lay = fft_layout(sd.win_start, sd.n_pos, sd.tmpl_len);
        pair_lo = lay.pair0; pair_hi = lay.pair0 + lay.n_pairs; n_seg = lay.n_seg;
        first_seg = sd.first_seg - a.sub_first_seg; first_pair = first_pair_in_sub(a.sub_first_pair, sd);
        sy = a.tconst[k].mac_scale;
        long long g0, g1;
        sushi_mac::group_range<SMAX, STEP>(pair_lo, pair_hi, &g0, &g1);
        jb0 = (int)g0; jb1 = (int)g1;                            // block indices fit 31 bits (sushi_hip_stream_add_spectra)
    }
    // the wave walks the union of its lanes' group ranges (wave-uniform loop bounds)
    const int wv_first = __builtin_amdgcn_readfirstlane(wave_min_i32(jb0));
    const int wv_last = __builtin_amdgcn_readfirstlane(wave_max_i32(jb1));
    const int wv_seg = __builtin_amdgcn_readfirstlane(wave_max_i32(n_seg));
    // (the low form's rows are whole low rows on every route)
    const TspecLane tsp = RE == ROWE ? tspec_lane(a.tspec, a.tspec_half, (size_t)first_seg, e0) : TspecLane{a.tspec + (size_t)first_seg * RE + e0, (size_t)RE, false};
    uint4* __restrict__ yout = a.y + (size_t)first_pair * RE + e0;
    const uint4* __restrict__ zsp = a.spec + e0;
    // one 16-byte slot per wave: the invalid lanes of a store instruction then add one request to it instead of a line per
    // search slot (a fifth of mac_kernel's write requests were dummy lines, and the CU's L1 write path is what it waits for)
    uint4* __restrict__ dummy = a.dummy + (size_t)(blockIdx.x % MAC_DUMMY_LINES) * MAC_THREADS + (threadIdx.x & ~63);
    const int z_zero = (int)(a.spec_blocks < 0x7fffffff ? a.spec_blocks : 0x7fffffff);
    for (int c0 = 0; c0 < wv_seg; c0 += SMAX) {                 // patterns longer than SMAX segments: SMAX at a time
        h8 tt[SMAX];
#pragma unroll
        for (int s = 0; s < SMAX; ++s) tt[s] = (c0 + s) < n_seg ? as_h8(tspec_entry(tsp, (size_t)(c0 + s))) : sushi_mac::zero_h8();
        const bool lane_chunk = c0 < n_seg;
        if (c0 == 0) mac_chunk<SMAX, false, ZROWS, RE>(a, c0, wv_first, wv_last, pair_lo, pair_hi, lane_chunk, tt, zsp, z_zero, yout, dummy, sy, slot, fb, zw);
        else if (SMAX == MAC_SMAX_LONG) mac_chunk<SMAX, true, ZROWS, RE>(a, c0, wv_first, wv_last, pair_lo, pair_hi, lane_chunk, tt, zsp, z_zero, yout, dummy, sy, slot, fb, zw);
    }
}

// Grid: MAC_CHUNKS bin chunks x items (in the order of their windows in the stream).  Workgroup b runs on XCD b % 8 (observed; speed only): every XCD
// owns MAC_CHUNKS / 8 bin chunks, takes them `chunk_group` at a time and walks the items in stream order for each
// group, so that the workgroups in flight on an XCD are the same few chunks of neighbouring items, whose windows
// overlap: a row fetched for one is found in that XCD's L2 by the others.
template <int RE>
__device__ __forceinline__ void mac_place(const MacArgs& a, int* item_idx, int* e0, int* slot, int* wave) {
    constexpr int CPX = RE / MAC_BW / 8;                        // chunks per XCD
    const int xcd = blockIdx.x & 7, kx = blockIdx.x >> 3;
    const int cg = a.chunk_group;
    const int per_group = cg * a.n_items;
    const int grp = kx / per_group;
    const int in_grp = kx - grp * per_group;
    *item_idx = in_grp / cg;
    const int chunk = xcd * CPX + grp * cg + (in_grp - *item_idx * cg);
    const int lane = threadIdx.x & 63;
    *wave = threadIdx.x >> 6;
    *e0 = chunk * MAC_BW + *wave * MAC_BPW + (lane % MAC_BPW);   // which entry of four bins
    *slot = lane / MAC_BPW;                                      // which of the item's searches
}

// The whole-row launch behind the band-split exclusion forms rows only for the searches whose listed pairs are too many to form one
// by one: it is given an item list of its own, made on the device (dense_repack_kernel), whose unused slots hold class -1.
__device__ __forceinline__ bool mac_item_wanted(const MacArgs& a, const int* __restrict__ item) { return item[0] >= 0; }

// RE = entries of a row: ROWE (whole spectra) or LROWE (the low-band rows of the band-split exclusion: the same walk over a
// quarter of the bins -- rows, pattern spectra and products only have to agree on one order of the entries).
template <int RE>
__global__ __launch_bounds__(MAC_THREADS, 3)
void mac_kernel(MacArgs a) {
    __shared__ uint4 zring[MAC_WAVES][2][MAC_SMAX_SHORT + 1][2][MAC_BPW];   // per wave: two groups of rows, each with its rotation (+ a row nobody reads)
    if (a.enable && *a.enable == 0) return;
    int item_idx, e0, slot, wave;
    mac_place<RE>(a, &item_idx, &e0, &slot, &wave);
    const int* __restrict__ item = a.items + (size_t)item_idx * (1 + MAC_SPW);
    if (!mac_item_wanted(a, item)) return;
    switch (item[0]) {                                          // class c holds patterns of up to 6 (c + 1) segments
        case 0: mac_item<6, MAC_SMAX_SHORT, RE>(a, item, e0, slot, zring[wave]); break;
        case 1: mac_item<12, MAC_SMAX_SHORT, RE>(a, item, e0, slot, zring[wave]); break;
        default: mac_item<18, MAC_SMAX_SHORT, RE>(a, item, e0, slot, zring[wave]); break;
    }
}

// Patterns of 19 .. 30 segments (and, 30 at a time, longer ones): up to 30 pattern spectra per lane, two waves per SIMD.
// One pass instead of mac_kernel's two with Y read back in between (BASELINE configs[4]: half of the events).
template <int RE>
__global__ __launch_bounds__(MAC_THREADS, 2)
void mac_long_kernel(MacArgs a) {
    __shared__ uint4 zring[MAC_WAVES][2][MAC_SMAX_LONG + 1][2][MAC_BPW];
    if (a.enable && *a.enable == 0) return;
    int item_idx, e0, slot, wave;
    mac_place<RE>(a, &item_idx, &e0, &slot, &wave);
    const int* __restrict__ item = a.items + (size_t)item_idx * (1 + MAC_SPW);
    if (!mac_item_wanted(a, item)) return;
    switch (item[0]) {
        case 3: mac_item<24, MAC_SMAX_LONG, RE>(a, item, e0, slot, zring[wave]); break;
        default: mac_item<30, MAC_SMAX_LONG, RE>(a, item, e0, slot, zring[wave]); break;
    }
}

// The multiply-accumulate of LISTED pairs (the band-split exclusion: the pairs transformed first and the pairs the bound
// could not exclude -- a few per cent of all), over whole rows.  A workgroup = 256 consecutive entries of one listed pair,
// a lane one entry: its sum over the pattern's segments in mac_kernel's own order and arithmetic (patterns beyond
// MAC_SMAX_LONG segments: that many per pass, the row re-rounded to halves in between, as mac_long_kernel leaves it).
struct MacListArgs {
    const uint4* spec;
    int64_t spec_blocks;
    const uint4* tspec;
    int tspec_half;                   // `tspec` holds half rows (TspecLane)
    uint4* y;                         // [pairs of the sub-batch][ROWE]
    const SearchDesc* searches;
    const TemplConsts* tconst;
    const int* pairmap;
    const int* list;                  // pairs to compute (indices inside the sub-batch)
    const int* count;                 // NULL, or how many entries of `list` exist
    int n_list;                       // entries of `list` when count is NULL
    int sub_first_seg;
    int sub_first_pair;
    const int* dense_search;          // NULL, or [searches of the sub-batch]: 1 = the dense multiply-accumulate forms this search's rows instead
    int long_only;                    // 1: only pairs of patterns beyond MAC_SMAX_LONG segments (mac_rows_kernel forms the others)
};
constexpr int MACL_THREADS = 256;
constexpr int MACL_PARTS = ROWE / MACL_THREADS;
__global__ __launch_bounds__(MACL_THREADS)
void mac_list_kernel(MacListArgs a) {
    typedef _Float16 h2 __attribute__((ext_vector_type(2)));
    const int n = a.count ? *a.count : a.n_list;
    const int z_zero = (int)(a.spec_blocks < 0x7fffffff ? a.spec_blocks : 0x7fffffff);
    for (long long it = blockIdx.x; it < (long long)n * MACL_PARTS; it += gridDim.x) {
        const int pr = a.list[it / MACL_PARTS];
        const int e = (int)(it % MACL_PARTS) * MACL_THREADS + threadIdx.x;
        const int k = a.pairmap[pr];
        if (a.dense_search && a.dense_search[k]) continue;
        const SearchDesc sd = a.searches[k];
        const FftLayout lay = fft_layout(sd.win_start, sd.n_pos, sd.tmpl_len);
        if (a.long_only && lay.n_seg <= MAC_SMAX_LONG) continue;
        const long long I = absolute_pair(lay, a.sub_first_pair, pr, sd);
        const float sy = a.tconst[k].mac_scale;
        const TspecLane tsp = tspec_lane(a.tspec, a.tspec_half, (size_t)(sd.first_seg - a.sub_first_seg), e);
        const uint4* __restrict__ zsp = a.spec + e;
        float re[sushi_mac::BINS], im[sushi_mac::BINS];
        for (int c0 = 0; c0 < lay.n_seg; c0 += MAC_SMAX_LONG) {
            sushi_mac::acc4 acc = sushi_mac::zero_acc();
            const int s_end = c0 + MAC_SMAX_LONG < lay.n_seg ? c0 + MAC_SMAX_LONG : lay.n_seg;
            // six segments at a time, all twelve loads requested before the first product (a segment past the end multiplies a
            // zero pattern entry: the sum is unchanged, as in the padded classes of mac_kernel)
            for (int s6 = c0; s6 < s_end; s6 += 6) {
                sushi_mac::h8 z[6], u[6];
#pragma unroll
                for (int t = 0; t < 6; ++t) {
                    const int sx = s6 + t < s_end ? s6 + t : s_end - 1;
                    const long long jj = FFT_STEP * I + sx;
                    z[t] = as_h8(zsp[(size_t)(jj < z_zero ? jj : z_zero) * ROWE]);
                    u[t] = as_h8(tspec_entry(tsp, (size_t)sx));
                }
#pragma unroll
                for (int t = 0; t < 6; ++t) {
                    const sushi_mac::h8 ut = s6 + t < s_end ? u[t] : sushi_mac::zero_h8();
                    const sushi_mac::zrow zr = {z[t], sushi_mac::rot_mi(z[t])};
                    sushi_mac::mac4(acc, ut, zr);
                }
            }
            unsigned o[sushi_mac::BINS];
#pragma unroll
            for (int q = 0; q < sushi_mac::BINS; ++q) {
                float r = acc.re[q] * sy, i = acc.im[q] * sy;
                if (c0 > 0) { r += re[q]; i += im[q]; }
                const h2 h = {(_Float16)r, (_Float16)i};
                o[q] = __builtin_bit_cast(unsigned, h);
                re[q] = (float)h.x; im[q] = (float)h.y;                      // what a later pass reads back
            }
            if (s_end == lay.n_seg) a.y[(size_t)pr * ROWE + e] = uint4{o[0], o[1], o[2], o[3]};
        }
    }
}
