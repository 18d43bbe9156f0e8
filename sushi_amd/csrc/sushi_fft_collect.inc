// sushi_amd/csrc/sushi_fft_collect.inc -- part of sushi_fft.hip (included there, inside its anonymous namespace; not a header of its own):
// collect_kernel: the candidates of flagged searches, tile by tile.

// Collection pass over the flagged searches of a sub-batch: the same transforms and scores again (bit for bit), now
// against the search's final threshold; every candidate goes to its tile's list, tiles with many candidates (or
// when the buffer is full) are marked dense.  A fixed grid strides over the (search, pair) items refine_kernel listed.
constexpr int SPARSE_MAX = SPARSE_TILE_MAX; // candidates per tile up to which they are listed; beyond: every position
constexpr int COLLECT_GRID = 1024;         // collect_kernel's workgroups: two per CU, twice over

template <int METHOD>
__global__ __launch_bounds__(FT, 8)
void collect_kernel(IfftArgs a) {
    __shared__ __attribute__((aligned(16))) float lds[LDS_FLOATS];
    __shared__ int tcnt[TILES_PER_PAIR], toff[TILES_PER_PAIR], tfill[TILES_PER_PAIR];
    const int n_items = *a.n_citems;
    if (n_items == 0) return;
    // refine_kernel listed, for every search it flagged, the pairs that can hold a candidate (all pairs for a search that goes
    // to every position): a fixed grid strides over that list -- every workgroup has work while there is any
    for (int it = blockIdx.x; it < n_items; it += gridDim.x) {
        {
            // everything an iteration needs is loaded inside it, off a thread index the compiler cannot see through: left to
            // hoist the transform's per-thread constants and addresses out of the loop it spilled hundreds of bytes of them
            int tid = threadIdx.x;
            asm volatile("" : "+v"(tid));
            const sushi_fft::WTwiddles tw = sushi_fft::load_wtwiddles<1>(tid, twiddles());
            const sushi_fft::MfmaB mb = dft16_operands(tid);
            const int lane = tid & 63;
            const int pr = __builtin_amdgcn_readfirstlane(a.citems[it]);
            const int k = __builtin_amdgcn_readfirstlane(a.pairmap[pr]);
            const int s_idx = a.first_search + k;                              // global search index
            const SearchDesc sd = a.searches[k];
            const FftLayout lay = fft_layout(sd.win_start, sd.n_pos, sd.tmpl_len);
            const TemplConsts tc = a.tconst[k];
            const bool everything = a.flags[s_idx] == 2;
            // smallest (score + bound) of the search; none (TM_CCOEFF_NORMED: every window uncertain): everything is a candidate
            const float U = a.gkeys[s_idx] == NO_KEY ? 4.0f : key_score(a.gkeys[s_idx]);
            const int i = pair_of_search(a.sub_first_pair, pr, sd);
            const int64_t qbase = (lay.pair0 + i) * (int64_t)FFT_STEP * FFT_SEG;
            const int64_t rel0 = qbase - sd.win_start;                     // position (relative to the window) of pos 0
            __syncthreads();                                               // previous item's shared state is consumed
            if (tid < TILES_PER_PAIR) { tcnt[tid] = 0; tfill[tid] = 0; toff[tid] = -1; }
            unsigned candmask = 0;                                         // bit q: scores[q] is a candidate
            int plo = 0, phi = 0;
            if (!everything) {
                PairScores ps;
                float zn, zn_c;
                sushi_fft::uint4v yl[4];
                (void)load_y(yl, a.y + (size_t)pr * (FN / 2), tid);
                score_pair<METHOD>(a, yl, mb, sd, tc, lay.pair0 + i, lds, tid, tw, ps, plo, phi, zn, zn_c);
                // the bound the pair was ranked with, as ifft_kernel stored it (the same scores again, bit for bit)
                const float e_pair = __uint_as_float((unsigned)(a.cand[(size_t)pr * FFT_ROW + FFT_CAND + 1] & 0xffffffffull));
#pragma unroll
                for (int q = 0; q < 2 * HPT; ++q) {
                    const bool c = fmaxf(ps.scores[q] - e_pair, 0.f) <= U;              // invalid positions hold +inf, uncertain ones -1
                    candmask |= c ? (1u << q) : 0u;
                    // all threads of the workgroup look at the same tile for a given q
                    const int tile = (FT * (q % HPT)) / TILE + (q / HPT) * (FH / TILE);
                    const unsigned long long b = __ballot(c);
                    if (lane == 0 && b) atomicAdd(&tcnt[tile], __popcll(b));
                }
            } else {
                const int64_t plo64 = sd.win_start - qbase;
                plo = (int)(plo64 < 0 ? 0 : plo64);
                const int64_t phi64 = (int64_t)sd.n_pos + (sd.win_start - qbase);
                phi = (int)(phi64 < 2 * FH ? phi64 : 2 * FH);
                __syncthreads();
                if (tid < TILES_PER_PAIR) {                                 // every tile that holds a valid position
                    const int t0 = tid * TILE;
                    if (t0 < phi && t0 + TILE > plo) tcnt[tid] = TILE;
                }
            }
            __syncthreads();
            if (tid == 0) {
                // One thread hands out this pair's tiles: ONE addition to each of the run's counters per workgroup (a tile at a time,
                // from 24 threads of every workgroup, the same-address atomics -- and a compare-and-swap loop among them -- were
                // most of this kernel's time).  The candidate buffer's counter never runs far past its capacity: a workgroup that
                // sees it full does not add to it (its tiles are evaluated at every position instead).
                // (a listed tile goes to exact_tiles_kernel in entries of at most SPARSE_UNIT candidates: what an entry costs is
                // bounded, and a workgroup's threads are all busy with it)
                int total = 0, nt = 0, n_sparse = 0, extra = 0;
                for (int t = 0; t < TILES_PER_PAIR; ++t) {
                    const int cnt = tcnt[t];
                    if (cnt > 0) { ++nt; if (cnt <= SPARSE_MAX) { total += cnt; ++n_sparse; extra += (cnt - 1) / SPARSE_UNIT; } }
                }
                if (nt > 0) {
                    int base = -1;
                    if (total > 0 && *(volatile int*)&a.sub->n_cand + total <= a.cand_cap) {
                        const int o = atomicAdd(&a.sub->n_cand, total);
                        if (o + total <= a.cand_cap) base = o;
                    }
                    // capacity: every tile of every pair + one entry per SPARSE_UNIT candidates of the candidate buffer
                    int slot = atomicAdd(&a.sub->n_tiles, nt + (base >= 0 ? extra : 0));
                    for (int t = 0; t < TILES_PER_PAIR; ++t) {
                        const int cnt = tcnt[t];
                        if (cnt <= 0) continue;
                        int off = -1;
                        if (cnt <= SPARSE_MAX && base >= 0) { off = base; base += cnt; }
                        toff[t] = off;
                        TileDesc td;
                        td.search = s_idx;
                        td.p0 = (int)(rel0 + (int64_t)t * TILE);
                        if (off >= 0) {
                            for (int u = 0; u < cnt; u += SPARSE_UNIT) {
                                td.off = off + u;
                                td.cnt = cnt - u < SPARSE_UNIT ? cnt - u : SPARSE_UNIT;
                                a.tiles[slot++] = td;
                            }
                        } else {
                            td.off = -1;
                            td.cnt = -1;
                            a.tiles[slot++] = td;
                        }
                    }
                    const int listed = base >= 0 || total == 0 ? n_sparse : 0;  // (all of the pair's sparse tiles are listed, or none)
                    if (listed > 0) {
                        atomicAdd(&a.counters->tiles_sparse, (unsigned long long)listed);
                        atomicAdd(&a.counters->candidates, (unsigned long long)total);
                    }
                    if (nt - listed > 0) atomicAdd(&a.counters->tiles_dense, (unsigned long long)(nt - listed));
                }
            }
            __syncthreads();
            if (candmask) {
#pragma unroll
                for (int q = 0; q < 2 * HPT; ++q) {
                    if (candmask & (1u << q)) {
                        const int tile = (FT * (q % HPT)) / TILE + (q / HPT) * (FH / TILE);
                        const int off = toff[tile];
                        if (off >= 0) {
                            const int pos = tid + FT * (q % HPT) + (q / HPT) * FH;
                            const int slot = atomicAdd(&tfill[tile], 1);
                            a.candbuf[off + slot] = (int32_t)(rel0 + pos);
                        }
                    }
                }
            }
        }
    }
}
