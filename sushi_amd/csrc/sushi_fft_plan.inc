// sushi_amd/csrc/sushi_fft_plan.inc -- part of sushi_fft.hip (included there, inside its anonymous namespace; not a header of its own):
// the host side's glue between a plan (plan_core.hpp and batch_core.hpp, which are host only and checked on the CPU) and the device:
// kernel launches by method / sample type, per-stage timing, a sub-batch's typed view of the batch's memory.

// A kernel instantiated per method / per sample type: `f` launches it with the template argument it is given, as a
// std::integral_constant / a null pointer of the sample type.
template <typename F> int launch_method(int method, F&& f) {
    if (method == SUSHI_HIP_METHOD_CCOEFF_NORMED) f(std::integral_constant<int, SUSHI_HIP_METHOD_CCOEFF_NORMED>());
    else f(std::integral_constant<int, SUSHI_HIP_METHOD_SQDIFF_NORMED>());
    return launch_ok();
}
template <typename F> int launch_dtype(int dtype, F&& f) {
    if (dtype == SUSHI_HIP_F32) f((float*)nullptr);
    else f((uint8_t*)nullptr);
    return launch_ok();
}

// ---- optional per-stage timing (sushi_hip_profile_begin / _end): HIP events on the launch streams ----
struct ProfSpan { hipEvent_t t0, t1; int stage; };
struct ProfCall { std::vector<ProfSpan> spans; };
bool g_prof_on = false;
std::vector<ProfCall> g_prof;

inline hipEvent_t prof_begin(ProfCall* pc, hipStream_t st) {
    if (!pc) return nullptr;
    hipEvent_t e = nullptr;
    if (hipEventCreate(&e) != hipSuccess) return nullptr;
    (void)hipEventRecord(e, st);
    return e;
}
inline void prof_end(ProfCall* pc, hipEvent_t t0, int stage, hipStream_t st) {
    if (!pc || !t0) return;
    hipEvent_t e = nullptr;
    if (hipEventCreate(&e) != hipSuccess) return;
    (void)hipEventRecord(e, st);
    pc->spans.push_back(ProfSpan{t0, e, stage});
}

// One sub-batch of a cut of a plan and where it works in the batch's memory `mem`: its lane's workspace (ws_layout, typed), its
// schedule and items, its small counters (SUBC_BYTES at its index in the cut: SubCounters, then its scount words), its pattern rows' norms.
struct SubView {
    const SubBatch& sb;
    int n_sub;
    uint32_t* tspec; uint4 *y, *tspec_low, *ylow, *dummy; unsigned long long* cand; TemplConsts* tconst; TileDesc* tiles; int32_t* candbuf;
    float *pair_lb, *slb, *acc, *tnorm_rest; unsigned char* audit_mark; SubCounters* sub; const int32_t *order, *items;
    int *pairmap, *plist, *slist, *slist2, *votes, *dense_search, *ditems, *citems;
    int *n_slist, *n_citems, *any_dense, *n_slist2, *n_dense_listed, *n_list3, *n_rest_items;     // the scount words (ScountSlot)
    SubView(char* mem, const BatchLayout& lay, size_t ws_lane, const SubBatch& s, size_t si) : sb(s), n_sub(s.b0 - s.a0) {
        const WsLayout w = ws_layout(s.pairs, s.segs, n_sub);
        char* p = mem + lay.ws + (size_t)s.lane * ws_lane;
        tspec = (uint32_t*)(p + w.tspec); y = (uint4*)(p + w.y); tspec_low = (uint4*)(p + w.tspec_low); ylow = (uint4*)(p + w.ylow); dummy = (uint4*)(p + w.dummy);
        cand = (unsigned long long*)(p + w.cand); tconst = (TemplConsts*)(p + w.tconst); tiles = (TileDesc*)(p + w.tiles); candbuf = (int32_t*)(p + w.candbuf);
        pair_lb = (float*)(p + w.pair_lb); slb = (float*)(p + w.slb); acc = (float*)(p + w.acc); tnorm_rest = (float*)(mem + lay.tnorm) + s.first_seg;
        audit_mark = (unsigned char*)(p + w.audit_mark); sub = (SubCounters*)(mem + lay.subc + si * SUBC_BYTES);
        int* const scount = (int*)sub + SUBC_SCOUNT;
        n_slist = scount + SC_SLIST; n_citems = scount + SC_CITEMS; any_dense = scount + SC_ANY_DENSE; n_slist2 = scount + SC_SLIST2;
        n_dense_listed = scount + SC_DENSE_LISTED; n_list3 = scount + SC_LIST3; n_rest_items = scount + SC_REST_ITEMS;
        order = (const int32_t*)(mem + lay.order) + s.order_first;
        items = (const int32_t*)(mem + lay.items) + (size_t)s.item_first[0] * (1 + MAC_SPW);   // (its two item lists lie next to each other)
        pairmap = (int*)(p + w.pairmap); plist = (int*)(p + w.plist); slist = (int*)(p + w.slist); slist2 = (int*)(p + w.slist2);
        votes = (int*)(p + w.votes); dense_search = (int*)(p + w.dense_search); ditems = (int*)(p + w.ditems); citems = (int*)(p + w.citems);
    }
};
