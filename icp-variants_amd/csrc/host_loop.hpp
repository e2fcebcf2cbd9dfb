// host_loop.hpp -- the ICP loop of one pose (icp_run, icp_iterate) and the stage-level entry points that drive the same launches by hand
// (icp_query_matches, icp_match, icp_correspond, icp_match_seeded).  Part of icp_hip.hip (included from there, after host_launch.hpp).
namespace {
// The plan of a run (icp_run, icp_iterate, icp_run_multistart), resolved up front (uploads) so that the loop itself is launch-only: the
// decimation factor of every iteration (icp_schedule; 0 = no selection, the full cloud) and its query set -- the level's cloud (a
// Morton-sorted copy for the BVH matcher without resampling), its selection, its size, its Morton order.
struct RunPlan {
    std::vector<int> factors, ns; std::vector<const Cloud*> clouds; std::vector<const int*> sels, orders;
    bool sorted_levels = false;      // BVH matcher without resampling: every level is a physical, Morton-sorted copy -> no index lists in the loop at all
    bool fixed_sets = true;          // no resampling: SELECT_ALL, or a normal-space draw held for the run
    int iters() const { return (int)factors.size(); }
    // seed the search with the previous iteration's neighbours when it matched the same queries: same level, it had work, no resampling
    bool seeded(int i) const { return i > 0 && factors[i] == factors[i - 1] && ns[i - 1] > 0 && fixed_sets; }
};

// ---- normal-space sampling: the launches of dev_nss.hpp ----
// The bucket of every source point for the current grid (cached per source and grid; a new grid also drops the levels sorted by it).
int nss_buckets(icp_ctx* c) {
    const int grid = c->nss_opt.grid, n = c->src.n;
    if (c->nss_bkt_grid == grid) return ICP_OK;
    int rc;
    for (auto& kv : c->nss_levels) release(kv.second);      // sorted by the buckets of another grid
    c->nss_levels.clear();
    const Cloud& s = c->src;
    if ((rc = ensure(c, c->nss_bkt, (size_t)n * 2))) return rc;
    hipLaunchKernelGGL(k_nss_bucket, dim3((n + 255) / 256), dim3(256), 0, c->stream, s.x.as<float>(), s.y.as<float>(), s.z.as<float>(),
                       s.nx.as<float>(), s.ny.as<float>(), s.nz.as<float>(), n, grid, c->nss_bkt.as<unsigned short>());
    HIPCK(c, hipGetLastError());
    c->nss_bkt_grid = grid;
    return ICP_OK;
}
// Once per level: the base set's candidates in a stable counting sort by bucket, the segment starts, the long segments.  Enqueued only.
int nss_level(icp_ctx* c, int factor, const int* base, int n_base, const NssLevel** out) {
    auto it = c->nss_levels.find(factor);
    if (it == c->nss_levels.end()) {
        NssLevel nl; int rc;
        const int nb = 6 * c->nss_opt.grid * c->nss_opt.grid, nblocks = (n_base + NSS_LEVEL_THREADS - 1) / NSS_LEVEL_THREADS;
        nl.n_base = n_base; nl.max_long = n_base / NSS_LONG; nl.max_chunks = n_base / NSS_CHUNK + nl.max_long;      // (a long segment has > NSS_LONG points; one partial chunk each)
        const int n_table = (nb + 1) * nblocks;
        if ((rc = ensure(c, nl.cand, (size_t)n_base * 4)) || (rc = ensure(c, nl.seg, (NSS_MAX_BUCKETS + 2) * 4)) || (rc = ensure(c, nl.longs, sizeof(NssLongs)))) { release(nl); return rc; }
        if ((rc = ensure(c, c->nss_table, (size_t)n_table * 4)) || (rc = ensure(c, c->nss_total, 4))) { release(nl); return rc; }
        const unsigned short* bkt = c->nss_bkt.as<unsigned short>();
        hipLaunchKernelGGL(k_nss_level_hist, dim3(nblocks), dim3(NSS_LEVEL_THREADS), 0, c->stream, base, n_base, bkt, nb, c->nss_table.as<int>(), nblocks);
        hipLaunchKernelGGL(k_select_scan, dim3(1), dim3(1024), 0, c->stream, c->nss_table.as<int>(), n_table, c->nss_total.as<int>());
        hipLaunchKernelGGL(k_nss_level_scatter, dim3(nblocks), dim3(NSS_LEVEL_THREADS), 0, c->stream, base, n_base, bkt, nb, c->nss_table.as<int>(), nblocks, nl.cand.as<int>());
        hipLaunchKernelGGL(k_nss_level_segs, dim3(1), dim3(NSS_QUOTA_THREADS), 0, c->stream, c->nss_table.as<int>(), nblocks, nb, nl.seg.as<int>(), nl.longs.as<NssLongs>());
        if (hipGetLastError() != hipSuccess) { release(nl); c->err = "normal-space sampling: a level launch failed"; return ICP_ERR_HIP; }
        it = c->nss_levels.emplace(factor, std::move(nl)).first;
    }
    *out = &it->second;
    return ICP_OK;
}
// n_draws draws of one level, for iterations word0 .. word0 + n_draws - 1, into slots word0 .. of sel_lists / sel_counts (slot stride cap).
// Scratch per slot: 2 rows of NSS_ROW words (quotas, thresholds) and, per possible long segment (max_long_all = n_src / NSS_LONG of them),
// 8 bytes of state and one 2048-bin histogram: 8 KB * n_src / 16384 = n_src / 2 bytes, an eighth of the slot's index list.
int nss_draw(icp_ctx* c, const NssLevel& nl, const int* base, uint32_t word0, int n_draws, int max_long_all, size_t cap) {
    const icp_params& p = c->prm;
    const int nb = 6 * c->nss_opt.grid * c->nss_opt.grid, n = nl.n_base, nblk = (n + 255) / 256, stride = nblk + 1;
    unsigned int* quota = c->nss_quota.as<unsigned int>() + (size_t)word0 * NSS_ROW; unsigned int* thr = c->nss_thr.as<unsigned int>() + (size_t)word0 * NSS_ROW;
    NssLongState* state = c->nss_state.as<NssLongState>() + (size_t)word0 * max_long_all;
    unsigned int* hist = c->nss_hist.as<unsigned int>() + (size_t)word0 * max_long_all * NSS_BINS;
    int* counts = c->sel_counts.as<int>() + word0; int* blocks = c->sel_blocks.as<int>();
    const int* cand = nl.cand.as<int>(); const int* seg = nl.seg.as<int>(); const NssLongs* longs = nl.longs.as<NssLongs>();
    const unsigned short* bkt = c->nss_bkt.as<unsigned short>();
    const uint32_t seed = p.selection_seed;
    const dim3 B(NSS_THREADS);
    hipLaunchKernelGGL(k_nss_quota, dim3(n_draws), dim3(NSS_QUOTA_THREADS), 0, c->stream, seg, nb, p.selection_proba, seed, word0, quota, thr);
    hipLaunchKernelGGL(k_nss_select_small, dim3(nb, n_draws), B, 0, c->stream, cand, seg, seed, word0, quota, thr);
    if (nl.max_long > 0) {
        const dim3 gh(nl.max_chunks, n_draws), gp(nl.max_long, n_draws);
        hipLaunchKernelGGL(k_nss_long_hist<1>, gh, B, 0, c->stream, cand, seg, longs, max_long_all, seed, word0, quota, state, hist);
        hipLaunchKernelGGL(k_nss_long_pick<1>, gp, B, 0, c->stream, seg, longs, max_long_all, quota, state, hist, thr);
        hipLaunchKernelGGL(k_nss_long_hist<2>, gh, B, 0, c->stream, cand, seg, longs, max_long_all, seed, word0, quota, state, hist);
        hipLaunchKernelGGL(k_nss_long_pick<2>, gp, B, 0, c->stream, seg, longs, max_long_all, quota, state, hist, thr);
        hipLaunchKernelGGL(k_nss_long_hist<3>, gh, B, 0, c->stream, cand, seg, longs, max_long_all, seed, word0, quota, state, hist);
        hipLaunchKernelGGL(k_nss_long_pick<3>, gp, B, 0, c->stream, seg, longs, max_long_all, quota, state, hist, thr);
    }
    hipLaunchKernelGGL(k_nss_count, dim3(nblk, n_draws), dim3(256), 0, c->stream, base, n, bkt, seed, word0, quota, thr, blocks, stride);
    hipLaunchKernelGGL(k_nss_scan, dim3(n_draws), dim3(1024), 0, c->stream, blocks, nblk, stride, counts);
    hipLaunchKernelGGL(k_nss_scatter, dim3(nblk, n_draws), dim3(256), 0, c->stream, base, n, bkt, seed, word0, quota, thr, blocks, stride, c->sel_lists.as<int>() + (size_t)word0 * cap, cap);
    HIPCK(c, hipGetLastError());
    return ICP_OK;
}
// The query sets of a run with selection = ICP_SELECT_NORMAL_SPACE: every draw made up front on the device, ONE copy of their sizes.
// resample: iteration i draws with word i from its level's base set (sels[i], ns[i] on entry).  Held: a factor's first iteration draws for
// all of them, and the list becomes a level of its own (c->nss_held), Morton-sorted for the BVH matcher like a multires level.
int nss_plan(icp_ctx* c, RunPlan& pl) {
    const icp_params& p = c->prm;
    const int iters = pl.iters(); int rc;
    const bool held = c->nss_opt.resample == 0;
    if (!c->src.has_normals) { c->err = "normal-space sampling (selection = 2) needs normals on the source"; return ICP_ERR_INVALID_ARG; }
    if (c->nss_held_stale || c->nss_held_proba != p.selection_proba || c->nss_held_seed != p.selection_seed) drop_nss(c, true);
    c->nss_held_proba = p.selection_proba; c->nss_held_seed = p.selection_seed;
    if ((rc = nss_buckets(c))) return rc;
    const size_t cap = (size_t)c->src.n; const int max_long_all = c->src.n / NSS_LONG;
    const size_t hist_bytes = (size_t)iters * max_long_all * NSS_BINS * 4;
    if ((rc = ensure(c, c->sel_lists, (size_t)iters * cap * 4)) || (rc = ensure(c, c->sel_counts, (size_t)iters * 4))) return rc;
    if ((rc = ensure(c, c->sel_blocks, (size_t)iters * ((cap + 255) / 256 + 1) * 4))) return rc;
    if ((rc = ensure(c, c->nss_quota, (size_t)iters * NSS_ROW * 4)) || (rc = ensure(c, c->nss_thr, (size_t)iters * NSS_ROW * 4))) return rc;
    if ((rc = ensure(c, c->nss_state, (size_t)iters * (max_long_all + 1) * sizeof(NssLongState)))) return rc;
    if (hist_bytes > c->nss_hist.cap || !c->nss_hist.p) {
        if ((rc = ensure(c, c->nss_hist, hist_bytes))) return rc;
        HIPCK(c, hipMemsetAsync(c->nss_hist.p, 0, c->nss_hist.cap, c->stream));      // every pick leaves its histogram cleared
    }
    HIPCK(c, hipMemsetAsync(c->sel_counts.p, 0, (size_t)iters * 4, c->stream));
    std::vector<int> first((size_t)iters);                   // the iteration whose draw iteration i uses
    std::vector<char> drawn((size_t)iters, 0);
    for (int i = 0; i < iters; i++) {
        first[i] = i;
        if (held) for (int j = 0; j < i; j++) if (pl.factors[j] == pl.factors[i]) { first[i] = j; break; }
    }
    for (int i = 0; i < iters;) {
        int run = 1;
        if (held) {
            auto it = c->nss_held.find(pl.factors[i]);
            if (first[i] != i || (it != c->nss_held.end() && it->second.word == (uint32_t)i)) { i++; continue; }
            if (it != c->nss_held.end()) { release(it->second.lv); c->nss_held.erase(it); }
        } else while (i + run < iters && pl.factors[i + run] == pl.factors[i]) run++;
        if (pl.ns[i] > 0) {
            const NssLevel* nl = nullptr;
            if ((rc = nss_level(c, pl.factors[i], pl.sels[i], pl.ns[i], &nl))) return rc;
            // (sel_blocks: the draws of a level use the buffer from its start; the next level's launches follow on the stream)
            if ((rc = nss_draw(c, *nl, pl.sels[i], (uint32_t)i, run, max_long_all, cap))) return rc;
        }
        for (int k = 0; k < run; k++) drawn[i + k] = 1;
        i += run;
    }
    std::vector<int> counts((size_t)iters);
    HIPCK(c, hipMemcpyAsync(counts.data(), c->sel_counts.p, (size_t)iters * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCK(c, hipStreamSynchronize(c->stream));
    for (int i = 0; i < iters; i++) {
        if (!held) { pl.sels[i] = c->sel_lists.as<int>() + (size_t)i * cap; pl.ns[i] = counts[i]; pl.orders[i] = nullptr; continue; }
        if (drawn[i]) {                                      // the list leaves the scratch: a level of its own
            NssHeld& h = c->nss_held[pl.factors[i]];
            h.word = (uint32_t)i; h.lv.n = counts[i];
            if ((rc = ensure(c, h.lv.idx, (size_t)(counts[i] > 0 ? counts[i] : 1) * 4))) return rc;
            if (counts[i] > 0) HIPCK(c, hipMemcpyAsync(h.lv.idx.p, c->sel_lists.as<int>() + (size_t)i * cap, (size_t)counts[i] * 4, hipMemcpyDeviceToDevice, c->stream));
        }
        Level& lv = c->nss_held[pl.factors[i]].lv;
        pl.ns[i] = lv.n; pl.orders[i] = nullptr;
        if (pl.sorted_levels) { pl.sels[i] = nullptr; if ((rc = get_sorted_held(c, lv, &pl.clouds[i]))) return rc; }
        else pl.sels[i] = lv.idx.as<int>();
    }
    return ICP_OK;
}

int make_plan(icp_ctx* c, bool single, RunPlan& pl) {
    const icp_params& p = c->prm;
    int rc;
    c->sel_last.clear();
    if (single) pl.factors.assign(1, 0);
    else {
        int32_t cnt = 0;
        if ((rc = icp_schedule(&p, c->src.n, nullptr, 0, &cnt))) { c->err = "multires with n_iterations < 1 never terminates in the reference"; return rc; }
        pl.factors.resize((size_t)cnt);
        if (cnt > 0) icp_schedule(&p, c->src.n, pl.factors.data(), cnt, &cnt);
    }
    const std::vector<int>& factors = pl.factors; std::vector<int>& ns = pl.ns; std::vector<const int*>& sels = pl.sels; std::vector<const int*>& orders = pl.orders;
    const int iters = pl.iters();
    const bool nss = !single && p.selection == ICP_SELECT_NORMAL_SPACE;
    const bool resample = !single && p.selection == ICP_SELECT_RANDOM;
    pl.fixed_sets = !resample && !(nss && c->nss_opt.resample != 0);
    sels.assign((size_t)iters, nullptr); ns.assign((size_t)iters, c->src.n); orders.assign((size_t)iters, nullptr); pl.clouds.assign((size_t)iters, &c->src);
    pl.sorted_levels = p.matching == ICP_MATCH_KNN && p.knn_backend == ICP_KNN_LBVH && pl.fixed_sets;
    if (iters == 0) return ICP_OK;
    for (int i = 0; i < iters; i++) {
        if (pl.sorted_levels && !nss) { if ((rc = get_sorted_level(c, factors[i], &pl.clouds[i], &ns[i]))) return rc; }
        else if (factors[i] > 0) { if ((rc = get_level(c, factors[i], &sels[i], &ns[i], nullptr))) return rc; }
    }
    if (nss && (rc = nss_plan(c, pl))) return rc;
    if (resample) {
        // RANDOM_SAMPLING (ICPOptimizer.h:549-550: resample at the start of every iteration, over the current level's cloud).
        // All resamples are drawn up front on the device; one small copy returns their sizes so the loop stays launch-only.
        double th = (double)p.selection_proba * 4294967296.0;
        const int take_all = th >= 4294967296.0 ? 1 : 0;
        const uint32_t threshold = th <= 0.0 ? 0u : (take_all ? 0xFFFFFFFFu : (uint32_t)th);
        const size_t cap = (size_t)c->src.n;
        if ((rc = ensure(c, c->sel_lists, (size_t)iters * cap * 4))) return rc;
        if ((rc = ensure(c, c->sel_counts, (size_t)iters * 4))) return rc;
        if ((rc = ensure(c, c->sel_blocks, (size_t)((cap + 255) / 256 + 1) * 4))) return rc;
        for (int i = 0; i < iters; i++) {
            const int nb = (ns[i] + 255) / 256;
            int* out = c->sel_lists.as<int>() + (size_t)i * cap;
            if (ns[i] > 0) {
                hipLaunchKernelGGL(k_select_count, dim3(nb), dim3(256), 0, c->stream, sels[i], ns[i], p.selection_seed, (uint32_t)i, threshold, take_all, c->sel_blocks.as<int>());
                hipLaunchKernelGGL(k_select_scan, dim3(1), dim3(1024), 0, c->stream, c->sel_blocks.as<int>(), nb, c->sel_counts.as<int>() + i);
                hipLaunchKernelGGL(k_select_scatter, dim3(nb), dim3(256), 0, c->stream, sels[i], ns[i], p.selection_seed, (uint32_t)i, threshold, take_all, c->sel_blocks.as<int>(), out);
            } else HIPCK(c, hipMemsetAsync(c->sel_counts.as<int>() + i, 0, 4, c->stream));
            sels[i] = out; orders[i] = nullptr;
        }
        HIPCK(c, hipGetLastError());
        std::vector<int> counts((size_t)iters);
        HIPCK(c, hipMemcpyAsync(counts.data(), c->sel_counts.p, (size_t)iters * 4, hipMemcpyDeviceToHost, c->stream));
        HIPCK(c, hipStreamSynchronize(c->stream));
        for (int i = 0; i < iters; i++) ns[i] = counts[i];
    }
    if (resample || nss) {                                   // icp_get_selection
        c->sel_last.resize((size_t)iters);
        for (int i = 0; i < iters; i++) {
            const int* list = sels[i];
            if (nss && pl.fixed_sets) list = c->nss_held[factors[i]].lv.idx.as<int>();
            c->sel_last[(size_t)i] = std::make_pair(ns[i] > 0 ? list : nullptr, ns[i]);
        }
    }
    return ICP_OK;
}

// Finishes the host copy hs of a run's records (every record of an iteration with work was written in full on the device): an empty
// iteration carries the pose before it (pose_in for iteration 0), rmse / benchmark_error are -1 where not recorded.  Copies up to max_out
// of the n_run records (all of the plan's, or those up to the iteration a converged run stopped after) to out and returns their first
// failing status.
int finish_records(const RunPlan& pl, int n_run, icp_iter_stats* hs, const float* pose_in, bool rmse, bool fontana, icp_iter_stats* out, int max_out) {
    int status = ICP_OK;
    for (int i = 0; i < n_run; i++) {
        const bool empty = pl.ns[i] <= 0;
        if (empty) { hs[i].n_src = 0; hs[i].n_valid = 0; hs[i].status = ICP_ERR_NO_CORRESPONDENCES; memcpy(hs[i].pose, i ? hs[i - 1].pose : pose_in, 64); }
        if (empty || !rmse) hs[i].rmse = -1.f;
        if (empty || !fontana) hs[i].benchmark_error = -1.f;
        if (hs[i].status != ICP_OK && status == ICP_OK) status = hs[i].status;
        if (out && i < max_out) out[i] = hs[i];
    }
    return status;
}

// The ring of a run of merged launches (dev_solve.hpp, "the ring form"), inside c->ring: n_slots pose slots in every replica, then
// n_rows totals rows (one per reduced launch), then -- unless the caller keeps it elsewhere (fault != nullptr) -- the run's fault word.
// Both partials buffers hold nbmax blocks: launch j writes one while the reducer riding in it folds the other.
struct Ring { PoseState* slots; unsigned long long* trows; int* run_fault; size_t slot_bytes; };
int make_ring(icp_ctx* c, int n_slots, int n_rows, int nbmax, int* fault, Ring& r) {
    static_assert(sizeof(PoseState) == 128, "a pose slot is 16 granules");
    int rc;
    r.slot_bytes = (size_t)n_slots * POSE_REPLICAS * POSE_REPLICA_STRIDE; const size_t tot_bytes = (size_t)n_rows * NSUM * 8;
    if ((rc = ensure(c, c->ring, r.slot_bytes + tot_bytes + (fault ? 0 : 64)))) return rc;
    if ((rc = ensure(c, c->partials, (size_t)nbmax * NSUM * 8))) return rc;
    if ((rc = ensure(c, c->partials2, (size_t)nbmax * NSUM * 8))) return rc;
    r.slots = c->ring.as<PoseState>(); r.trows = (unsigned long long*)(c->ring.as<char>() + r.slot_bytes);
    r.run_fault = fault ? fault : (int*)(c->ring.as<char>() + r.slot_bytes + tot_bytes);
    return ICP_OK;
}
double* ring_partials(const icp_ctx* c, int j) { return (j & 1) ? c->partials2.as<double>() : c->partials.as<double>(); }
// The reducer riding in launch j of the ring (j = 0: none): it folds launch j - 1's partials (n_prev queries) at the pose of slot j - 1
// and publishes the next pose into ps_out.
RingParams ring_params(const icp_ctx* c, const Ring& r, int j, int n_prev, PoseState* ps_out) {
    RingParams rp; memset(&rp, 0, sizeof(rp));
    rp.run_fault = r.run_fault;
    if (j > 0) {
        rp.n_red = NSUM_USED;
        rp.red_partials = ring_partials(c, j - 1); rp.red_nblocks = fused_nblocks(n_prev);
        rp.totals_row = r.trows + (size_t)(j - 1) * NSUM; rp.ps_in = loop_slot(r.slots, j - 1, 0); rp.ps_out = ps_out; rp.n_src = n_prev;
    }
    return rp;
}

// The tail of a run's result block: what lies behind the iteration records in c->stats, at the same offsets in the page-locked staging.
// Device code holds pointers into it (RingParams::final_out / run_fault, ConvergeParams::words / trace): no member may move.
struct RunTail {
    PoseState final_pose;                 // the pose state after the last iteration (merged form: written by its closing launch)
    int merged_fault, spare[3];           // the merged form's fault word; k_run_init clears it and the 15 words behind it
    int merged_cvg[12];                   // of which these serve as the merged form's convergence control words (CONV_*, dev_converge.hpp)
    char unused[64];
    int cvg_state[CONV_STATE_BYTES / 4];  // the separate form's convergence state block: control words | search pose | final pose state
    icp_convergence_step* trace() { return (icp_convergence_step*)(this + 1); }      // one step per iteration, behind the tail
    // the bytes in use with stopping on a converged pose (dev_converge.hpp): the whole tail and n_trace steps of the trace
    static constexpr size_t used_bytes(int n_trace) { return sizeof(RunTail) + (size_t)n_trace * sizeof(icp_convergence_step); }
};
static_assert(offsetof(RunTail, merged_fault) == 128 && offsetof(RunTail, merged_cvg) == 144 && offsetof(RunTail, unused) == 192 && offsetof(RunTail, cvg_state) == 256 && sizeof(RunTail) == 512, "the layout the device was handed");

// The merged form's time stamps (RingStamps, dev_solve.hpp) as the host sees them: t0[j] / t1[j] = start / end of launch j, j = 0 ..
// iters, launch `iters` being the closing one; ticks of the device's wall clock.
struct RunStamps {
    static size_t bytes(int iters) { return (size_t)2 * (iters + 1) * 8; }
    static unsigned long long* t0(void* base) { return (unsigned long long*)base; }
    static unsigned long long* t1(void* base, int iters) { return (unsigned long long*)base + (iters + 1); }
};
// Which iterations of a run of `iters` report their stage times: mode 0 none, 1 all, N > 1 every Nth, the offset rotating with `phase`
// (the context's run counter).
void sample_iterations(int mode, unsigned phase, int iters, std::vector<char>& sampled) {
    sampled.assign((size_t)iters, 0);
    for (int i = 0; i < iters; i++) sampled[(size_t)i] = mode == 1 || (mode > 1 && (i + (int)(phase % (unsigned)mode)) % mode == 0);
}
// The stamps of a merged run -> icp_timing and the per-iteration arrays (n_done entries each; any may be nullptr).  Pure host arithmetic:
// ticks become milliseconds at ticks_per_ms, the rate the runtime reports for the device.  An iteration IS one launch: match = its span,
// no post stage of its own (0), and a "solve" only behind the run's last iteration: the closing launch's span.  Only sampled iterations
// below n_done are reported (the others stay -1; a run that stopped early has real stamps up to n_done only); the sums are scaled by
// n_done / sampled.  total = the closing launch's end - the first launch's start, whatever the mode.
void stamps_to_timing(const unsigned long long* t0, const unsigned long long* t1, int iters, int n_done, const char* sampled, double ticks_per_ms,
                      icp_timing* t, float* match_ms, float* post_ms, float* solve_ms) {
    auto ms = [&](unsigned long long from, unsigned long long to) { return (double)(long long)(to - from) / ticks_per_ms; };
    memset(t, 0, sizeof(*t)); t->iterations = n_done;
    double sum_match = 0, sum_solve = 0; int n_ev = 0;
    for (int i = 0; i < n_done; i++) {
        float a = -1.f, b = -1.f, d = -1.f;
        if (sampled[i]) {
            n_ev++;
            a = (float)ms(t0[i], t1[i]); b = 0.f; d = i == iters - 1 ? (float)ms(t0[iters], t1[iters]) : 0.f;
            sum_match += a; sum_solve += d;
        }
        if (match_ms) match_ms[i] = a;
        if (post_ms) post_ms[i] = b;
        if (solve_ms) solve_ms[i] = d;
    }
    if (n_ev > 0) { const double f = (double)n_done / n_ev; t->match_ms = sum_match * f; t->solve_ms = sum_solve * f; }
    t->sampled_iterations = n_ev;
    t->total_ms = ms(t0[0], t1[iters]);
}

// What run_loop's prologue hands the form that enqueues the run.  lay_out places the run in the page-locked staging -- [pose state up |
// records down | tail down | trace down, runs that may stop | stamps down | LM records down, non-linear runs only], every part on a
// 256-byte boundary -- and sizes c->stats (records | tail | trace at the same distances: what the separate form copies back, and in
// either form the control words the device itself reads during the run); the accessors are the host's and the device's views of the parts.  Stage timing (TimeMeasure.h:20-26): mode N > 1 reports only every Nth iteration (`sampled`,
// offset rotating from run to run) and scales the sums.  The merged form takes its times from the device's clock (RunStamps): nothing on
// the stream, no cost to the run.  The separate form brackets with HIP events, each ~4 us of stream time: event slots 4 per iteration +
// run start / run end, and the form fills ev[i] of a sampled iteration with the ones it records.
// eligible[i] = the host's half of iteration i's eligibility to stop the run (cvg), from the plan's factors.
struct IterEvents { hipEvent_t start = nullptr, matched = nullptr, posted = nullptr, end = nullptr; };   // posted / end: nullptr = the form has no such stage to bracket
struct LoopRun {
    RunPlan pl; bool lm, robust, recip, rmse, fontana, cvg; std::vector<char> sampled, eligible; std::vector<IterEvents> ev; int n_enqueued = 0;
    bool stamp_blocks = false;           // merged form: the matcher blocks stamp their ends (any timing mode but 0)
    PoseState ps_in;                     // merged form: the incoming pose state, an argument of its first launch
    size_t pin_stats = 256, pin_tail, pin_stamps, pin_lm, pin_bytes, stats_bytes;      // offsets into the staging and its size; the size of c->stats
    void lay_out(int iters, bool with_lm, bool with_cvg) {
        auto pad = [](size_t b) { return (b + 255) & ~(size_t)255; };
        const size_t trace_pad = with_cvg ? pad((size_t)iters * sizeof(icp_convergence_step)) : 0;
        pin_tail = pin_stats + pad((size_t)iters * sizeof(icp_iter_stats)); pin_stamps = pin_tail + sizeof(RunTail) + trace_pad;
        pin_lm = pin_stamps + pad(RunStamps::bytes(iters));
        pin_bytes = pin_lm + (with_lm ? (size_t)iters * sizeof(icp_lm_summary) : 0);
        stats_bytes = pin_stamps - pin_stats;
    }
    size_t records_bytes() const { return pin_tail - pin_stats; }      // the records of every iteration, padded
    RunTail* dev_tail(const icp_ctx* c) const { return (RunTail*)(c->stats.as<char>() + records_bytes()); }
    icp_iter_stats* host_records(const icp_ctx* c) const { return (icp_iter_stats*)(c->pinned.as<char>() + pin_stats); }
    RunTail* host_tail(const icp_ctx* c) const { return (RunTail*)(c->pinned.as<char>() + pin_tail); }
    unsigned long long* host_stamps(const icp_ctx* c) const { return (unsigned long long*)(c->pinned.as<char>() + pin_stamps); }
    icp_lm_summary* host_lm(const icp_ctx* c) const { return (icp_lm_summary*)(c->pinned.as<char>() + pin_lm); }
};
// The separate form enqueues a run that may stop in chunks of this many iterations and reads the stop word between them: the chunk size
// trades host round trips against iterations enqueued in vain.  Time only, never results.  2: the fastest of {1, 2, 4, 8} on the bench
// pair with GICP (1.17 / 1.16 / 1.19 / 1.17 ms for a run that stops after 13 of 50 iterations; tools/time_converge.py).
#ifndef ICP_CONVERGE_CHUNK
#define ICP_CONVERGE_CHUNK 2
#endif
constexpr int CONVERGE_CHUNK = ICP_CONVERGE_CHUNK;
ConvergeParams converge_params(const icp_ctx* c, const LoopRun& r, int i, int* words, icp_convergence_step* trace) {
    ConvergeParams cp; memset(&cp, 0, sizeof(cp));
    if (!r.cvg) return cp;
    const icp_convergence_options& o = c->cvg_opt;
    cp.on = 1; cp.eligible = r.eligible[(size_t)i]; cp.index = i; cp.min_iterations = o.min_iterations; cp.patience = o.patience;
    cp.rotation_eps = o.rotation_eps; cp.translation_eps = o.translation_eps;
    cp.trace = trace; cp.words = words;
    return cp;
}
hipEvent_t loop_event(const icp_ctx* c, int i, int k) { return c->events[(size_t)2 + 4 * i + k]; }      // the separate form's

// The merged form: point-to-plane through the fused BVH matcher on sorted levels, nothing else on the stream between two iterations.
// Launch i = [reducer of iteration i - 1 | matcher of iteration i]; one reducer-only launch closes the run.  A run that stops on a converged
// pose (dev_converge.hpp) is still enqueued whole: the launches behind the stop find a stopped slot and drain at launch cost.  Pose slots and totals rows
// are written once per run; both rings are reset here, so nothing survives an aborted run.
// Nothing but launches goes on the stream.  In: the incoming pose state (r.ps_in) is an argument of k_run_init, which also leaves it in
// c->ps.  Out: the result block -- records | final pose state | fault and convergence words | trace | stamps -- is written by the
// launches straight into the page-locked staging, which the device addresses (c->pinned.dev): what only the host reads (records, trace
// steps, final pose state, stamps) by the launch that produces it; the control words the device itself reads stay in c->stats, and the
// closing launch copies them over as its last act.  The host reads the block behind run_loop's hipStreamSynchronize.
// Stage times: the launches stamp the device's clock themselves (RingStamps, dev_solve.hpp) -- no event, no bracket on the stream; the
// launch starts and the run's end in every mode (total_ms), the matcher blocks' ends in every mode but 0.
int enqueue_merged(icp_ctx* c, LoopRun& r) {
    const icp_params& p = c->prm; const RunPlan& pl = r.pl;
    const int iters = pl.iters(); RunTail* tail = r.dev_tail(c);
    int rc, nbmax = POST_BLOCKS;
    for (int i = 0; i < iters; i++) { const int nb = fused_nblocks(pl.ns[i]); if (nb > nbmax) nbmax = nb; }
    Ring ring;
    if ((rc = make_ring(c, iters + 1, iters, nbmax, &tail->merged_fault, ring))) return rc;
    if (r.stamp_blocks && (rc = ensure(c, c->block_t1, (size_t)2 * nbmax * 8))) return rc;
    if ((rc = ensure(c, c->ps, sizeof(PoseState)))) return rc;
    char* out = (char*)c->pinned.dev;                    // the result block as the device addresses it: the offsets of lay_out
    icp_iter_stats* out_records = (icp_iter_stats*)(out + r.pin_stats); RunTail* out_tail = (RunTail*)(out + r.pin_tail);
    unsigned long long* stamps = (unsigned long long*)(out + r.pin_stamps);
    unsigned long long* t0 = RunStamps::t0(stamps); unsigned long long* t1 = RunStamps::t1(stamps, iters);
    auto block_t1 = [&](int j) { return r.stamp_blocks ? c->block_t1.as<unsigned long long>() + (size_t)(j & 1) * nbmax : nullptr; };
    const int n_stamps = 2 * (iters + 1), n_init = (iters + 1) * POSE_REPLICAS * 16 + iters * NSUM + 16 + n_stamps;
    hipLaunchKernelGGL(k_run_init, dim3((n_init + 255) / 256), dim3(256), 0, c->stream, r.ps_in, c->ps.as<PoseState>(), ring.slots, iters + 1, ring.trows, iters * NSUM, ring.run_fault, 16, stamps, n_stamps);
    auto reducer = [&](int i) {                          // of iteration i - 1, riding in launch i (i = iters: the closing launch)
        RingParams rp = ring_params(c, ring, i, i > 0 ? pl.ns[i - 1] : 0, loop_slot(ring.slots, i, 0));
        if (i > 0) { rp.stats = out_records + (i - 1); rp.cv = converge_params(c, r, i - 1, tail->merged_cvg, out_tail->trace()); }
        rp.st.t0 = t0 + i;
        if (i < iters) rp.st.block_t1 = block_t1(i);
        if (i > 0 && r.stamp_blocks) { rp.st.prev_block_t1 = block_t1(i - 1); rp.st.prev_t1 = t1 + (i - 1); }
        if (i == iters) { rp.final_out = &out_tail->final_pose; rp.words_out = &out_tail->merged_fault; rp.st.end = t1 + iters; }
        return rp;
    };
    for (int i = 0; i < iters; i++) {
        QuerySet q{pl.clouds[i], pl.sels[i], pl.ns[i], 0, p.color_icp != 0 && p.matching == ICP_MATCH_KNN, pl.seeded(i), pl.orders[i]};
        MergeLaunch ml; ml.rp = reducer(i); ml.slot = loop_slot(ring.slots, i, 0); ml.partials = ring_partials(c, i);
        int fused = 0;
        if ((rc = launch_match(c, q, &fused, &ml))) return rc;
        if (!fused) { c->err = "merged loop: the matcher did not take the fused path"; return ICP_ERR_HIP; }
    }
    hipLaunchKernelGGL(k_ring_reduce_solve, dim3(NSUM_USED), dim3(RING_THREADS), 0, c->stream, reducer(iters));      // nothing behind the last iteration to ride in
    HIPCK(c, hipGetLastError());
    r.n_enqueued = iters;
    return ICP_OK;
}

// The separate form, which every configuration can take: per iteration the matcher (its post stage fused where the matcher can), then
// the post stage and the reduce / solve -- or the robust chain in front, or the non-linear optimiser behind -- and the convergence
// measures.  Back come the records, the pose state and the LM records.  Events: slot 0 in front of the matcher, 1 behind it, 2 behind a
// post stage of its own (none behind a fused matcher), 3 at the iteration's end; the matcher's time counts from the previous iteration's
// slot 3 when that one was sampled.  Stopping on a converged pose: k_converge_step closes every iteration, and the iterations go out in
// chunks of CONVERGE_CHUNK with one 4-byte read of the stop word between two chunks; with the option off the sequence is unchanged.
int enqueue_separate(icp_ctx* c, LoopRun& r) {
    const icp_params& p = c->prm; const RunPlan& pl = r.pl;
    const int iters = pl.iters(); int rc;
    if ((rc = rearm_handover(c))) return rc;
    RunTail* tail = r.dev_tail(c); RunTail* htail = r.host_tail(c);
    if (r.cvg) {
        hipLaunchKernelGGL(k_converge_init, dim3(1), dim3(64), 0, c->stream, c->ps.as<PoseState>(), tail->cvg_state);
        HIPCK(c, hipGetLastError());
    }
    HIPCK(c, hipEventRecord(c->events[0], c->stream));
    int n_enq = 0;
    for (int i = 0; i < iters; i++) {
        if (r.cvg && i > 0 && i % CONVERGE_CHUNK == 0) {      // between two chunks: has the run stopped?
            const int* stop = &htail->cvg_state[CONV_STOPPED];
            HIPCK(c, hipMemcpyAsync((void*)stop, &tail->cvg_state[CONV_STOPPED], 4, hipMemcpyDeviceToHost, c->stream));
            HIPCK(c, hipStreamSynchronize(c->stream));
            if (*stop) break;
        }
        n_enq = i + 1;
        icp_iter_stats* d_st = c->stats.as<icp_iter_stats>() + i;
        const bool ev = r.sampled[i] != 0;
        if (ev) {
            r.ev[i].start = (i > 0 && r.sampled[i - 1]) ? loop_event(c, i - 1, 3) : loop_event(c, i, 0);
            r.ev[i].matched = loop_event(c, i, 1); r.ev[i].end = loop_event(c, i, 3);
            HIPCK(c, hipEventRecord(loop_event(c, i, 0), c->stream));
        }
        if (pl.ns[i] > 0) {
            // (keep_records: the fused matcher writes its records for k_lm_eval)
            QuerySet q{pl.clouds[i], pl.sels[i], pl.ns[i], 0, p.color_icp != 0 && p.matching == ICP_MATCH_KNN, pl.seeded(i), pl.orders[i], r.lm};
            int fused = 0;
            if ((rc = launch_match(c, q, !r.robust && !r.recip ? &fused : nullptr))) return rc;
            if (r.recip && (rc = launch_reciprocal(c, q, c->rcp_stats.as<icp_reciprocal_stats>() + i))) return rc;      // in front of the robust chain
            if (ev) HIPCK(c, hipEventRecord(r.ev[i].matched, c->stream));
            if (ev && !fused) r.ev[i].posted = loop_event(c, i, 2);      // fused epilogue: there is no separate post stage to bracket
            if (r.lm) rc = launch_post_and_lm(c, *pl.clouds[i], pl.sels[i], pl.ns[i], d_st, c->lm_sums.as<icp_lm_summary>() + i, r.ev[i].posted, fused);
            else rc = launch_post_and_solve(c, *pl.clouds[i], pl.sels[i], pl.ns[i], d_st, nullptr, 1, r.ev[i].posted, fused, r.robust ? c->rob_stats.as<icp_robust_stats>() + i : nullptr);
            if (rc) return rc;
        } else if (ev) HIPCK(c, hipEventRecord(r.ev[i].matched, c->stream));
        if (r.rmse && (rc = enqueue_rmse(c, &d_st->rmse))) return rc;
        if (r.fontana && (rc = enqueue_fontana(c, &d_st->benchmark_error))) return rc;
        if (r.cvg) {
            hipLaunchKernelGGL(k_converge_step, dim3(1), dim3(64), 0, c->stream, converge_params(c, r, i, tail->cvg_state, tail->trace()), c->ps.as<PoseState>(), pl.ns[i] > 0 ? d_st : nullptr);
            HIPCK(c, hipGetLastError());
        }
        if (ev) HIPCK(c, hipEventRecord(r.ev[i].end, c->stream));
    }
    r.n_enqueued = n_enq;
    HIPCK(c, hipEventRecord(c->events[1], c->stream));
    HIPCK(c, hipMemcpyAsync(r.host_records(c), c->stats.p, (size_t)n_enq * sizeof(icp_iter_stats), hipMemcpyDeviceToHost, c->stream));
    HIPCK(c, hipMemcpyAsync(&htail->final_pose, c->ps.p, sizeof(PoseState), hipMemcpyDeviceToHost, c->stream));
    if (r.cvg) HIPCK(c, hipMemcpyAsync(htail->cvg_state, tail->cvg_state, RunTail::used_bytes(n_enq) - offsetof(RunTail, cvg_state), hipMemcpyDeviceToHost, c->stream));      // the state block and the trace behind it
    if (r.lm) HIPCK(c, hipMemcpyAsync(r.host_lm(c), c->lm_sums.p, (size_t)n_enq * sizeof(icp_lm_summary), hipMemcpyDeviceToHost, c->stream));
    return ICP_OK;
}

// try_merged: take the merged form when the configuration allows it (the context's merge_loop; false when a merged run has given up).
int run_loop(icp_ctx* c, float pose_inout[16], icp_iter_stats* stats, int32_t max_stats, int32_t* n_run, bool single, bool try_merged) {
    const icp_params& p = c->prm;
    int rc;
    DrainOnError guard(c);
    if ((rc = set_device(c))) return rc;
    if ((rc = check_ready(c, true, true))) return rc;
    if ((rc = gicp_prepare(c))) return rc;
    if ((rc = colored_prepare(c))) return rc;
    LoopRun r{};
    const RunPlan& pl = r.pl;
    if ((rc = make_plan(c, single, r.pl))) return rc;
    const int iters = pl.iters();
    if (n_run) *n_run = 0;
    const bool lm = r.lm = c->lm_on;      // the non-linear optimiser: the separate form, its records kept for k_lm_eval
    const bool robust = r.robust = robust_on(c);      // trimmed / robust mode: the separate form with the stand-alone matcher, as GICP runs
    const bool recip = r.recip = reciprocal_on(c);      // reciprocal rejection: the same form, k_reciprocal between the matcher and the post stage
    c->lm_last.clear(); c->rob_last.clear(); c->rcp_last.clear();
    const bool cvg = r.cvg = !single && c->cvg_opt.enabled != 0;      // icp_iterate ignores the option and leaves the last run's result alone
    if (!single) { c->cvg_trace.clear(); c->cvg_last = icp_convergence_result{0, 0, iters, -1.f, -1.f}; }
    if (robust && lm) { c->err = "the non-linear optimiser does not support robust mode (icp_set_robust_options)"; return ICP_ERR_INVALID_ARG; }
    if (recip && (rc = reciprocal_check(c))) return rc;
    if (iters == 0) return guard.done();
    if (robust && (rc = robust_prepare(c, iters))) return rc;
    if (recip && (rc = reciprocal_prepare(c, iters))) return rc;
    r.lay_out(iters, lm, cvg);
    if ((rc = ensure_pinned(c, r.pin_bytes))) return rc;
    if (lm && (rc = ensure(c, c->lm_sums, (size_t)iters * sizeof(icp_lm_summary)))) return rc;
    float pose_in[16]; memcpy(pose_in, pose_inout, 64);        // the record of an empty iteration 0 carries the incoming pose
    if ((rc = ensure(c, c->stats, r.stats_bytes))) return rc;
    r.eligible.assign((size_t)iters, 0);
    for (int i = 0; i < iters; i++) r.eligible[(size_t)i] = pl.factors[i] == pl.factors[iters - 1] && (i == 0 || pl.factors[i] == pl.factors[i - 1]);
    const bool rmse = r.rmse = (p.record_rmse & 1) && c->conv_n > 0;
    const bool fontana = r.fontana = (p.record_rmse & 2) && c->conv_n > 0;
    bool merged = try_merged && !lm && !robust && !recip && !single && iters >= 2 && pl.sorted_levels && p.metric == ICP_METRIC_POINT_TO_PLANE && !rmse && !fontana;
    for (int i = 0; merged && i < iters; i++) if (pl.ns[i] <= 0) merged = false;
    sample_iterations(c->stage_timing, c->timing_phase++, iters, r.sampled);
    r.stamp_blocks = c->stage_timing != 0;
    if (merged) make_pose_state(pose_inout, &r.ps_in);    // (travels with the first launch)
    else if ((rc = write_pose(c, pose_inout))) return rc;
    if (merged) {
        if (c->wall_ticks_per_ms <= 0) { int khz = 0; HIPCK(c, hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, c->device)); c->wall_ticks_per_ms = khz; }
        if (c->wall_ticks_per_ms <= 0) { c->err = "the runtime reports no wall clock rate for the device"; return ICP_ERR_HIP; }
    } else { r.ev.assign((size_t)iters, IterEvents()); if ((rc = ensure_events(c, (size_t)iters * 4 + 2))) return rc; }
    if ((rc = merged ? enqueue_merged(c, r) : enqueue_separate(c, r))) return rc;
    std::vector<icp_robust_stats> rob((size_t)(robust ? iters : 0));
    if (robust) HIPCK(c, hipMemcpyAsync(rob.data(), c->rob_stats.p, (size_t)iters * sizeof(icp_robust_stats), hipMemcpyDeviceToHost, c->stream));
    std::vector<icp_reciprocal_stats> rcp((size_t)(recip ? iters : 0));      // (an iteration without work keeps the {0, 0} of reciprocal_prepare)
    if (recip) HIPCK(c, hipMemcpyAsync(rcp.data(), c->rcp_stats.p, (size_t)iters * sizeof(icp_reciprocal_stats), hipMemcpyDeviceToHost, c->stream));
    HIPCK(c, hipStreamSynchronize(c->stream));
    c->rcp_last.swap(rcp);
    for (int i = 0; robust && i < iters; i++) if (pl.ns[i] <= 0) rob[(size_t)i] = icp_robust_stats{0, 0, -1.f, -1.f};      // (no work: nothing was written)
    c->rob_last.swap(rob);
    RunTail* htail = r.host_tail(c);
    const PoseState* hp = &htail->final_pose;
    if (merged) {
        c->merged_runs++;
        const int rf = htail->merged_fault;
        if ((hp->fault && hp->fault != SLOT_STOPPED) || rf) {      // (a stopped slot is the run's result, not a fault)
            // the 6 x 6 system failed the rank guard (the eigen-decomposition lives in k_reduce_solve only), or a bounded wait ran out:
            // the same run again, from the incoming pose, in the separate form
            c->merged_fallbacks++;
            if (c->trace) fprintf(stderr, "[icp_hip] merged loop gave up: slot fault %d, abort word %d -> the run again with separate launches\n", hp->fault, rf);
            guard.ok = true;                                 // synchronised
            memcpy(pose_inout, pose_in, 64);
            return run_loop(c, pose_inout, stats, max_stats, n_run, single, false);
        }
    }
    int n_done = iters; bool stopped = false;
    if (cvg) {
        const int* cw = merged ? htail->merged_cvg : htail->cvg_state;
        if (cw[CONV_STOPPED]) {
            stopped = true; n_done = cw[CONV_RUN];
            if (n_done < 1 || n_done > r.n_enqueued) { c->err = "the device reports a stop outside the iterations that were enqueued"; return ICP_ERR_HIP; }
            if (!merged) hp = (const PoseState*)(cw + CONV_FINAL);      // c->ps has moved on with the iterations enqueued behind the stop
        }
    }
    memcpy(pose_inout, hp->pose, 64);
    if (!merged && hp->fault) { c->err = "reduction hand-over timed out on the device (k_reduce_solve)"; return ICP_ERR_HIP; }
    if (lm) {
        c->lm_last.resize((size_t)n_done);
        memcpy(c->lm_last.data(), r.host_lm(c), (size_t)n_done * sizeof(icp_lm_summary));
        for (int i = 0; i < n_done; i++)
            if (pl.ns[i] <= 0) { memset(&c->lm_last[(size_t)i], 0, sizeof(icp_lm_summary)); c->lm_last[(size_t)i].termination = ICP_LM_NO_RESIDUALS; }
    }
    if (robust) c->rob_last.resize((size_t)n_done);
    if (recip) c->rcp_last.resize((size_t)n_done);
    const int status = finish_records(pl, n_done, r.host_records(c), pose_in, rmse, fontana, stats, max_stats);
    if (n_run) *n_run = n_done;
    if (!single) { c->cvg_last.converged = stopped; c->cvg_last.iterations_run = n_done; }
    if (cvg) {
        const icp_convergence_step* tr = htail->trace();
        c->cvg_trace.assign(tr, tr + n_done);
        c->cvg_last.rotation = tr[n_done - 1].rotation; c->cvg_last.translation = tr[n_done - 1].translation;
    }
    icp_timing& t = c->timing; memset(&t, 0, sizeof(t)); t.iterations = n_done;
    c->it_match_ms.assign((size_t)n_done, -1.f); c->it_post_ms.assign((size_t)n_done, -1.f); c->it_solve_ms.assign((size_t)n_done, -1.f);
    if (merged) {                                         // the device's clock: the stamps lie in the result block
        unsigned long long* hst = r.host_stamps(c);
        stamps_to_timing(RunStamps::t0(hst), RunStamps::t1(hst, iters), iters, n_done, r.sampled.data(), c->wall_ticks_per_ms, &t, c->it_match_ms.data(), c->it_post_ms.data(), c->it_solve_ms.data());
        for (int i = 0; c->trace && i < n_done; i++)
            if (r.sampled[i]) fprintf(stderr, "[icp_hip] it %2d  n %d  match %.4f  post %.4f  solve %.4f ms\n", i, pl.ns[i], c->it_match_ms[(size_t)i], c->it_post_ms[(size_t)i], c->it_solve_ms[(size_t)i]);
    } else {
        double ev_match = 0, ev_post = 0, ev_solve = 0; int n_ev = 0;
        for (int i = 0; i < n_done; i++) {
            if (!r.sampled[i]) continue;
            n_ev++;
            const IterEvents& e = r.ev[i];
            float a = 0, b = 0, d = 0;
            HIPCK(c, hipEventElapsedTime(&a, e.start, e.matched));
            if (e.posted) HIPCK(c, hipEventElapsedTime(&b, e.matched, e.posted));
            if (e.end) HIPCK(c, hipEventElapsedTime(&d, e.posted ? e.posted : e.matched, e.end));
            ev_match += a; ev_post += b; ev_solve += d;
            c->it_match_ms[(size_t)i] = a; c->it_post_ms[(size_t)i] = b; c->it_solve_ms[(size_t)i] = d;
            if (c->trace) fprintf(stderr, "[icp_hip] it %2d  n %d  match %.4f  post %.4f  solve %.4f ms\n", i, pl.ns[i], a, b, d);
        }
        if (n_ev > 0) {                                   // sampled: scale to all the iterations
            const double f = (double)n_done / n_ev;
            t.match_ms += ev_match * f; t.weight_reject_build_ms += ev_post * f; t.solve_ms += ev_solve * f;
        }
        t.sampled_iterations = n_ev;
        float tot = 0; HIPCK(c, hipEventElapsedTime(&tot, c->events[0], c->events[1])); t.total_ms = tot;
    }
    if (status != ICP_OK) c->err = "no valid correspondences in at least one iteration (reference would hang in ASSERT)";
    guard.ok = true;                                     // synchronised above; `status` reports empty iterations, not a HIP failure
    return status;
}
}  // namespace

// Iteration schedule of LinearICPOptimizer::estimatePose: ICPOptimizer.h:503-516 (coarsest level),
// :540 (loop condition `i < nIter || multires`) and :634-655 (refinement).  Pure host logic.
int icp_schedule(const icp_params* p, int32_t n_src, int32_t* factors_out, int32_t max_out, int32_t* count_out) {
    if (!p || !count_out || n_src < 0) return ICP_ERR_INVALID_ARG;
    int cnt = 0;
    if (!p->multires) {
        for (int i = 0; i < p->n_iterations; i++) { if (factors_out && cnt < max_out) factors_out[cnt] = 0; cnt++; }
    } else {
        if (p->n_iterations < 1) return ICP_ERR_INVALID_ARG;     // `i >= m_nIterations - 1` is unsigned in the reference: never true
        float res = 1.0f; int osz = n_src;
        while (1) { osz = (int)(osz / 2.0); if (osz < 100) break; res *= 2.0f; }      // MULTI_RESOLUTION_MINIMUM_POINTS :21
        for (int i = 0;; ++i) {
            if (factors_out && cnt < max_out) factors_out[cnt] = (int)res;
            cnt++;
            if (res == 1.0f && i >= p->n_iterations - 1) break;
            if (res == 1.0f) continue;
            res /= 2.0f; if (res < 1.0f) res = 1.0f;
        }
    }
    *count_out = cnt;
    return ICP_OK;
}

int icp_iterate(icp_ctx* c, float pose_inout[16], icp_iter_stats* stats) {
    if (!c || !pose_inout) { if (c) c->err = "icp_iterate: bad argument"; return ICP_ERR_INVALID_ARG; }
    return run_loop(c, pose_inout, stats, stats ? 1 : 0, nullptr, true, c->merge_loop);
}

int icp_run(icp_ctx* c, float pose_inout[16], icp_iter_stats* stats, int32_t max_stats, int32_t* n_iterations_run) {
    if (!c || !pose_inout) { if (c) c->err = "icp_run: bad argument"; return ICP_ERR_INVALID_ARG; }
    return run_loop(c, pose_inout, stats, stats ? max_stats : 0, n_iterations_run, false, c->merge_loop);
}

int icp_query_matches(icp_ctx* c, const float* transformed_xyz, const uint8_t* rgba, int32_t n, icp_match_t* out) {
    if (!c || !transformed_xyz || !out || n <= 0) { if (c) c->err = "icp_query_matches: bad argument"; return ICP_ERR_INVALID_ARG; }
    int rc;
    DrainOnError guard(c);
    if ((rc = set_device(c))) return rc;
    if ((rc = check_ready(c, false, false))) return rc;
    const bool colors = rgba != nullptr;
    if (c->prm.matching == ICP_MATCH_KNN && colors && !c->tgt.has_colors) {      // NearestNeighbor.h:240-243
        c->err = "index built without colours: call queryMatches without colours";
        return ICP_ERR_COLOR_MISMATCH;
    }
    if ((rc = upload_cloud(c, c->qry, transformed_xyz, nullptr, rgba, n, false))) return rc;
    QuerySet q{&c->qry, nullptr, n, 1, colors && c->prm.matching == ICP_MATCH_KNN, false, nullptr};
    if ((rc = launch_match(c, q))) return rc;
    HIPCK(c, hipMemcpyAsync(out, c->matches.p, (size_t)n * sizeof(icp_match_t), hipMemcpyDeviceToHost, c->stream));
    HIPCK(c, hipStreamSynchronize(c->stream));
    return guard.done();
}

int icp_match(icp_ctx* c, const float pose[16], icp_match_t* out, float* d2_out) {
    if (!c || !pose || !out) { if (c) c->err = "icp_match_t: bad argument"; return ICP_ERR_INVALID_ARG; }
    int rc;
    DrainOnError guard(c);
    if ((rc = set_device(c))) return rc;
    if ((rc = check_ready(c, true, false))) return rc;
    if ((rc = write_pose(c, pose))) return rc;
    const int* full_order = nullptr;
    if ((rc = get_full_order(c, &full_order))) return rc;
    QuerySet q{&c->src, nullptr, c->src.n, 0, c->prm.color_icp != 0 && c->prm.matching == ICP_MATCH_KNN, false, full_order};
    if ((rc = launch_match(c, q))) return rc;
    HIPCK(c, hipMemcpyAsync(out, c->matches.p, (size_t)q.n * sizeof(icp_match_t), hipMemcpyDeviceToHost, c->stream));
    if (d2_out) HIPCK(c, hipMemcpyAsync(d2_out, c->d2.p, (size_t)q.n * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCK(c, hipStreamSynchronize(c->stream));
    return guard.done();
}

int icp_correspond(icp_ctx* c, const float pose[16], icp_match_t* out, double* sums_out, int32_t* n_valid_out) {
    if (!c || !pose) { if (c) c->err = "icp_correspond: bad argument"; return ICP_ERR_INVALID_ARG; }
    int rc;
    DrainOnError guard(c);
    if ((rc = set_device(c))) return rc;
    if ((rc = check_ready(c, true, true))) return rc;
    if ((rc = gicp_prepare(c))) return rc;
    if ((rc = colored_prepare(c))) return rc;
    const bool robust = robust_on(c);
    const bool recip = reciprocal_on(c);
    c->rob_last.clear(); c->rcp_last.clear();
    if (recip && (rc = reciprocal_check(c))) return rc;
    if (robust && (rc = robust_prepare(c, 1))) return rc;
    if (recip && (rc = reciprocal_prepare(c, 1))) return rc;
    if ((rc = write_pose(c, pose))) return rc;
    const int* full_order = nullptr;
    if ((rc = get_full_order(c, &full_order))) return rc;
    QuerySet q{&c->src, nullptr, c->src.n, 0, c->prm.color_icp != 0 && c->prm.matching == ICP_MATCH_KNN, false, full_order};
    if ((rc = launch_match(c, q))) return rc;
    if (recip && (rc = launch_reciprocal(c, q, c->rcp_stats.as<icp_reciprocal_stats>()))) return rc;
    if ((rc = ensure(c, c->sums, NSUM * 8))) return rc;
    if ((rc = rearm_handover(c))) return rc;
    if ((rc = launch_post_and_solve(c, c->src, nullptr, q.n, nullptr, c->sums.as<double>(), 0, nullptr, 0, robust ? c->rob_stats.as<icp_robust_stats>() : nullptr))) return rc;
    double hs[NSUM]; int fault = 0;
    icp_robust_stats rs; icp_reciprocal_stats rcs;
    if (out) HIPCK(c, hipMemcpyAsync(out, c->matches.p, (size_t)q.n * sizeof(icp_match_t), hipMemcpyDeviceToHost, c->stream));
    HIPCK(c, hipMemcpyAsync(hs, c->sums.p, NSUM * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCK(c, hipMemcpyAsync(&fault, &c->ps.as<PoseState>()->fault, 4, hipMemcpyDeviceToHost, c->stream));
    if (robust) HIPCK(c, hipMemcpyAsync(&rs, c->rob_stats.p, sizeof(rs), hipMemcpyDeviceToHost, c->stream));
    if (recip) HIPCK(c, hipMemcpyAsync(&rcs, c->rcp_stats.p, sizeof(rcs), hipMemcpyDeviceToHost, c->stream));
    HIPCK(c, hipStreamSynchronize(c->stream));
    if (robust) c->rob_last.assign(1, rs);
    if (recip) c->rcp_last.assign(1, rcs);
    if (fault) { c->err = "reduction hand-over timed out on the device (k_reduce_solve)"; return ICP_ERR_HIP; }
    if (sums_out) { memset(sums_out, 0, 64 * 8); memcpy(sums_out, hs, NSUM * 8); }
    if (n_valid_out) *n_valid_out = (int32_t)hs[SUM_N];
    return guard.done();
}

// The fused matcher driven launch by launch with caller-dictated poses: launch 0 unseeded, launch j > 0 seeded + incremental exactly
// as iteration j of icp_run runs it, in the form icp_run takes for the configuration (the merged ring launches or the separate
// launches: same kernel, same buffers, same grid); the last launch's records come back in source order.
int icp_match_seeded(icp_ctx* c, const float* poses, int32_t n_poses, icp_match_t* out, float* d2_out) {
    if (!c || !poses || n_poses <= 0) { if (c) c->err = "icp_match_seeded: bad argument"; return ICP_ERR_INVALID_ARG; }
    const icp_params& p = c->prm;
    if (p.metric == ICP_METRIC_GICP) { c->err = "icp_match_seeded: GICP has no fused matcher"; return ICP_ERR_INVALID_ARG; }
    if (p.metric == ICP_METRIC_COLORED) { c->err = "icp_match_seeded: colored ICP has no fused matcher"; return ICP_ERR_INVALID_ARG; }
    if (robust_on(c)) { c->err = "icp_match_seeded: robust mode (icp_set_robust_options) has no fused matcher"; return ICP_ERR_INVALID_ARG; }
    if (reciprocal_on(c)) { c->err = "icp_match_seeded: reciprocal rejection (icp_set_reciprocal_options) has no fused matcher"; return ICP_ERR_INVALID_ARG; }
    if (p.matching != ICP_MATCH_KNN || p.knn_backend != ICP_KNN_LBVH || p.metric == ICP_METRIC_SYMMETRIC) {
        c->err = "icp_match_seeded: needs k-NN matching on the LBVH backend with the fused point-to-point / point-to-plane matcher"; return ICP_ERR_INVALID_ARG;
    }
    int rc;
    DrainOnError guard(c);
    if ((rc = set_device(c))) return rc;
    if ((rc = check_ready(c, true, true))) return rc;
    const Cloud* cloud = nullptr; int n = 0;
    if ((rc = get_sorted_level(c, 0, &cloud, &n))) return rc;
    // ring: what run_loop launches for this configuration one launch per iteration (the merged loop, dev_solve.hpp "the ring form"):
    // k_knn_bvh_post_ring, launch j > 0 with the reducer of launch j - 1 in its first NSUM_USED blocks and the matcher blocks behind them.
    // Every matcher waits on slot j, filled here up front with the caller's pose j; the reducers fold the previous launch's partials
    // (the same ring as run_loop's) and publish into a scratch slot nobody waits on.  Otherwise (point-to-point, ICP_HIP_MERGE=0):
    // the separate k_knn_bvh_post launches, each at the pose written in front of it.
    const bool ring = c->merge_loop && !c->lm_on && p.metric == ICP_METRIC_POINT_TO_PLANE;
    std::vector<unsigned long long> slot_image;              // (read by the copy below until the synchronisation at the end)
    Ring rg{nullptr, nullptr, nullptr, 0};
    if (ring) {
        const int nb = fused_nblocks(n), n_rows = n_poses > 1 ? n_poses - 1 : 1;    // totals rows: one per reduced launch
        if ((rc = make_ring(c, n_poses + 1, n_rows, nb > POST_BLOCKS ? nb : POST_BLOCKS, nullptr, rg))) return rc;
        // slots 0 .. n_poses - 1 in every replica, encoded as the reducer publishes a slot (16 granules of PoseState, fault word zero);
        // slot n_poses, the reducers' scratch, starts empty
        slot_image.assign(rg.slot_bytes / 8, GRANULE_EMPTY);
        for (int j = 0; j < n_poses; j++) {
            PoseState ps; memset(&ps, 0, sizeof(ps)); memcpy(ps.pose, poses + (size_t)16 * j, 64); normal_matrix_from_pose(ps.pose, ps.nmat);
            const unsigned long long* g = (const unsigned long long*)&ps;
            for (int r = 0; r < POSE_REPLICAS; r++)
                for (int q = 0; q < 16; q++)
                    slot_image[((size_t)j * POSE_REPLICAS + r) * (POSE_REPLICA_STRIDE / 8) + q] = g[q] == GRANULE_EMPTY ? g[q] ^ 1ull : g[q];
        }
        HIPCK(c, hipMemcpyAsync(rg.slots, slot_image.data(), rg.slot_bytes, hipMemcpyHostToDevice, c->stream));
        const int n_init = n_rows * NSUM + 16;               // the totals rows empty, the fault word zero (k_run_init without its pose slots)
        hipLaunchKernelGGL(k_run_init, dim3((n_init + 255) / 256), dim3(256), 0, c->stream, PoseState{}, nullptr, rg.slots, 0, rg.trows, n_rows * NSUM, rg.run_fault, 16, nullptr, 0);      // (no pose slots: the argument is not read)
        HIPCK(c, hipGetLastError());
    }
    for (int j = 0; j < n_poses; j++) {
        if (!ring && (rc = write_pose(c, poses + (size_t)16 * j))) return rc;
        QuerySet q{cloud, nullptr, n, 0, p.color_icp != 0, j > 0, nullptr, j == n_poses - 1};      // (only the last launch's records are read)
        MergeLaunch ml; memset(&ml.rp, 0, sizeof(ml.rp)); ml.slot = nullptr; ml.partials = nullptr;
        if (ring) {                                          // the reducer's pose goes to the scratch slot
            ml.rp = ring_params(c, rg, j, n, loop_slot(rg.slots, n_poses, 0));
            ml.slot = loop_slot(rg.slots, j, 0); ml.partials = ring_partials(c, j);
        }
        int fused = 0;
        if ((rc = launch_match(c, q, &fused, ring ? &ml : nullptr))) return rc;
        if (!fused) { c->err = "icp_match_seeded: the matcher did not take the fused path"; return ICP_ERR_INVALID_ARG; }
        if (!ring) {
            int hf = 0;
            HIPCK(c, hipMemcpyAsync(&hf, &c->ps.as<PoseState>()->fault, 4, hipMemcpyDeviceToHost, c->stream));
            HIPCK(c, hipStreamSynchronize(c->stream));       // the pose staging area is reused by the next launch
            if (hf) { c->err = "icp_match_seeded: a bounded wait of the matcher ran out (k_knn_bvh_post)"; return ICP_ERR_HIP; }
        }
    }
    if (ring) {
        int hf = 0;
        HIPCK(c, hipMemcpyAsync(&hf, rg.run_fault, 4, hipMemcpyDeviceToHost, c->stream));
        HIPCK(c, hipStreamSynchronize(c->stream));
        if (hf) { c->err = "icp_match_seeded: a bounded wait of the merged launches ran out (k_knn_bvh_post_ring)"; return ICP_ERR_HIP; }
    }
    std::vector<int> pos((size_t)n); std::vector<icp_match_t> m((size_t)n); std::vector<float> d((size_t)n);
    HIPCK(c, hipMemcpyAsync(pos.data(), c->levels[0].sorted_idx.p, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCK(c, hipMemcpyAsync(m.data(), c->matches.p, (size_t)n * sizeof(icp_match_t), hipMemcpyDeviceToHost, c->stream));
    HIPCK(c, hipMemcpyAsync(d.data(), c->d2.p, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCK(c, hipStreamSynchronize(c->stream));
    for (int t = 0; t < n; t++) {                            // sorted position -> source index
        if (out) out[pos[(size_t)t]] = m[(size_t)t];
        if (d2_out) d2_out[pos[(size_t)t]] = d[(size_t)t];
    }
    return guard.done();
}
