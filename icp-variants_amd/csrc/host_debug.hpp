// host_debug.hpp -- development and test hooks that are not part of icp_hip.h (tests/ and tools/ call them through ctypes): icp_debug_*,
// the hardware self test, and the one kernel they own (k_debug_pos_of).  Part of icp_hip.hip (included from there, last).
extern "C" {
// Development builds (ICP_DEBUG_STEPS=1): how each query of the LAST matcher launch was resolved, in the order the launch indexed its
// queries (Morton order for a run): 0 = verified without a walk, -2 = second tier (two leaves), -1 = a walk (a walk shared over the wave
// has no per-query length); with ICP_DEBUG_TIMES=1 the buffer holds per-wave phase stamps instead (tools/dev_wave_times.py).
int icp_debug_steps(icp_ctx* c, int32_t* out, int32_t n) {
    if (!c || !out || n <= 0 || !c->dbg_steps.p || (size_t)n * 4 > c->dbg_steps.cap) return ICP_ERR_INVALID_ARG;
    int rc;
    if ((rc = set_device(c))) return rc;
    HIPCK(c, hipMemcpy(out, c->dbg_steps.p, (size_t)n * 4, hipMemcpyDeviceToHost));
    return ICP_OK;
}

// Development / test hooks (not part of icp_hip.h; called by tests/ through ctypes).
//   icp_debug_counters        : how many runs of this context took the merged loop, and how many of those had to be repeated with the
//                               separate k_reduce_solve launches (rank-deficient system, or a bounded wait that ran out).
//   icp_debug_poison_handover : leaves a stale, valid-looking total in slot `slot` of k_reduce_solve's hand-over area -- what a run cut
//                               short between a block's publish and block 0's re-arm would leave behind.  The next call must not see it.
int icp_debug_ring_times(icp_ctx* c, int32_t* out, int32_t n) {     // development builds (ICP_DEBUG_TIMES): the reducer blocks' clock stamps of the last merged launch
#if ICP_DEBUG_TIMES
    if (!c || !out || n < (NSUM_USED + 1) * 8) return ICP_ERR_INVALID_ARG;
    int rc;
    if ((rc = set_device(c))) return rc;
    HIPCK(c, hipMemcpyFromSymbol(out, HIP_SYMBOL(icpdev::g_ring_dbg), (size_t)(NSUM_USED + 1) * 8 * 4));
    return ICP_OK;
#else
    (void)c; (void)out; (void)n;
    return ICP_ERR_INVALID_ARG;
#endif
}
int icp_debug_dev_counters(icp_ctx* c, uint32_t* out16, int32_t reset) {     // development builds (ICP_DEBUG_TIMES): the device's event counters (g_dev_counts) since the last reset
#if ICP_DEBUG_TIMES
    if (!c || !out16) return ICP_ERR_INVALID_ARG;
    int rc;
    if ((rc = set_device(c))) return rc;
    HIPCK(c, hipStreamSynchronize(c->stream));
    HIPCK(c, hipMemcpyFromSymbol(out16, HIP_SYMBOL(icpdev::g_dev_counts), 64));
    if (reset == 2) HIPCK(c, hipMemcpyFromSymbol(out16, HIP_SYMBOL(icpdev::g_walk_trace), 256));      // (reset == 2: the caller's buffer has 64 words and wants the trace of the last sparse walk instead, tools/dev_walk_trace.py)
    if (reset) { uint32_t z[16] = {0}; HIPCK(c, hipMemcpyToSymbol(HIP_SYMBOL(icpdev::g_dev_counts), z, 64)); }
    return ICP_OK;
#else
    (void)c; (void)out16; (void)reset;
    return ICP_ERR_INVALID_ARG;
#endif
}
//   icp_debug_wave_slot       : host evaluation of the fused matcher's block -> wave mapping (fused_wave_slot): which stretch of 64 queries
//                               wave w of logical block lb takes in a grid of mgrid blocks; *waves_per_block receives BVH_THREADS / 64.  No GPU needed.
//   icp_debug_pos_of_mismatches: entries of the resident target's position-by-index map that do not point back at their record (must be 0).
int icp_debug_wave_slot(int32_t lb, int32_t w, int32_t mgrid, int32_t* waves_per_block) {
    if (waves_per_block) *waves_per_block = BVH_THREADS / WAVE;
    if (lb < 0 || lb >= mgrid || w < 0 || w >= BVH_THREADS / WAVE) return -1;
    return icpdev::fused_wave_slot(lb, w, mgrid);
}
//   icp_debug_stamp_times     : the host arithmetic that turns a merged run's device-clock stamps into icp_timing and the per-iteration
//                               arrays (sample_iterations + stamps_to_timing, host_loop.hpp), on the caller's stamps: t0 / t1 hold
//                               iters + 1 ticks each (entry iters: the closing launch), n_done iterations ran, the timing mode and the
//                               context's run counter pick the reported iterations.  The three arrays receive n_done floats.  No GPU needed.
int icp_debug_stamp_times(const uint64_t* t0, const uint64_t* t1, int32_t iters, int32_t n_done, int32_t mode, uint32_t phase, double ticks_per_ms,
                          icp_timing* timing, float* match_ms, float* post_ms, float* solve_ms) {
    if (!t0 || !t1 || !timing || iters < 1 || n_done < 1 || n_done > iters || mode < 0 || !(ticks_per_ms > 0)) return ICP_ERR_INVALID_ARG;
    std::vector<char> sampled;
    sample_iterations(mode, phase, iters, sampled);
    stamps_to_timing((const unsigned long long*)t0, (const unsigned long long*)t1, iters, n_done, sampled.data(), ticks_per_ms, timing, match_ms, post_ms, solve_ms);
    return ICP_OK;
}
//   icp_debug_wall_clock_khz  : the rate of the device's wall clock as the runtime reports it (hipDeviceAttributeWallClockRate), which is
//                               what the merged loop's stamps are converted with: one tick is 1 / khz milliseconds.
int icp_debug_wall_clock_khz(icp_ctx* c, int32_t* khz) {
    if (!c || !khz) return ICP_ERR_INVALID_ARG;
    int v = 0;
    HIPCK(c, hipDeviceGetAttribute(&v, hipDeviceAttributeWallClockRate, c->device));
    *khz = v;
    return ICP_OK;
}
__global__ void k_debug_pos_of(const icpdev::TgtRec* recs, const int* pos_of, int n_slots, int* bad) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_slots && recs[i].idx >= 0 && pos_of[recs[i].idx] != i) atomicAdd(bad, 1);
}
int icp_debug_pos_of_mismatches(icp_ctx* c, int32_t* n_bad, int32_t* n_checked) {
    if (!c || !n_bad || !c->bvh.valid) return ICP_ERR_INVALID_ARG;
    int rc;
    if ((rc = set_device(c))) return rc;
    const int n_slots = (c->bvh.n_leaves > 0 ? c->bvh.n_leaves : 1) * BVH_LEAF;
    if ((rc = ensure(c, c->d_count, 4))) return rc;
    HIPCK(c, hipMemsetAsync(c->d_count.p, 0, 4, c->stream));
    hipLaunchKernelGGL(k_debug_pos_of, dim3((n_slots + 255) / 256), dim3(256), 0, c->stream, c->bvh.recs.as<icpdev::TgtRec>(), c->bvh.pos_of.as<int>(), n_slots, c->d_count.as<int>());
    HIPCK(c, hipMemcpyAsync(n_bad, c->d_count.p, 4, hipMemcpyDeviceToHost, c->stream));
    HIPCK(c, hipStreamSynchronize(c->stream));
    if (n_checked) *n_checked = c->bvh.n_valid;
    return ICP_OK;
}
//   icp_debug_live_bytes      : device bytes the library holds right now, over every context of the process (its own allocations, views
//                               not counted): a create -> use -> destroy cycle must leave it where it found it.  No context needed.
int icp_debug_live_bytes(int64_t* out) {
    if (!out) return ICP_ERR_INVALID_ARG;
    *out = (int64_t)g_live_bytes.load();
    return ICP_OK;
}
//   icp_debug_reciprocal_naive: on != 0 makes reciprocal rejection take the naive route on this context (a written-out query cloud, a full
//                               k_knn_bvh search against the source tree, a compare pass) -- the yardstick of tools/time_reciprocal.py.
int icp_debug_reciprocal_naive(icp_ctx* c, int32_t on) {
    if (!c) return ICP_ERR_INVALID_ARG;
    c->rcp_naive = on != 0;
    return ICP_OK;
}
int icp_debug_counters(icp_ctx* c, int32_t* merged_runs, int32_t* merged_fallbacks) {
    if (!c) return ICP_ERR_INVALID_ARG;
    if (merged_runs) *merged_runs = c->merged_runs;
    if (merged_fallbacks) *merged_fallbacks = c->merged_fallbacks;
    return ICP_OK;
}
int icp_debug_poison_handover(icp_ctx* c, int32_t slot, double value) {
    if (!c || slot < 0 || slot >= NSUM) return ICP_ERR_INVALID_ARG;
    int rc;
    if ((rc = set_device(c))) return rc;
    if (!c->totals.p && (rc = rearm_handover(c))) return rc;
    HIPCK(c, hipMemcpyAsync(c->totals.as<double>() + slot, &value, 8, hipMemcpyHostToDevice, c->stream));
    HIPCK(c, hipStreamSynchronize(c->stream));
    return ICP_OK;
}

//   icp_debug_loop_sums       : the 34 sums the LOOP reduced, which no entry point of icp_hip.h returns (icp_correspond never fuses: its sums
//                               come from k_post + k_reduce_solve whatever the matcher).  Runs iteration `iteration` of the plan icp_run makes
//                               for the context's clouds and params (make_plan: the level's cloud or its `sel` list, its Morton order), at
//                               `pose`, unseeded, in the form asked for, whatever ICP_HIP_MERGE says:
//                                 form 0, separate: the launches of enqueue_separate's loop body -- launch_match allowed to fuse, then
//                                   launch_post_and_solve with SolveParams::sums_out set (k_reduce_solve's optional copy).  Every linear
//                                   configuration takes it.
//                                 form 1, merged: enqueue_merged itself on a run of two iterations (the one asked for, then the plan's next, or
//                                   the same again behind the last): k_knn_bvh_post_ring, the reducer of the first riding in front of the
//                                   second's matcher blocks, the closing k_ring_reduce_solve.  The sums are row 0 of the totals ring, read
//                                   back after the run (a granule is the double's bits; the writer flips bit 0 of an all-ones NaN only).
//                                   Refused (ICP_ERR_INVALID_ARG) unless run_loop would merge: k-NN matching on the LBVH backend,
//                                   point-to-plane, no random resampling (selection 0, or 2 held), a plan of >= 2 iterations none of which is
//                                   empty, no rmse / benchmark-error recording.
//                               Both refuse the non-linear optimiser, robust mode and reciprocal rejection (their loops run other chains).
//                               sums_out[64]: the layout of icp_correspond's.  pose_out: the pose the iteration composed.  route_out[4]:
//                               kernel family that accumulated (0 k_post / k_post_gicp / k_post_colored, 1 k_knn_bvh_post, 2
//                               k_knn_bvh_post_ring), DIM of the matcher, WIDE (0 / 1; -1 for the brute-force and projective matchers), and the
//                               fault word of the composed pose slot (merged: 2 = the rank guard failed and run_loop would repeat the run in
//                               the separate form; the sums are the ring's all the same, pose_out is the incoming pose, n_valid sums[0]).
int icp_debug_loop_sums(icp_ctx* c, const float pose[16], int32_t form, int32_t iteration, double* sums_out, int32_t* n_valid_out, float* pose_out, int32_t* route_out) {
    if (!c || !pose || !sums_out || !n_valid_out || !pose_out || !route_out || (form != 0 && form != 1)) { if (c) c->err = "icp_debug_loop_sums: bad argument"; return ICP_ERR_INVALID_ARG; }
    const icp_params& p = c->prm;
    int rc;
    DrainOnError guard(c);
    if ((rc = set_device(c))) return rc;
    if ((rc = check_ready(c, true, true))) return rc;
    if ((rc = gicp_prepare(c))) return rc;
    if ((rc = colored_prepare(c))) return rc;
    if (c->lm_on || robust_on(c) || reciprocal_on(c)) { c->err = "icp_debug_loop_sums: the non-linear optimiser, robust mode and reciprocal rejection run other chains"; return ICP_ERR_INVALID_ARG; }
    RunPlan pl;
    if ((rc = make_plan(c, false, pl))) return rc;
    const int iters = pl.iters(), it = iteration;
    if (it < 0 || it >= iters || pl.ns[it] <= 0) { c->err = "icp_debug_loop_sums: no such iteration in the plan, or it has no queries"; return ICP_ERR_INVALID_ARG; }
    const bool colors = p.color_icp != 0 && p.matching == ICP_MATCH_KNN;
    const bool lbvh = p.matching == ICP_MATCH_KNN && p.knn_backend == ICP_KNN_LBVH;
    double hs[NSUM]; icp_iter_stats st; memset(&st, 0, sizeof(st)); PoseState hp; int family = 0;
    if (form == 0) {
        if ((rc = ensure(c, c->stats, 512)) || (rc = ensure(c, c->sums, NSUM * 8))) return rc;
        if ((rc = rearm_handover(c))) return rc;
        if ((rc = write_pose(c, pose))) return rc;
        QuerySet q{pl.clouds[it], pl.sels[it], pl.ns[it], 0, colors, false, pl.orders[it], false};
        int fused = 0;
        if ((rc = launch_match(c, q, &fused))) return rc;
        if ((rc = launch_post_and_solve(c, *pl.clouds[it], pl.sels[it], pl.ns[it], c->stats.as<icp_iter_stats>(), c->sums.as<double>(), 1, nullptr, fused, nullptr))) return rc;
        family = fused ? 1 : 0;
        HIPCK(c, hipMemcpyAsync(hs, c->sums.p, NSUM * 8, hipMemcpyDeviceToHost, c->stream));
        HIPCK(c, hipMemcpyAsync(&st, c->stats.p, sizeof(st), hipMemcpyDeviceToHost, c->stream));
        HIPCK(c, hipMemcpyAsync(&hp, c->ps.p, sizeof(hp), hipMemcpyDeviceToHost, c->stream));
        HIPCK(c, hipStreamSynchronize(c->stream));
        if (hp.fault) { c->err = "reduction hand-over timed out on the device (k_reduce_solve)"; return ICP_ERR_HIP; }
    } else {
        const bool rec = (p.record_rmse & 3) && c->conv_n > 0;
        bool merged = iters >= 2 && pl.sorted_levels && p.metric == ICP_METRIC_POINT_TO_PLANE && !rec;
        for (int i = 0; merged && i < iters; i++) if (pl.ns[i] <= 0) merged = false;
        if (!merged) { c->err = "icp_debug_loop_sums: the loop of this configuration does not take the merged form"; return ICP_ERR_INVALID_ARG; }
        const int two[2] = {it, it + 1 < iters ? it + 1 : it};
        LoopRun r{};
        r.pl.sorted_levels = pl.sorted_levels; r.pl.fixed_sets = pl.fixed_sets;
        for (int k : two) { r.pl.factors.push_back(pl.factors[k]); r.pl.ns.push_back(pl.ns[k]); r.pl.clouds.push_back(pl.clouds[k]); r.pl.sels.push_back(pl.sels[k]); r.pl.orders.push_back(pl.orders[k]); }
        r.lay_out(2, false, false);
        if ((rc = ensure_pinned(c, r.pin_bytes))) return rc;
        make_pose_state(pose, &r.ps_in);
        if ((rc = ensure(c, c->stats, r.stats_bytes))) return rc;
        r.sampled.assign(2, 0); r.eligible.assign(2, 0);
        if ((rc = enqueue_merged(c, r))) return rc;
        unsigned long long row[NSUM];      // row 0 of the totals ring: behind the 3 pose slots (make_ring)
        HIPCK(c, hipMemcpyAsync(row, c->ring.as<char>() + (size_t)3 * POSE_REPLICAS * POSE_REPLICA_STRIDE, NSUM * 8, hipMemcpyDeviceToHost, c->stream));
        HIPCK(c, hipMemcpyAsync(&hp, loop_slot(c->ring.as<PoseState>(), 1, 0), sizeof(hp), hipMemcpyDeviceToHost, c->stream));      // slot 1: the pose the first iteration composed
        HIPCK(c, hipStreamSynchronize(c->stream));
        if (r.host_tail(c)->merged_fault || hp.fault == 1) { c->err = "icp_debug_loop_sums: a bounded wait of the merged launches ran out"; return ICP_ERR_HIP; }
        for (int a = 0; a < NSUM; a++) {
            if (a < NSUM_USED && row[a] == GRANULE_EMPTY) { c->err = "icp_debug_loop_sums: a total of the ring was never written"; return ICP_ERR_HIP; }
            if (a < NSUM_USED) memcpy(&hs[a], &row[a], 8); else hs[a] = 0.0;
        }
        if (hp.fault) { memcpy(st.pose, pose, 64); st.n_valid = (int)hs[SUM_N]; }      // the chain was cut: no record was written
        else memcpy(&st, r.host_records(c), sizeof(st));
        family = 2;
    }
    const Bvh& b = colors ? c->bvh6 : c->bvh;
    route_out[0] = family; route_out[1] = colors ? 6 : 3; route_out[2] = lbvh ? (b.Lq > 8 ? 1 : 0) : -1; route_out[3] = hp.fault;
    memset(sums_out, 0, 64 * 8); memcpy(sums_out, hs, NSUM * 8);
    *n_valid_out = st.n_valid;
    memcpy(pose_out, st.pose, 64);
    return guard.done();
}

//   icp_debug_walk_steps      : the two steps of the shared walk on the caller's arrays, one lane per item, with the device functions the
//                               matchers run (dev_bvh.hpp: leaf_eval<3>, quad_lb<3>).  Leaves and nodes are 128-byte records in the layouts
//                               of BvhLeafT<3> / BvhQuadT<3>.  Per leaf: query lq[3], leaf number, state in (best, b2, b3 | bi, bpos, l2) ->
//                               state out in the same order, and leaf_eval's flags (bit 0: winner update, bit 1: sequential scan).  Per
//                               node: query nq[3] -> the four child bounds.  empty_box[2] receives (lo, hi) of an empty child as
//                               k_bvh_quad_nodes stores it.  tests/test_gpu_walk_steps.py compares all of it bitwise with NumPy.
__global__ void k_debug_walk_steps(int n_leaves, const icpdev::BvhLeafT<3>* leaves, const float* lq, const int* leaf_no, const float* sf, const int* si, float* of, int* oi,
                                   int n_nodes, const icpdev::BvhQuadT<3>* nodes, const float* nq, float* bounds) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_leaves) {
        icpdev::f2 p2[3];
        for (int k = 0; k < 3; k++) { p2[k].x = lq[3 * i + k]; p2[k].y = p2[k].x; }
        float best = sf[3 * i], b2 = sf[3 * i + 1], b3 = sf[3 * i + 2]; int bi = si[3 * i], bpos = si[3 * i + 1], l2 = si[3 * i + 2];
        const int flags = icpdev::leaf_eval<3>(leaves + i, leaf_no[i], p2, best, bi, bpos, b2, l2, b3);
        of[3 * i] = best; of[3 * i + 1] = b2; of[3 * i + 2] = b3; oi[4 * i] = bi; oi[4 * i + 1] = bpos; oi[4 * i + 2] = l2; oi[4 * i + 3] = flags;
    }
    if (i < n_nodes) {
        icpdev::f2 p2[3], l01, l23;
        for (int k = 0; k < 3; k++) { p2[k].x = nq[3 * i + k]; p2[k].y = p2[k].x; }
        icpdev::quad_lb<3>(nodes + i, p2, l01, l23);
        bounds[4 * i] = l01.x; bounds[4 * i + 1] = l01.y; bounds[4 * i + 2] = l23.x; bounds[4 * i + 3] = l23.y;
    }
}
int icp_debug_walk_steps(icp_ctx* c, int32_t n_leaves, const void* leaves, const float* lq, const int32_t* leaf_no, const float* sf, const int32_t* si, float* of, int32_t* oi,
                         int32_t n_nodes, const void* nodes, const float* nq, float* bounds, float* empty_box) {
    if (!c || n_leaves < 0 || n_nodes < 0 || n_leaves > (1 << 20) || n_nodes > (1 << 20)) return ICP_ERR_INVALID_ARG;
    if (n_leaves > 0 && (!leaves || !lq || !leaf_no || !sf || !si || !of || !oi)) return ICP_ERR_INVALID_ARG;
    if (n_nodes > 0 && (!nodes || !nq || !bounds)) return ICP_ERR_INVALID_ARG;
    if (empty_box) { empty_box[0] = icpdev::BVH_QUAD_EMPTY_LO; empty_box[1] = icpdev::BVH_QUAD_EMPTY_HI; }
    const int n = n_leaves > n_nodes ? n_leaves : n_nodes;
    if (n == 0) return ICP_OK;
    int rc;
    if ((rc = set_device(c))) return rc;
    DrainOnError guard(c);
    // one staging area: inputs (leaves, lq, leaf_no, sf, si, nodes, nq), then outputs (of, oi, bounds)
    const size_t L = (size_t)n_leaves, N = (size_t)n_nodes;
    auto up = [](size_t x) { return (x + 127) & ~(size_t)127; };      // (every section on a 128-byte line, as the records are in the tree)
    const size_t o_lq = 128 * L, o_no = up(o_lq + 12 * L), o_sf = up(o_no + 4 * L), o_si = up(o_sf + 12 * L), o_nd = up(o_si + 12 * L), o_nq = o_nd + 128 * N, o_of = up(o_nq + 12 * N),
                 o_oi = up(o_of + 12 * L), o_bd = up(o_oi + 16 * L), total = o_bd + 16 * N;
    if ((rc = ensure(c, c->staging, total))) return rc;
    char* d = c->staging.as<char>();
    if (L) {
        HIPCK(c, hipMemcpyAsync(d, leaves, 128 * L, hipMemcpyHostToDevice, c->stream));
        HIPCK(c, hipMemcpyAsync(d + o_lq, lq, 12 * L, hipMemcpyHostToDevice, c->stream));
        HIPCK(c, hipMemcpyAsync(d + o_no, leaf_no, 4 * L, hipMemcpyHostToDevice, c->stream));
        HIPCK(c, hipMemcpyAsync(d + o_sf, sf, 12 * L, hipMemcpyHostToDevice, c->stream));
        HIPCK(c, hipMemcpyAsync(d + o_si, si, 12 * L, hipMemcpyHostToDevice, c->stream));
    }
    if (N) {
        HIPCK(c, hipMemcpyAsync(d + o_nd, nodes, 128 * N, hipMemcpyHostToDevice, c->stream));
        HIPCK(c, hipMemcpyAsync(d + o_nq, nq, 12 * N, hipMemcpyHostToDevice, c->stream));
    }
    hipLaunchKernelGGL(k_debug_walk_steps, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, n_leaves, (const icpdev::BvhLeafT<3>*)d, (const float*)(d + o_lq), (const int*)(d + o_no),
                       (const float*)(d + o_sf), (const int*)(d + o_si), (float*)(d + o_of), (int*)(d + o_oi), n_nodes, (const icpdev::BvhQuadT<3>*)(d + o_nd), (const float*)(d + o_nq), (float*)(d + o_bd));
    HIPCK(c, hipGetLastError());
    if (L) {
        HIPCK(c, hipMemcpyAsync(of, d + o_of, 12 * L, hipMemcpyDeviceToHost, c->stream));
        HIPCK(c, hipMemcpyAsync(oi, d + o_oi, 16 * L, hipMemcpyDeviceToHost, c->stream));
    }
    if (N) HIPCK(c, hipMemcpyAsync(bounds, d + o_bd, 16 * N, hipMemcpyDeviceToHost, c->stream));
    HIPCK(c, hipStreamSynchronize(c->stream));
    return guard.done();
}

// ---- hardware self test (not part of icp_hip.h; called by tests/ through ctypes) ------------------------------------------
// One wave folds n_values (<= 32) doubles per lane with wave_transpose_reduce_gen; out[v] = the wave total of value v read from
// the lane wave_value_of_lane says holds it.  tests/test_gpu_selftest.py replays the same pairing with numpy: bit-identical.
int icp_selftest_wave_reduce(icp_ctx* c, const double* in, double* out, int32_t* lane_of) {
    if (!c || !in || !out || !lane_of) return ICP_ERR_INVALID_ARG;
    int rc;
    if ((rc = set_device(c))) return rc;
    DrainOnError guard(c);
    if ((rc = ensure(c, c->staging, 64 * 27 * 8 + 27 * 8 + 27 * 4 + 64))) return rc;
    double* d_in = c->staging.as<double>(); double* d_out = d_in + 64 * 27; int* d_lane = (int*)(d_out + 27);
    HIPCK(c, hipMemcpyAsync(d_in, in, 64 * 27 * 8, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(k_selftest_wave_reduce, dim3(1), dim3(64), 0, c->stream, d_in, d_out, d_lane);
    HIPCK(c, hipGetLastError());
    HIPCK(c, hipMemcpyAsync(out, d_out, 27 * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCK(c, hipMemcpyAsync(lane_of, d_lane, 27 * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCK(c, hipStreamSynchronize(c->stream));
    return guard.done();
}
}  // extern "C"
