// host_multi.hpp -- icp_run_multistart: the loop of host_loop.hpp's separate form with every start as blockIdx.y of each launch, and the
// score of the final poses (dev_multi.hpp).  Part of icp_hip.hip (included from there, after host_loop.hpp).
// Multi-start ICP (dev_multi.hpp): run_loop's generic per-iteration form -- matcher (+ post) and reduce / solve -- with start s as blockIdx.y
// of every launch, each start in slices of its own (pose state, search state, records, partials, hand-over, iteration records).  The ticket
// hand-over of k_reduce_solve, not the polling one: no block waits for another, so the K x 34 reducer blocks need not be resident together.
constexpr int MULTISTART_MAX = 256;
int icp_run_multistart(icp_ctx* c, const float* initial_poses, int32_t n_starts, icp_start_result* results, icp_iter_stats* stats,
                       int32_t max_stats, int32_t* n_iterations_run, int32_t* best_out) {
    if (!c) return ICP_ERR_INVALID_ARG;
    if (!initial_poses || !results || n_starts < 1 || n_starts > MULTISTART_MAX || max_stats < 0) {
        c->err = "icp_run_multistart: bad argument (initial_poses and results non-NULL, 1 <= n_starts <= 256, max_stats >= 0)"; return ICP_ERR_INVALID_ARG;
    }
    const icp_params& p = c->prm;
    if (p.matching != ICP_MATCH_KNN) { c->err = "icp_run_multistart: projective matching is not supported"; return ICP_ERR_INVALID_ARG; }
    if (p.knn_backend != ICP_KNN_LBVH) { c->err = "icp_run_multistart: the brute-force k-NN backend is not supported"; return ICP_ERR_INVALID_ARG; }
    if (p.record_rmse != 0) { c->err = "icp_run_multistart: record_rmse is not supported"; return ICP_ERR_INVALID_ARG; }
    if (c->lm_on) { c->err = "icp_run_multistart: the non-linear optimiser is not supported"; return ICP_ERR_INVALID_ARG; }
    if (c->prm.metric == ICP_METRIC_GICP) { c->err = "icp_run_multistart: GICP is not supported"; return ICP_ERR_INVALID_ARG; }
    if (c->prm.metric == ICP_METRIC_COLORED) { c->err = "icp_run_multistart: colored ICP is not supported"; return ICP_ERR_INVALID_ARG; }
    if (reciprocal_on(c)) { c->err = "icp_run_multistart: reciprocal rejection (icp_set_reciprocal_options) is not supported"; return ICP_ERR_INVALID_ARG; }
    if (robust_on(c)) { c->err = "icp_run_multistart: robust mode (icp_set_robust_options) is not supported"; return ICP_ERR_INVALID_ARG; }
    if (c->cvg_opt.enabled) { c->err = "icp_run_multistart: stopping on a converged pose (icp_set_convergence_options) is not supported: the starts share their launches"; return ICP_ERR_INVALID_ARG; }
    int rc;
    DrainOnError guard(c);
    if ((rc = set_device(c))) return rc;
    if ((rc = check_ready(c, true, true))) return rc;
    const int K = n_starts;
    RunPlan pl;
    if ((rc = make_plan(c, false, pl))) return rc;
    const int iters = pl.iters();
    const std::vector<int>& ns = pl.ns; const std::vector<const int*>& sels = pl.sels; const std::vector<const int*>& orders = pl.orders;
    if (n_iterations_run) *n_iterations_run = 0;
    // the score's queries: the full-resolution source, Morton-sorted; its index: the 3-D tree over the target's xyz (built on demand)
    const Cloud* full = nullptr; int n_full = 0;
    if ((rc = get_sorted_level(c, 0, &full, &n_full))) return rc;
    if (!c->bvh.valid && (rc = build_bvh<3>(c, c->bvh, target_coords3(c)))) return rc;
    const bool colors = p.color_icp != 0;
    if (colors && !c->bvh6.valid && (rc = build_bvh<6>(c, c->bvh6, target_coords6(c)))) return rc;
    const bool fused = p.metric != ICP_METRIC_SYMMETRIC;
    // per-start slices, sized for the largest query set of the run
    int nmax = n_full, nbmax = POST_BLOCKS;
    for (int i = 0; i < iters; i++) { if (ns[i] > nmax) nmax = ns[i]; if (fused && fused_nblocks(ns[i]) > nbmax) nbmax = fused_nblocks(ns[i]); }
    MultiStride ms;
    ms.q = ((size_t)nmax + 63) / 64 * 64; ms.partials = (size_t)nbmax * NSUM; ms.totals = NSUM + 1; ms.stats = iters > 0 ? iters : 1;
    const size_t Kz = (size_t)K;
    const struct { DevBuf* buf; size_t bytes; } slices[] = {
        {&c->ms_ps, Kz * sizeof(PoseState)}, {&c->ms_nn, Kz * ms.q * 4}, {&c->ms_st, Kz * ms.q * 16}, {&c->ms_st2, Kz * ms.q * 8}, {&c->ms_rec, Kz * ms.q * sizeof(icp_match_t)},
        {&c->ms_d2, Kz * ms.q * 4}, {&c->ms_partials, Kz * ms.partials * 8}, {&c->ms_totals, Kz * ms.totals * 8}, {&c->ms_stats, Kz * (size_t)ms.stats * sizeof(icp_iter_stats)},
        {&c->ms_score, Kz * MSCORE_BLOCKS * 3 * 8}, {&c->ms_res, Kz * sizeof(icp_start_result)}};
    for (const auto& sl : slices) if ((rc = ensure(c, *sl.buf, sl.bytes))) return rc;
    // page-locked staging: [pose states up | records down | results down]
    const size_t pin_rec = (Kz * sizeof(PoseState) + 255) & ~(size_t)255, pin_res = pin_rec + ((Kz * (size_t)ms.stats * sizeof(icp_iter_stats) + 255) & ~(size_t)255);
    if ((rc = ensure_pinned(c, pin_res + Kz * sizeof(icp_start_result)))) return rc;
    PoseState* hps = c->pinned.as<PoseState>();
    for (int s = 0; s < K; s++) {
        memset(&hps[s], 0, sizeof(PoseState)); memcpy(hps[s].pose, initial_poses + (size_t)16 * s, 64); normal_matrix_from_pose(hps[s].pose, hps[s].nmat);
    }
    PoseState* d_ps = c->ms_ps.as<PoseState>();
    HIPCK(c, hipMemcpyAsync(d_ps, hps, Kz * sizeof(PoseState), hipMemcpyHostToDevice, c->stream));
    HIPCK(c, hipMemsetAsync(c->ms_totals.p, 0, Kz * ms.totals * 8, c->stream));      // K tickets (and totals) armed: rearm_handover's ticket form
    const BvhViewT<3> view3 = make_view<3>(c->bvh, target_coords3(c));
    const BvhViewT<6> view6 = make_view<6>(c->bvh6, target_coords6(c));      // (launched only with colours, when bvh6 is built)
    const size_t lds_fused = colors ? fused_lds_bytes<6>() : fused_lds_bytes<3>();
    for (int i = 0; i < iters; i++) {
        if (ns[i] <= 0) continue;                                // an empty iteration: nothing runs, the records are filled in below
        const int n = ns[i];
        const Cloud* q = pl.clouds[i];
        KnnParams kp = knn_params(c, *q, sels[i], n);
        kp.ps = d_ps; kp.fault = &d_ps->fault;
        kp.nn_raw = c->ms_nn.as<int>();
        kp.use_prev = pl.seeded(i) ? 1 : 0;
        if (p.knn_incremental) { kp.qstate = c->ms_st.as<float4>(); kp.qstate2 = c->ms_st2.as<float2>(); kp.incremental = 1; }
        PostParams pp = make_post_params(c, *q, sels[i], n);
        pp.ps = d_ps; pp.partials = c->ms_partials.as<double>();
        int nb;
        if (fused) {                                             // k_knn_bvh_post: records not kept
            kp.out = nullptr; kp.d2_out = nullptr; pp.matches = nullptr;
            nb = fused_nblocks(n);
            const dim3 g((unsigned)nb, (unsigned)K);
            if (colors) hipLaunchKernelGGL(pick_wide(view6.Lq, k_knn_bvh_post_multi<6, false>, k_knn_bvh_post_multi<6, true>), g, dim3(BVH_THREADS), lds_fused, c->stream, kp, view6, orders[i], pp, ms);
            else hipLaunchKernelGGL(pick_wide(view3.Lq, k_knn_bvh_post_multi<3, false>, k_knn_bvh_post_multi<3, true>), g, dim3(BVH_THREADS), lds_fused, c->stream, kp, view3, orders[i], pp, ms);
        } else {                                                 // k_knn_bvh, then k_post
            kp.out = c->ms_rec.as<icp_match_t>(); kp.d2_out = c->ms_d2.as<float>(); pp.matches = c->ms_rec.as<icp_match_t>();
            const dim3 g((unsigned)((n + BVH_THREADS - 1) / BVH_THREADS), (unsigned)K);
            if (colors) hipLaunchKernelGGL(k_knn_bvh_multi<6>, g, dim3(BVH_THREADS), WALK_LDS_BYTES, c->stream, kp, view6, orders[i], ms);
            else hipLaunchKernelGGL(k_knn_bvh_multi<3>, g, dim3(BVH_THREADS), WALK_LDS_BYTES, c->stream, kp, view3, orders[i], ms);
            nb = post_nblocks(n);
            hipLaunchKernelGGL(k_post_multi, dim3((unsigned)nb, (unsigned)K), dim3(POST_THREADS), 0, c->stream, pp, ms);
        }
        SolveParams sp; memset(&sp, 0, sizeof(sp));
        sp.partials = c->ms_partials.as<double>(); sp.nblocks = nb; sp.ps = d_ps; sp.metric = p.metric;
        sp.totals = c->ms_totals.as<double>(); sp.n_src = n; sp.update_pose = 1; sp.spin = 0;
        icp_iter_stats* d_st = c->ms_stats.as<icp_iter_stats>() + i;
        const dim3 gr(NSUM_USED, (unsigned)K);
        if (p.metric == ICP_METRIC_SYMMETRIC) {
            sp.phase = 0; sp.stats = nullptr;
            hipLaunchKernelGGL(k_reduce_solve_multi, gr, dim3(SOLVE_THREADS), 0, c->stream, sp, ms);      // means
            hipLaunchKernelGGL(k_sym_accumulate_multi, dim3((unsigned)nb, (unsigned)K), dim3(POST_THREADS), 0, c->stream, pp, ms);
            sp.phase = 1;
        } else sp.phase = 0;
        sp.stats = d_st;
        hipLaunchKernelGGL(k_reduce_solve_multi, gr, dim3(SOLVE_THREADS), 0, c->stream, sp, ms);
        HIPCK(c, hipGetLastError());
    }
    {   // score at the final poses: every full-resolution source point, unseeded, in 3-D
        KnnParams kp = knn_params(c, *full, nullptr, n_full);
        kp.ps = d_ps; kp.fault = &d_ps->fault; kp.scr = kp.scg = kp.scb = nullptr;      // (3-D: no colour planes)
        kp.out = c->ms_rec.as<icp_match_t>(); kp.d2_out = c->ms_d2.as<float>();
        if (n_full > 0) hipLaunchKernelGGL(k_knn_bvh_multi<3>, dim3((unsigned)((n_full + BVH_THREADS - 1) / BVH_THREADS), (unsigned)K), dim3(BVH_THREADS), WALK_LDS_BYTES, c->stream, kp, view3, nullptr, ms);
        ScoreParams sc; sc.sx = kp.sx; sc.sy = kp.sy; sc.sz = kp.sz; sc.n = n_full; sc.matches = kp.out; sc.d2 = kp.d2_out; sc.q = ms.q; sc.partials = c->ms_score.as<double>();
        hipLaunchKernelGGL(k_score_multi, dim3(MSCORE_BLOCKS, (unsigned)K), dim3(MSCORE_THREADS), 0, c->stream, sc);
        hipLaunchKernelGGL(k_score_fold, dim3((unsigned)((K + 63) / 64)), dim3(64), 0, c->stream, c->ms_score.as<double>(), MSCORE_BLOCKS, d_ps, K, c->ms_res.as<icp_start_result>());
        HIPCK(c, hipGetLastError());
    }
    icp_iter_stats* hrec = (icp_iter_stats*)(c->pinned.as<char>() + pin_rec);
    icp_start_result* hres = (icp_start_result*)(c->pinned.as<char>() + pin_res);
    if (iters > 0) HIPCK(c, hipMemcpyAsync(hrec, c->ms_stats.p, Kz * (size_t)ms.stats * sizeof(icp_iter_stats), hipMemcpyDeviceToHost, c->stream));
    HIPCK(c, hipMemcpyAsync(hres, c->ms_res.p, Kz * sizeof(icp_start_result), hipMemcpyDeviceToHost, c->stream));
    HIPCK(c, hipMemcpyAsync(hps, d_ps, Kz * sizeof(PoseState), hipMemcpyDeviceToHost, c->stream));     // (the fault words)
    HIPCK(c, hipStreamSynchronize(c->stream));
    guard.ok = true;
    for (int s = 0; s < K; s++)
        if (hps[s].fault) { c->err = "icp_run_multistart: a bounded wait of the matcher ran out on the device"; return ICP_ERR_HIP; }
    int best = 0;
    for (int s = 0; s < K; s++) {
        icp_iter_stats* hs = hrec + (size_t)s * ms.stats;
        const int status = finish_records(pl, iters, hs, initial_poses + (size_t)16 * s, false, false, stats ? stats + (size_t)s * max_stats : nullptr, max_stats);
        results[s] = hres[s];
        results[s].status = status;
        const icp_start_result& a = results[s], &b = results[best];
        if (a.n_inliers > b.n_inliers || (a.n_inliers == b.n_inliers && a.inlier_rmse < b.inlier_rmse)) best = s;      // ties: smaller rmse, then lower index
    }
    if (n_iterations_run) *n_iterations_run = iters;
    if (best_out) *best_out = best;
    return ICP_OK;
}
