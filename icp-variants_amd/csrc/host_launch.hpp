// host_launch.hpp -- one iteration's launches, enqueued and never waited for: the matcher (brute force, projective, BVH, BVH with the post
// stage fused, its merged-ring form), the robust chain, the post stage with the reduce / solve or the non-linear optimiser behind it, and
// the two convergence measures.  Part of icp_hip.hip (included from there, after host_index.hpp).
namespace {
// One launch of the merged loop: the pose slot its matcher blocks wait for, where they leave their partials, and the reducer that rides in front.
struct MergeLaunch { RingParams rp; const PoseState* slot; double* partials; };   // (the launch's time stamps travel in rp.st: nothing on the stream brackets it)

// Launch shapes written once.  LDS of the stand-alone BVH matcher: the shared walk's records.  LDS of the fused matcher: the same, reused
// by the (smaller) block reduction of the post stage once the traversal stacks are dead, + the board of the cross-wave hand-over.
constexpr size_t WALK_LDS_BYTES = (size_t)ICP_SHARE_ROWS * BVH_THREADS * 8;
template <int DIM> size_t fused_lds_bytes() {
    const size_t red_bytes = (size_t)(BVH_THREADS / WAVE) * 33 * 8;
    return (WALK_LDS_BYTES > red_bytes ? WALK_LDS_BYTES : red_bytes) + xw_lds_bytes<DIM, BVH_THREADS>();
}
// grid of a post-stage kernel over n records (grid-stride loops past POST_BLOCKS)
int post_nblocks(int n) { const int nb = (n + POST_THREADS - 1) / POST_THREADS; return nb > POST_BLOCKS ? POST_BLOCKS : nb < 1 ? 1 : nb; }
// WIDE: a tree of more than 8 four-wide levels takes the <DIM, true> instantiation of a matcher
template <class K> K pick_wide(int Lq, K narrow, K wide) { return Lq <= 8 ? narrow : wide; }

struct QuerySet { const Cloud* cl; const int* sel; int n; int pretransformed; bool use_colors; bool seed_prev; const int* order; bool keep_records = false; };   // cl/sel: also what the post stage reads; keep_records: a fused matcher also writes its Match records and distances (the loop itself never reads them)

int ensure_qpack(icp_ctx* c, int n) {
    if ((size_t)n <= c->q_cap && c->qpack.p) return ICP_OK;
    int rc;
    c->q_cap = ((size_t)n + 63) / 64 * 64;
    if ((rc = ensure(c, c->qpack, c->q_cap * 28))) return rc;
    set_view(c->nn_raw, c->qpack.p, c->q_cap * 4); set_view(c->qstate, c->qpack.as<char>() + c->q_cap * 4, c->q_cap * 16);
    set_view(c->qstate2, c->qpack.as<char>() + c->q_cap * 20, c->q_cap * 8);
    return ICP_OK;
}

// The pose-independent part of a matcher launch's KnnParams: the query cloud and its selection, the target, the distance threshold.  The
// caller adds the pose state and fault word, the outputs and the search state; everything it leaves out is null / 0 (nseg: 1).
KnnParams knn_params(const icp_ctx* c, const Cloud& q, const int* sel, int n) {
    KnnParams kp; memset(&kp, 0, sizeof(kp));
    kp.sx = q.x.as<float>(); kp.sy = q.y.as<float>(); kp.sz = q.z.as<float>(); kp.scr = q.cr.as<float>(); kp.scg = q.cg.as<float>(); kp.scb = q.cb.as<float>();
    kp.sel = sel; kp.n = n;
    kp.tx = c->tgt.x.as<float>(); kp.ty = c->tgt.y.as<float>(); kp.tz = c->tgt.z.as<float>();
    kp.tcr = c->tgt.cr.as<float>(); kp.tcg = c->tgt.cg.as<float>(); kp.tcb = c->tgt.cb.as<float>();
    kp.mpad = c->tgt.npad; kp.max_dist = c->prm.max_distance; kp.nseg = 1;
    return kp;
}

PostParams make_post_params(icp_ctx* c, const Cloud& src, const int* sel, int n) {
    const icp_params& p = c->prm;
    PostParams pp;
    pp.sx = src.x.as<float>(); pp.sy = src.y.as<float>(); pp.sz = src.z.as<float>();
    pp.snx = src.nx.as<float>(); pp.sny = src.ny.as<float>(); pp.snz = src.nz.as<float>();
    pp.srgba = src.rgba.as<uint32_t>(); pp.sel = sel; pp.n = n;
    pp.tx = c->tgt.x.as<float>(); pp.ty = c->tgt.y.as<float>(); pp.tz = c->tgt.z.as<float>();
    pp.tnx = c->tgt.nx.as<float>(); pp.tny = c->tgt.ny.as<float>(); pp.tnz = c->tgt.nz.as<float>(); pp.trgba = c->tgt.rgba.as<uint32_t>();
    pp.ps = c->ps.as<PoseState>(); pp.matches = c->matches.as<icp_match_t>();
    pp.metric = p.metric; pp.weighting = p.weighting; pp.rejection = p.rejection;
    pp.max_dist = p.max_distance; pp.cos_reject = c->cos_reject; pp.partials = c->partials.as<double>();
    return pp;
}

// fuse != nullptr: run the post stage (weight / reject / accumulate) as the epilogue of the search; *fused_blocks receives the
// number of block partials written.
template <int DIM>
int launch_bvh_query(icp_ctx* c, Bvh& b, const CoordPtrs<DIM>& cp, const KnnParams& kp, const int* order, int n, const Cloud* fuse, bool keep_records, int* fused_blocks, const MergeLaunch* ml = nullptr) {
    int rc;
    if (!b.valid && (rc = build_bvh<DIM>(c, b, cp))) return rc;
    const BvhViewT<DIM> bv = make_view<DIM>(b, cp);
    const int nb = fuse ? fused_nblocks(n) : (n + BVH_THREADS - 1) / BVH_THREADS;
    if (fuse) {
        if ((rc = ensure(c, c->partials, (size_t)(nb > POST_BLOCKS ? nb : POST_BLOCKS) * NSUM * 8))) return rc;
        PostParams pp = make_post_params(c, *fuse, kp.sel, n);
        KnnParams kf = kp; kf.out = nullptr;
        if (!keep_records) { pp.matches = nullptr; kf.d2_out = nullptr; }     // the loop never reads the records of a fused iteration, nor the distances
        const size_t lds = fused_lds_bytes<DIM>();
        if (ml) {                                                                  // merged loop: reducer blocks in front, pose through the ring
            kf.ps = ml->slot; pp.ps = ml->slot; pp.partials = ml->partials; kf.fault = ml->rp.run_fault;
            const auto ring = pick_wide(b.Lq, k_knn_bvh_post_ring<DIM, false>, k_knn_bvh_post_ring<DIM, true>);
            hipLaunchKernelGGL(ring, dim3(nb + ml->rp.n_red), dim3(BVH_THREADS), lds, c->stream, kf, bv, order, pp, ml->rp);
        }
        else hipLaunchKernelGGL(pick_wide(b.Lq, k_knn_bvh_post<DIM, false>, k_knn_bvh_post<DIM, true>), dim3(nb), dim3(BVH_THREADS), lds, c->stream, kf, bv, order, pp);
        *fused_blocks = nb;
    } else hipLaunchKernelGGL(k_knn_bvh<DIM>, dim3(nb), dim3(BVH_THREADS), WALK_LDS_BYTES, c->stream, kp, bv, order);
    HIPCK(c, hipGetLastError());
    return ICP_OK;
}

// Enqueue the matching stage (no sync).  fused_blocks != nullptr allows the BVH matcher to run the post stage as its epilogue;
// it is set to the number of block partials written, or left 0 when the matcher in use does not fuse.
int launch_match(icp_ctx* c, const QuerySet& q, int* fused_blocks = nullptr, const MergeLaunch* ml = nullptr) {
    const icp_params& p = c->prm;
    int rc;
    if (fused_blocks) *fused_blocks = 0;
    if ((rc = ensure(c, c->matches, (size_t)q.n * sizeof(icp_match_t))) || (rc = ensure(c, c->d2, (size_t)q.n * 4))) return rc;
    if (p.matching == ICP_MATCH_PROJECTIVE) {
        ProjParams pp;
        pp.sx = q.cl->x.as<float>(); pp.sy = q.cl->y.as<float>(); pp.sz = q.cl->z.as<float>(); pp.sel = q.sel; pp.n = q.n;
        pp.tx = c->tgt.x.as<float>(); pp.ty = c->tgt.y.as<float>(); pp.tz = c->tgt.z.as<float>();
        pp.width = p.width; pp.height = p.height; pp.fx = p.fx; pp.fy = p.fy; pp.mx = p.cx; pp.my = p.cy; pp.window = 12;   // NearestNeighbor.h:319
        pp.ps = c->ps.as<PoseState>(); pp.pretransformed = q.pretransformed; pp.max_dist = p.max_distance;
        pp.out = c->matches.as<icp_match_t>(); pp.d2_out = c->d2.as<float>();
        hipLaunchKernelGGL(k_projective, dim3((q.n + 255) / 256), dim3(256), 0, c->stream, pp);
        HIPCK(c, hipGetLastError());
        return ICP_OK;
    }
    KnnParams kp = knn_params(c, *q.cl, q.sel, q.n);
    kp.ps = c->ps.as<PoseState>(); kp.pretransformed = q.pretransformed; kp.fault = &c->ps.as<PoseState>()->fault;
    kp.out = c->matches.as<icp_match_t>(); kp.d2_out = c->d2.as<float>();
    if (p.knn_backend == ICP_KNN_LBVH) {
        // neighbour positions and the incremental search's state in ONE allocation, sections a fixed number of elements apart
        // (int nn_raw[q_cap] | float4 qstate[q_cap] | float2 qstate2[q_cap])
        if ((rc = ensure_qpack(c, q.n))) return rc;
        kp.nn_raw = c->nn_raw.as<int>(); kp.use_prev = q.seed_prev ? 1 : 0;
#if ICP_DEBUG_STEPS
        if ((rc = ensure(c, c->dbg_steps, (size_t)q.n * 4))) return rc;
        kp.dbg_steps = c->dbg_steps.as<int>(); kp.dbg_waves = fused_nblocks(q.n) * (BVH_THREADS / WAVE);
#endif
        if (p.knn_incremental && !q.pretransformed) {
            kp.qstate = c->qstate.as<float4>(); kp.qstate2 = c->qstate2.as<float2>(); kp.incremental = 1;
        }
        const Cloud* fuse = (fused_blocks != nullptr && p.metric != ICP_METRIC_SYMMETRIC && p.metric != ICP_METRIC_GICP && p.metric != ICP_METRIC_COLORED && !q.pretransformed) ? q.cl : nullptr;
        if (q.use_colors) return launch_bvh_query<6>(c, c->bvh6, target_coords6(c), kp, q.order, q.n, fuse, q.keep_records, fused_blocks, fuse ? ml : nullptr);
        return launch_bvh_query<3>(c, c->bvh, target_coords3(c), kp, q.order, q.n, fuse, q.keep_records, fused_blocks, fuse ? ml : nullptr);
    }
    const int bx = (q.n + WAVE - 1) / WAVE;
    const int nch = kp.mpad / KNN_CH;
    int nseg = 1;
    if (bx < 1024) { nseg = (2048 + bx - 1) / bx; if (nseg > nch / 4) nseg = nch / 4; if (nseg < 1) nseg = 1; }
    kp.nseg = nseg;
    if (nseg > 1) {
        if ((rc = ensure(c, c->best64, (size_t)q.n * 8))) return rc;
        kp.best64 = c->best64.as<unsigned long long>();
        const unsigned long long init = ((unsigned long long)0x7F7FFFFFu << 32) | 0xFFFFFFFFull;   // (FLT_MAX, idx -1)
        hipLaunchKernelGGL(k_fill_u64, dim3((q.n + 255) / 256), dim3(256), 0, c->stream, kp.best64, q.n, init);
    }
    if (q.use_colors) hipLaunchKernelGGL(k_knn_brute<6>, dim3(bx, nseg), dim3(256), 0, c->stream, kp);
    else              hipLaunchKernelGGL(k_knn_brute<3>, dim3(bx, nseg), dim3(256), 0, c->stream, kp);
    if (nseg > 1)
        hipLaunchKernelGGL(k_knn_finalize, dim3((q.n + 255) / 256), dim3(256), 0, c->stream, kp.best64, q.n, p.max_distance,
                           c->matches.as<icp_match_t>(), c->d2.as<float>());
    HIPCK(c, hipGetLastError());
    return ICP_OK;
}

// The hand-over slots of k_reduce_solve (NSUM self-validating totals + the ticket) back to "nothing written": enqueued at the start of
// every entry point that launches it, so that whatever an earlier call left behind -- a run cut short by a HIP error between a
// block's publish and block 0's re-arm, a total that arrived after block 0 had given up -- can never be taken for a result.
int rearm_handover(icp_ctx* c) {
    int rc;
    if ((rc = ensure(c, c->totals, NSUM * 8 + 8))) return rc;
    HIPCK(c, hipMemsetAsync(c->totals.p, 0, NSUM * 8 + 8, c->stream));
    hipLaunchKernelGGL(k_fill_u64, dim3(1), dim3(64), 0, c->stream, c->totals.as<unsigned long long>(), NSUM, TOTAL_SENTINEL);
    HIPCK(c, hipGetLastError());
    return ICP_OK;
}

// The sorted position -> original source index map of a Morton-sorted level's cloud; nullptr for the resident source itself.
const int* level_src_orig(icp_ctx* c, const Cloud& src) {
    if (&src == &c->src) return nullptr;
    for (auto& kv : c->levels) if (&kv.second.sorted == &src) return kv.second.sorted_idx.as<int>();
    for (auto& kv : c->nss_held) if (&kv.second.lv.sorted == &src) return kv.second.lv.sorted_idx.as<int>();
    return nullptr;
}

// What k_post_gicp reads beside the post parameters: the cached GICP normals (gicp_prepare has made them current) and, when the post stage
// runs over a Morton-sorted level, that level's sorted position -> original index map.
GicpPost gicp_post_params(icp_ctx* c, const Cloud& src) {
    GicpPost g; memset(&g, 0, sizeof(g));
    const bool own_t = c->gicp_opt.covariance_k == 0, own_s = own_t;
    g.tnx = own_t ? c->tgt.nx.as<float>() : c->gicp_n[0][0].as<float>(); g.tny = own_t ? c->tgt.ny.as<float>() : c->gicp_n[0][1].as<float>(); g.tnz = own_t ? c->tgt.nz.as<float>() : c->gicp_n[0][2].as<float>();
    g.snx = own_s ? c->src.nx.as<float>() : c->gicp_n[1][0].as<float>(); g.sny = own_s ? c->src.ny.as<float>() : c->gicp_n[1][1].as<float>(); g.snz = own_s ? c->src.nz.as<float>() : c->gicp_n[1][2].as<float>();
    g.src_orig = level_src_orig(c, src);
    g.one_minus_eps = 1.0 - (double)c->gicp_opt.epsilon;
    return g;
}

// What k_post_colored reads beside the post parameters: the cached colour gradients of the target (colored_prepare has made them current).
ColoredPost colored_post_params(icp_ctx* c) {
    ColoredPost g;
    g.gx = c->col_grad[0].as<float>(); g.gy = c->col_grad[1].as<float>(); g.gz = c->col_grad[2].as<float>();
    g.lambda = (double)c->col_opt.lambda_geometric;
    return g;
}

// Trimmed / robust mode (icp_robust_options, dev_robust.hpp) is on: anything but kernel NONE with overlap 1.
bool robust_on(const icp_ctx* c) { return c->rob_opt.kernel != ICP_ROBUST_NONE || c->rob_opt.overlap < 1.f; }

// Loop start with robust mode on (run_loop, icp_correspond): the chain's state and `slots` per-iteration records allocated, the histograms
// cleared (k_robust_finish leaves them cleared; this covers a first use and a call cut short), the key buffer sized for the whole source.
int robust_prepare(icp_ctx* c, int slots) {
    int rc;
    if ((rc = ensure(c, c->rob_state, sizeof(RobustState)))) return rc;
    if ((rc = ensure(c, c->rob_stats, (size_t)(slots > 0 ? slots : 1) * sizeof(icp_robust_stats)))) return rc;
    if ((rc = ensure(c, c->rob_keys, (size_t)(c->src.n > 0 ? c->src.n : 1) * 4))) return rc;      // (no iteration queries more points)
    HIPCK(c, hipMemsetAsync(c->rob_state.p, 0, sizeof(RobustState), c->stream));
    return ICP_OK;
}

// The robust chain over the records the matcher left (no sync): keys + first histogram, two select passes, the one-block finish, trim and
// reweight.  The post kernels behind it get the records as they are (weighting CONSTANT, no rejection): see launch_post_and_solve.
int launch_robust(icp_ctx* c, const PostParams& pp, int n, icp_robust_stats* d_rstats) {
    int rc;
    if ((rc = ensure(c, c->rob_keys, (size_t)(n > 0 ? n : 1) * 4))) return rc;
    static const float standard[4] = {0.f, 1.345f, 2.3849f, 4.6851f};
    const icp_robust_options& o = c->rob_opt;
    RobustParams rp;
    rp.st = c->rob_state.as<RobustState>(); rp.keys = c->rob_keys.as<unsigned int>(); rp.stats = d_rstats;
    rp.kernel = o.kernel; rp.linear_weight = c->prm.metric == ICP_METRIC_POINT_TO_POINT ? 1 : 0;
    rp.tuning = o.tuning > 0.f ? o.tuning : standard[o.kernel]; rp.sigma = o.sigma; rp.overlap = o.overlap; rp.n = n;
    int nb = (n + ROBUST_THREADS - 1) / ROBUST_THREADS; if (nb > ROBUST_BLOCKS) nb = ROBUST_BLOCKS; if (nb < 1) nb = 1;
    hipLaunchKernelGGL(k_robust_eval, dim3(nb), dim3(ROBUST_THREADS), 0, c->stream, pp, rp);
    hipLaunchKernelGGL(k_robust_select<1>, dim3(nb), dim3(ROBUST_THREADS), 0, c->stream, rp);
    hipLaunchKernelGGL(k_robust_select<2>, dim3(nb), dim3(ROBUST_THREADS), 0, c->stream, rp);
    hipLaunchKernelGGL(k_robust_finish, dim3(1), dim3(ROBUST_THREADS), 0, c->stream, rp);
    hipLaunchKernelGGL(k_robust_apply, dim3(nb), dim3(ROBUST_THREADS), 0, c->stream, pp, rp);
    HIPCK(c, hipGetLastError());
    return ICP_OK;
}

// Reciprocal rejection (icp_reciprocal_options, dev_reciprocal.hpp) is on.
bool reciprocal_on(const icp_ctx* c) { return c->rcp_opt.enabled != 0; }

// The configurations a loop with reciprocal rejection refuses (run_loop, icp_correspond).
int reciprocal_check(icp_ctx* c) {
    if (c->prm.color_icp) { c->err = "reciprocal rejection (icp_set_reciprocal_options) does not support color_icp = 1: a 6-D forward search against a 3-D reverse one is not a mutual test"; return ICP_ERR_INVALID_ARG; }
    if (c->lm_on) { c->err = "the non-linear optimiser does not support reciprocal rejection (icp_set_reciprocal_options)"; return ICP_ERR_INVALID_ARG; }
    return ICP_OK;
}

// Loop start with reciprocal rejection on (run_loop, icp_correspond): the BVH over the full-resolution resident source current (built on
// first use; finish_source drops it), `slots` per-iteration records allocated and zero.  The build waits for the device; the loop does not.
int reciprocal_prepare(icp_ctx* c, int slots) {
    int rc;
    Bvh& b = c->src_bvh;
    if (!b.valid) {
        if ((rc = finite_list(c, c->src, false, c->src_rflag, c->src_finite, &b.n_valid))) return rc;
        b.d_finite = c->src_finite.as<int>(); b.n_ids = c->src.n; b.attrs = nullptr;
        CoordPtrs<3> cp; cp.c[0] = c->src.x.as<float>(); cp.c[1] = c->src.y.as<float>(); cp.c[2] = c->src.z.as<float>();
        if ((rc = build_bvh<3>(c, b, cp))) return rc;
    }
    const size_t bytes = (size_t)(slots > 0 ? slots : 1) * sizeof(icp_reciprocal_stats);
    if ((rc = ensure(c, c->rcp_stats, bytes))) return rc;
    HIPCK(c, hipMemsetAsync(c->rcp_stats.p, 0, bytes, c->stream));
    return ICP_OK;
}

// The reciprocal test over the records the matcher left for the query set q (no sync): one launch, one thread per query in the level's
// Morton order; non-mutual records become {-1, 0}, the counts go to d_stats (reciprocal_prepare has run).
int launch_reciprocal(icp_ctx* c, const QuerySet& q, icp_reciprocal_stats* d_stats) {
    const Bvh& b = c->src_bvh;
    CoordPtrs<3> cp; cp.c[0] = c->src.x.as<float>(); cp.c[1] = c->src.y.as<float>(); cp.c[2] = c->src.z.as<float>();
    RecipParams rp; memset(&rp, 0, sizeof(rp));
    rp.matches = c->matches.as<icp_match_t>(); rp.n = q.n; rp.order = q.order; rp.sel = q.sel; rp.src_orig = level_src_orig(c, *q.cl);
    rp.tx = c->tgt.x.as<float>(); rp.ty = c->tgt.y.as<float>(); rp.tz = c->tgt.z.as<float>();
    rp.ps = c->ps.as<PoseState>(); rp.stats = d_stats;
    rp.tree_depth = 0; while ((1 << rp.tree_depth) < b.Lp) rp.tree_depth++;
    if (c->rcp_naive) {                                      // the comparison route of tools/time_reciprocal.py: never the product's
        int rc;
        for (DevBuf& d : c->rcp_q) if ((rc = ensure(c, d, (size_t)q.n * 4))) return rc;
        if ((rc = ensure(c, c->rcp_nn, (size_t)q.n * sizeof(icp_match_t)))) return rc;
        float* qx = c->rcp_q[0].as<float>(); float* qy = c->rcp_q[1].as<float>(); float* qz = c->rcp_q[2].as<float>();
        hipLaunchKernelGGL(k_reciprocal_queries, dim3((q.n + 255) / 256), dim3(256), 0, c->stream, rp, qx, qy, qz);
        KnnParams kp; memset(&kp, 0, sizeof(kp));
        kp.sx = qx; kp.sy = qy; kp.sz = qz; kp.n = q.n; kp.tx = cp.c[0]; kp.ty = cp.c[1]; kp.tz = cp.c[2]; kp.mpad = c->src.npad;
        kp.ps = rp.ps; kp.pretransformed = 1; kp.max_dist = FLT_MAX; kp.out = c->rcp_nn.as<icp_match_t>(); kp.nseg = 1;
        kp.fault = &c->ps.as<PoseState>()->fault;
        hipLaunchKernelGGL(k_knn_bvh<3>, dim3((q.n + BVH_THREADS - 1) / BVH_THREADS), dim3(BVH_THREADS), WALK_LDS_BYTES, c->stream, kp, make_view<3>(b, cp), q.order);
        hipLaunchKernelGGL(k_reciprocal_compare, dim3((q.n + BVH_THREADS - 1) / BVH_THREADS), dim3(BVH_THREADS), 0, c->stream, rp, c->rcp_nn.as<icp_match_t>());
        HIPCK(c, hipGetLastError());
        return ICP_OK;
    }
    const size_t lds = (size_t)(rp.tree_depth + 1) * BVH_THREADS * 2;
    hipLaunchKernelGGL(k_reciprocal, dim3((q.n + BVH_THREADS - 1) / BVH_THREADS), dim3(BVH_THREADS), lds, c->stream, rp, make_view<3>(b, cp));
    HIPCK(c, hipGetLastError());
    return ICP_OK;
}

// Enqueue weight + reject + accumulate (+ symmetric second pass) + reduce/solve (no sync).  Robust mode (d_rstats: the iteration's record,
// robust_prepare has run): the robust chain first, then the post kernels on its final records.
int launch_post_and_solve(icp_ctx* c, const Cloud& src, const int* sel, int n, icp_iter_stats* d_stats, double* d_sums_out, int update_pose,
                          hipEvent_t ev_after_post, int fused_blocks = 0, icp_robust_stats* d_rstats = nullptr) {
    const icp_params& p = c->prm;
    int rc;
    if (!fused_blocks && (rc = ensure(c, c->partials, (size_t)POST_BLOCKS * NSUM * 8))) return rc;
    if (!c->totals.p && (rc = rearm_handover(c))) return rc;      // (the entry points re-arm before their first launch; this covers a first use)
    PostParams pp = make_post_params(c, src, sel, n);
    int nb = post_nblocks(n);
    if (d_rstats && !fused_blocks) {
        if ((rc = launch_robust(c, pp, n, d_rstats))) return rc;
        pp.weighting = ICP_WEIGHT_CONSTANT; pp.rejection = 0;      // post_eval takes each final weight as it is, re-applies only the validity filter
    }
    if (fused_blocks) nb = fused_blocks;                    // the matcher already wrote the block partials
    else if (p.metric == ICP_METRIC_GICP) hipLaunchKernelGGL(k_post_gicp, dim3(nb), dim3(POST_THREADS), 0, c->stream, pp, gicp_post_params(c, src));
    else if (p.metric == ICP_METRIC_COLORED) hipLaunchKernelGGL(k_post_colored, dim3(nb), dim3(POST_THREADS), 0, c->stream, pp, colored_post_params(c));
    else hipLaunchKernelGGL(k_post, dim3(nb), dim3(POST_THREADS), 0, c->stream, pp);
    SolveParams sp; memset(&sp, 0, sizeof(sp));
    // (GICP's and colored ICP's sums have point-to-plane's layout and take its solve and composition: k_reduce_solve as it is, dev_gicp.hpp)
    sp.partials = c->partials.as<double>(); sp.nblocks = nb; sp.ps = c->ps.as<PoseState>();
    sp.metric = (p.metric == ICP_METRIC_GICP || p.metric == ICP_METRIC_COLORED) ? ICP_METRIC_POINT_TO_PLANE : p.metric;
    sp.totals = c->totals.as<double>(); sp.ticket = (unsigned*)(c->totals.as<double>() + NSUM);
    sp.n_src = n; sp.update_pose = update_pose; sp.spin = 1;
    auto reduce_solve = [&]() { hipLaunchKernelGGL(k_reduce_solve, dim3(NSUM_USED), dim3(SOLVE_THREADS), 0, c->stream, sp); };
    const bool sym = p.metric == ICP_METRIC_SYMMETRIC;
    if (sym) {                                                   // first pass: the means (no record, no sums), then the second accumulation
        reduce_solve();
        hipLaunchKernelGGL(k_sym_accumulate, dim3(nb), dim3(POST_THREADS), 0, c->stream, pp);
    }
    if (ev_after_post) HIPCK(c, hipEventRecord(ev_after_post, c->stream));
    sp.phase = sym ? 1 : 0; sp.stats = d_stats; sp.sums_out = d_sums_out;
    reduce_solve();
    HIPCK(c, hipGetLastError());
    return ICP_OK;
}

// The non-linear optimiser in place of the reduce / solve (no sync): the post stage with its records kept (unless the fused matcher
// already left them), then one ceres::Solve as k_lm_eval at x = 0 + k_lm_step, and max_num_iterations more (k_lm_eval, k_lm_step)
// pairs -- enough for any solve: every step launch either ends it or leaves one candidate for the next eval, one LM iteration further
// on.  Launches after the end find the state's `done` and return.
int launch_post_and_lm(icp_ctx* c, const Cloud& src, const int* sel, int n, icp_iter_stats* d_stats, icp_lm_summary* d_summary,
                       hipEvent_t ev_after_post, int fused_blocks) {
    int rc;
    if (!fused_blocks) {
        if ((rc = ensure(c, c->partials, (size_t)POST_BLOCKS * NSUM * 8))) return rc;
        hipLaunchKernelGGL(k_post, dim3(post_nblocks(n)), dim3(POST_THREADS), 0, c->stream, make_post_params(c, src, sel, n));
    }
    if (ev_after_post) HIPCK(c, hipEventRecord(ev_after_post, c->stream));
    // [LmState | evaluation point x = 0 | the candidate's]: slot 0 written once, when the buffer is made
    const bool fresh = c->lm_state.p == nullptr;
    if ((rc = ensure(c, c->lm_state, sizeof(LmState) + 2 * sizeof(LmRot)))) return rc;
    LmRot* rots = (LmRot*)(c->lm_state.as<char>() + sizeof(LmState));
    if (fresh) hipLaunchKernelGGL(k_lm_init, dim3(1), dim3(WAVE), 0, c->stream, rots);
    if ((rc = ensure(c, c->lm_partials, (size_t)LM_NSUM * LM_BLOCKS * 8))) return rc;
    int nb = (n + LM_THREADS - 1) / LM_THREADS; if (nb > LM_BLOCKS) nb = LM_BLOCKS; if (nb < 1) nb = 1;
    LmEvalParams ep; memset(&ep, 0, sizeof(ep));
    ep.pp = make_post_params(c, src, sel, n); ep.st = c->lm_state.as<LmState>(); ep.partials = c->lm_partials.as<double>();
    static_assert(sizeof(LmState) % 8 == 0, "the evaluation points follow the state");
    LmStepParams sp; memset(&sp, 0, sizeof(sp));
    sp.partials = c->lm_partials.as<double>(); sp.nblocks = nb; sp.st = c->lm_state.as<LmState>(); sp.rot = rots + 1; sp.opt = c->lm_opt;
    sp.ps = c->ps.as<PoseState>(); sp.stats = d_stats; sp.summary = d_summary; sp.n_src = n;
    for (int k = 0; k <= c->lm_opt.max_num_iterations; k++) {
        ep.first = sp.first = k == 0 ? 1 : 0; ep.rot = rots + (k == 0 ? 0 : 1);
        hipLaunchKernelGGL(k_lm_eval, dim3(nb), dim3(LM_THREADS), 0, c->stream, ep);
        hipLaunchKernelGGL(k_lm_step, dim3(1), dim3(WAVE), 0, c->stream, sp);
    }
    HIPCK(c, hipGetLastError());
    return ICP_OK;
}

// ConvergenceMeasure::rmseAlignmentError of the resident convergence reference under the device pose state -> *d_out (device)
int enqueue_rmse(icp_ctx* c, float* d_out) {
    int rc;
    if ((rc = ensure(c, c->rmse_partials, 256 * 2 * 8))) return rc;
    hipLaunchKernelGGL(k_rmse_partial, dim3(256), dim3(256), 0, c->stream, c->conv_src.x.as<float>(), c->conv_src.y.as<float>(), c->conv_src.z.as<float>(),
                       c->conv_ref.x.as<float>(), c->conv_ref.y.as<float>(), c->conv_ref.z.as<float>(), c->conv_n, c->ps.as<PoseState>(), c->rmse_partials.as<double>());
    hipLaunchKernelGGL(k_rmse_finish, dim3(1), dim3(64), 0, c->stream, c->rmse_partials.as<double>(), 256, d_out);
    HIPCK(c, hipGetLastError());
    return ICP_OK;
}

static int enqueue_fontana(icp_ctx* c, float* d_out) {
    int rc;
    if ((rc = ensure(c, c->fontana_partials, (size_t)256 * 5 * 8))) return rc;
    double* cpart = c->fontana_partials.as<double>(); double* epart = cpart + 256 * 4;
    hipLaunchKernelGGL(k_fontana_centroid, dim3(256), dim3(256), 0, c->stream, c->conv_src.x.as<float>(), c->conv_src.y.as<float>(), c->conv_src.z.as<float>(),
                       c->conv_n, c->ps.as<PoseState>(), cpart);
    hipLaunchKernelGGL(k_fontana_error, dim3(256), dim3(256), 0, c->stream, c->conv_src.x.as<float>(), c->conv_src.y.as<float>(), c->conv_src.z.as<float>(),
                       c->conv_ref.x.as<float>(), c->conv_ref.y.as<float>(), c->conv_ref.z.as<float>(), c->conv_n, c->ps.as<PoseState>(), cpart, 256, epart);
    hipLaunchKernelGGL(k_fontana_finish, dim3(1), dim3(64), 0, c->stream, epart, 256, c->conv_n, d_out);
    HIPCK(c, hipGetLastError());
    return ICP_OK;
}
}  // namespace
