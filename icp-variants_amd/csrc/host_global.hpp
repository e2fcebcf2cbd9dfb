// host_global.hpp -- global registration: the feature cache of a resident cloud, the feature matcher, RANSAC and their entry points
// (dev_fpfh.hpp; contract in include/icp_hip.h, icp_global_options).  Part of icp_hip.hip (included from there, after host_depth.hpp).
namespace {
constexpr int GLOBAL_MAX_HYPOTHESES = 65536, GLOBAL_MAX_BEST = 256;

bool global_k_ok(int k) { return k == 5 || k == 10 || k == 20; }

// The features of the target (which 0) or the source (1) into the context's cache: k_fpfh_spfh<k> over the target's own BVH when it
// exists, else over the scratch tree of icp_estimate_normals (as gicp_normals builds it), then k_fpfh over the keypoints.  Enqueued only.
int fpfh_features(icp_ctx* c, int which) {
    Cloud& cl = which ? c->src : c->tgt;
    if (cl.n <= 0) { c->err = which ? "no source cloud (icp_set_source)" : "no target cloud (icp_set_target)"; return which ? ICP_ERR_NO_SOURCE : ICP_ERR_NO_TARGET; }
    if (!cl.has_normals) { c->err = which ? "global registration: the source has no normals" : "global registration: the target has no normals"; return ICP_ERR_INVALID_ARG; }
    const int k = c->glob_opt.k, stride = c->glob_opt.feature_stride;
    if (!global_k_ok(k)) { c->err = "global registration: k must be 5, 10 or 20"; return ICP_ERR_INVALID_ARG; }
    FpfhCache& f = c->fpfh[which];
    if (f.ready && f.k == k && f.stride == stride && f.n == cl.n) return ICP_OK;
    f.ready = false;
    const int n = cl.n, nk = (n + stride - 1) / stride;
    int rc;
    if ((rc = ensure(c, f.nb_idx, (size_t)n * k * 4))) return rc;
    if ((rc = ensure(c, f.nb_d2, (size_t)n * k * 4))) return rc;
    if ((rc = ensure(c, f.counts, (size_t)n * FPFH_DIM))) return rc;
    if ((rc = ensure(c, f.pairs, (size_t)n * 4))) return rc;
    if ((rc = ensure(c, f.feat, (size_t)nk * FPFH_DIM * 4))) return rc;
    NeighbourTree t;
    if ((rc = neighbour_tree(c, cl, which == 0 ? &c->bvh : nullptr, c->gicp_flag, &t))) return rc;
    const float *nx = cl.nx.as<float>(), *ny = cl.ny.as<float>(), *nz = cl.nz.as<float>();
    int* ni = f.nb_idx.as<int>(); float* nd = f.nb_d2.as<float>(); uint8_t* cnt = f.counts.as<uint8_t>(); int* pr = f.pairs.as<int>();
    if (k == 5) hipLaunchKernelGGL(k_fpfh_spfh<5>, t.grid, t.block, t.lds, c->stream, t.bv, n, t.depth, nx, ny, nz, ni, nd, cnt, pr);
    else if (k == 10) hipLaunchKernelGGL(k_fpfh_spfh<10>, t.grid, t.block, t.lds, c->stream, t.bv, n, t.depth, nx, ny, nz, ni, nd, cnt, pr);
    else hipLaunchKernelGGL(k_fpfh_spfh<20>, t.grid, t.block, t.lds, c->stream, t.bv, n, t.depth, nx, ny, nz, ni, nd, cnt, pr);
    FpfhParams fp;
    fp.x = cl.x.as<float>(); fp.y = cl.y.as<float>(); fp.z = cl.z.as<float>(); fp.nx = nx; fp.ny = ny; fp.nz = nz;
    fp.stride = stride; fp.nk = nk; fp.K = k; fp.nb_idx = ni; fp.nb_d2 = nd; fp.counts = cnt; fp.pairs = pr; fp.feat = f.feat.as<float>();
    hipLaunchKernelGGL(k_fpfh, dim3((nk + 255) / 256), dim3(256), 0, c->stream, fp);
    HIPCK(c, hipGetLastError());
    f.k = k; f.stride = stride; f.n = n; f.nk = nk; f.ready = true;
    return ICP_OK;
}

// One direction of the matcher: queries qf (nq rows) against tf (nt rows) into best64 (preset to "no match" here).
int feature_match_launch(icp_ctx* c, const float* qf, int nq, const float* tf, int nt, DevBuf& best) {
    int rc;
    if ((rc = ensure(c, best, (size_t)nq * 8))) return rc;
    hipLaunchKernelGGL(k_fill_u64, dim3((nq + 255) / 256), dim3(256), 0, c->stream, best.as<unsigned long long>(), nq, ~0ull);
    const int qblocks = (nq + FM_THREADS - 1) / FM_THREADS, ntiles = (nt + FM_TILE - 1) / FM_TILE;
    int nseg = 1;                                  // few query blocks: split the target tiles so that about 1024 blocks are in flight
    while (nseg < ntiles && (long long)qblocks * nseg < 1024) nseg *= 2;
    if (nseg > ntiles) nseg = ntiles;
    hipLaunchKernelGGL(k_feature_match, dim3((unsigned)qblocks, (unsigned)nseg), dim3(FM_THREADS), 0, c->stream, qf, nq, tf, nt, nseg, best.as<unsigned long long>());
    HIPCK(c, hipGetLastError());
    return ICP_OK;
}

// Features of both clouds, the matcher (both directions with mutual = 1), the compacted list: gm_idx = [src_idx M | tgt_idx M] (at a
// stride of nk_src), gm_pts = the pairs' points (6 planes at the same stride).  Waits for the stream once (the count).
int global_correspondences(icp_ctx* c, int* m_out) {
    int rc;
    if ((rc = fpfh_features(c, 0))) return rc;
    if ((rc = fpfh_features(c, 1))) return rc;
    const FpfhCache &ft = c->fpfh[0], &fs = c->fpfh[1];
    if (ft.stride != fs.stride) { c->err = "global registration: internal error (stride)"; return ICP_ERR_INVALID_ARG; }
    const bool mutual = c->glob_opt.mutual != 0;
    if ((rc = feature_match_launch(c, fs.feat.as<float>(), fs.nk, ft.feat.as<float>(), ft.nk, c->gm_best[0]))) return rc;
    if (mutual && (rc = feature_match_launch(c, ft.feat.as<float>(), ft.nk, fs.feat.as<float>(), fs.nk, c->gm_best[1]))) return rc;
    if ((rc = ensure(c, c->gm_fwd, (size_t)fs.nk * 4))) return rc;
    if ((rc = ensure(c, c->gm_keep, (size_t)fs.nk))) return rc;
    hipLaunchKernelGGL(k_feature_match_finalize, dim3((fs.nk + 255) / 256), dim3(256), 0, c->stream, c->gm_best[0].as<unsigned long long>(),
                       mutual ? c->gm_best[1].as<unsigned long long>() : nullptr, fs.nk, c->gm_fwd.as<int>(), c->gm_keep.as<uint8_t>());
    HIPCK(c, hipGetLastError());
    int M = 0;
    if ((rc = compact_flagged(c, c->gm_keep.as<uint8_t>(), fs.nk, 1, c->gm_list, &M))) return rc;
    const size_t cap = (size_t)fs.nk;
    if ((rc = ensure(c, c->gm_idx, 2 * cap * 4))) return rc;
    if ((rc = ensure(c, c->gm_pts, 6 * cap * 4))) return rc;
    if (M > 0) {
        CorrPlanes cp;
        for (int a = 0; a < 3; a++) { cp.s[a] = c->gm_pts.as<float>() + (size_t)a * cap; cp.t[a] = c->gm_pts.as<float>() + (size_t)(3 + a) * cap; }
        const SoA3 s = {c->src.x.as<float>(), c->src.y.as<float>(), c->src.z.as<float>()}, t = {c->tgt.x.as<float>(), c->tgt.y.as<float>(), c->tgt.z.as<float>()};
        hipLaunchKernelGGL(k_corr_gather, dim3((M + 255) / 256), dim3(256), 0, c->stream, c->gm_list.as<int>(), c->gm_fwd.as<int>(), M, fs.stride, s, t,
                           c->gm_idx.as<int>(), c->gm_idx.as<int>() + cap, cp);
        HIPCK(c, hipGetLastError());
    }
    *m_out = M;
    return ICP_OK;
}

// the argument checks of the getters below
int global_getter_args(icp_ctx* c, int32_t which, int32_t max_points, bool have_out, const char* name) {
    if ((which != ICP_CLOUD_TARGET && which != ICP_CLOUD_SOURCE) || max_points < 0 || (!have_out && max_points > 0)) {
        c->err = std::string(name) + ": bad argument (which 0 or 1, max_points >= 0, output pointers non-NULL unless max_points = 0)"; return ICP_ERR_INVALID_ARG;
    }
    return ICP_OK;
}
}  // namespace

int icp_global_options_default(icp_global_options* o) {
    if (!o) return ICP_ERR_INVALID_ARG;
    o->k = 20; o->feature_stride = 1; o->mutual = 1; o->n_hypotheses = 4096; o->edge_similarity = 0.9f; o->inlier_distance = 0.005f; o->seed = 0u; o->n_best = 16;
    return ICP_OK;
}
int icp_set_global_options(icp_ctx* c, const icp_global_options* o) {
    if (!c) return ICP_ERR_INVALID_ARG;
    icp_global_options v;
    if (o) v = *o; else icp_global_options_default(&v);
    if (!global_k_ok(v.k)) { c->err = "icp_set_global_options: k must be 5, 10 or 20"; return ICP_ERR_INVALID_ARG; }
    if (v.feature_stride < 1 || (v.mutual != 0 && v.mutual != 1) || v.n_hypotheses < 1 || v.n_hypotheses > GLOBAL_MAX_HYPOTHESES || v.n_best < 1 || v.n_best > GLOBAL_MAX_BEST ||
        !(v.edge_similarity >= 0.f && v.edge_similarity <= 1.f) || !(std::isfinite(v.inlier_distance) && v.inlier_distance > 0.f)) {
        c->err = "icp_set_global_options: need feature_stride >= 1, mutual in {0, 1}, 1 <= n_hypotheses <= 65536, 1 <= n_best <= 256, 0 <= edge_similarity <= 1, inlier_distance > 0";
        return ICP_ERR_INVALID_ARG;
    }
    c->glob_opt = v;
    c->fpfh[0].ready = c->fpfh[1].ready = false;
    return ICP_OK;
}
int icp_get_global_options(const icp_ctx* c, icp_global_options* o) { if (!c || !o) return ICP_ERR_INVALID_ARG; *o = c->glob_opt; return ICP_OK; }

int icp_compute_features(icp_ctx* c, int32_t which) {
    if (!c) return ICP_ERR_INVALID_ARG;
    if (which < ICP_CLOUD_TARGET || which > ICP_CLOUD_BOTH) { c->err = "icp_compute_features: which must be ICP_CLOUD_TARGET, ICP_CLOUD_SOURCE or ICP_CLOUD_BOTH"; return ICP_ERR_INVALID_ARG; }
    int rc;
    DrainOnError guard(c);
    if ((rc = set_device(c))) return rc;
    if (which != ICP_CLOUD_SOURCE && (rc = fpfh_features(c, 0))) return rc;
    if (which != ICP_CLOUD_TARGET && (rc = fpfh_features(c, 1))) return rc;
    HIPCK(c, hipStreamSynchronize(c->stream));
    return guard.done();
}
int icp_get_features(icp_ctx* c, int32_t which, float* out, int32_t max_points, int32_t* n_out) {
    if (!c) return ICP_ERR_INVALID_ARG;
    int rc;
    if ((rc = global_getter_args(c, which, max_points, out != nullptr, "icp_get_features"))) return rc;
    DrainOnError guard(c);
    if ((rc = set_device(c))) return rc;
    if ((rc = fpfh_features(c, which))) return rc;
    const FpfhCache& f = c->fpfh[which];
    const int m = max_points < f.nk ? max_points : f.nk;
    if (n_out) *n_out = f.nk;
    if (m > 0) HIPCK(c, hipMemcpyAsync(out, f.feat.p, (size_t)m * FPFH_DIM * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCK(c, hipStreamSynchronize(c->stream));
    return guard.done();
}
int icp_get_spfh(icp_ctx* c, int32_t which, uint8_t* counts, int32_t* pairs, int32_t max_points, int32_t* n_out) {
    if (!c) return ICP_ERR_INVALID_ARG;
    int rc;
    if ((rc = global_getter_args(c, which, max_points, counts && pairs, "icp_get_spfh"))) return rc;
    DrainOnError guard(c);
    if ((rc = set_device(c))) return rc;
    if ((rc = fpfh_features(c, which))) return rc;
    const FpfhCache& f = c->fpfh[which];
    const int m = max_points < f.n ? max_points : f.n;
    if (n_out) *n_out = f.n;
    if (m > 0) {
        HIPCK(c, hipMemcpyAsync(counts, f.counts.p, (size_t)m * FPFH_DIM, hipMemcpyDeviceToHost, c->stream));
        HIPCK(c, hipMemcpyAsync(pairs, f.pairs.p, (size_t)m * 4, hipMemcpyDeviceToHost, c->stream));
    }
    HIPCK(c, hipStreamSynchronize(c->stream));
    return guard.done();
}
int icp_get_feature_neighbours(icp_ctx* c, int32_t which, int32_t* idx, float* d2, int32_t max_points, int32_t* n_out) {
    if (!c) return ICP_ERR_INVALID_ARG;
    int rc;
    if ((rc = global_getter_args(c, which, max_points, idx && d2, "icp_get_feature_neighbours"))) return rc;
    DrainOnError guard(c);
    if ((rc = set_device(c))) return rc;
    if ((rc = fpfh_features(c, which))) return rc;
    const FpfhCache& f = c->fpfh[which];
    const int m = max_points < f.n ? max_points : f.n;
    if (n_out) *n_out = f.n;
    if (m > 0) {
        HIPCK(c, hipMemcpyAsync(idx, f.nb_idx.p, (size_t)m * f.k * 4, hipMemcpyDeviceToHost, c->stream));
        HIPCK(c, hipMemcpyAsync(d2, f.nb_d2.p, (size_t)m * f.k * 4, hipMemcpyDeviceToHost, c->stream));
    }
    HIPCK(c, hipStreamSynchronize(c->stream));
    return guard.done();
}
int icp_match_features(icp_ctx* c, int32_t* src_idx, int32_t* tgt_idx, int32_t max_pairs, int32_t* m_out) {
    if (!c) return ICP_ERR_INVALID_ARG;
    if (max_pairs < 0 || (max_pairs > 0 && (!src_idx || !tgt_idx))) { c->err = "icp_match_features: bad argument (max_pairs >= 0, output pointers non-NULL unless max_pairs = 0)"; return ICP_ERR_INVALID_ARG; }
    int rc, M = 0;
    DrainOnError guard(c);
    if ((rc = set_device(c))) return rc;
    if ((rc = global_correspondences(c, &M))) return rc;
    if (m_out) *m_out = M;
    const int m = max_pairs < M ? max_pairs : M;
    if (m > 0) {
        HIPCK(c, hipMemcpyAsync(src_idx, c->gm_idx.p, (size_t)m * 4, hipMemcpyDeviceToHost, c->stream));
        HIPCK(c, hipMemcpyAsync(tgt_idx, c->gm_idx.as<int>() + c->fpfh[1].nk, (size_t)m * 4, hipMemcpyDeviceToHost, c->stream));
    }
    HIPCK(c, hipStreamSynchronize(c->stream));
    return guard.done();
}
int icp_register_global(icp_ctx* c, float* poses_out, icp_global_hypothesis* best_out, int32_t* n_out) {
    if (!c) return ICP_ERR_INVALID_ARG;
    if (!poses_out || !n_out) { c->err = "icp_register_global: poses_out and n_out must not be NULL"; return ICP_ERR_INVALID_ARG; }
    *n_out = 0;
    c->glob_last.clear();
    int rc, M = 0;
    DrainOnError guard(c);
    if ((rc = set_device(c))) return rc;
    if ((rc = global_correspondences(c, &M))) return rc;
    if (M < 3) {
        HIPCK(c, hipStreamSynchronize(c->stream));
        guard.ok = true;
        c->err = "icp_register_global: fewer than 3 feature correspondences"; return ICP_ERR_NO_CORRESPONDENCES;
    }
    const icp_global_options& o = c->glob_opt;
    const int H = o.n_hypotheses;
    if ((rc = ensure(c, c->gm_hyp, (size_t)H * sizeof(icp_global_hypothesis)))) return rc;
    RansacParams rp;
    const size_t cap = (size_t)c->fpfh[1].nk;
    for (int a = 0; a < 3; a++) { rp.s[a] = c->gm_pts.as<float>() + (size_t)a * cap; rp.t[a] = c->gm_pts.as<float>() + (size_t)(3 + a) * cap; }
    rp.M = M; rp.H = H; rp.seed = o.seed; rp.edge_similarity = (double)o.edge_similarity; rp.inlier_d2 = o.inlier_distance * o.inlier_distance;
    rp.hyp = c->gm_hyp.as<icp_global_hypothesis>();
    hipLaunchKernelGGL(k_ransac_fit, dim3((H + 63) / 64), dim3(64), 0, c->stream, rp);
    hipLaunchKernelGGL(k_ransac_score, dim3((unsigned)H), dim3(RANSAC_THREADS), 0, c->stream, rp);
    HIPCK(c, hipGetLastError());
    c->glob_last.resize((size_t)H);
    HIPCK(c, hipMemcpyAsync(c->glob_last.data(), c->gm_hyp.p, (size_t)H * sizeof(icp_global_hypothesis), hipMemcpyDeviceToHost, c->stream));
    HIPCK(c, hipStreamSynchronize(c->stream));
    guard.ok = true;
    // ranking of the valid hypotheses: more inliers, then the smaller sum, then the lower h
    std::vector<int> order;
    for (int h = 0; h < H; h++) if (c->glob_last[(size_t)h].status == ICP_GLOBAL_VALID) order.push_back(h);
    if (order.empty()) { c->err = "icp_register_global: no valid hypothesis (every draw was repeated, failed the edge test or was degenerate)"; return ICP_ERR_NO_CORRESPONDENCES; }
    const std::vector<icp_global_hypothesis>& g = c->glob_last;
    std::sort(order.begin(), order.end(), [&g](int a, int b) {
        const icp_global_hypothesis &x = g[(size_t)a], &y = g[(size_t)b];
        if (x.n_inliers != y.n_inliers) return x.n_inliers > y.n_inliers;
        if (x.sum_d2 != y.sum_d2) return x.sum_d2 < y.sum_d2;
        return a < b;
    });
    const int nb = (int)order.size() < o.n_best ? (int)order.size() : o.n_best;
    for (int r = 0; r < nb; r++) {
        memcpy(poses_out + (size_t)16 * r, g[(size_t)order[(size_t)r]].pose, 64);
        if (best_out) best_out[r] = g[(size_t)order[(size_t)r]];
    }
    *n_out = nb;
    return ICP_OK;
}
int icp_get_global_hypotheses(const icp_ctx* c, icp_global_hypothesis* out, int32_t max_out, int32_t* count_out) {
    if (!c || max_out < 0 || (!out && max_out > 0)) return ICP_ERR_INVALID_ARG;
    const int32_t n = (int32_t)c->glob_last.size();
    for (int32_t i = 0; i < n && i < max_out; i++) out[i] = c->glob_last[(size_t)i];
    if (count_out) *count_out = n;
    return ICP_OK;
}
