// host_index.hpp -- everything built once per cloud: the Morton order of the queries, the kd-ordered BVH of the target (buildIndex), the
// multi-resolution levels of the source, the bookkeeping behind a new target / source, and the k-neighbour passes over a tree (GICP
// normals, colour gradients, icp_estimate_normals).  Part of icp_hip.hip (included from there, after host_ctx.hpp).
namespace {
// Morton order of the query positions [0, n) of a selection (sel == nullptr: the full source): out[t] = position.
// rocPRIM sorts 370 k pairs with its MERGE sort (radix_sort_config's limit: 1 M items): a block sort and nine merge passes of two
// launches each -- 19 launches of ~8 us per sort, four sorts per scan (three axis orders for the index, the Morton order of the queries).
// rocPRIM's Onesweep radix sort instead (merge limit 0: a histogram launch and one pass per 8 key bits) was measured in round 3 and set
// aside: fewer launches, more time (icp_set_target 1.34-1.39 against 1.31-1.35 ms, a batch of 16 pairs 480-523 against 523-541 pairs/s).
using SortCfg = rocprim::radix_sort_config<rocprim::default_config, rocprim::default_config, rocprim::default_config, 1024 * 1024>;
int build_query_order(icp_ctx* c, const int* d_sel, int n, DevBuf& out) {
    int rc;
    if ((rc = ensure(c, c->okeys, (size_t)n * 8))) return rc;
    if ((rc = ensure(c, c->okeys2, (size_t)n * 8))) return rc;
    if ((rc = ensure(c, c->ovals, (size_t)n * 4))) return rc;
    if ((rc = ensure(c, out, (size_t)n * 4))) return rc;
    hipLaunchKernelGGL(k_query_keys, dim3((n + 255) / 256), dim3(256), 0, c->stream, c->src.x.as<float>(), c->src.y.as<float>(), c->src.z.as<float>(), d_sel, n,
                       c->src_box.as<unsigned int>(), c->okeys.as<unsigned long long>(), c->ovals.as<int>());
    size_t temp_bytes = 0;
    HIPCK(c, rocprim::radix_sort_pairs<SortCfg>(nullptr, temp_bytes, c->okeys.as<unsigned long long>(), c->okeys2.as<unsigned long long>(), c->ovals.as<int>(), out.as<int>(), (size_t)n, 0, 64, c->stream));
    if ((rc = ensure(c, c->otemp, temp_bytes))) return rc;
    HIPCK(c, rocprim::radix_sort_pairs<SortCfg>(c->otemp.p, temp_bytes, c->okeys.as<unsigned long long>(), c->okeys2.as<unsigned long long>(), c->ovals.as<int>(), out.as<int>(), (size_t)n, 0, 64, c->stream));
    HIPCK(c, hipGetLastError());
    return ICP_OK;
}

// Build the kd-ordered BVH of the resident target on the device (once per icp_set_target; = buildIndex).
template <int DIM>
int build_bvh(icp_ctx* c, Bvh& b, const CoordPtrs<DIM>& cp) {
    int rc;
    if (!c->build_ev[0]) HIPCK(c, hipEventCreate(&c->build_ev[0].e));      // owned by the context: nothing to leak on an error return
    if (!c->build_ev[1]) HIPCK(c, hipEventCreate(&c->build_ev[1].e));
    const hipEvent_t e0 = c->build_ev[0], e1 = c->build_ev[1];
    HIPCK(c, hipEventRecord(e0, c->stream));
    const int nv = b.n_valid;
    b.n_leaves = (nv + BVH_LEAF - 1) / BVH_LEAF;
    b.Lp = 1; while (b.Lp < b.n_leaves) b.Lp <<= 1;
    int depth = 0; while ((1 << depth) < b.Lp) depth++;          // internal levels 0 .. depth-1
    const int n_inner = b.Lp - 1;
    const int n_slots = (b.n_leaves > 0 ? b.n_leaves : 1) * BVH_LEAF;
    const int cap = nv > 0 ? nv : 1;
    if ((rc = ensure(c, b.keys, (size_t)cap * 4))) return rc;
    if ((rc = ensure(c, b.keys2, (size_t)cap * 4))) return rc;
    if ((rc = ensure(c, b.vals, (size_t)cap * 4))) return rc;
    if ((rc = ensure(c, b.vals2, (size_t)cap * 4))) return rc;
    if ((rc = ensure(c, b.leaves, (size_t)(n_slots / BVH_LEAF) * sizeof(BvhLeafT<DIM>)))) return rc;
    if ((rc = ensure(c, b.recs, (size_t)n_slots * sizeof(TgtRec)))) return rc;
    if ((rc = ensure(c, b.pos_of, (size_t)(b.n_ids > 0 ? b.n_ids : 1) * 4))) return rc;      // position by original index (knn_walk_shared, XW)
    if ((rc = ensure(c, b.nodes, (size_t)(n_inner > 0 ? n_inner : 1) * sizeof(BvhNodeT<DIM>)))) return rc;
    int* perm = b.vals.as<int>(); int* perm2 = b.vals2.as<int>();
    if (nv > 0) {
        // finite targets in index order (device list from icp_set_target)
        HIPCK(c, hipMemcpyAsync(perm, b.d_finite, (size_t)nv * 4, hipMemcpyDeviceToDevice, c->stream));
        const int gb = (nv + 255) / 256;
        // segment (node) size at level d in points: BVH_LEAF * Lp / 2^d = 1 << seg_shift(d)
        auto seg_shift = [&](int d) { int sh = 0; const long long seg = (long long)BVH_LEAF * b.Lp >> d; while ((1LL << sh) < seg) sh++; return sh; };
        // upper levels (slices > 2048 points) from presorted axes: see dev_bvh.hpp
        int n_upper = 0;
        while (n_upper < depth && seg_shift(n_upper) > 11) n_upper++;
        if (n_upper > 0) {
            for (int k = 0; k < 2 * DIM; k++) if ((rc = ensure(c, b.axl[k], (size_t)cap * 4))) return rc;
            if ((rc = ensure(c, b.side, (size_t)(b.n_ids > 0 ? b.n_ids : 1)))) return rc;
            if ((rc = ensure(c, b.axis_of_node, (size_t)1 << n_upper))) return rc;
            unsigned int* k32 = b.keys.as<unsigned int>(); unsigned int* k32b = b.keys2.as<unsigned int>();
            size_t tb = 0;
            HIPCK(c, rocprim::radix_sort_pairs<SortCfg>(nullptr, tb, k32, k32b, perm, perm2, (size_t)nv, 0, 32, c->stream));
            if ((rc = ensure(c, b.temp, tb))) return rc;
            const int nblk = (nv + PRS_THREADS - 1) / PRS_THREADS;
            if ((rc = ensure(c, b.scanr, (size_t)2 * DIM * nblk * 4))) return rc;
            int* blk_cnt = b.scanr.as<int>(); int* blk_off = blk_cnt + (size_t)DIM * nblk;
            int* cur[DIM]; int* alt[DIM];
            for (int k = 0; k < DIM; k++) {           // one stable sort per axis (ids arrive in increasing order: ties keep index order)
                cur[k] = b.axl[k].as<int>(); alt[k] = b.axl[DIM + k].as<int>();
                hipLaunchKernelGGL(k_axis_keys, dim3(gb), dim3(256), 0, c->stream, cp.c[k], b.d_finite, nv, k32);
                HIPCK(c, rocprim::radix_sort_pairs<SortCfg>(b.temp.p, tb, k32, k32b, b.d_finite, cur[k], (size_t)nv, 0, 32, c->stream));
            }
            for (int d = 0; d < n_upper; d++) {
                const int sh = seg_shift(d);
                AxisLists<DIM> al, ao; for (int k = 0; k < DIM; k++) { al.L[k] = cur[k]; ao.L[k] = alt[k]; }
                const int n_nodes = 1 << d;
                hipLaunchKernelGGL(k_presort_axis<DIM>, dim3((n_nodes + 255) / 256), dim3(256), 0, c->stream, cp, al, nv, sh, n_nodes, b.axis_of_node.as<unsigned char>());
                hipLaunchKernelGGL(k_presort_side<DIM>, dim3(gb), dim3(256), 0, c->stream, al, nv, sh, b.axis_of_node.as<unsigned char>(), b.side.as<unsigned char>());
                hipLaunchKernelGGL(k_presort_count<DIM>, dim3(nblk, DIM), dim3(PRS_THREADS), 0, c->stream, al, b.side.as<unsigned char>(), nv, blk_cnt);
                hipLaunchKernelGGL(k_presort_blockscan, dim3(DIM), dim3(1024), 0, c->stream, blk_cnt, nblk, blk_off);
                hipLaunchKernelGGL(k_presort_scatter<DIM>, dim3(nblk, DIM), dim3(PRS_THREADS), 0, c->stream, al, b.side.as<unsigned char>(), blk_off, nv, sh, ao);
                for (int k = 0; k < DIM; k++) { int* t = cur[k]; cur[k] = alt[k]; alt[k] = t; }
            }
            HIPCK(c, hipMemcpyAsync(perm, cur[0], (size_t)nv * 4, hipMemcpyDeviceToDevice, c->stream));      // any list: the block kernel sorts inside its slices
            HIPCK(c, hipGetLastError());
        }
        if (n_upper < depth) {                       // slices of <= 2048 points: all remaining levels inside LDS, one launch
            hipLaunchKernelGGL(k_bvh_block_levels<DIM>, dim3((nv + BLV_POINTS - 1) / BLV_POINTS), dim3(BLV_THREADS), 0, c->stream, cp, perm, nv, seg_shift(n_upper), perm2);
            int* t = perm; perm = perm2; perm2 = t;
        }
    }
    {
        const bool nrm = b.attrs && b.attrs->has_normals, col = b.attrs && b.attrs->has_colors;
        hipLaunchKernelGGL(k_bvh_gather<DIM>, dim3((n_slots + 255) / 256), dim3(256), 0, c->stream, cp,
                           nrm ? b.attrs->nx.as<float>() : nullptr, nrm ? b.attrs->ny.as<float>() : nullptr, nrm ? b.attrs->nz.as<float>() : nullptr,
                           col ? b.attrs->rgba.as<uint32_t>() : nullptr, perm, nv, n_slots, b.leaves.as<BvhLeafT<DIM>>(), b.recs.as<TgtRec>(), b.pos_of.as<int>());
    }
    for (int d = depth - 1; d >= 0; d--) {
        const int count = 1 << d, first = count - 1;
        hipLaunchKernelGGL(k_bvh_nodes<DIM>, dim3((count + 255) / 256), dim3(256), 0, c->stream, b.leaves.as<BvhLeafT<DIM>>(), b.n_leaves, b.Lp, first, count,
                           d == depth - 1 ? 1 : 0, b.nodes.as<BvhNodeT<DIM>>());
    }
    {   // 4-wide view of the same tree (two binary levels per step) for the 1-NN walk
        const int pad = depth & 1;
        b.Lq = (depth + pad) / 2;
        const long long nq = ((1ll << (2 * b.Lq)) - 1) / 3;
        if ((rc = ensure(c, b.qnodes, (size_t)(nq > 0 ? nq : 1) * sizeof(BvhQuadT<DIM>)))) return rc;
        if (nq > 0) hipLaunchKernelGGL(k_bvh_quad_nodes<DIM>, dim3((unsigned)((nq * 4 + 255) / 256)), dim3(256), 0, c->stream, b.nodes.as<BvhNodeT<DIM>>(), pad, b.Lq, b.qnodes.as<BvhQuadT<DIM>>());
    }
    HIPCK(c, hipGetLastError());
    HIPCK(c, hipEventRecord(e1, c->stream));
    HIPCK(c, hipEventSynchronize(e1));
    float ms = 0; HIPCK(c, hipEventElapsedTime(&ms, e0, e1)); b.build_ms = ms;
    b.valid = true;
    return ICP_OK;
}

CoordPtrs<3> target_coords3(const icp_ctx* c) { CoordPtrs<3> cp; cp.c[0] = c->tgt.x.as<float>(); cp.c[1] = c->tgt.y.as<float>(); cp.c[2] = c->tgt.z.as<float>(); return cp; }
CoordPtrs<6> target_coords6(const icp_ctx* c) {
    CoordPtrs<6> cp; cp.c[0] = c->tgt.x.as<float>(); cp.c[1] = c->tgt.y.as<float>(); cp.c[2] = c->tgt.z.as<float>();
    cp.c[3] = c->tgt.cr.as<float>(); cp.c[4] = c->tgt.cg.as<float>(); cp.c[5] = c->tgt.cb.as<float>(); return cp;
}

// What the kernels get of a built tree: its device arrays and sizes, and the coordinate planes it was built over.
template <int DIM>
BvhViewT<DIM> make_view(const Bvh& b, const CoordPtrs<DIM>& cp) {
    BvhViewT<DIM> bv; bv.leaves = b.leaves.as<BvhLeafT<DIM>>(); bv.nodes = b.nodes.as<BvhNodeT<DIM>>(); bv.n_valid = b.n_valid; bv.Lp = b.Lp; bv.tgt = cp;
    bv.qnodes = b.qnodes.as<BvhQuadT<DIM>>(); bv.Lq = b.Lq; bv.recs = b.recs.as<TgtRec>(); bv.pos_of = b.pos_of.as<int>();
    return bv;
}

// The tree to search a resident cloud's k nearest neighbours in, and the launch shape of the k-neighbour kernels over it (one thread per
// point): `own` when it is a valid tree over this cloud (the target's), else the scratch tree (nrm_bvh, nrm_finite) rebuilt over the cloud,
// the finite flags of that build going to `flag`.
struct NeighbourTree { BvhViewT<3> bv; int depth; dim3 grid, block; size_t lds; };
int neighbour_tree(icp_ctx* c, const Cloud& cl, Bvh* own, DevBuf& flag, NeighbourTree* t) {
    int rc;
    CoordPtrs<3> cp; cp.c[0] = cl.x.as<float>(); cp.c[1] = cl.y.as<float>(); cp.c[2] = cl.z.as<float>();
    Bvh* b = own;
    if (!b || !b->valid) {
        b = &c->nrm_bvh; b->valid = false;
        if ((rc = finite_list(c, cl, false, flag, c->nrm_finite, &b->n_valid))) return rc;
        b->d_finite = c->nrm_finite.as<int>(); b->n_ids = cl.n;
        if ((rc = build_bvh<3>(c, *b, cp))) return rc;
    }
    t->bv = make_view<3>(*b, cp);
    t->depth = 0; while ((1 << t->depth) < b->Lp) t->depth++;
    t->grid = dim3((cl.n + BVH_THREADS - 1) / BVH_THREADS); t->block = dim3(BVH_THREADS); t->lds = (size_t)(t->depth + 1) * BVH_THREADS * 2;
    return ICP_OK;
}

// Selection for a decimation factor: PointCloud::getCoarseResolution (PointCloud.h:325-343).
int get_level(icp_ctx* c, int factor, const int** d_idx, int* n_out, const int** d_order) {
    auto it = c->levels.find(factor);
    if (it == c->levels.end()) {
        Level lv;
        int rc;
        if (factor > 0) {
            const int count = (c->src.n + factor - 1) / factor;              // candidates i = 0, factor, 2 factor, ... (PointCloud.h:331)
            if ((rc = ensure(c, c->staging, (size_t)count))) return rc;
            hipLaunchKernelGGL(k_stride_flags, dim3((count + 255) / 256), dim3(256), 0, c->stream, c->src_flag.as<uint8_t>(), c->src.n, factor, count, c->staging.as<uint8_t>());
            HIPCK(c, hipGetLastError());
            if ((rc = compact_flagged(c, c->staging.as<uint8_t>(), count, factor, lv.idx, &lv.n))) return rc;
        } else lv.n = c->src.n;                                   // factor 0: every point, no index list
        it = c->levels.emplace(factor, std::move(lv)).first;
    }
    *d_idx = it->second.idx.as<int>(); *n_out = it->second.n;
    if (d_order) {
        *d_order = nullptr;
        if (it->second.n > 0) {
            if (!it->second.order.p) { int rc; if ((rc = build_query_order(c, it->second.idx.as<int>(), it->second.n, it->second.order))) return rc; }
            *d_order = it->second.order.as<int>();
        }
    }
    return ICP_OK;
}

// Morton order of the whole resident source for the stage-level entry points (results stay in source order); nullptr
// when the BVH matcher is not in use.
int get_full_order(icp_ctx* c, const int** out) {
    *out = nullptr;
    const icp_params& p = c->prm;
    if (!(p.matching == ICP_MATCH_KNN && p.knn_backend == ICP_KNN_LBVH) || c->src.n <= 0) return ICP_OK;
    const int* idx; int n;
    return get_level(c, 0, &idx, &n, out);
}

// A level's points physically permuted into Morton order (d_idx: its selection, d_order: its Morton order; n > 0).
int build_sorted_copy(icp_ctx* c, Level& lv, const int* d_idx, const int* d_order, int n) {
    int rc;
    if ((rc = ensure(c, lv.sorted_idx, (size_t)n * 4))) return rc;
    const dim3 g((n + 255) / 256), b(256);
    hipLaunchKernelGGL(k_compose_idx, g, b, 0, c->stream, d_idx, d_order, n, lv.sorted_idx.as<int>());
    const int* si = lv.sorted_idx.as<int>();
    Cloud& d = lv.sorted; const Cloud& s = c->src;
    d.n = n; d.npad = n; d.has_normals = s.has_normals; d.has_colors = s.has_colors;
    DevBuf* dst[9] = {&d.x, &d.y, &d.z, &d.nx, &d.ny, &d.nz, &d.cr, &d.cg, &d.cb};
    const DevBuf* srcp[9] = {&s.x, &s.y, &s.z, &s.nx, &s.ny, &s.nz, &s.cr, &s.cg, &s.cb};
    const size_t stride = ((size_t)n + 63) / 64 * 64;                         // elements between two planes
    if ((rc = ensure(c, lv.pack, 10 * stride * 4))) return rc;
    for (int k = 0; k < 9; k++) set_view(*dst[k], lv.pack.as<float>() + (size_t)k * stride, stride * 4);
    set_view(d.rgba, lv.pack.as<float>() + 9 * stride, stride * 4);
    for (int k = 0; k < 9; k++) {
        if (!srcp[k]->p) continue;
        hipLaunchKernelGGL(k_gather_f32, g, b, 0, c->stream, srcp[k]->as<float>(), si, n, dst[k]->as<float>());
    }
    if (s.rgba.p) hipLaunchKernelGGL(k_gather_u32, g, b, 0, c->stream, s.rgba.as<uint32_t>(), si, n, d.rgba.as<uint32_t>());
    HIPCK(c, hipGetLastError());
    lv.sorted_valid = true;
    return ICP_OK;
}
// The level's points physically permuted into Morton order (built once per icp_set_source and level).
int get_sorted_level(icp_ctx* c, int factor, const Cloud** cloud, int* n_out) {
    const int* d_idx; const int* d_order; int n, rc;
    if ((rc = get_level(c, factor, &d_idx, &n, &d_order))) return rc;
    Level& lv = c->levels[factor];
    *n_out = n;
    if (!lv.sorted_valid && n > 0 && (rc = build_sorted_copy(c, lv, d_idx, d_order, n))) return rc;
    *cloud = &lv.sorted;
    return ICP_OK;
}
// The same for a held normal-space draw, a level of its own (its index list is there already).
int get_sorted_held(icp_ctx* c, Level& lv, const Cloud** cloud) {
    int rc;
    if (!lv.sorted_valid && lv.n > 0) {
        if (!lv.order.p && (rc = build_query_order(c, lv.idx.as<int>(), lv.n, lv.order))) return rc;
        if ((rc = build_sorted_copy(c, lv, lv.idx.as<int>(), lv.order.as<int>(), lv.n))) return rc;
    }
    *cloud = &lv.sorted;
    return ICP_OK;
}
void drop_nss(icp_ctx* c, bool held_only) {
    for (auto& kv : c->nss_held) release(kv.second.lv);
    c->nss_held.clear(); c->nss_held_stale = false;
    if (held_only) return;
    for (auto& kv : c->nss_levels) release(kv.second);
    c->nss_levels.clear(); c->nss_bkt_grid = 0;
}

// Bookkeeping behind a freshly written target (icp_set_target, the promotion of a batch's source, icp_set_target_depth): the finite
// list (non-finite targets can never win the strict-< argmin: they stay out of the tree) and, for the k-NN BVH backend, buildIndex.
int finish_target(icp_ctx* c, bool with_colors) {
    int rc;
    Bvh& b = c->bvh;
    c->bvh6.valid = false;
    b.valid = false; b.n_valid = 0;
    c->gicp_ready[0] = false; c->vg_ready = false;
    c->col_ready = false;
    c->fpfh[0].ready = false;
    if ((rc = finite_list(c, c->tgt, false, c->tgt_flag, c->tgt_finite, &b.n_valid))) return rc;
    b.d_finite = c->tgt_finite.as<int>(); b.n_ids = c->tgt.n;
    c->bvh6.d_finite = b.d_finite; c->bvh6.n_valid = b.n_valid; c->bvh6.n_ids = c->tgt.n;
    b.attrs = &c->tgt; c->bvh6.attrs = &c->tgt;
    if (c->prm.knn_backend == ICP_KNN_LBVH && c->prm.matching == ICP_MATCH_KNN) {                         // buildIndex; otherwise built on first use
        if (c->prm.color_icp && with_colors) return build_bvh<6>(c, c->bvh6, target_coords6(c));
        return build_bvh<3>(c, b, target_coords3(c));
    }
    return ICP_OK;
}
// Bookkeeping behind a freshly written source (icp_set_source, icp_set_source_depth): validity of a source point for the multi-resolution
// selections (finite point && finite normal, PointCloud.h:334), the bounding box of the finite points (Morton order of the queries), and the
// selections of the previous source dropped.  Enqueued only: nothing waits for the device here.
int finish_source(icp_ctx* c) {
    int rc;
    const int n = c->src.n; const Cloud& s = c->src;
    for (auto& kv : c->levels) release(kv.second);
    c->levels.clear();
    drop_nss(c, false); c->sel_last.clear();
    c->gicp_ready[1] = false;
    c->fpfh[1].ready = false;
    c->src_bvh.valid = false;                                // the reverse index of reciprocal rejection: rebuilt at its next use
    if (n <= 0) return ICP_OK;
    if ((rc = ensure(c, c->src_flag, (size_t)n))) return rc;
    if ((rc = ensure(c, c->src_box, 32))) return rc;
    hipLaunchKernelGGL(k_mark_finite, dim3((n + 255) / 256), dim3(256), 0, c->stream, s.x.as<float>(), s.y.as<float>(), s.z.as<float>(),
                       s.has_normals ? s.nx.as<float>() : nullptr, s.has_normals ? s.ny.as<float>() : nullptr, s.has_normals ? s.nz.as<float>() : nullptr, n, c->src_flag.as<uint8_t>());
    HIPCK(c, hipMemsetAsync(c->src_box.p, 0xFF, 12, c->stream));
    HIPCK(c, hipMemsetAsync((char*)c->src_box.p + 12, 0x00, 12, c->stream));
    hipLaunchKernelGGL(k_bbox, dim3(256), dim3(256), 0, c->stream, s.x.as<float>(), s.y.as<float>(), s.z.as<float>(), n, c->src_box.as<unsigned int>());
    HIPCK(c, hipGetLastError());
    return ICP_OK;
}

// GICP normals of the target (which 0) or the source (1) into the context's cache (icp_gicp_options, dev_gicp.hpp): covariance_k = 0 reads
// the cloud's own normals (nothing to compute); otherwise k_gicp_normals<k> over the target's own BVH when it exists, else over a scratch
// tree of the cloud (icp_estimate_normals' tree and finite list: they are rebuilt by every call that uses them).  Enqueued only.
int gicp_normals(icp_ctx* c, int which) {
    Cloud& cl = which ? c->src : c->tgt;
    const int k = c->gicp_opt.covariance_k;
    if (k == 0) {
        if (!cl.has_normals) { c->err = "GICP with covariance_k = 0 needs normals on both clouds"; return ICP_ERR_INVALID_ARG; }
        return ICP_OK;
    }
    if (c->gicp_ready[which]) return ICP_OK;
    const int n = cl.n;
    int rc;
    for (DevBuf& d : c->gicp_n[which]) if ((rc = ensure(c, d, (size_t)n * 4))) return rc;
    NeighbourTree t;
    if ((rc = neighbour_tree(c, cl, which == 0 ? &c->bvh : nullptr, c->gicp_flag, &t))) return rc;
    float* o[3] = {c->gicp_n[which][0].as<float>(), c->gicp_n[which][1].as<float>(), c->gicp_n[which][2].as<float>()};
    if (k == 5) hipLaunchKernelGGL(k_gicp_normals<5>, t.grid, t.block, t.lds, c->stream, t.bv, n, t.depth, o[0], o[1], o[2]);
    else if (k == 10) hipLaunchKernelGGL(k_gicp_normals<10>, t.grid, t.block, t.lds, c->stream, t.bv, n, t.depth, o[0], o[1], o[2]);
    else hipLaunchKernelGGL(k_gicp_normals<20>, t.grid, t.block, t.lds, c->stream, t.bv, n, t.depth, o[0], o[1], o[2]);
    HIPCK(c, hipGetLastError());
    c->gicp_ready[which] = true;
    return ICP_OK;
}
// Loop start with metric = GICP (run_loop, icp_correspond): the unsupported forms refused, both clouds' GICP normals current.
int gicp_prepare(icp_ctx* c) {
    if (c->prm.metric != ICP_METRIC_GICP) return ICP_OK;
    if (c->prm.matching != ICP_MATCH_KNN) { c->err = "GICP needs k-NN matching (projective matching is not supported)"; return ICP_ERR_INVALID_ARG; }
    if (c->lm_on) { c->err = "GICP is not supported by the non-linear optimiser"; return ICP_ERR_INVALID_ARG; }
    int rc;
    if ((rc = gicp_normals(c, 0))) return rc;
    return gicp_normals(c, 1);
}

// Colour gradients of the target into the context's cache (icp_colored_options, dev_colored.hpp): k_color_gradients<k> over the target's
// own BVH when it exists, else over the scratch tree of icp_estimate_normals, as gicp_normals builds it.  Enqueued only.
int color_gradients(icp_ctx* c) {
    Cloud& cl = c->tgt;
    if (!cl.has_normals || !cl.has_colors) { c->err = "colored ICP needs a target with normals and colours"; return ICP_ERR_INVALID_ARG; }
    if (c->col_ready) return ICP_OK;
    const int n = cl.n, k = c->col_opt.gradient_k;
    int rc;
    for (DevBuf& d : c->col_grad) if ((rc = ensure(c, d, (size_t)n * 4))) return rc;
    NeighbourTree t;
    if ((rc = neighbour_tree(c, cl, &c->bvh, c->gicp_flag, &t))) return rc;
    const float *nx = cl.nx.as<float>(), *ny = cl.ny.as<float>(), *nz = cl.nz.as<float>();
    const uint32_t* rgba = cl.rgba.as<uint32_t>();
    float* o[3] = {c->col_grad[0].as<float>(), c->col_grad[1].as<float>(), c->col_grad[2].as<float>()};
    if (k == 5) hipLaunchKernelGGL(k_color_gradients<5>, t.grid, t.block, t.lds, c->stream, t.bv, n, t.depth, nx, ny, nz, rgba, o[0], o[1], o[2]);
    else if (k == 10) hipLaunchKernelGGL(k_color_gradients<10>, t.grid, t.block, t.lds, c->stream, t.bv, n, t.depth, nx, ny, nz, rgba, o[0], o[1], o[2]);
    else hipLaunchKernelGGL(k_color_gradients<20>, t.grid, t.block, t.lds, c->stream, t.bv, n, t.depth, nx, ny, nz, rgba, o[0], o[1], o[2]);
    HIPCK(c, hipGetLastError());
    c->col_ready = true;
    return ICP_OK;
}
// Loop start with metric = colored (run_loop, icp_correspond): the unsupported forms refused, the target's colour gradients current.
int colored_prepare(icp_ctx* c) {
    if (c->prm.metric != ICP_METRIC_COLORED) return ICP_OK;
    if (c->prm.matching != ICP_MATCH_KNN) { c->err = "colored ICP needs k-NN matching (projective matching is not supported)"; return ICP_ERR_INVALID_ARG; }
    if (c->lm_on) { c->err = "colored ICP is not supported by the non-linear optimiser"; return ICP_ERR_INVALID_ARG; }
    if (!c->src.has_colors) { c->err = "colored ICP needs colours on the source"; return ICP_ERR_INVALID_ARG; }
    return color_gradients(c);
}
// The first m elements of three device planes to the host, interleaved (out[3 i + q]); waits for the stream.
int download_planes3(icp_ctx* c, const DevBuf* x, const DevBuf* y, const DevBuf* z, int m, float* out) {
    const DevBuf* pl[3] = {x, y, z};
    std::vector<float> h((size_t)m * 3);
    for (int q = 0; q < 3 && m > 0; q++) HIPCK(c, hipMemcpyAsync(h.data() + (size_t)q * m, pl[q]->p, (size_t)m * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCK(c, hipStreamSynchronize(c->stream));
    for (int i = 0; i < m; i++) for (int q = 0; q < 3; q++) out[(size_t)i * 3 + q] = h[(size_t)q * m + i];
    return ICP_OK;
}
}  // namespace

int icp_set_target(icp_ctx* c, const float* xyz, const float* normals, const uint8_t* rgba, int32_t n) {
    if (!c || !xyz || n <= 0) { if (c) c->err = "icp_set_target: null points or n <= 0"; return ICP_ERR_INVALID_ARG; }
    int rc;
    DrainOnError guard(c);
    if ((rc = set_device(c))) return rc;
    if ((rc = upload_cloud(c, c->tgt, xyz, normals, rgba, n, true))) return rc;
    return guard.done(finish_target(c, rgba != nullptr));
}

// Not part of icp_hip.h (icp_batch_run's own): the resident SOURCE becomes the target -- what icp_set_target(the same arrays) would leave,
// without the trip through the host: consecutive scan pairs (k, k + 1) share scan k + 1, the source of pair k and the target of pair
// k + 1 (main.cpp:411-498 loads it twice).  Plane copies on the device (+inf padding as upload_cloud does), then the same finite filter
// and index build.  Colours are not carried (ICP_ERR_INVALID_ARG when colour ICP is on).
extern "C" int icp_internal_promote_source_to_target(icp_ctx* c) {
    if (!c) return ICP_ERR_INVALID_ARG;
    if (c->src.n <= 0) { c->err = "promote: no source cloud"; return ICP_ERR_NO_SOURCE; }
    if (c->prm.color_icp || c->prm.weighting == ICP_WEIGHT_COLORS) { c->err = "promote: colours are not carried"; return ICP_ERR_INVALID_ARG; }
    int rc;
    DrainOnError guard(c);
    if ((rc = set_device(c))) return rc;
    const Cloud& sc = c->src; Cloud& tg = c->tgt;
    const int n = sc.n, npad = ((n + 63) / 64) * 64;
    for (DevBuf* pl : {&tg.x, &tg.y, &tg.z}) if ((rc = ensure(c, *pl, (size_t)npad * 4))) return rc;
    if (sc.has_normals) for (DevBuf* pl : {&tg.nx, &tg.ny, &tg.nz}) if ((rc = ensure(c, *pl, (size_t)n * 4))) return rc;
    Planes6 pl;
    pl.s[0] = sc.x.as<float>(); pl.s[1] = sc.y.as<float>(); pl.s[2] = sc.z.as<float>();
    pl.d[0] = tg.x.as<float>(); pl.d[1] = tg.y.as<float>(); pl.d[2] = tg.z.as<float>();
    pl.s[3] = sc.has_normals ? sc.nx.as<float>() : nullptr; pl.s[4] = sc.has_normals ? sc.ny.as<float>() : nullptr; pl.s[5] = sc.has_normals ? sc.nz.as<float>() : nullptr;
    pl.d[3] = sc.has_normals ? tg.nx.as<float>() : nullptr; pl.d[4] = sc.has_normals ? tg.ny.as<float>() : nullptr; pl.d[5] = sc.has_normals ? tg.nz.as<float>() : nullptr;
    hipLaunchKernelGGL(k_copy_planes_pad, dim3((npad + 255) / 256, 6), dim3(256), 0, c->stream, pl, n, npad);
    HIPCK(c, hipGetLastError());
    tg.n = n; tg.npad = npad; tg.has_normals = sc.has_normals; tg.has_colors = false;
    c->src_bvh.valid = false;                                // the promoted scan's pair is over: its reverse index goes with it
    return guard.done(finish_target(c, false));
}

int icp_set_source(icp_ctx* c, const float* xyz, const float* normals, const uint8_t* rgba, int32_t n) {
    if (!c || !xyz || n <= 0) { if (c) c->err = "icp_set_source: null points or n <= 0"; return ICP_ERR_INVALID_ARG; }
    int rc;
    DrainOnError guard(c);
    if ((rc = set_device(c))) return rc;
    if ((rc = upload_cloud(c, c->src, xyz, normals, rgba, n, false))) return rc;
    if ((rc = finish_source(c))) return rc;
    HIPCK(c, hipStreamSynchronize(c->stream));           // entry-point contract: the caller's arrays are free, the stream is idle
    return guard.done();
}

int icp_get_color_gradients(icp_ctx* c, float* out, int32_t max_points, int32_t* n_out) {
    if (!c) return ICP_ERR_INVALID_ARG;
    if (max_points < 0 || (!out && max_points > 0)) { c->err = "icp_get_color_gradients: bad argument (max_points >= 0)"; return ICP_ERR_INVALID_ARG; }
    int rc;
    DrainOnError guard(c);
    if ((rc = set_device(c))) return rc;
    const Cloud& cl = c->tgt;
    if (cl.n <= 0) { c->err = "no target cloud (icp_set_target)"; return ICP_ERR_NO_TARGET; }
    if ((rc = color_gradients(c))) return rc;
    if (n_out) *n_out = cl.n;
    return guard.done(download_planes3(c, &c->col_grad[0], &c->col_grad[1], &c->col_grad[2], max_points < cl.n ? max_points : cl.n, out));
}
int icp_get_gicp_normals(icp_ctx* c, int32_t which, float* out, int32_t max_points, int32_t* n_out) {
    if (!c) return ICP_ERR_INVALID_ARG;
    if ((which != 0 && which != 1) || max_points < 0 || (!out && max_points > 0)) { c->err = "icp_get_gicp_normals: bad argument (which 0 or 1, max_points >= 0)"; return ICP_ERR_INVALID_ARG; }
    int rc;
    DrainOnError guard(c);
    if ((rc = set_device(c))) return rc;
    const Cloud& cl = which ? c->src : c->tgt;
    if (cl.n <= 0) { c->err = which ? "no source cloud (icp_set_source)" : "no target cloud (icp_set_target)"; return which ? ICP_ERR_NO_SOURCE : ICP_ERR_NO_TARGET; }
    if ((rc = gicp_normals(c, which))) return rc;
    const bool own = c->gicp_opt.covariance_k == 0;
    if (n_out) *n_out = cl.n;
    const DevBuf* g = c->gicp_n[which];
    return guard.done(download_planes3(c, own ? &cl.nx : &g[0], own ? &cl.ny : &g[1], own ? &cl.nz : &g[2], max_points < cl.n ? max_points : cl.n, out));
}

int icp_estimate_normals(icp_ctx* c, const float* xyz, int32_t n, int32_t k, const float viewpoint[3], float* normals_out, float* curvature_out) {
    if (!c || !xyz || !normals_out || n <= 0 || k < 3 || k > 8) { if (c) c->err = "icp_estimate_normals: bad argument (k must be 3..8)"; return ICP_ERR_INVALID_ARG; }
    int rc;
    DrainOnError guard(c);
    if ((rc = set_device(c))) return rc;
    Cloud& cl = c->nrm_cloud;
    if ((rc = upload_cloud(c, cl, xyz, nullptr, nullptr, n, false))) return rc;
    NeighbourTree t;
    if ((rc = neighbour_tree(c, cl, nullptr, c->tgt_flag, &t))) return rc;      // (tgt_flag is scratch here: only its list is kept)
    if ((rc = ensure(c, c->staging, (size_t)n * 16))) return rc;
    float* d_n = c->staging.as<float>(); float* d_c = d_n + (size_t)n * 3;
    const float vx = viewpoint ? viewpoint[0] : 0.f, vy = viewpoint ? viewpoint[1] : 0.f, vz = viewpoint ? viewpoint[2] : 0.f;
    switch (k) {
        case 3: hipLaunchKernelGGL(k_normals_knn<3>, t.grid, t.block, t.lds, c->stream, t.bv, n, t.depth, vx, vy, vz, d_n, d_c); break;
        case 4: hipLaunchKernelGGL(k_normals_knn<4>, t.grid, t.block, t.lds, c->stream, t.bv, n, t.depth, vx, vy, vz, d_n, d_c); break;
        case 5: hipLaunchKernelGGL(k_normals_knn<5>, t.grid, t.block, t.lds, c->stream, t.bv, n, t.depth, vx, vy, vz, d_n, d_c); break;
        case 6: hipLaunchKernelGGL(k_normals_knn<6>, t.grid, t.block, t.lds, c->stream, t.bv, n, t.depth, vx, vy, vz, d_n, d_c); break;
        case 7: hipLaunchKernelGGL(k_normals_knn<7>, t.grid, t.block, t.lds, c->stream, t.bv, n, t.depth, vx, vy, vz, d_n, d_c); break;
        default: hipLaunchKernelGGL(k_normals_knn<8>, t.grid, t.block, t.lds, c->stream, t.bv, n, t.depth, vx, vy, vz, d_n, d_c); break;
    }
    HIPCK(c, hipGetLastError());
    HIPCK(c, hipMemcpyAsync(normals_out, d_n, (size_t)n * 12, hipMemcpyDeviceToHost, c->stream));
    if (curvature_out) HIPCK(c, hipMemcpyAsync(curvature_out, d_c, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCK(c, hipStreamSynchronize(c->stream));
    return guard.done();
}
