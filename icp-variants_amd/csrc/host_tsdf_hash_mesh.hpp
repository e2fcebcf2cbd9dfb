// host_tsdf_hash_mesh.hpp -- icp_tsdf_mesh_hashed: the zero level set of the context's HASHED TSDF volume as an indexed triangle mesh, extracted
// on the block pool; only the mesh crosses to the host, scratch scales with the blocks in use; icp_tsdf_mesh_color_hashed: the same mesh with
// a colour per vertex from the colour pool.  Kernels: dev_tsdf_hash_mesh.hpp, dev_tsdf_hash_mesh_color.hpp; contract: include/icp_hip.h,
// DESIGN.md sections 6y and 6zc.  From the totals on, the mesh call is host_tsdf_mesh.hpp's tm_finish with this file's fill and colour passes.
// Part of icp_hip.hip (included from there, after host_tsdf_hash.hpp and host_tsdf_mesh.hpp).
namespace {
// The context's scratch, indexed by block rank: [observed | negative | valid] words (8 per block each), the mask bytes, the run bases, the
// 27 neighbour ranks, the two block tables and the two totals, order[rank] and rank_of[pool index].
struct HtmScratch { unsigned long long *obs, *neg, *valid; uint8_t* mask; int *base, *nbr, *vblk, *tblk, *tot, *order, *rank_of; };
int htm_scratch(icp_ctx* c, int n, HtmScratch& s) {
    int rc;
    if ((rc = ensure(c, c->tm_bits, (size_t)n * 192))) return rc;
    if ((rc = ensure(c, c->tm_mask, (size_t)n * 512))) return rc;
    if ((rc = ensure(c, c->tm_base, (size_t)n * 32))) return rc;
    if ((rc = ensure(c, c->tm_nbr, (size_t)n * 108))) return rc;
    if ((rc = ensure(c, c->tm_blk, (size_t)n * 8 + 16))) return rc;
    if ((rc = ensure(c, c->tm_ord, (size_t)n * 8))) return rc;
    s.obs = c->tm_bits.as<unsigned long long>(); s.neg = s.obs + (size_t)n * 8; s.valid = s.neg + (size_t)n * 8;
    s.mask = c->tm_mask.as<uint8_t>(); s.base = c->tm_base.as<int>(); s.nbr = c->tm_nbr.as<int>();
    s.vblk = c->tm_blk.as<int>(); s.tblk = s.vblk + n; s.tot = s.tblk + n;
    s.order = c->tm_ord.as<int>(); s.rank_of = s.order + n;
    return ICP_OK;
}
// The order of the blocks: their keys to the host (8 bytes per block), (key, pool index) pairs sorted, order and rank_of uploaded.  One
// host wait; nothing is kept between calls.  h: order, then rank_of (must live until the stream has been waited for).
int htm_order(icp_ctx* c, int n, const HtmScratch& s, std::vector<int>& h) {
    HIPCK(c, hipStreamSynchronize(c->stream));
    std::vector<unsigned long long> keys((size_t)n);
    HIPCK(c, hipMemcpy(keys.data(), c->th_pkey.p, (size_t)n * 8, hipMemcpyDeviceToHost));
    std::vector<std::pair<unsigned long long, int>> order((size_t)n);
    for (int i = 0; i < n; i++) order[(size_t)i] = {keys[(size_t)i], i};
    std::sort(order.begin(), order.end());
    h.resize((size_t)n * 2);
    for (int e = 0; e < n; e++) { h[(size_t)e] = order[(size_t)e].second; h[(size_t)n + (size_t)order[(size_t)e].second] = e; }
    HIPCK(c, hipMemcpyAsync(s.order, h.data(), (size_t)n * 8, hipMemcpyHostToDevice, c->stream));
    return ICP_OK;
}
// The passes, enqueued; ev (optional): an event recorded after each of the seven steps (ev[0] .. ev[6]).
int htm_enqueue_count(icp_ctx* c, int n, const HtmScratch& s, float min_weight, Event* ev = nullptr) {
    const dim3 grid((unsigned)n), block(512);
    const unsigned long long *obs = s.obs, *neg = s.neg, *valid = s.valid;
    const int *order = s.order, *nbr = s.nbr;
    hipLaunchKernelGGL(k_htm_neighbours, dim3((unsigned)((n * 27 + 255) / 256)), dim3(256), 0, c->stream, htsdf_view(c), n, order, (const int*)s.rank_of, s.nbr);
    if (ev) HIPCK(c, hipEventRecord(ev[0].e, c->stream));
    hipLaunchKernelGGL(k_htm_classify, grid, block, 0, c->stream, (const float2*)c->th_pool.as<float2>(), order, min_weight, s.obs, s.neg);
    if (ev) HIPCK(c, hipEventRecord(ev[1].e, c->stream));
    hipLaunchKernelGGL(k_htm_cells, grid, block, 0, c->stream, nbr, obs, s.valid);
    if (ev) HIPCK(c, hipEventRecord(ev[2].e, c->stream));
    hipLaunchKernelGGL(k_htm_count, grid, block, 0, c->stream, nbr, neg, valid, s.mask, s.vblk, s.tblk);
    if (ev) HIPCK(c, hipEventRecord(ev[3].e, c->stream));
    hipLaunchKernelGGL(k_select_scan, dim3(1), dim3(1024), 0, c->stream, s.vblk, n, s.tot);
    hipLaunchKernelGGL(k_select_scan, dim3(1), dim3(1024), 0, c->stream, s.tblk, n, s.tot + 1);
    if (ev) HIPCK(c, hipEventRecord(ev[4].e, c->stream));
    HIPCK(c, hipGetLastError());
    return ICP_OK;
}
int htm_enqueue_fill(icp_ctx* c, int n, const HtmScratch& s, float* d_vert, float* d_nrm, uint32_t* d_tris, Event* ev = nullptr) {
    const dim3 grid((unsigned)n), block(512);
    hipLaunchKernelGGL(k_htm_vertices, grid, block, 0, c->stream, htsdf_view(c), (const int*)s.order, (const int*)s.nbr, (const unsigned long long*)s.valid, (const uint8_t*)s.mask,
                       (const int*)s.vblk, s.base, d_vert, d_nrm);
    if (ev) HIPCK(c, hipEventRecord(ev[5].e, c->stream));
    hipLaunchKernelGGL(k_htm_triangles, grid, block, 0, c->stream, (const int*)s.nbr, (const unsigned long long*)s.neg, (const unsigned long long*)s.valid, (const uint8_t*)s.mask,
                       (const int*)s.base, (const int*)s.tblk, d_tris);
    if (ev) HIPCK(c, hipEventRecord(ev[6].e, c->stream));
    HIPCK(c, hipGetLastError());
    return ICP_OK;
}
int htm_check_call(icp_ctx* c, float min_weight, const char* who) {
    int rc;
    if ((rc = htsdf_check(c, who))) return rc;      // no volume; a dense volume
    if (!(std::isfinite(min_weight) && min_weight >= 0.f)) { c->err = std::string(who) + ": min_weight must be finite and >= 0"; return ICP_ERR_INVALID_ARG; }
    if ((long long)c->th_nblk * 512 > (long long)(INT32_MAX / 12)) {
        char buf[160];
        snprintf(buf, sizeof(buf), "%s: the volume's %d blocks hold more than INT32_MAX / 12 voxels", who, c->th_nblk);
        c->err = buf; return ICP_ERR_INVALID_ARG;
    }
    return ICP_OK;
}
// the colour pass, enqueued after htm_enqueue_fill (it reads the run bases k_htm_vertices wrote): one packed colour per vertex
int htm_enqueue_colors(icp_ctx* c, int n, const HtmScratch& s, uint32_t* d_col) {
    hipLaunchKernelGGL(k_htm_colors, dim3((unsigned)n), dim3(512), 0, c->stream, (const float2*)c->th_pool.as<float2>(), (const float4*)c->th_cpool.as<float4>(), (const int*)s.order,
                       (const int*)s.nbr, (const uint8_t*)s.mask, (const int*)s.base, d_col);
    HIPCK(c, hipGetLastError());
    return ICP_OK;
}
// Both mesh calls.  color (icp_tsdf_mesh_color_hashed): needs the colour pool; colors_out (optional) receives one packed colour per vertex.
int htsdf_mesh(icp_ctx* c, float min_weight, int32_t max_vertices, int32_t max_triangles, float* vertices_out, float* normals_out, uint8_t* colors_out, bool color,
               uint32_t* triangles_out, int32_t* n_vertices_out, int32_t* n_triangles_out, const std::string& who, const McCall* cluster = nullptr) {
    if (n_vertices_out) *n_vertices_out = 0;
    if (n_triangles_out) *n_triangles_out = 0;
    int rc;
    if (color && (rc = htsdf_check_color(c, who.c_str()))) return rc;      // no volume; a dense volume; no colours
    if ((rc = htm_check_call(c, min_weight, who.c_str()))) return rc;
    if (!n_vertices_out || !n_triangles_out) { c->err = who + ": null count pointer"; return ICP_ERR_INVALID_ARG; }
    const bool count_only = !vertices_out && !normals_out && !colors_out && !triangles_out;
    if (!count_only && (!vertices_out || !triangles_out)) {
        c->err = who + (color ? ": vertices_out and triangles_out go together (normals_out and colors_out may be NULL)" : ": vertices_out and triangles_out go together (normals_out alone may be NULL)");
        return ICP_ERR_INVALID_ARG;
    }
    const int n = c->th_nblk;
    if (n == 0) return ICP_OK;                           // no block: no surface
    DrainOnError guard(c);
    if ((rc = set_device(c))) return rc;
    HtmScratch s;
    std::vector<int> h_order;
    if ((rc = htm_scratch(c, n, s))) return rc;
    if ((rc = htm_order(c, n, s, h_order))) return rc;
    if ((rc = htm_enqueue_count(c, n, s, min_weight))) return rc;
    return tm_finish(c, guard, s.tot, max_vertices, max_triangles, vertices_out, normals_out, colors_out, triangles_out, n_vertices_out, n_triangles_out, count_only, who,
                     [&](float* d_vert, float* d_nrm, uint32_t* d_tris) { return htm_enqueue_fill(c, n, s, d_vert, d_nrm, d_tris); },
                     [&](uint32_t* d_col) { return htm_enqueue_colors(c, n, s, d_col); }, cluster);
}
}  // namespace

int icp_tsdf_mesh_hashed(icp_ctx* c, float min_weight, int32_t max_vertices, int32_t max_triangles, float* vertices_out, float* normals_out, uint32_t* triangles_out,
                         int32_t* n_vertices_out, int32_t* n_triangles_out) {
    if (!c) return ICP_ERR_INVALID_ARG;
    return htsdf_mesh(c, min_weight, max_vertices, max_triangles, vertices_out, normals_out, nullptr, false, triangles_out, n_vertices_out, n_triangles_out, "icp_tsdf_mesh_hashed");
}
int icp_tsdf_mesh_color_hashed(icp_ctx* c, float min_weight, int32_t max_vertices, int32_t max_triangles, float* vertices_out, float* normals_out, uint8_t* colors_out,
                               uint32_t* triangles_out, int32_t* n_vertices_out, int32_t* n_triangles_out) {
    if (!c) return ICP_ERR_INVALID_ARG;
    return htsdf_mesh(c, min_weight, max_vertices, max_triangles, vertices_out, normals_out, colors_out, true, triangles_out, n_vertices_out, n_triangles_out,
                      "icp_tsdf_mesh_color_hashed");
}

// Not part of icp_hip.h (tools/time_htsdf_color_view.py): the device time of ALL passes of one icp_tsdf_mesh_color_hashed (those of
// icp_debug_htsdf_mesh_time plus the colour pass) between two events on the context's stream; a counting run outside the bracket sizes the arrays.
extern "C" int icp_debug_htsdf_mesh_color_time(icp_ctx* c, float min_weight, float* device_ms_out) {
    if (!c || !device_ms_out) return ICP_ERR_INVALID_ARG;
    const char* who = "icp_debug_htsdf_mesh_color_time";
    int rc;
    if ((rc = htsdf_check_color(c, who))) return rc;
    if ((rc = htm_check_call(c, min_weight, who))) return rc;
    const int n = c->th_nblk;
    if (n == 0) { c->err = std::string(who) + ": the volume holds no block"; return ICP_ERR_INVALID_ARG; }
    DrainOnError guard(c);
    if ((rc = set_device(c))) return rc;
    HtmScratch s;
    std::vector<int> h_order;
    if ((rc = htm_scratch(c, n, s))) return rc;
    if ((rc = htm_order(c, n, s, h_order))) return rc;
    if ((rc = htm_enqueue_count(c, n, s, min_weight))) return rc;
    int tot[2] = {0, 0};
    if ((rc = read_count(c, s.tot, tot, 2))) return rc;
    const int nv = tot[0], nt = tot[1];
    if (nv < 0 || nt < 0) { c->err = std::string(who) + ": count out of range"; return ICP_ERR_HIP; }
    const size_t bv = (size_t)nv * 12, bt = (size_t)nt * 12;
    if ((rc = ensure(c, c->tm_out, 2 * bv + bt + (size_t)nv * 4))) return rc;
    char* d = c->tm_out.as<char>();
    rc = timed_ms(c, device_ms_out, [&] {
        int r = htm_enqueue_count(c, n, s, min_weight);
        if (!r) r = htm_enqueue_fill(c, n, s, (float*)d, (float*)(d + bv), (uint32_t*)(d + 2 * bv));
        if (!r && nv > 0) r = htm_enqueue_colors(c, n, s, (uint32_t*)(d + 2 * bv + bt));
        return r;
    });
    if (rc) return rc;
    return guard.done();
}

// Not part of icp_hip.h (tools/time_htsdf_mesh.py): the device time of ALL passes of one icp_tsdf_mesh_hashed (neighbours, counting, the two
// scans, scatter, with normals) between two events on the context's stream, and the host time of the order (key download, sort, upload)
// in front of them.  A counting run outside the bracket sizes the output arrays.  pass_ms_out (optional, 7 floats): a second run with an event
// after every step -- neighbours, classify, cells, count, the two scans, vertices, triangles.  counts_out (optional): V, T, blocks.
extern "C" int icp_debug_htsdf_mesh_time(icp_ctx* c, float min_weight, float* device_ms_out, float* host_order_ms_out, float* pass_ms_out, int32_t* counts_out) {
    if (!c || !device_ms_out || !host_order_ms_out) return ICP_ERR_INVALID_ARG;
    const char* who = "icp_debug_htsdf_mesh_time";
    int rc;
    if ((rc = htm_check_call(c, min_weight, who))) return rc;
    const int n = c->th_nblk;
    if (n == 0) { c->err = std::string(who) + ": the volume holds no block"; return ICP_ERR_INVALID_ARG; }
    DrainOnError guard(c);
    if ((rc = set_device(c))) return rc;
    if ((rc = ensure_events(c, 8))) return rc;
    HtmScratch s;
    std::vector<int> h_order;
    if ((rc = htm_scratch(c, n, s))) return rc;
    HIPCK(c, hipStreamSynchronize(c->stream));
    const auto t0 = std::chrono::steady_clock::now();
    if ((rc = htm_order(c, n, s, h_order))) return rc;
    HIPCK(c, hipStreamSynchronize(c->stream));
    *host_order_ms_out = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if ((rc = htm_enqueue_count(c, n, s, min_weight))) return rc;
    int tot[2] = {0, 0};
    if ((rc = read_count(c, s.tot, tot, 2))) return rc;
    const int nv = tot[0], nt = tot[1];
    if (nv < 0 || nt < 0) { c->err = std::string(who) + ": count out of range"; return ICP_ERR_HIP; }
    if (counts_out) { counts_out[0] = nv; counts_out[1] = nt; counts_out[2] = n; }
    const size_t bv = (size_t)nv * 12, bt = (size_t)nt * 12;
    if ((rc = ensure(c, c->tm_out, 2 * bv + bt))) return rc;
    char* d = c->tm_out.as<char>();
    rc = timed_ms(c, device_ms_out, [&] {
        int r = htm_enqueue_count(c, n, s, min_weight);
        return r ? r : htm_enqueue_fill(c, n, s, (float*)d, (float*)(d + bv), (uint32_t*)(d + 2 * bv));
    });
    if (rc) return rc;
    if (pass_ms_out) {
        HIPCK(c, hipEventRecord(c->events[0], c->stream));
        if ((rc = htm_enqueue_count(c, n, s, min_weight, c->events.data() + 1))) return rc;
        if ((rc = htm_enqueue_fill(c, n, s, (float*)d, (float*)(d + bv), (uint32_t*)(d + 2 * bv), c->events.data() + 1))) return rc;
        HIPCK(c, hipStreamSynchronize(c->stream));
        for (int k = 0; k < 7; k++) HIPCK(c, hipEventElapsedTime(pass_ms_out + k, c->events[(size_t)k], c->events[(size_t)k + 1]));
    }
    return guard.done();
}
