// host_mesh_cluster.hpp -- icp_mesh_cluster: vertex clustering of any indexed triangle mesh, host to host; icp_tsdf_mesh_clustered: the mesh of
// the context's TSDF volume, dense or hashed, clustered where the extraction staged it, so that only the clustered mesh crosses to the host.
// Kernels: dev_mesh_cluster.hpp; contract: include/icp_hip.h, DESIGN.md section 6zk.
// Part of icp_hip.hip (included from there, after host_tsdf_mesh.hpp and host_tsdf_hash_mesh.hpp, whose tm_finish hands the staged mesh over).
namespace {
constexpr int MC_MAX_ELEMS = 1 << 27;                // vertices and triangles of a mesh to cluster
constexpr int MC_NPASS = 8;                          // timed steps: clear, vertices, classify, insert, survive + scan, leaders + scan + rank | accumulate, finalize + triangles
// One clustering call: the options, the caller's arrays and capacities, where the counts go.  device_only (icp_debug_mesh_cluster_time):
// the clustered mesh is built in mc_out and not copied; pass_ms (optional, MC_NPASS floats): an event after every step.
struct McCall {
    icp_mesh_cluster_options opt; int32_t max_vertices, max_triangles;
    float* vertices_out; float* normals_out; uint8_t* colors_out; uint32_t* triangles_out;
    icp_mesh_cluster_info* info; int32_t *n_vertices_out, *n_triangles_out;
    const char* who; bool device_only, device_normals, device_colors, combine; float* pass_ms;
};
bool mc_wants_normals(const McCall& k) { return k.device_only ? k.device_normals : k.normals_out != nullptr; }
bool mc_wants_colors(const McCall& k) { return k.device_only ? k.device_colors : k.colors_out != nullptr; }
int mc_check_options(icp_ctx* c, const icp_mesh_cluster_options* o, const char* who) {
    if (!o) { c->err = std::string(who) + ": null options"; return ICP_ERR_INVALID_ARG; }
    if (!(std::isfinite(o->cell_size) && o->cell_size > 0.f)) { c->err = std::string(who) + ": cell_size must be finite and > 0"; return ICP_ERR_INVALID_ARG; }
    if (!(std::isfinite(o->origin[0]) && std::isfinite(o->origin[1]) && std::isfinite(o->origin[2]))) { c->err = std::string(who) + ": origin must be finite"; return ICP_ERR_INVALID_ARG; }
    return ICP_OK;
}
int mc_check_outputs(icp_ctx* c, const McCall& k, bool have_normals, bool have_colors) {
    const std::string who = k.who;
    if (k.max_vertices < 0 || k.max_triangles < 0) { c->err = who + ": negative capacity"; return ICP_ERR_INVALID_ARG; }
    const bool count_only = !k.vertices_out && !k.normals_out && !k.colors_out && !k.triangles_out;
    if (!count_only && (!k.vertices_out || !k.triangles_out)) { c->err = who + ": vertices_out and triangles_out go together (normals_out and colors_out may be NULL)"; return ICP_ERR_INVALID_ARG; }
    if (k.normals_out && !have_normals) { c->err = who + ": normals_out needs normals"; return ICP_ERR_INVALID_ARG; }
    if (k.colors_out && !have_colors) { c->err = who + ": colors_out needs colors"; return ICP_ERR_INVALID_ARG; }
    return ICP_OK;
}
int mc_log2cap(int n) {                              // the smallest power of two >= 2 n, and >= 16
    int L = 4;
    while (((long long)1 << L) < 2ll * n) L++;
    return L;
}
// The clustering of a mesh that lies on the device (d_nrm, d_col: optional).  Writes k.info and the two counts; fills and copies the
// arrays unless the call only counts; waits for the stream.  The caller holds the DrainOnError guard.
int mc_run(icp_ctx* c, const McCall& k, int V, int T, const float* d_vert, const float* d_nrm, const uint32_t* d_col, const uint32_t* d_tris) {
    int rc;
    icp_mesh_cluster_info& info = *k.info;
    memset(&info, 0, sizeof(info));
    info.n_vertices_in = V; info.n_triangles_in = T;
    if (k.n_vertices_out) *k.n_vertices_out = 0;
    if (k.n_triangles_out) *k.n_triangles_out = 0;
    if (k.pass_ms) for (int a = 0; a < MC_NPASS; a++) k.pass_ms[a] = 0.f;
    if (V == 0) { info.n_invalid_triangles = T; return ICP_OK; }      // no vertex: every index is out of range
    const std::string who = k.who;
    const bool timed = k.pass_ms != nullptr;
    if (timed && (rc = ensure_events(c, MC_NPASS + 2))) return rc;
    auto mark = [&](int e) -> int { if (timed) HIPCK(c, hipEventRecord(c->events[(size_t)e], c->stream)); return ICP_OK; };
    const McGrid g = {k.opt.cell_size, {k.opt.origin[0], k.opt.origin[1], k.opt.origin[2]}};
    const int Lc = mc_log2cap(V), Lt = mc_log2cap(T > 0 ? T : 1), nbv = (V + 255) / 256, nbt = (T + 255) / 256;
    const size_t capc = (size_t)1 << Lc, capt = (size_t)1 << Lt;
    // scratch: the cell table [keys 8 | first 4 | ref 4] per slot; per vertex [slot | cluster slot by rank], the leader block table, the counters;
    // per triangle the canonical triple (16 bytes), its slot, the triangle table, the survivor block table
    if ((rc = ensure(c, c->mc_tab, capc * 16))) return rc;
    if ((rc = ensure(c, c->mc_vtx, ((size_t)V * 2 + (size_t)nbv + MC_NCTR) * 4))) return rc;
    if (T > 0 && (rc = ensure(c, c->mc_tri, (size_t)T * 20 + capt * 4 + (size_t)nbt * 4))) return rc;
    unsigned long long* keys = c->mc_tab.as<unsigned long long>(); unsigned* first = (unsigned*)(keys + capc); int* ref = (int*)(first + capc);
    int* vslot = c->mc_vtx.as<int>(); int* cl_slot = vslot + V; int* vblk = cl_slot + V; int* ctr = vblk + nbv;
    uint4* canon = c->mc_tri.as<uint4>(); unsigned* ttab = (unsigned*)(canon + T); int* tslot = (int*)(ttab + capt); int* tblk = tslot + T;
    const dim3 gv((unsigned)nbv), gt((unsigned)nbt), b(256);
    if ((rc = mark(0))) return rc;
    HIPCK(c, hipMemsetAsync(keys, 0xFF, capc * 12, c->stream));
    HIPCK(c, hipMemsetAsync(ref, 0, capc * 4, c->stream));
    HIPCK(c, hipMemsetAsync(ctr, 0, MC_NCTR * 4, c->stream));
    if (T > 0) HIPCK(c, hipMemsetAsync(ttab, 0xFF, capt * 4, c->stream));
    if ((rc = mark(1))) return rc;
    hipLaunchKernelGGL(k_mc_vertices, gv, b, 0, c->stream, V, d_vert, g, keys, Lc, first, vslot, ctr);
    if ((rc = mark(2))) return rc;
    if (T > 0) {
        hipLaunchKernelGGL(k_mc_classify, gt, b, 0, c->stream, V, T, d_tris, (const int*)vslot, (const unsigned*)first, canon, ctr);
        if ((rc = mark(3))) return rc;
        hipLaunchKernelGGL(k_mc_tri_insert, gt, b, 0, c->stream, T, (const uint4*)canon, ttab, Lt, tslot);
        if ((rc = mark(4))) return rc;
        hipLaunchKernelGGL(k_mc_survive, gt, b, 0, c->stream, V, T, d_tris, (const int*)vslot, (const uint4*)canon, (const int*)tslot, (const unsigned*)ttab, ref, tblk, ctr);
        hipLaunchKernelGGL(k_select_scan, dim3(1), dim3(1024), 0, c->stream, tblk, nbt, ctr + MC_TRIANGLES);
        if ((rc = mark(5))) return rc;
        hipLaunchKernelGGL(k_mc_leaders, gv, b, 0, c->stream, V, (const int*)vslot, (const unsigned*)first, (const int*)ref, vblk);
        hipLaunchKernelGGL(k_select_scan, dim3(1), dim3(1024), 0, c->stream, vblk, nbv, ctr + MC_VERTICES);
        hipLaunchKernelGGL(k_mc_rank, gv, b, 0, c->stream, V, (const int*)vslot, (const unsigned*)first, ref, (const int*)vblk, cl_slot);
        if ((rc = mark(6))) return rc;
    } else {
        for (int e = 3; e <= 6; e++) if ((rc = mark(e))) return rc;
    }
    HIPCK(c, hipGetLastError());
    int h[MC_NCTR];                                      // the counters and both totals back in one copy: the call's only wait before the outputs
    if ((rc = read_count(c, ctr, h, MC_NCTR))) return rc;
    if (timed) for (int a = 0; a < 6; a++) HIPCK(c, hipEventElapsedTime(k.pass_ms + a, c->events[(size_t)a], c->events[(size_t)a + 1]));
    const int nv = h[MC_VERTICES], nt = h[MC_TRIANGLES];
    if (nv < 0 || nt < 0 || nv > V || nt > T) { c->err = who + ": count out of range"; return ICP_ERR_HIP; }
    info.n_invalid_vertices = h[MC_INVALID_V]; info.n_invalid_triangles = h[MC_INVALID_T]; info.n_cells = h[MC_CELLS];
    info.n_degenerate = h[MC_DEGENERATE]; info.n_duplicate = h[MC_DUPLICATE]; info.n_vertices = nv; info.n_triangles = nt;
    if (k.n_vertices_out) *k.n_vertices_out = nv;
    if (k.n_triangles_out) *k.n_triangles_out = nt;
    const bool count_only = !k.device_only && !k.vertices_out && !k.normals_out && !k.colors_out && !k.triangles_out;
    if (count_only) return ICP_OK;
    if (!k.device_only && (nv > k.max_vertices || nt > k.max_triangles)) {
        char buf[240];
        snprintf(buf, sizeof(buf), "%s: the clustered mesh has %d vertices and %d triangles, the arrays hold %d and %d", k.who, nv, nt, k.max_vertices, k.max_triangles);
        c->err = buf;
        return ICP_ERR_INVALID_ARG;                      // (synchronised by the count read)
    }
    if (nv == 0) return ICP_OK;                          // (then no triangle survived either)
    const bool with_n = mc_wants_normals(k) && d_nrm, with_c = mc_wants_colors(k) && d_col;
    // the accumulators, by rank: [S 24 | M 24 | C 24 | n 4 | k 4] bytes per cluster, the planes a call does not need left out
    const size_t pl = (size_t)nv * 24;
    if ((rc = ensure(c, c->mc_acc, pl * (1 + (with_n ? 1 : 0) + (with_c ? 1 : 0)) + (size_t)nv * 8))) return rc;
    McAcc A;
    char* a = c->mc_acc.as<char>();
    A.nv = nv; A.S = (unsigned long long*)a; a += pl;
    A.M = with_n ? (unsigned long long*)a : nullptr; if (with_n) a += pl;
    A.C = with_c ? (unsigned long long*)a : nullptr; if (with_c) a += pl;
    A.n = (unsigned*)a; A.k = A.n + nv;
    // the clustered mesh staged like tm_out: [vertices 12 V | normals 12 V | triangles 12 T | colours 4 V]
    const size_t bv = (size_t)nv * 12, bn = with_n ? bv : 0, bt = (size_t)nt * 12, bc = with_c ? (size_t)nv * 4 : 0;
    if ((rc = ensure(c, c->mc_out, bv + bn + bt + bc))) return rc;
    char* d = c->mc_out.as<char>();
    float* o_vert = (float*)d; float* o_nrm = with_n ? (float*)(d + bv) : nullptr; uint32_t* o_tris = (uint32_t*)(d + bv + bn);
    uint32_t* o_col = with_c ? (uint32_t*)(d + bv + bn + bt) : nullptr;
    if ((rc = mark(7))) return rc;
    HIPCK(c, hipMemsetAsync(c->mc_acc.p, 0, (size_t)((char*)(A.k + nv) - c->mc_acc.as<char>()), c->stream));
    if (k.combine) hipLaunchKernelGGL(k_mc_accumulate<true>, gv, b, 0, c->stream, V, d_vert, with_n ? d_nrm : nullptr, with_c ? d_col : nullptr, g, (const int*)vslot, (const int*)ref, A);
    else hipLaunchKernelGGL(k_mc_accumulate<false>, gv, b, 0, c->stream, V, d_vert, with_n ? d_nrm : nullptr, with_c ? d_col : nullptr, g, (const int*)vslot, (const int*)ref, A);
    if ((rc = mark(8))) return rc;
    hipLaunchKernelGGL(k_mc_finalize, dim3((unsigned)((nv + 255) / 256)), b, 0, c->stream, g, (const unsigned long long*)keys, (const int*)cl_slot, A, o_vert, o_nrm, o_col);
    hipLaunchKernelGGL(k_mc_triangles, gt, b, 0, c->stream, V, T, d_tris, (const int*)vslot, (const uint4*)canon, (const int*)tslot, (const unsigned*)ttab, (const int*)ref,
                       (const int*)tblk, o_tris);
    if ((rc = mark(9))) return rc;
    HIPCK(c, hipGetLastError());
    if (!k.device_only) {
        HIPCK(c, hipMemcpyAsync(k.vertices_out, o_vert, bv, hipMemcpyDeviceToHost, c->stream));
        if (with_n) HIPCK(c, hipMemcpyAsync(k.normals_out, o_nrm, bn, hipMemcpyDeviceToHost, c->stream));
        if (with_c) HIPCK(c, hipMemcpyAsync(k.colors_out, o_col, bc, hipMemcpyDeviceToHost, c->stream));
        if (nt > 0) HIPCK(c, hipMemcpyAsync(k.triangles_out, o_tris, bt, hipMemcpyDeviceToHost, c->stream));
    }
    HIPCK(c, hipStreamSynchronize(c->stream));
    if (timed) for (int e = 6; e < MC_NPASS; e++) HIPCK(c, hipEventElapsedTime(k.pass_ms + e, c->events[(size_t)e + 1], c->events[(size_t)e + 2]));
    return ICP_OK;
}
// tm_finish's clustered tail: the staged mesh (m: null for an empty one) clustered where it lies.
int mc_finish_staged(icp_ctx* c, DrainOnError& guard, const McCall& k, int nv, int nt, const TmStaged* m) {
    if (nv > MC_MAX_ELEMS || nt > MC_MAX_ELEMS) {
        char buf[240];
        snprintf(buf, sizeof(buf), "%s: the mesh to cluster has %d vertices and %d triangles, more than 2^27", k.who, nv, nt);
        c->err = buf;
        return guard.done(ICP_ERR_INVALID_ARG);
    }
    const int rc = mc_run(c, k, nv, nt, m ? m->d_vert : nullptr, m ? m->d_nrm : nullptr, m && m->bc ? m->d_col : nullptr, m ? m->d_tris : nullptr);
    return guard.done(rc);
}
void mc_zero(icp_mesh_cluster_info* info, int32_t* nv, int32_t* nt) {
    if (info) memset(info, 0, sizeof(*info));
    if (nv) *nv = 0;
    if (nt) *nt = 0;
}
// The volume's mesh call with the clustered tail: dense or hashed, as the context holds it.
int mc_volume_mesh(icp_ctx* c, float min_weight, bool color, const McCall& k) {
    if (!c->tsdf_on) { c->err = std::string(k.who) + ": no volume (icp_tsdf_create / icp_tsdf_create_hashed)"; return ICP_ERR_INVALID_ARG; }
    int32_t nv = 0, nt = 0;                              // (the mesh calls want their count pointers; the clustered counts go through k)
    if (c->tsdf_hashed) return htsdf_mesh(c, min_weight, k.max_vertices, k.max_triangles, k.vertices_out, k.normals_out, k.colors_out, color, k.triangles_out, &nv, &nt, k.who, &k);
    return tsdf_mesh(c, min_weight, k.max_vertices, k.max_triangles, k.vertices_out, k.normals_out, k.colors_out, color, k.triangles_out, &nv, &nt, k.who, &k);
}
}  // namespace

int icp_mesh_cluster(icp_ctx* c, int32_t n_vertices, int32_t n_triangles, const float* vertices, const float* normals, const uint8_t* colors, const uint32_t* triangles,
                     const icp_mesh_cluster_options* opt, int32_t max_vertices, int32_t max_triangles, float* vertices_out, float* normals_out, uint8_t* colors_out,
                     uint32_t* triangles_out, icp_mesh_cluster_info* info_out) {
    if (!c) return ICP_ERR_INVALID_ARG;
    const char* who = "icp_mesh_cluster";
    if (!info_out) { c->err = std::string(who) + ": null info_out"; return ICP_ERR_INVALID_ARG; }
    mc_zero(info_out, nullptr, nullptr);
    int rc;
    if ((rc = mc_check_options(c, opt, who))) return rc;
    if (n_vertices < 0 || n_vertices > MC_MAX_ELEMS || n_triangles < 0 || n_triangles > MC_MAX_ELEMS) { c->err = std::string(who) + ": n_vertices and n_triangles must lie in 0 .. 2^27"; return ICP_ERR_INVALID_ARG; }
    if ((n_vertices > 0 && !vertices) || (n_triangles > 0 && !triangles)) { c->err = std::string(who) + ": null vertices or triangles"; return ICP_ERR_INVALID_ARG; }
    const McCall k = {*opt, max_vertices, max_triangles, vertices_out, normals_out, colors_out, triangles_out, info_out, nullptr, nullptr, who, false, false, false, c->mc_combine, nullptr};
    if ((rc = mc_check_outputs(c, k, normals != nullptr, colors != nullptr))) return rc;
    DrainOnError guard(c);
    if ((rc = set_device(c))) return rc;
    const int V = n_vertices, T = n_triangles;
    // the input staged like tm_out: [vertices 12 V | normals 12 V | triangles 12 T | colours 4 V]
    const size_t bv = (size_t)V * 12, bn = normals ? bv : 0, bt = (size_t)T * 12, bc = colors ? (size_t)V * 4 : 0;
    if ((rc = ensure(c, c->mc_in, bv + bn + bt + bc))) return rc;
    char* d = c->mc_in.as<char>();
    if (V > 0) HIPCK(c, hipMemcpyAsync(d, vertices, bv, hipMemcpyHostToDevice, c->stream));
    if (V > 0 && normals) HIPCK(c, hipMemcpyAsync(d + bv, normals, bn, hipMemcpyHostToDevice, c->stream));
    if (T > 0) HIPCK(c, hipMemcpyAsync(d + bv + bn, triangles, bt, hipMemcpyHostToDevice, c->stream));
    if (V > 0 && colors) HIPCK(c, hipMemcpyAsync(d + bv + bn + bt, colors, bc, hipMemcpyHostToDevice, c->stream));
    rc = mc_run(c, k, V, T, (const float*)d, normals ? (const float*)(d + bv) : nullptr, colors ? (const uint32_t*)(d + bv + bn + bt) : nullptr, (const uint32_t*)(d + bv + bn));
    if (rc) return rc;
    HIPCK(c, hipStreamSynchronize(c->stream));
    return guard.done();
}

int icp_tsdf_mesh_clustered(icp_ctx* c, float min_weight, const icp_mesh_cluster_options* opt, int32_t with_colors, int32_t max_vertices, int32_t max_triangles,
                            float* vertices_out, float* normals_out, uint8_t* colors_out, uint32_t* triangles_out, int32_t* n_vertices_out, int32_t* n_triangles_out,
                            icp_mesh_cluster_info* info_out) {
    if (!c) return ICP_ERR_INVALID_ARG;
    const char* who = "icp_tsdf_mesh_clustered";
    mc_zero(info_out, n_vertices_out, n_triangles_out);
    if (!info_out || !n_vertices_out || !n_triangles_out) { c->err = std::string(who) + ": null count or info pointer"; return ICP_ERR_INVALID_ARG; }
    int rc;
    if ((rc = mc_check_options(c, opt, who))) return rc;
    const McCall k = {*opt, max_vertices, max_triangles, vertices_out, normals_out, colors_out, triangles_out, info_out, n_vertices_out, n_triangles_out, who, false, false, false, c->mc_combine, nullptr};
    if ((rc = mc_check_outputs(c, k, true, with_colors != 0))) return rc;
    return mc_volume_mesh(c, min_weight, with_colors != 0, k);
}

// Not part of icp_hip.h (tools/time_mesh_cluster.py): the device time of every clustering step of one icp_tsdf_mesh_clustered with normals
// (and colours with with_colors), an event after each -- pass_ms_out: MC_NPASS floats, clear, vertices, classify, insert, survive + scan,
// leaders + scan + rank, accumulate (with its clear), finalize + triangles.  The clustered mesh stays on the device.  combine: the form of
// the accumulate to time (1: neighbouring lanes combined, 0: one set of atomic adds per vertex); info_out: the counts of the run.
extern "C" int icp_debug_mesh_cluster_time(icp_ctx* c, float min_weight, const icp_mesh_cluster_options* opt, int32_t with_colors, int32_t combine, float* pass_ms_out,
                                           icp_mesh_cluster_info* info_out) {
    if (!c || !pass_ms_out || !info_out) return ICP_ERR_INVALID_ARG;
    const char* who = "icp_debug_mesh_cluster_time";
    int rc;
    if ((rc = mc_check_options(c, opt, who))) return rc;
    int32_t nv = 0, nt = 0;
    const McCall k = {*opt, 0, 0, nullptr, nullptr, nullptr, nullptr, info_out, &nv, &nt, who, true, true, with_colors != 0, combine != 0, pass_ms_out};
    return mc_volume_mesh(c, min_weight, with_colors != 0, k);
}
