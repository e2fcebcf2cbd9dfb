// host_tsdf_mesh.hpp -- icp_tsdf_mesh: the zero level set of the context's TSDF volume as an indexed triangle mesh, extracted on the device;
// only the mesh crosses to the host; icp_tsdf_mesh_color: the same mesh with a colour per vertex from the volume's colour array.
// Kernels: dev_tsdf_mesh.hpp, dev_tsdf_mesh_color.hpp; contract: include/icp_hip.h, DESIGN.md sections 6n and 6p.
// tm_finish, the tail both storages' mesh calls share from the totals on, lives here (host_tsdf_hash_mesh.hpp passes its own passes in);
// tm_stage is its seam between the mesh filled on the device and the copy back, where icp_tsdf_mesh_clustered takes the mesh over.
// Part of icp_hip.hip (included from there, after host_tsdf.hpp).
namespace {
TmDiv tm_make_div(uint32_t d) {
    int L = 0;
    while (((uint64_t)1 << L) < d) L++;
    TmDiv r;
    r.m = (uint32_t)((((uint64_t)1 << 32) * (((uint64_t)1 << L) - d)) / d + 1);
    r.s1 = L < 1 ? L : 1; r.s2 = L > 1 ? L - 1 : 0;
    return r;
}
TmGrid tm_grid(const icp_ctx* c) {
    const icp_tsdf_options& o = c->tsdf_opt;
    TmGrid g;
    g.nx = o.dims[0]; g.ny = o.dims[1]; g.nz = o.dims[2];
    g.plane = g.nx * g.ny; g.n = g.plane * g.nz; g.nruns = (g.n + 63) / 64;
    g.dx = tm_make_div((uint32_t)g.nx); g.dp = tm_make_div((uint32_t)g.plane);
    return g;
}
int tm_blocks(const TmGrid& g) { return (g.n + TM_BLOCK_VOXELS - 1) / TM_BLOCK_VOXELS; }
// The context's scratch: [observed | negative | valid] bitmaps, the mask bytes, the run bases, the two block tables, the two totals.
struct TmScratch { unsigned long long *obs, *neg, *valid; uint8_t* mask; int *base, *vblk, *tblk, *tot; };
int tm_scratch(icp_ctx* c, const TmGrid& g, TmScratch& s) {
    int rc;
    const int nb = tm_blocks(g);
    if ((rc = ensure(c, c->tm_bits, (size_t)g.nruns * 24))) return rc;
    if ((rc = ensure(c, c->tm_mask, (size_t)g.nruns * 64))) return rc;
    if ((rc = ensure(c, c->tm_base, (size_t)g.nruns * 4))) return rc;
    if ((rc = ensure(c, c->tm_blk, (size_t)nb * 8 + 16))) return rc;
    s.obs = c->tm_bits.as<unsigned long long>(); s.neg = s.obs + g.nruns; s.valid = s.neg + g.nruns;
    s.mask = c->tm_mask.as<uint8_t>(); s.base = c->tm_base.as<int>();
    s.vblk = c->tm_blk.as<int>(); s.tblk = s.vblk + nb; s.tot = s.tblk + nb;
    return ICP_OK;
}
// The counting passes, enqueued: bitmaps, mask bytes, the two block tables scanned into offsets, the totals in s.tot[0..1].
int tm_enqueue_count(icp_ctx* c, const TmGrid& g, const TmScratch& s, float min_weight) {
    const dim3 grid((unsigned)tm_blocks(g)), block(256);
    hipLaunchKernelGGL(k_tm_classify, grid, block, 0, c->stream, (const float2*)c->tsdf_vox.as<float2>(), g, min_weight, s.obs, s.neg);
    hipLaunchKernelGGL(k_tm_cells, grid, block, 0, c->stream, g, (const unsigned long long*)s.obs, s.valid);
    hipLaunchKernelGGL(k_tm_count, grid, block, 0, c->stream, g, (const unsigned long long*)s.neg, (const unsigned long long*)s.valid, s.mask, s.vblk, s.tblk);
    hipLaunchKernelGGL(k_select_scan, dim3(1), dim3(1024), 0, c->stream, s.vblk, tm_blocks(g), s.tot);
    hipLaunchKernelGGL(k_select_scan, dim3(1), dim3(1024), 0, c->stream, s.tblk, tm_blocks(g), s.tot + 1);
    HIPCK(c, hipGetLastError());
    return ICP_OK;
}
// The scatter passes, enqueued, into device arrays of the counted sizes (d_nrm may be null).
int tm_enqueue_fill(icp_ctx* c, const TmGrid& g, const TmScratch& s, float* d_vert, float* d_nrm, uint32_t* d_tris) {
    const dim3 grid((unsigned)tm_blocks(g)), block(256);
    hipLaunchKernelGGL(k_tm_vertices, grid, block, 0, c->stream, tsdf_view(c), g, (const unsigned long long*)s.valid, (const uint8_t*)s.mask, (const int*)s.vblk, s.base, d_vert, d_nrm);
    hipLaunchKernelGGL(k_tm_triangles, grid, block, 0, c->stream, g, (const unsigned long long*)s.neg, (const unsigned long long*)s.valid, (const uint8_t*)s.mask, (const int*)s.base,
                       (const int*)s.tblk, d_tris);
    HIPCK(c, hipGetLastError());
    return ICP_OK;
}
int tm_check_call(icp_ctx* c, float min_weight, const char* who) {
    if (!c->tsdf_on) { c->err = std::string(who) + ": no volume (icp_tsdf_create)"; return ICP_ERR_INVALID_ARG; }
    if (int rd = tsdf_check_dense(c, who)) return rd;
    if (!(std::isfinite(min_weight) && min_weight >= 0.f)) { c->err = std::string(who) + ": min_weight must be finite and >= 0"; return ICP_ERR_INVALID_ARG; }
    if (tsdf_voxels(c) > (size_t)(INT32_MAX / 12)) { c->err = std::string(who) + ": the volume has more than INT32_MAX / 12 voxels"; return ICP_ERR_INVALID_ARG; }
    return ICP_OK;
}
// The seam between "filled on the device" and "copied back": a mesh of the counted sizes staged in tm_out, [vertices 12 V | normals 12 V |
// triangles 12 T | colours 4 V], with fill(d_vert, d_nrm, d_tris) and -- when colours are asked for -- colors(d_col) enqueued.
struct TmStaged { float* d_vert; float* d_nrm; uint32_t* d_tris; uint32_t* d_col; size_t bv, bn, bt, bc; };
template <class Fill, class Colors>
int tm_stage(icp_ctx* c, int nv, int nt, bool with_normals, bool with_colors, TmStaged& m, Fill&& fill, Colors&& colors) {
    int rc;
    m.bv = (size_t)nv * 12; m.bn = with_normals ? m.bv : 0; m.bt = (size_t)nt * 12; m.bc = with_colors ? (size_t)nv * 4 : 0;
    if ((rc = ensure(c, c->tm_out, m.bv + m.bn + m.bt + m.bc))) return rc;
    char* d = c->tm_out.as<char>();
    m.d_vert = (float*)d; m.d_nrm = with_normals ? (float*)(d + m.bv) : nullptr; m.d_tris = (uint32_t*)(d + m.bv + m.bn);
    m.d_col = (uint32_t*)(d + m.bv + m.bn + m.bt);
    if ((rc = fill(m.d_vert, m.d_nrm, m.d_tris))) return rc;
    if (with_colors && nv > 0 && (rc = colors(m.d_col))) return rc;
    return ICP_OK;
}
// The clustered tail (host_mesh_cluster.hpp, icp_tsdf_mesh_clustered): what a mesh call hands the staged mesh to instead of copying it back.
struct McCall;
int mc_finish_staged(icp_ctx* c, DrainOnError& guard, const McCall& k, int nv, int nt, const TmStaged* m);
bool mc_wants_normals(const McCall& k);
bool mc_wants_colors(const McCall& k);
// What both storages' mesh calls do once the counting passes are enqueued: the two totals back in one copy, the counts reported and
// checked against the arrays, the outputs staged (tm_stage), the arrays copied back, the stream waited for.  cluster: the staged mesh
// goes to mc_finish_staged where it lies, and the counts, the capacities and the arrays are that call's.
template <class Fill, class Colors>
int tm_finish(icp_ctx* c, DrainOnError& guard, const int* d_tot, int32_t max_vertices, int32_t max_triangles, float* vertices_out, float* normals_out, uint8_t* colors_out,
              uint32_t* triangles_out, int32_t* n_vertices_out, int32_t* n_triangles_out, bool count_only, const std::string& who, Fill&& fill, Colors&& colors,
              const McCall* cluster = nullptr) {
    int rc;
    int tot[2] = {0, 0};                                 // both totals back in one copy
    if ((rc = read_count(c, d_tot, tot, 2))) return rc;
    const int nv = tot[0], nt = tot[1];
    if (nv < 0 || nt < 0) { c->err = who + ": count out of range"; return ICP_ERR_HIP; }
    TmStaged m;
    if (cluster) {
        if (nv == 0 && nt == 0) return mc_finish_staged(c, guard, *cluster, 0, 0, nullptr);
        if ((rc = tm_stage(c, nv, nt, mc_wants_normals(*cluster), mc_wants_colors(*cluster), m, fill, colors))) return rc;
        return mc_finish_staged(c, guard, *cluster, nv, nt, &m);
    }
    *n_vertices_out = nv; *n_triangles_out = nt;
    if (count_only) return guard.done();
    if (nv > max_vertices || nt > max_triangles) {
        char buf[200];
        snprintf(buf, sizeof(buf), "%s: the mesh has %d vertices and %d triangles, the arrays hold %d and %d", who.c_str(), nv, nt, max_vertices, max_triangles);
        c->err = buf;
        return guard.done(ICP_ERR_INVALID_ARG);      // (synchronised by the count read)
    }
    if (nv == 0 && nt == 0) return guard.done();
    if ((rc = tm_stage(c, nv, nt, normals_out != nullptr, colors_out != nullptr, m, fill, colors))) return rc;
    if (colors_out && nv > 0) HIPCK(c, hipMemcpyAsync(colors_out, m.d_col, m.bc, hipMemcpyDeviceToHost, c->stream));
    if (nv > 0) HIPCK(c, hipMemcpyAsync(vertices_out, m.d_vert, m.bv, hipMemcpyDeviceToHost, c->stream));
    if (nv > 0 && normals_out) HIPCK(c, hipMemcpyAsync(normals_out, m.d_nrm, m.bn, hipMemcpyDeviceToHost, c->stream));
    if (nt > 0) HIPCK(c, hipMemcpyAsync(triangles_out, m.d_tris, m.bt, hipMemcpyDeviceToHost, c->stream));
    HIPCK(c, hipStreamSynchronize(c->stream));
    return guard.done();
}
// Both mesh calls.  color (icp_tsdf_mesh_color): needs the colour array; colors_out (optional) receives one packed colour per vertex.
int tsdf_mesh(icp_ctx* c, float min_weight, int32_t max_vertices, int32_t max_triangles, float* vertices_out, float* normals_out, uint8_t* colors_out, bool color,
              uint32_t* triangles_out, int32_t* n_vertices_out, int32_t* n_triangles_out, const std::string& who, const McCall* cluster = nullptr) {
    if (n_vertices_out) *n_vertices_out = 0;
    if (n_triangles_out) *n_triangles_out = 0;
    int rc;
    if ((rc = tm_check_call(c, min_weight, who.c_str()))) return rc;
    if (color && (rc = tsdf_check_color(c, who.c_str()))) return rc;
    if (!n_vertices_out || !n_triangles_out) { c->err = who + ": null count pointer"; return ICP_ERR_INVALID_ARG; }
    const bool count_only = !vertices_out && !normals_out && !colors_out && !triangles_out;
    if (!count_only && (!vertices_out || !triangles_out)) {
        c->err = who + (color ? ": vertices_out and triangles_out go together (normals_out and colors_out may be NULL)" : ": vertices_out and triangles_out go together (normals_out alone may be NULL)");
        return ICP_ERR_INVALID_ARG;
    }
    DrainOnError guard(c);
    if ((rc = set_device(c))) return rc;
    const TmGrid g = tm_grid(c);
    TmScratch s;
    if ((rc = tm_scratch(c, g, s))) return rc;
    if ((rc = tm_enqueue_count(c, g, s, min_weight))) return rc;
    return tm_finish(c, guard, s.tot, max_vertices, max_triangles, vertices_out, normals_out, colors_out, triangles_out, n_vertices_out, n_triangles_out, count_only, who,
                     [&](float* d_vert, float* d_nrm, uint32_t* d_tris) { return tm_enqueue_fill(c, g, s, d_vert, d_nrm, d_tris); },
                     [&](uint32_t* d_col) -> int {
                         hipLaunchKernelGGL(k_tm_colors, dim3((unsigned)tm_blocks(g)), dim3(256), 0, c->stream, tsdf_view(c), (const float4*)c->tsdf_col.as<float4>(), g, (const uint8_t*)s.mask,
                                            (const int*)s.vblk, d_col);
                         HIPCK(c, hipGetLastError());
                         return ICP_OK;
                     },
                     cluster);
}
}  // namespace

int icp_tsdf_mesh(icp_ctx* c, float min_weight, int32_t max_vertices, int32_t max_triangles, float* vertices_out, float* normals_out, uint32_t* triangles_out,
                  int32_t* n_vertices_out, int32_t* n_triangles_out) {
    if (!c) return ICP_ERR_INVALID_ARG;
    return tsdf_mesh(c, min_weight, max_vertices, max_triangles, vertices_out, normals_out, nullptr, false, triangles_out, n_vertices_out, n_triangles_out, "icp_tsdf_mesh");
}
int icp_tsdf_mesh_color(icp_ctx* c, float min_weight, int32_t max_vertices, int32_t max_triangles, float* vertices_out, float* normals_out, uint8_t* colors_out,
                        uint32_t* triangles_out, int32_t* n_vertices_out, int32_t* n_triangles_out) {
    if (!c) return ICP_ERR_INVALID_ARG;
    return tsdf_mesh(c, min_weight, max_vertices, max_triangles, vertices_out, normals_out, colors_out, true, triangles_out, n_vertices_out, n_triangles_out, "icp_tsdf_mesh_color");
}

// Not part of icp_hip.h (tools/time_tsdf_mesh.py): the device time of ALL passes of one icp_tsdf_mesh (counting, the two scans, scatter, with
// normals) between two events on the context's stream.  A counting run outside the bracket sizes the output arrays first.
extern "C" int icp_debug_tsdf_mesh_time(icp_ctx* c, float min_weight, float* ms_out) {
    if (!c || !ms_out) return ICP_ERR_INVALID_ARG;
    int rc;
    if ((rc = tm_check_call(c, min_weight, "icp_debug_tsdf_mesh_time"))) return rc;
    DrainOnError guard(c);
    if ((rc = set_device(c))) return rc;
    const TmGrid g = tm_grid(c);
    TmScratch s;
    if ((rc = tm_scratch(c, g, s))) return rc;
    if ((rc = tm_enqueue_count(c, g, s, min_weight))) return rc;
    int tot[2] = {0, 0};                                 // both totals back in one copy
    if ((rc = read_count(c, s.tot, tot, 2))) return rc;
    const int nv = tot[0], nt = tot[1];
    const size_t bv = (size_t)nv * 12, bt = (size_t)nt * 12;
    if ((rc = ensure(c, c->tm_out, 2 * bv + bt))) return rc;
    char* d = c->tm_out.as<char>();
    rc = timed_ms(c, ms_out, [&] {
        int r = tm_enqueue_count(c, g, s, min_weight);
        return r ? r : tm_enqueue_fill(c, g, s, (float*)d, (float*)(d + bv), (uint32_t*)(d + 2 * bv));
    });
    if (rc) return rc;
    return guard.done();
}

// Not part of icp_hip.h (tests/test_tsdf_mesh_host.py): the device's case table, evaluated on the host.  table_out: 6 x 16 x 7 ints -- the
// number of triangles, then the local edge rank of its six slots (-1: unused); corners_out: 6 x 4 corner codes dx + 2 dy + 4 dz.  No GPU needed.
extern "C" int icp_debug_tsdf_mesh_table(int32_t* table_out, int32_t* corners_out) {
    if (!table_out || !corners_out) return ICP_ERR_INVALID_ARG;
    const TmTable T = tm_make_table();
    for (int p = 0; p < 6; p++) {
        for (int a = 0; a < 4; a++) corners_out[p * 4 + a] = (T.q[p] >> (3 * a)) & 7;
        for (int m = 0; m < 16; m++) {
            int32_t* o = table_out + (p * 16 + m) * 7;
            const int nt = (int)(T.e[p][m] & 3u);
            o[0] = nt;
            for (int s = 0; s < 6; s++) o[1 + s] = s < 3 * nt ? (int)((T.e[p][m] >> (2 + 3 * s)) & 7u) : -1;
        }
    }
    return ICP_OK;
}
