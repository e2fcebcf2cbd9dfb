// host_tsdf.hpp -- frame-to-model tracking: the context's TSDF volume (icp_tsdf_*), the model as target (icp_set_target_tsdf) and the tracking
// loop over it (icp_track_depth_model); the volume's optional colour array and the coloured forms of all three (icp_tsdf_color_*,
// icp_tsdf_integrate_color, icp_tsdf_raycast_color, icp_set_target_tsdf_color, icp_track_depth_model_color).  Kernels: dev_tsdf.hpp;
// contract: include/icp_hip.h, DESIGN.md sections 6m and 6p.  One body per call shape, for the dense and the hashed volume, with and
// without colour: tsdf_raycast_to_host behind the four ray-cast calls, set_target_tsdf_call behind the four targets, track_depth_model
// behind the four tracking loops; the public functions here and in host_tsdf_hash_raycast.hpp keep their own leading checks.
// Part of icp_hip.hip (included from there, after host_depth.hpp).
namespace {
const char* tsdf_options_error(const icp_tsdf_options* o) {
    if (!o) return "null options";
    for (int a = 0; a < 3; a++) if (o->dims[a] < 2) return "every dimension must be >= 2";
    if ((long long)o->dims[0] * o->dims[1] * o->dims[2] > 0x7FFFFFFFll) return "nx * ny * nz must not exceed INT32_MAX";
    for (int a = 0; a < 3; a++) if (!std::isfinite(o->origin[a])) return "the origin must be finite";
    if (!(std::isfinite(o->voxel_size) && o->voxel_size > 0.f)) return "voxel_size must be finite and > 0";
    if (!(std::isfinite(o->truncation) && o->truncation > 0.f)) return "truncation must be finite and > 0";
    if (!(std::isfinite(o->max_weight) && o->max_weight >= 1.f)) return "max_weight must be finite and >= 1";
    if (!(std::isfinite(o->min_depth) && std::isfinite(o->max_depth) && o->min_depth > 0.f && o->min_depth < o->max_depth)) return "need 0 < min_depth < max_depth";
    if (!(o->ray_step == 0.f || (o->ray_step > 0.f && o->ray_step <= o->truncation))) return "ray_step must be 0 (truncation / 2) or in (0, truncation]";
    const float step = o->ray_step == 0.f ? o->truncation / 2.f : o->ray_step;
    if (!(((double)o->max_depth - o->min_depth) / step <= 1048576.0)) return "(max_depth - min_depth) / ray_step must not exceed 2^20";      // bounds every ray's march
    return nullptr;
}
bool is_identity16(const float* m) {
    for (int k = 0; k < 16; k++) if (m[k] != ((k % 5 == 0) ? 1.f : 0.f)) return false;
    return true;
}
// what host_tsdf_hash.hpp defines for a hashed volume
int htsdf_integrate_slot(icp_ctx* c, int slot, const icp_depth_camera& cam, const float pose[16], int* d_count, const char* who, bool color = false);
int htsdf_reset(icp_ctx* c);
int htsdf_raycast_launch(icp_ctx* c, const icp_depth_camera& cam, const float pose[16], bool soa, const TsdfRayOut& o, const TsdfColorOut* co = nullptr);      // (host_tsdf_hash_raycast.hpp, DESIGN.md sections 6z and 6zc)
int htsdf_check_color(icp_ctx* c, const char* who);
void htsdf_drop(icp_ctx* c);
// the calls that need the dense box: refused on a hashed volume, with nothing touched
int tsdf_check_dense(icp_ctx* c, const char* who) {
    if (c->tsdf_on && c->tsdf_hashed) { c->err = std::string(who) + ": not supported on a hashed volume (icp_tsdf_create_hashed): it needs the dense box of icp_tsdf_create"; return ICP_ERR_INVALID_ARG; }
    return ICP_OK;
}
// the four calls that address the DENSE colour array: a coloured hashed volume is pointed at the calls that read and write its blocks
int tsdf_check_dense_colors(icp_ctx* c, const char* who) {
    if (c->tsdf_on && c->tsdf_hashed && c->th_color) {
        c->err = std::string(who) + ": not supported on a hashed volume (icp_tsdf_create_color_hashed): it addresses the dense colour array; the colours of the blocks are read and written by icp_get_tsdf_color_hashed and icp_tsdf_upload_color_hashed";
        return ICP_ERR_INVALID_ARG;
    }
    return ICP_OK;
}
// the volume is hashed and holds colours: the coloured calls that work on the blocks take it
bool tsdf_hashed_color(const icp_ctx* c) { return c->tsdf_on && c->tsdf_hashed && c->th_color; }
int tsdf_check_call(icp_ctx* c, const icp_depth_camera* cam, const float* pose, const char* who, bool hashed_ok = false) {
    if (!c->tsdf_on) { c->err = std::string(who) + ": no volume (icp_tsdf_create)"; return ICP_ERR_INVALID_ARG; }
    if (!hashed_ok) { int rc; if ((rc = tsdf_check_dense(c, who))) return rc; }
    if (!depth_camera_ok(cam) || !pose) { c->err = std::string(who) + ": bad camera or null pose"; return ICP_ERR_INVALID_ARG; }
    if (!is_identity16(cam->extrinsics)) { c->err = std::string(who) + ": the depth extrinsics must be the identity"; return ICP_ERR_INVALID_ARG; }
    return ICP_OK;
}
int tsdf_check_color(icp_ctx* c, const char* who) {
    if (!c->tsdf_on) { c->err = std::string(who) + ": no volume (icp_tsdf_create)"; return ICP_ERR_INVALID_ARG; }
    { int rc; if ((rc = tsdf_check_dense(c, who))) return rc; }
    if (!c->tsdf_col_on) { c->err = std::string(who) + ": the volume has no colour array (icp_tsdf_color_create)"; return ICP_ERR_INVALID_ARG; }
    return ICP_OK;
}
size_t tsdf_voxels(const icp_ctx* c) { return (size_t)c->tsdf_opt.dims[0] * c->tsdf_opt.dims[1] * c->tsdf_opt.dims[2]; }
TsdfVol tsdf_view(const icp_ctx* c) {
    const icp_tsdf_options& o = c->tsdf_opt;
    TsdfVol v;
    v.vox = c->tsdf_vox.as<float2>(); v.nx = o.dims[0]; v.ny = o.dims[1]; v.nz = o.dims[2];
    v.ox = o.origin[0]; v.oy = o.origin[1]; v.oz = o.origin[2]; v.s = o.voxel_size;
    v.trunc = o.truncation; v.max_w = o.max_weight; v.min_d = o.min_depth; v.max_d = o.max_depth; v.step = o.ray_step;
    return v;
}
TsdfCam tsdf_cam(const icp_depth_camera& cam) { TsdfCam t; t.width = cam.width; t.height = cam.height; t.fx = cam.fx; t.fy = cam.fy; t.cx = cam.cx; t.cy = cam.cy; return t; }

// The frame in upload slot `slot` fused into the volume at `pose`, enqueued on the context's stream; d_count (optional): zeroed, then the
// number of voxels written.  color: the slot's colour frame goes into the colour array as well (d_count[1]: the voxels coloured).
int tsdf_integrate_slot(icp_ctx* c, int slot, const icp_depth_camera& cam, const float pose[16], int* d_count, bool color = false) {
    TsdfMat m; memset(&m, 0, sizeof(m));
    invert_extrinsics(pose, m.m);                    // the affine inverse in fp64, rounded once: 3x3 row-major, then t
    const TsdfVol v = tsdf_view(c);
    HIPCK(c, hipStreamWaitEvent(c->stream, c->depth_up[slot], 0));
    if (d_count) HIPCK(c, hipMemsetAsync(d_count, 0, color ? 8 : 4, c->stream));
    const dim3 grid((v.nx + 63) / 64, (v.ny + 3) / 4, (v.nz + TSDF_KCHUNK - 1) / TSDF_KCHUNK);
    const float* depth = c->depth_dev[slot].as<float>();
    if (color) hipLaunchKernelGGL(k_tsdf_integrate_color, grid, dim3(64, 4), 0, c->stream, v, tsdf_cam(cam), m, depth, d_count,
                                  (const uint32_t*)(depth + (size_t)cam.width * cam.height), c->tsdf_col.as<float4>(), d_count ? d_count + 1 : nullptr);
    else hipLaunchKernelGGL(k_tsdf_integrate, grid, dim3(64, 4), 0, c->stream, v, tsdf_cam(cam), m, depth, d_count);
    HIPCK(c, hipGetLastError());
    return ICP_OK;
}
// The ray-cast from `pose`, enqueued; the hit count lands in tsdf_cnt (zeroed first).  co: with colours, the coloured hits in tsdf_cnt[1].
int tsdf_raycast_launch(icp_ctx* c, const icp_depth_camera& cam, const float pose[16], bool soa, const TsdfRayOut& o, const TsdfColorOut* co = nullptr) {
    int rc;
    if ((rc = ensure(c, c->tsdf_cnt, 16))) return rc;
    TsdfMat m; memcpy(m.m, pose, 64);
    HIPCK(c, hipMemsetAsync(c->tsdf_cnt.p, 0, co ? 8 : 4, c->stream));
    const dim3 grid((cam.width + 15) / 16, (cam.height + 15) / 16);
    int* cnt = c->tsdf_cnt.as<int>();
    const float4* col = c->tsdf_col.as<float4>();
    if (co && soa) hipLaunchKernelGGL(k_tsdf_raycast_color<true>, grid, dim3(256), 0, c->stream, tsdf_view(c), tsdf_cam(cam), m, o, cnt, col, *co, cnt + 1);
    else if (co) hipLaunchKernelGGL(k_tsdf_raycast_color<false>, grid, dim3(256), 0, c->stream, tsdf_view(c), tsdf_cam(cam), m, o, cnt, col, *co, cnt + 1);
    else if (soa) hipLaunchKernelGGL(k_tsdf_raycast<true>, grid, dim3(256), 0, c->stream, tsdf_view(c), tsdf_cam(cam), m, o, c->tsdf_cnt.as<int>());
    else hipLaunchKernelGGL(k_tsdf_raycast<false>, grid, dim3(256), 0, c->stream, tsdf_view(c), tsdf_cam(cam), m, o, c->tsdf_cnt.as<int>());
    HIPCK(c, hipGetLastError());
    return ICP_OK;
}
// the ray-cast of whichever storage the caller's checks have found
int tsdf_raycast_any(icp_ctx* c, const icp_depth_camera& cam, const float pose[16], bool soa, const TsdfRayOut& o, const TsdfColorOut* co, bool hashed) {
    return hashed ? htsdf_raycast_launch(c, cam, pose, soa, o, co) : tsdf_raycast_launch(c, cam, pose, soa, o, co);
}
// The staging layout of a ray-cast to the host, [depth 4n | vertices 12n | normals 12n | rgba 4n (color)]: the planes asked for, the rest null.
int tsdf_ray_stage(icp_ctx* c, size_t n, bool color, bool depth, bool vert, bool nrm, bool rgba, TsdfRayOut* o, TsdfColorOut* co) {
    int rc;
    if ((rc = ensure(c, c->staging, n * (color ? 32 : 28)))) return rc;
    float* d = c->staging.as<float>();
    memset(o, 0, sizeof(*o));
    o->depth = depth ? d : nullptr; o->vert = vert ? d + n : nullptr; o->nrm = nrm ? d + 4 * n : nullptr;
    *co = {rgba ? (uint32_t*)(d + 7 * n) : nullptr, nullptr, nullptr, nullptr};
    return ICP_OK;
}
// The four ray-cast-to-host calls behind their checks: staged, launched (color: the coloured ray-cast; hashed: the hashed volume's), the
// planes asked for copied back, the count read -- the one host wait.
int tsdf_raycast_to_host(icp_ctx* c, const icp_depth_camera& cam, const float pose[16], float* depth_out, float* vertices_out, float* normals_out, uint8_t* rgba_out,
                         int32_t* n_hits_out, int32_t* n_colored_out, bool color, bool hashed) {
    int rc;
    DrainOnError guard(c);
    if ((rc = set_device(c))) return rc;
    const size_t n = (size_t)cam.width * cam.height;
    TsdfRayOut o; TsdfColorOut co;
    if ((rc = tsdf_ray_stage(c, n, color, depth_out, vertices_out, normals_out, rgba_out, &o, &co))) return rc;
    if ((rc = tsdf_raycast_any(c, cam, pose, false, o, color ? &co : nullptr, hashed))) return rc;
    if (depth_out) HIPCK(c, hipMemcpyAsync(depth_out, o.depth, n * 4, hipMemcpyDeviceToHost, c->stream));
    if (vertices_out) HIPCK(c, hipMemcpyAsync(vertices_out, o.vert, n * 12, hipMemcpyDeviceToHost, c->stream));
    if (normals_out) HIPCK(c, hipMemcpyAsync(normals_out, o.nrm, n * 12, hipMemcpyDeviceToHost, c->stream));
    if (rgba_out) HIPCK(c, hipMemcpyAsync(rgba_out, co.rgba, n * 4, hipMemcpyDeviceToHost, c->stream));
    int cnt[2] = {0, 0};
    if ((rc = read_count(c, c->tsdf_cnt.p, cnt, color ? 2 : 1))) return rc;
    if (n_hits_out) *n_hits_out = cnt[0];
    if (n_colored_out) *n_colored_out = cnt[1];
    return guard.done();
}
// The model as target, from the arguments already checked: the ray-cast into the target's planes, the hit count, finish_target.
// *hits_out = 0 with ICP_ERR_NO_TARGET leaves an empty target.  color: the coloured ray-cast, colours into the target's colour planes;
// a hit without colour is a hole and *hits_out counts the coloured hits.  hashed: the ray-cast of the hashed volume (with color: its coloured one).
int set_target_tsdf(icp_ctx* c, const icp_depth_camera& cam, const float pose[16], int* hits_out, const char* who, bool color = false, bool hashed = false) {
    int rc;
    Cloud& tg = c->tgt;
    const int n = cam.width * cam.height, npad = (n + 63) / 64 * 64;
    *hits_out = 0;
    for (DevBuf* pl : {&tg.x, &tg.y, &tg.z, &tg.nx, &tg.ny, &tg.nz}) if ((rc = ensure(c, *pl, (size_t)npad * 4))) return rc;
    if (color) { for (DevBuf* pl : {&tg.rgba, &tg.cr, &tg.cg, &tg.cb}) if ((rc = ensure(c, *pl, (size_t)npad * 4))) return rc; }
    else for (DevBuf* pl : {&tg.rgba, &tg.cr, &tg.cg, &tg.cb}) release(*pl);
    TsdfRayOut o; memset(&o, 0, sizeof(o));
    o.x = tg.x.as<float>(); o.y = tg.y.as<float>(); o.z = tg.z.as<float>(); o.nx = tg.nx.as<float>(); o.ny = tg.ny.as<float>(); o.nz = tg.nz.as<float>(); o.npad = npad;
    const TsdfColorOut co = {tg.rgba.as<uint32_t>(), tg.cr.as<float>(), tg.cg.as<float>(), tg.cb.as<float>()};
    if ((rc = tsdf_raycast_any(c, cam, pose, true, o, color ? &co : nullptr, hashed))) return rc;
    int hits = 0;
    if ((rc = read_count(c, c->tsdf_cnt.p, &hits))) return rc;      // (the coloured target's holes are its uncoloured hits: both counts agree)
    tg.has_normals = true; tg.has_colors = color;
    if (hits <= 0) {
        tg.n = 0; tg.npad = 0; c->bvh.valid = false; c->bvh6.valid = false;
        c->gicp_ready[0] = false; c->col_ready = false; c->fpfh[0].ready = false;
        c->err = std::string(who) + (color ? ": the ray-cast of the model hits nothing that has a colour" : ": the ray-cast of the model hits nothing");
        return ICP_ERR_NO_TARGET;
    }
    tg.n = n; tg.npad = npad;
    *hits_out = hits;
    return finish_target(c, color);
}
// The four icp_set_target_tsdf* calls behind their checks.
int set_target_tsdf_call(icp_ctx* c, const icp_depth_camera& cam, const float pose[16], int32_t* n_points_out, const char* who, bool color, bool hashed) {
    int rc;
    DrainOnError guard(c);
    if ((rc = set_device(c))) return rc;
    int hits = 0;
    rc = set_target_tsdf(c, cam, pose, &hits, who, color, hashed);
    if (rc == ICP_ERR_NO_TARGET) return guard.done(rc);      // (synchronised by the count read)
    if (rc) return rc;
    if (n_points_out) *n_points_out = hits;
    HIPCK(c, hipStreamSynchronize(c->stream));
    return guard.done();
}
// icp_debug_tsdf_time and icp_debug_tsdf_color_time behind their checks: ONE integrate (which = 0, the frame staged outside the bracket) or
// ONE ray-cast to the host-layout arrays (which = 1) inside timed_ms.
int tsdf_time(icp_ctx* c, int32_t which, const float* depth, const uint8_t* rgbx, const icp_depth_camera& cam, const float pose[16], float* ms_out, bool color) {
    int rc;
    DrainOnError guard(c);
    if ((rc = set_device(c))) return rc;
    const size_t n = (size_t)cam.width * cam.height;
    if (which == 0) {
        if ((rc = stage_depth(c, 0, depth, rgbx, (int)n, c->stream))) return rc;
        HIPCK(c, hipStreamSynchronize(c->stream));
        if ((rc = timed_ms(c, ms_out, [&] { return tsdf_integrate_slot(c, 0, cam, pose, c->tsdf_cnt.as<int>(), color); }))) return rc;
    } else {
        TsdfRayOut o; TsdfColorOut co;
        if ((rc = tsdf_ray_stage(c, n, color, true, true, true, true, &o, &co))) return rc;
        if ((rc = timed_ms(c, ms_out, [&] { return tsdf_raycast_launch(c, cam, pose, false, o, color ? &co : nullptr); }))) return rc;
    }
    return guard.done();
}
// pose <- pose dT: the fp64 product of the two column-major 4x4, rounded once.
void compose_pose(float pose[16], const float dT[16]) {
    float out[16];
    for (int cc = 0; cc < 4; cc++)
        for (int r = 0; r < 4; r++)
            out[cc * 4 + r] = (float)((((double)pose[r] * dT[cc * 4] + (double)pose[4 + r] * dT[cc * 4 + 1]) + (double)pose[8 + r] * dT[cc * 4 + 2]) + (double)pose[12 + r] * dT[cc * 4 + 3]);
    memcpy(pose, out, 64);
}
}  // namespace

int icp_tsdf_options_default(icp_tsdf_options* o) {
    if (!o) return ICP_ERR_INVALID_ARG;
    memset(o, 0, sizeof(*o));
    o->voxel_size = 0.05f; o->truncation = 0.25f; o->max_weight = 64.f; o->min_depth = 0.3f; o->max_depth = 8.f; o->ray_step = 0.f;
    return ICP_OK;
}
int icp_tsdf_options_check(const icp_tsdf_options* o) { return tsdf_options_error(o) ? ICP_ERR_INVALID_ARG : ICP_OK; }

int icp_tsdf_reset(icp_ctx* c) {
    if (!c) return ICP_ERR_INVALID_ARG;
    if (!c->tsdf_on) { c->err = "icp_tsdf_reset: no volume (icp_tsdf_create)"; return ICP_ERR_INVALID_ARG; }
    int rc;
    DrainOnError guard(c);
    if ((rc = set_device(c))) return rc;
    if (c->tsdf_hashed) { if ((rc = htsdf_reset(c))) return rc; return guard.done(); }
    HIPCK(c, hipMemsetAsync(c->tsdf_vox.p, 0, tsdf_voxels(c) * 8, c->stream));      // tsdf 0, weight 0
    if (c->tsdf_col_on) HIPCK(c, hipMemsetAsync(c->tsdf_col.p, 0, tsdf_voxels(c) * 16, c->stream));
    HIPCK(c, hipStreamSynchronize(c->stream));
    return guard.done();
}
int icp_tsdf_release(icp_ctx* c) {
    if (!c) return ICP_ERR_INVALID_ARG;
    if (!c->tsdf_on) { c->err = "icp_tsdf_release: no volume (icp_tsdf_create)"; return ICP_ERR_INVALID_ARG; }
    int rc;
    if ((rc = set_device(c))) return rc;
    HIPCK(c, hipStreamSynchronize(c->stream));
    release(c->tsdf_vox);
    release(c->tsdf_col); c->tsdf_col_on = false;
    if (c->tsdf_hashed) htsdf_drop(c);
    for (DevBuf* d : {&c->tm_bits, &c->tm_mask, &c->tm_base, &c->tm_blk, &c->tm_out, &c->tm_nbr, &c->tm_ord}) release(*d);      // the mesh extraction's scratch goes with the volume
    release(c->tc_acc); c->tc_voxels = 0;             // and the cloud integrate's accumulators
    release(c->tcc_acc); c->tcc_voxels = 0;
    c->tsdf_on = false;
    return ICP_OK;
}
int icp_tsdf_create(icp_ctx* c, const icp_tsdf_options* opt) {
    if (!c) return ICP_ERR_INVALID_ARG;
    if (const char* why = tsdf_options_error(opt)) { c->err = std::string("icp_tsdf_create: ") + why; return ICP_ERR_INVALID_ARG; }
    int rc;
    if ((rc = set_device(c))) return rc;
    if (c->tsdf_on) { HIPCK(c, hipStreamSynchronize(c->stream)); release(c->tsdf_vox); release(c->tsdf_col); c->tsdf_col_on = false; if (c->tsdf_hashed) htsdf_drop(c); release(c->tc_acc); c->tc_voxels = 0; release(c->tcc_acc); c->tcc_voxels = 0; c->tsdf_on = false; }
    c->tsdf_opt = *opt;
    if (c->tsdf_opt.ray_step == 0.f) c->tsdf_opt.ray_step = opt->truncation / 2.f;
    if ((rc = ensure(c, c->tsdf_vox, tsdf_voxels(c) * 8))) return rc;
    if ((rc = ensure(c, c->tsdf_cnt, 16))) return rc;
    c->tsdf_on = true;
    return icp_tsdf_reset(c);
}

// The two host arrays and the interleaved device volume, a slab of at most 4 Mi voxels at a time through a host block.
int icp_tsdf_download(icp_ctx* c, float* tsdf_out, float* weight_out) {
    if (!c) return ICP_ERR_INVALID_ARG;
    if (!c->tsdf_on) { c->err = "icp_tsdf_download: no volume (icp_tsdf_create)"; return ICP_ERR_INVALID_ARG; }
    if (int rd = tsdf_check_dense(c, "icp_tsdf_download")) return rd;
    int rc;
    if ((rc = set_device(c))) return rc;
    HIPCK(c, hipStreamSynchronize(c->stream));
    const size_t n = tsdf_voxels(c), slab = (size_t)4 << 20;
    std::vector<float> h(2 * (n < slab ? n : slab));
    for (size_t at = 0; at < n; at += slab) {
        const size_t m = n - at < slab ? n - at : slab;
        HIPCK(c, hipMemcpy(h.data(), c->tsdf_vox.as<float>() + 2 * at, m * 8, hipMemcpyDeviceToHost));
        if (tsdf_out) for (size_t i = 0; i < m; i++) tsdf_out[at + i] = h[2 * i];
        if (weight_out) for (size_t i = 0; i < m; i++) weight_out[at + i] = h[2 * i + 1];
    }
    return ICP_OK;
}
int icp_tsdf_upload(icp_ctx* c, const float* tsdf, const float* weight) {
    if (!c) return ICP_ERR_INVALID_ARG;
    if (!c->tsdf_on) { c->err = "icp_tsdf_upload: no volume (icp_tsdf_create)"; return ICP_ERR_INVALID_ARG; }
    if (int rd = tsdf_check_dense(c, "icp_tsdf_upload")) return rd;
    if (!tsdf || !weight) { c->err = "icp_tsdf_upload: null array"; return ICP_ERR_INVALID_ARG; }
    int rc;
    if ((rc = set_device(c))) return rc;
    HIPCK(c, hipStreamSynchronize(c->stream));
    const size_t n = tsdf_voxels(c), slab = (size_t)4 << 20;
    std::vector<float> h(2 * (n < slab ? n : slab));
    for (size_t at = 0; at < n; at += slab) {
        const size_t m = n - at < slab ? n - at : slab;
        for (size_t i = 0; i < m; i++) { h[2 * i] = tsdf[at + i]; h[2 * i + 1] = weight[at + i]; }
        HIPCK(c, hipMemcpy(c->tsdf_vox.as<float>() + 2 * at, h.data(), m * 8, hipMemcpyHostToDevice));
    }
    return ICP_OK;
}

// ---- the colour array: one float4 (R, G, B, Wc) per voxel next to the geometry's float2
int icp_tsdf_color_create(icp_ctx* c) {
    if (!c) return ICP_ERR_INVALID_ARG;
    if (!c->tsdf_on) { c->err = "icp_tsdf_color_create: no volume (icp_tsdf_create)"; return ICP_ERR_INVALID_ARG; }
    if (int rd = tsdf_check_dense_colors(c, "icp_tsdf_color_create")) return rd;
    if (int rd = tsdf_check_dense(c, "icp_tsdf_color_create")) return rd;
    int rc;
    DrainOnError guard(c);
    if ((rc = set_device(c))) return rc;
    if ((rc = ensure(c, c->tsdf_col, tsdf_voxels(c) * 16))) return rc;
    c->tsdf_col_on = true;
    HIPCK(c, hipMemsetAsync(c->tsdf_col.p, 0, tsdf_voxels(c) * 16, c->stream));
    HIPCK(c, hipStreamSynchronize(c->stream));
    return guard.done();
}
int icp_tsdf_color_release(icp_ctx* c) {
    if (!c) return ICP_ERR_INVALID_ARG;
    int rc;
    if ((rc = tsdf_check_dense_colors(c, "icp_tsdf_color_release"))) return rc;
    if ((rc = tsdf_check_color(c, "icp_tsdf_color_release"))) return rc;
    if ((rc = set_device(c))) return rc;
    HIPCK(c, hipStreamSynchronize(c->stream));
    release(c->tsdf_col); c->tsdf_col_on = false;
    return ICP_OK;
}
// The host arrays (rgb n x 3, weight n) and the interleaved device array, a slab of at most 1 Mi voxels at a time through a host block.
int icp_tsdf_color_download(icp_ctx* c, float* rgb_out, float* weight_out) {
    if (!c) return ICP_ERR_INVALID_ARG;
    int rc;
    if ((rc = tsdf_check_dense_colors(c, "icp_tsdf_color_download"))) return rc;
    if ((rc = tsdf_check_color(c, "icp_tsdf_color_download"))) return rc;
    if ((rc = set_device(c))) return rc;
    HIPCK(c, hipStreamSynchronize(c->stream));
    const size_t n = tsdf_voxels(c), slab = (size_t)1 << 20;
    std::vector<float> h(4 * (n < slab ? n : slab));
    for (size_t at = 0; at < n; at += slab) {
        const size_t m = n - at < slab ? n - at : slab;
        HIPCK(c, hipMemcpy(h.data(), c->tsdf_col.as<float>() + 4 * at, m * 16, hipMemcpyDeviceToHost));
        if (rgb_out) for (size_t i = 0; i < m; i++) for (int q = 0; q < 3; q++) rgb_out[3 * (at + i) + q] = h[4 * i + q];
        if (weight_out) for (size_t i = 0; i < m; i++) weight_out[at + i] = h[4 * i + 3];
    }
    return ICP_OK;
}
int icp_tsdf_color_upload(icp_ctx* c, const float* rgb, const float* weight) {
    if (!c) return ICP_ERR_INVALID_ARG;
    int rc;
    if ((rc = tsdf_check_dense_colors(c, "icp_tsdf_color_upload"))) return rc;
    if ((rc = tsdf_check_color(c, "icp_tsdf_color_upload"))) return rc;
    if (!rgb || !weight) { c->err = "icp_tsdf_color_upload: null array"; return ICP_ERR_INVALID_ARG; }
    if ((rc = set_device(c))) return rc;
    HIPCK(c, hipStreamSynchronize(c->stream));
    const size_t n = tsdf_voxels(c), slab = (size_t)1 << 20;
    std::vector<float> h(4 * (n < slab ? n : slab));
    for (size_t at = 0; at < n; at += slab) {
        const size_t m = n - at < slab ? n - at : slab;
        for (size_t i = 0; i < m; i++) { for (int q = 0; q < 3; q++) h[4 * i + q] = rgb[3 * (at + i) + q]; h[4 * i + 3] = weight[at + i]; }
        HIPCK(c, hipMemcpy(c->tsdf_col.as<float>() + 4 * at, h.data(), m * 16, hipMemcpyHostToDevice));
    }
    return ICP_OK;
}

int icp_tsdf_integrate(icp_ctx* c, const float* depth, const icp_depth_camera* cam, const float pose[16], int32_t* n_updated_out) {
    if (!c) return ICP_ERR_INVALID_ARG;
    if (n_updated_out) *n_updated_out = 0;
    int rc;
    if ((rc = tsdf_check_call(c, cam, pose, "icp_tsdf_integrate", true))) return rc;
    if (!depth) { c->err = "icp_tsdf_integrate: null depth frame"; return ICP_ERR_INVALID_ARG; }
    DrainOnError guard(c);
    if ((rc = set_device(c))) return rc;
    if ((rc = stage_depth(c, 0, depth, nullptr, cam->width * cam->height, c->stream))) return rc;
    if (c->tsdf_hashed) rc = htsdf_integrate_slot(c, 0, *cam, pose, c->tsdf_cnt.as<int>(), "icp_tsdf_integrate");
    else rc = tsdf_integrate_slot(c, 0, *cam, pose, c->tsdf_cnt.as<int>());
    if (rc) return rc;
    int n = 0;
    if ((rc = read_count(c, c->tsdf_cnt.p, &n))) return rc;
    if (n_updated_out) *n_updated_out = n;
    return guard.done();
}

int icp_tsdf_integrate_color(icp_ctx* c, const float* depth, const uint8_t* rgbx, const icp_depth_camera* cam, const float pose[16], int32_t* n_updated_out,
                             int32_t* n_colored_out) {
    if (!c) return ICP_ERR_INVALID_ARG;
    if (n_updated_out) *n_updated_out = 0;
    if (n_colored_out) *n_colored_out = 0;
    int rc;
    const bool hcol = tsdf_hashed_color(c);          // (a hashed volume without colours is refused as every dense-box call is)
    if ((rc = tsdf_check_call(c, cam, pose, "icp_tsdf_integrate_color", hcol))) return rc;
    if (!hcol && (rc = tsdf_check_color(c, "icp_tsdf_integrate_color"))) return rc;
    if (!depth || !rgbx) { c->err = "icp_tsdf_integrate_color: null depth or colour frame"; return ICP_ERR_INVALID_ARG; }
    DrainOnError guard(c);
    if ((rc = set_device(c))) return rc;
    if ((rc = stage_depth(c, 0, depth, rgbx, cam->width * cam->height, c->stream))) return rc;
    if (hcol) rc = htsdf_integrate_slot(c, 0, *cam, pose, c->tsdf_cnt.as<int>(), "icp_tsdf_integrate_color", true);
    else rc = tsdf_integrate_slot(c, 0, *cam, pose, c->tsdf_cnt.as<int>(), true);
    if (rc) return rc;
    int n[2] = {0, 0};
    if ((rc = read_count(c, c->tsdf_cnt.p, n, 2))) return rc;
    if (n_updated_out) *n_updated_out = n[0];
    if (n_colored_out) *n_colored_out = n[1];
    return guard.done();
}

int icp_tsdf_raycast(icp_ctx* c, const icp_depth_camera* cam, const float pose[16], float* depth_out, float* vertices_out, float* normals_out,
                     int32_t* n_hits_out) {
    if (!c) return ICP_ERR_INVALID_ARG;
    if (n_hits_out) *n_hits_out = 0;
    int rc;
    if ((rc = tsdf_check_call(c, cam, pose, "icp_tsdf_raycast"))) return rc;
    return tsdf_raycast_to_host(c, *cam, pose, depth_out, vertices_out, normals_out, nullptr, n_hits_out, nullptr, false, false);
}

int icp_set_target_tsdf(icp_ctx* c, const icp_depth_camera* cam, const float pose[16], int32_t* n_points_out) {
    if (!c) return ICP_ERR_INVALID_ARG;
    if (n_points_out) *n_points_out = 0;
    int rc;
    if ((rc = tsdf_check_call(c, cam, pose, "icp_set_target_tsdf"))) return rc;
    return set_target_tsdf_call(c, *cam, pose, n_points_out, "icp_set_target_tsdf", false, false);
}

int icp_tsdf_raycast_color(icp_ctx* c, const icp_depth_camera* cam, const float pose[16], float* depth_out, float* vertices_out, float* normals_out,
                           uint8_t* rgba_out, int32_t* n_hits_out, int32_t* n_colored_out) {
    if (!c) return ICP_ERR_INVALID_ARG;
    if (n_hits_out) *n_hits_out = 0;
    if (n_colored_out) *n_colored_out = 0;
    int rc;
    if ((rc = tsdf_check_call(c, cam, pose, "icp_tsdf_raycast_color"))) return rc;
    if ((rc = tsdf_check_color(c, "icp_tsdf_raycast_color"))) return rc;
    return tsdf_raycast_to_host(c, *cam, pose, depth_out, vertices_out, normals_out, rgba_out, n_hits_out, n_colored_out, true, false);
}

int icp_set_target_tsdf_color(icp_ctx* c, const icp_depth_camera* cam, const float pose[16], int32_t* n_points_out) {
    if (!c) return ICP_ERR_INVALID_ARG;
    if (n_points_out) *n_points_out = 0;
    int rc;
    if ((rc = tsdf_check_call(c, cam, pose, "icp_set_target_tsdf_color"))) return rc;
    if ((rc = tsdf_check_color(c, "icp_set_target_tsdf_color"))) return rc;
    return set_target_tsdf_call(c, *cam, pose, n_points_out, "icp_set_target_tsdf_color", true, false);
}

// Both tracking loops.  color (icp_track_depth_model_color): frames staged with their colour frame, the coloured target, the source with
// colours, the coloured integration -- and the colour modes, which the geometric loop refuses, accepted.  hashed
// (icp_track_depth_model_hashed; with color icp_track_depth_model_color_hashed): the target from the hashed ray-cast, the integrate
// htsdf_integrate_slot -- its touch waits for the host once per integrated frame, and once more per growth of the pool.
static int track_depth_model(icp_ctx* c, const float* depth_frames, const uint8_t* rgbx_frames, bool color, int32_t n_frames, const icp_depth_camera* cam,
                             const icp_depth_options* source_opt, const float* gt_frames, float pose_inout[16], icp_track_frame* out, const std::string& who,
                             bool hashed = false) {
    if (!depth_frames || n_frames < 1 || !pose_inout || (n_frames > 1 && !out)) { c->err = who + ": bad argument"; return ICP_ERR_INVALID_ARG; }
    int rc;
    if ((rc = tsdf_check_call(c, cam, pose_inout, who.c_str(), hashed))) return rc;
    if ((rc = check_depth_args(c, cam, source_opt, who.c_str()))) return rc;
    const icp_params& p = c->prm;
    if (p.matching == ICP_MATCH_PROJECTIVE && (p.fx != cam->fx || p.fy != cam->fy || p.cx != cam->cx || p.cy != cam->cy || p.width != cam->width || p.height != cam->height)) {
        c->err = who + ": the camera of the params differs from the depth camera"; return ICP_ERR_INVALID_ARG;
    }
    if (color) {
        if (!rgbx_frames) { c->err = who + ": null colour frames"; return ICP_ERR_INVALID_ARG; }
        if ((rc = hashed ? htsdf_check_color(c, who.c_str()) : tsdf_check_color(c, who.c_str()))) return rc;
        if (!source_opt->fix_color_index) {
            c->err = who + ": source_opt->fix_color_index must be set (the model holds each pixel's own bytes, the reference's shifted bytes would compare unlike things)";
            return ICP_ERR_INVALID_ARG;
        }
    } else if ((p.matching == ICP_MATCH_KNN && p.color_icp) || p.weighting == ICP_WEIGHT_COLORS || p.metric == ICP_METRIC_COLORED) {
        c->err = who + ": the model has no colours (colour ICP, colour weighting and the colored metric are not supported)"; return ICP_ERR_INVALID_ARG;
    }
    if (p.metric == ICP_METRIC_GICP) { c->err = who + ": GICP is not supported (its per-target covariance pass would run every frame)"; return ICP_ERR_INVALID_ARG; }
    DrainOnError guard(c);
    if ((rc = set_device(c))) return rc;
    const int n = cam->width * cam->height;
    auto frame_rgbx = [&](int k) { return color ? rgbx_frames + (size_t)k * n * 4 : nullptr; };
    auto integrate = [&](int slot) { return hashed ? htsdf_integrate_slot(c, slot, *cam, pose_inout, nullptr, who.c_str(), color) : tsdf_integrate_slot(c, slot, *cam, pose_inout, nullptr, color); };
    if (!c->depth_stream) HIPCK(c, hipStreamCreateWithFlags(&c->depth_stream.s, hipStreamNonBlocking));
    // frame 0 into the model at the incoming pose; frame 1 goes up meanwhile
    if ((rc = stage_depth(c, 0, depth_frames, frame_rgbx(0), n, c->stream, -1, cam->width))) return rc;
    if ((rc = integrate(0))) return rc;
    if (n_frames > 1 && (rc = stage_depth(c, 1, depth_frames + (size_t)n, frame_rgbx(1), n, c->depth_stream, -1, cam->width))) return rc;
    if (gt_frames && n_frames > 1 && (rc = track_rmse_prepare(c, n_frames))) return rc;
    static const float identity[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    int first_err = ICP_OK;
    auto fail = [&](icp_track_frame& r, int status, const std::string& why) {
        r.status = status; memcpy(r.pose, pose_inout, 64);
        if (first_err == ICP_OK) { first_err = status; c->err = why; }
    };
    for (int k = 1; k < n_frames; k++) {
        icp_track_frame& r = out[k - 1];
        memset(&r, 0, sizeof(r)); r.initial_rmse = r.final_rmse = -1.f;
        const int slot = k & 1;
        int hits = 0, kept = 0;
        // the model seen from the current pose (the count read waits for the stream: the integration of frame k - 1 has left its slot)
        const int trc = set_target_tsdf(c, *cam, pose_inout, &hits, who.c_str(), color, hashed);
        if (trc != ICP_OK && trc != ICP_ERR_NO_TARGET) return trc;
        if ((rc = depth_to_cloud(c, slot, *cam, *source_opt, color, c->src, false, &kept))) return rc;
        // frame k + 1 goes up on the second stream while frame k iterates (its slot was last read by frame k - 1, which has finished)
        if (k + 1 < n_frames && (rc = stage_depth(c, slot ^ 1, depth_frames + (size_t)(k + 1) * n, frame_rgbx(k + 1), n, c->depth_stream, -1, cam->width))) return rc;
        if ((rc = finish_source(c))) return rc;
        r.n_src = kept;
        if (trc == ICP_ERR_NO_TARGET) { fail(r, ICP_ERR_NO_TARGET, who + (color ? ": the ray-cast of the model hits nothing that has a colour" : ": the ray-cast of the model hits nothing")); continue; }
        if (kept == 0) { fail(r, ICP_ERR_NO_SOURCE, who + ": a frame keeps no points"); continue; }
        float* d_rmse = gt_frames ? c->track_rmse.as<float>() + (size_t)(k - 1) * 2 : nullptr;
        if (gt_frames) {
            // the convergence reference: the source moved by pose_before^-1 gt_k, composed in fp64 and rounded once
            double Ri[9], ti[3];
            invert_affine(pose_inout, Ri, ti);
            const float* g = gt_frames + (size_t)(k - 1) * 16;
            Pose16 G; memset(&G, 0, sizeof(G)); G.m[15] = 1.f;
            for (int rr = 0; rr < 3; rr++) {
                for (int cc = 0; cc < 3; cc++) G.m[cc * 4 + rr] = (float)((Ri[rr * 3] * g[cc * 4] + Ri[rr * 3 + 1] * g[cc * 4 + 1]) + Ri[rr * 3 + 2] * g[cc * 4 + 2]);
                G.m[12 + rr] = (float)(((Ri[rr * 3] * g[12] + Ri[rr * 3 + 1] * g[13]) + Ri[rr * 3 + 2] * g[14]) + ti[rr]);
            }
            if ((rc = track_reference(c, kept, G))) return rc;
            if ((rc = track_rmse_at(c, 0, identity, d_rmse))) return rc;
        }
        float dT[16]; memcpy(dT, identity, 64);
        int32_t iters = 0;
        rc = run_loop(c, dT, nullptr, 0, &iters, false, c->merge_loop);
        if (rc == ICP_ERR_HIP) return rc;
        r.iterations = iters; r.status = rc;
        if (rc != ICP_OK && first_err == ICP_OK) first_err = rc;      // (the message is run_loop's)
        if (gt_frames && (rc = track_rmse_at(c, 1, dT, d_rmse + 1))) return rc;
        if (r.status == ICP_OK) {
            compose_pose(pose_inout, dT);
            if ((rc = integrate(slot))) return rc;
        }
        memcpy(r.pose, pose_inout, 64);
    }
    HIPCK(c, hipStreamSynchronize(c->stream));
    HIPCK(c, hipStreamSynchronize(c->depth_stream));
    if (gt_frames && n_frames > 1 && (rc = track_rmse_finish(c, n_frames, out, [](const icp_track_frame& r) { return r.n_src > 0 && r.status != ICP_ERR_NO_TARGET; }))) return rc;
    guard.ok = true;
    return first_err;
}
int icp_track_depth_model(icp_ctx* c, const float* depth_frames, int32_t n_frames, const icp_depth_camera* cam, const icp_depth_options* source_opt,
                          const float* gt_frames, float pose_inout[16], icp_track_frame* out) {
    if (!c) return ICP_ERR_INVALID_ARG;
    return track_depth_model(c, depth_frames, nullptr, false, n_frames, cam, source_opt, gt_frames, pose_inout, out, "icp_track_depth_model");
}
int icp_track_depth_model_color(icp_ctx* c, const float* depth_frames, const uint8_t* rgbx_frames, int32_t n_frames, const icp_depth_camera* cam,
                                const icp_depth_options* source_opt, const float* gt_frames, float pose_inout[16], icp_track_frame* out) {
    if (!c) return ICP_ERR_INVALID_ARG;
    return track_depth_model(c, depth_frames, rgbx_frames, true, n_frames, cam, source_opt, gt_frames, pose_inout, out, "icp_track_depth_model_color");
}

// Not part of icp_hip.h (tools/time_tsdf.py): the device time of ONE integrate (which = 0, the frame staged outside the bracket) or ONE
// ray-cast to the host-layout arrays (which = 1) between two events on the context's stream.
extern "C" int icp_debug_tsdf_time(icp_ctx* c, int32_t which, const float* depth, const icp_depth_camera* cam, const float pose[16], float* ms_out) {
    if (!c || !ms_out || which < 0 || which > 1) return ICP_ERR_INVALID_ARG;
    int rc;
    if ((rc = tsdf_check_call(c, cam, pose, "icp_debug_tsdf_time"))) return rc;
    if (which == 0 && !depth) return ICP_ERR_INVALID_ARG;
    return tsdf_time(c, which, depth, nullptr, *cam, pose, ms_out, false);
}

// Not part of icp_hip.h (tools/time_tsdf_color.py): icp_debug_tsdf_time for the coloured kernels -- ONE icp_tsdf_integrate_color (which = 0,
// the frames staged outside the bracket) or ONE icp_tsdf_raycast_color to the host-layout arrays (which = 1).
extern "C" int icp_debug_tsdf_color_time(icp_ctx* c, int32_t which, const float* depth, const uint8_t* rgbx, const icp_depth_camera* cam, const float pose[16],
                                         float* ms_out) {
    if (!c || !ms_out || which < 0 || which > 1) return ICP_ERR_INVALID_ARG;
    int rc;
    if ((rc = tsdf_check_call(c, cam, pose, "icp_debug_tsdf_color_time"))) return rc;
    if ((rc = tsdf_check_color(c, "icp_debug_tsdf_color_time"))) return rc;
    if (which == 0 && (!depth || !rgbx)) return ICP_ERR_INVALID_ARG;
    return tsdf_time(c, which, depth, rgbx, *cam, pose, ms_out, true);
}
