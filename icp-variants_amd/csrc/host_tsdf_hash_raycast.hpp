// host_tsdf_hash_raycast.hpp -- the hashed volume seen from a pose and tracked frame-to-model: icp_tsdf_raycast_hashed,
// icp_set_target_tsdf_hashed, icp_track_depth_model_hashed, and their coloured forms on a coloured hashed volume:
// icp_tsdf_raycast_color_hashed, icp_set_target_tsdf_color_hashed, icp_track_depth_model_color_hashed.  Kernels: dev_tsdf_hash_raycast.hpp,
// dev_tsdf_hash_raycast_color.hpp.  The target and the tracking loop are host_tsdf.hpp's set_target_tsdf and track_depth_model, which launch
// this file's ray-cast and host_tsdf_hash.hpp's integrate when they are told the volume is hashed.  Contract: include/icp_hip.h, DESIGN.md
// sections 6z and 6zc.
// Part of icp_hip.hip (included from there, after host_tsdf_hash.hpp).
namespace {
// no volume; a dense volume: refused with the call's name, nothing touched
int htsdf_ray_check(icp_ctx* c, const char* who, const char* dense_call) {
    if (!c->tsdf_on) { c->err = std::string(who) + ": no volume (icp_tsdf_create_hashed)"; return ICP_ERR_INVALID_ARG; }
    if (!c->tsdf_hashed) { c->err = std::string(who) + ": the volume is dense (icp_tsdf_create): use " + dense_call; return ICP_ERR_INVALID_ARG; }
    return ICP_OK;
}
// no volume; a dense volume; a hashed volume without colours
int htsdf_ray_check_color(icp_ctx* c, const char* who, const char* dense_call) {
    int rc;
    if ((rc = htsdf_ray_check(c, who, dense_call))) return rc;
    if (!c->th_color) { c->err = std::string(who) + ": the hashed volume has no colours (icp_tsdf_create_color_hashed)"; return ICP_ERR_INVALID_ARG; }
    return ICP_OK;
}
// tsdf_raycast_launch on the hashed volume: enqueued; the hit count lands in tsdf_cnt (zeroed first).  co: with colours from the colour
// pool, the coloured hits in tsdf_cnt[1].
int htsdf_raycast_launch(icp_ctx* c, const icp_depth_camera& cam, const float pose[16], bool soa, const TsdfRayOut& o, const TsdfColorOut* co) {
    int rc;
    if ((rc = ensure(c, c->tsdf_cnt, 16))) return rc;
    TsdfMat m; memcpy(m.m, pose, 64);
    HtRay r; r.min_d = c->tsdf_opt.min_depth; r.step = c->tsdf_opt.ray_step;
    HIPCK(c, hipMemsetAsync(c->tsdf_cnt.p, 0, co ? 8 : 4, c->stream));
    const dim3 grid((cam.width + 15) / 16, (cam.height + 15) / 16);
    int* cnt = c->tsdf_cnt.as<int>();
    const float4* cpool = c->th_cpool.as<float4>();
    if (co && soa) hipLaunchKernelGGL(k_htsdf_raycast_color<true>, grid, dim3(256), 0, c->stream, htsdf_view(c), r, tsdf_cam(cam), m, o, cnt, cpool, *co, cnt + 1);
    else if (co) hipLaunchKernelGGL(k_htsdf_raycast_color<false>, grid, dim3(256), 0, c->stream, htsdf_view(c), r, tsdf_cam(cam), m, o, cnt, cpool, *co, cnt + 1);
    else if (soa) hipLaunchKernelGGL(k_htsdf_raycast<true>, grid, dim3(256), 0, c->stream, htsdf_view(c), r, tsdf_cam(cam), m, o, c->tsdf_cnt.as<int>());
    else hipLaunchKernelGGL(k_htsdf_raycast<false>, grid, dim3(256), 0, c->stream, htsdf_view(c), r, tsdf_cam(cam), m, o, c->tsdf_cnt.as<int>());
    HIPCK(c, hipGetLastError());
    return ICP_OK;
}
}  // namespace

int icp_tsdf_raycast_hashed(icp_ctx* c, const icp_depth_camera* cam, const float pose[16], float* depth_out, float* vertices_out, float* normals_out,
                            int32_t* n_hits_out) {
    if (!c) return ICP_ERR_INVALID_ARG;
    if (n_hits_out) *n_hits_out = 0;
    const char* who = "icp_tsdf_raycast_hashed";
    int rc;
    if ((rc = htsdf_ray_check(c, who, "icp_tsdf_raycast"))) return rc;
    if ((rc = tsdf_check_call(c, cam, pose, who, true))) return rc;
    DrainOnError guard(c);
    if ((rc = set_device(c))) return rc;
    const size_t n = (size_t)cam->width * cam->height;
    if ((rc = ensure(c, c->staging, n * 28))) return rc;      // [depth 4n | vertices 12n | normals 12n]
    float* d = c->staging.as<float>();
    TsdfRayOut o; memset(&o, 0, sizeof(o));
    o.depth = depth_out ? d : nullptr; o.vert = vertices_out ? d + n : nullptr; o.nrm = normals_out ? d + 4 * n : nullptr;
    if ((rc = htsdf_raycast_launch(c, *cam, pose, false, o))) return rc;
    if (depth_out) HIPCK(c, hipMemcpyAsync(depth_out, o.depth, n * 4, hipMemcpyDeviceToHost, c->stream));
    if (vertices_out) HIPCK(c, hipMemcpyAsync(vertices_out, o.vert, n * 12, hipMemcpyDeviceToHost, c->stream));
    if (normals_out) HIPCK(c, hipMemcpyAsync(normals_out, o.nrm, n * 12, hipMemcpyDeviceToHost, c->stream));
    int hits = 0;
    if ((rc = read_count(c, c->tsdf_cnt.p, &hits))) return rc;      // (the one host wait)
    if (n_hits_out) *n_hits_out = hits;
    return guard.done();
}

int icp_set_target_tsdf_hashed(icp_ctx* c, const icp_depth_camera* cam, const float pose[16], int32_t* n_points_out) {
    if (!c) return ICP_ERR_INVALID_ARG;
    if (n_points_out) *n_points_out = 0;
    const char* who = "icp_set_target_tsdf_hashed";
    int rc;
    if ((rc = htsdf_ray_check(c, who, "icp_set_target_tsdf"))) return rc;
    if ((rc = tsdf_check_call(c, cam, pose, who, true))) return rc;
    DrainOnError guard(c);
    if ((rc = set_device(c))) return rc;
    int hits = 0;
    rc = set_target_tsdf(c, *cam, pose, &hits, who, false, true);
    if (rc == ICP_ERR_NO_TARGET) return guard.done(rc);      // (synchronised by the count read)
    if (rc) return rc;
    if (n_points_out) *n_points_out = hits;
    HIPCK(c, hipStreamSynchronize(c->stream));
    return guard.done();
}

// track_depth_model with the hashed ray-cast as the target and htsdf_integrate_slot as the integrate.  Host waits per tracked frame: the
// dense loop's (the hit count, the run's) and the touch's counters, plus one per growth of the pool.
int icp_track_depth_model_hashed(icp_ctx* c, const float* depth_frames, int32_t n_frames, const icp_depth_camera* cam, const icp_depth_options* source_opt,
                                 const float* gt_frames, float pose_inout[16], icp_track_frame* out) {
    if (!c) return ICP_ERR_INVALID_ARG;
    const char* who = "icp_track_depth_model_hashed";
    int rc;
    if ((rc = htsdf_ray_check(c, who, "icp_track_depth_model"))) return rc;
    return track_depth_model(c, depth_frames, nullptr, false, n_frames, cam, source_opt, gt_frames, pose_inout, out, who, true);
}

// ---- the coloured forms: icp_tsdf_raycast_color, icp_set_target_tsdf_color and icp_track_depth_model_color read
// through the blocks
int icp_tsdf_raycast_color_hashed(icp_ctx* c, const icp_depth_camera* cam, const float pose[16], float* depth_out, float* vertices_out, float* normals_out,
                                  uint8_t* rgba_out, int32_t* n_hits_out, int32_t* n_colored_out) {
    if (!c) return ICP_ERR_INVALID_ARG;
    if (n_hits_out) *n_hits_out = 0;
    if (n_colored_out) *n_colored_out = 0;
    const char* who = "icp_tsdf_raycast_color_hashed";
    int rc;
    if ((rc = htsdf_ray_check_color(c, who, "icp_tsdf_raycast_color"))) return rc;
    if ((rc = tsdf_check_call(c, cam, pose, who, true))) return rc;
    DrainOnError guard(c);
    if ((rc = set_device(c))) return rc;
    const size_t n = (size_t)cam->width * cam->height;
    if ((rc = ensure(c, c->staging, n * 32))) return rc;      // [depth 4n | vertices 12n | normals 12n | rgba 4n]
    float* d = c->staging.as<float>();
    TsdfRayOut o; memset(&o, 0, sizeof(o));
    o.depth = depth_out ? d : nullptr; o.vert = vertices_out ? d + n : nullptr; o.nrm = normals_out ? d + 4 * n : nullptr;
    const TsdfColorOut co = {rgba_out ? (uint32_t*)(d + 7 * n) : nullptr, nullptr, nullptr, nullptr};
    if ((rc = htsdf_raycast_launch(c, *cam, pose, false, o, &co))) return rc;
    if (depth_out) HIPCK(c, hipMemcpyAsync(depth_out, o.depth, n * 4, hipMemcpyDeviceToHost, c->stream));
    if (vertices_out) HIPCK(c, hipMemcpyAsync(vertices_out, o.vert, n * 12, hipMemcpyDeviceToHost, c->stream));
    if (normals_out) HIPCK(c, hipMemcpyAsync(normals_out, o.nrm, n * 12, hipMemcpyDeviceToHost, c->stream));
    if (rgba_out) HIPCK(c, hipMemcpyAsync(rgba_out, co.rgba, n * 4, hipMemcpyDeviceToHost, c->stream));
    int cnt[2] = {0, 0};
    if ((rc = read_count(c, c->tsdf_cnt.p, cnt, 2))) return rc;      // (the one host wait)
    if (n_hits_out) *n_hits_out = cnt[0];
    if (n_colored_out) *n_colored_out = cnt[1];
    return guard.done();
}

int icp_set_target_tsdf_color_hashed(icp_ctx* c, const icp_depth_camera* cam, const float pose[16], int32_t* n_points_out) {
    if (!c) return ICP_ERR_INVALID_ARG;
    if (n_points_out) *n_points_out = 0;
    const char* who = "icp_set_target_tsdf_color_hashed";
    int rc;
    if ((rc = htsdf_ray_check_color(c, who, "icp_set_target_tsdf_color"))) return rc;
    if ((rc = tsdf_check_call(c, cam, pose, who, true))) return rc;
    DrainOnError guard(c);
    if ((rc = set_device(c))) return rc;
    int hits = 0;
    rc = set_target_tsdf(c, *cam, pose, &hits, who, true, true);
    if (rc == ICP_ERR_NO_TARGET) return guard.done(rc);      // (synchronised by the count read)
    if (rc) return rc;
    if (n_points_out) *n_points_out = hits;
    HIPCK(c, hipStreamSynchronize(c->stream));
    return guard.done();
}

// track_depth_model with the coloured hashed ray-cast as the target and the coloured htsdf_integrate_slot as the integrate.  Host waits:
// icp_track_depth_model_hashed's.
int icp_track_depth_model_color_hashed(icp_ctx* c, const float* depth_frames, const uint8_t* rgbx_frames, int32_t n_frames, const icp_depth_camera* cam,
                                       const icp_depth_options* source_opt, const float* gt_frames, float pose_inout[16], icp_track_frame* out) {
    if (!c) return ICP_ERR_INVALID_ARG;
    const char* who = "icp_track_depth_model_color_hashed";
    int rc;
    if ((rc = htsdf_ray_check_color(c, who, "icp_track_depth_model_color"))) return rc;
    return track_depth_model(c, depth_frames, rgbx_frames, true, n_frames, cam, source_opt, gt_frames, pose_inout, out, who, true);
}

// Not part of icp_hip.h (tools/time_htsdf_color_view.py): icp_debug_htsdf_raycast_time for ONE coloured ray-cast of the hashed volume.
extern "C" int icp_debug_htsdf_raycast_color_time(icp_ctx* c, const icp_depth_camera* cam, const float pose[16], float* ms_out) {
    if (!c || !ms_out) return ICP_ERR_INVALID_ARG;
    const char* who = "icp_debug_htsdf_raycast_color_time";
    int rc;
    if ((rc = htsdf_ray_check_color(c, who, "icp_debug_tsdf_color_time"))) return rc;
    if ((rc = tsdf_check_call(c, cam, pose, who, true))) return rc;
    DrainOnError guard(c);
    if ((rc = set_device(c))) return rc;
    if ((rc = ensure_events(c, 2))) return rc;
    const size_t n = (size_t)cam->width * cam->height;
    if ((rc = ensure(c, c->staging, n * 32))) return rc;
    float* d = c->staging.as<float>();
    TsdfRayOut o; memset(&o, 0, sizeof(o));
    o.depth = d; o.vert = d + n; o.nrm = d + 4 * n;
    const TsdfColorOut co = {(uint32_t*)(d + 7 * n), nullptr, nullptr, nullptr};
    HIPCK(c, hipEventRecord(c->events[0], c->stream));
    if ((rc = htsdf_raycast_launch(c, *cam, pose, false, o, &co))) return rc;
    HIPCK(c, hipEventRecord(c->events[1], c->stream));
    HIPCK(c, hipStreamSynchronize(c->stream));
    HIPCK(c, hipEventElapsedTime(ms_out, c->events[0], c->events[1]));
    return guard.done();
}

// Not part of icp_hip.h (tools/time_htsdf_raycast.py): the device time of ONE ray-cast of the hashed volume to the host-layout arrays
// between two events on the context's stream (icp_debug_tsdf_time's which = 1, for the hashed volume).
extern "C" int icp_debug_htsdf_raycast_time(icp_ctx* c, const icp_depth_camera* cam, const float pose[16], float* ms_out) {
    if (!c || !ms_out) return ICP_ERR_INVALID_ARG;
    const char* who = "icp_debug_htsdf_raycast_time";
    int rc;
    if ((rc = htsdf_ray_check(c, who, "icp_debug_tsdf_time"))) return rc;
    if ((rc = tsdf_check_call(c, cam, pose, who, true))) return rc;
    DrainOnError guard(c);
    if ((rc = set_device(c))) return rc;
    if ((rc = ensure_events(c, 2))) return rc;
    const size_t n = (size_t)cam->width * cam->height;
    if ((rc = ensure(c, c->staging, n * 28))) return rc;
    float* d = c->staging.as<float>();
    TsdfRayOut o; memset(&o, 0, sizeof(o));
    o.depth = d; o.vert = d + n; o.nrm = d + 4 * n;
    HIPCK(c, hipEventRecord(c->events[0], c->stream));
    if ((rc = htsdf_raycast_launch(c, *cam, pose, false, o))) return rc;
    HIPCK(c, hipEventRecord(c->events[1], c->stream));
    HIPCK(c, hipStreamSynchronize(c->stream));
    HIPCK(c, hipEventElapsedTime(ms_out, c->events[0], c->events[1]));
    return guard.done();
}
