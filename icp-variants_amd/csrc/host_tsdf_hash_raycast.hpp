// host_tsdf_hash_raycast.hpp -- the hashed volume seen from a pose and tracked frame-to-model: icp_tsdf_raycast_hashed,
// icp_set_target_tsdf_hashed, icp_track_depth_model_hashed, and their coloured forms on a coloured hashed volume:
// icp_tsdf_raycast_color_hashed, icp_set_target_tsdf_color_hashed, icp_track_depth_model_color_hashed.  Kernels: dev_tsdf_hash_raycast.hpp,
// dev_tsdf_hash_raycast_color.hpp.  The bodies are host_tsdf.hpp's tsdf_raycast_to_host, set_target_tsdf_call and track_depth_model, which launch
// this file's ray-cast and host_tsdf_hash.hpp's integrate when they are told the volume is hashed; the functions here are their own checks.  Contract: include/icp_hip.h, DESIGN.md
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
    return tsdf_raycast_to_host(c, *cam, pose, depth_out, vertices_out, normals_out, nullptr, n_hits_out, nullptr, false, true);
}

int icp_set_target_tsdf_hashed(icp_ctx* c, const icp_depth_camera* cam, const float pose[16], int32_t* n_points_out) {
    if (!c) return ICP_ERR_INVALID_ARG;
    if (n_points_out) *n_points_out = 0;
    const char* who = "icp_set_target_tsdf_hashed";
    int rc;
    if ((rc = htsdf_ray_check(c, who, "icp_set_target_tsdf"))) return rc;
    if ((rc = tsdf_check_call(c, cam, pose, who, true))) return rc;
    return set_target_tsdf_call(c, *cam, pose, n_points_out, who, false, true);
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
    return tsdf_raycast_to_host(c, *cam, pose, depth_out, vertices_out, normals_out, rgba_out, n_hits_out, n_colored_out, true, true);
}

int icp_set_target_tsdf_color_hashed(icp_ctx* c, const icp_depth_camera* cam, const float pose[16], int32_t* n_points_out) {
    if (!c) return ICP_ERR_INVALID_ARG;
    if (n_points_out) *n_points_out = 0;
    const char* who = "icp_set_target_tsdf_color_hashed";
    int rc;
    if ((rc = htsdf_ray_check_color(c, who, "icp_set_target_tsdf_color"))) return rc;
    if ((rc = tsdf_check_call(c, cam, pose, who, true))) return rc;
    return set_target_tsdf_call(c, *cam, pose, n_points_out, who, true, true);
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

// icp_debug_htsdf_raycast_time and its coloured form behind their checks: ONE ray-cast of the hashed volume to the host-layout arrays inside timed_ms.
static int htsdf_raycast_time(icp_ctx* c, const icp_depth_camera& cam, const float pose[16], float* ms_out, bool color) {
    int rc;
    DrainOnError guard(c);
    if ((rc = set_device(c))) return rc;
    TsdfRayOut o; TsdfColorOut co;
    if ((rc = tsdf_ray_stage(c, (size_t)cam.width * cam.height, color, true, true, true, true, &o, &co))) return rc;
    if ((rc = timed_ms(c, ms_out, [&] { return htsdf_raycast_launch(c, cam, pose, false, o, color ? &co : nullptr); }))) return rc;
    return guard.done();
}

// Not part of icp_hip.h (tools/time_htsdf_color_view.py): icp_debug_htsdf_raycast_time for ONE coloured ray-cast of the hashed volume.
extern "C" int icp_debug_htsdf_raycast_color_time(icp_ctx* c, const icp_depth_camera* cam, const float pose[16], float* ms_out) {
    if (!c || !ms_out) return ICP_ERR_INVALID_ARG;
    const char* who = "icp_debug_htsdf_raycast_color_time";
    int rc;
    if ((rc = htsdf_ray_check_color(c, who, "icp_debug_tsdf_color_time"))) return rc;
    if ((rc = tsdf_check_call(c, cam, pose, who, true))) return rc;
    return htsdf_raycast_time(c, *cam, pose, ms_out, true);
}

// Not part of icp_hip.h (tools/time_htsdf_raycast.py): the device time of ONE ray-cast of the hashed volume to the host-layout arrays
// between two events on the context's stream (icp_debug_tsdf_time's which = 1, for the hashed volume).
extern "C" int icp_debug_htsdf_raycast_time(icp_ctx* c, const icp_depth_camera* cam, const float pose[16], float* ms_out) {
    if (!c || !ms_out) return ICP_ERR_INVALID_ARG;
    const char* who = "icp_debug_htsdf_raycast_time";
    int rc;
    if ((rc = htsdf_ray_check(c, who, "icp_debug_tsdf_time"))) return rc;
    if ((rc = tsdf_check_call(c, cam, pose, who, true))) return rc;
    return htsdf_raycast_time(c, *cam, pose, ms_out, false);
}
