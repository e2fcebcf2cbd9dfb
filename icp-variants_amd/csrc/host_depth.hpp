// host_depth.hpp -- depth frames as clouds: back-projection, icp_set_target_depth / icp_set_source_depth, the frame-to-reference tracker
// (icp_track_depth_frames) and the per-frame mesh (icp_depth_mesh).  Part of icp_hip.hip (included from there, after host_multi.hpp).
namespace {
// Inverse of a rigid/affine 4x4 (column-major, bottom row ignored) in fp64: 3x3 row-major R^-1 and t^-1 = -R^-1 t.
void invert_affine(const float* m, double Ri[9], double ti[3]) {
    double R[9], t[3];
    for (int r = 0; r < 3; r++) { for (int k = 0; k < 3; k++) R[r * 3 + k] = m[k * 4 + r]; t[r] = m[12 + r]; }
    const double det = R[0] * (R[4] * R[8] - R[5] * R[7]) - R[1] * (R[3] * R[8] - R[5] * R[6]) + R[2] * (R[3] * R[7] - R[4] * R[6]);
    const double q[9] = {(R[4] * R[8] - R[5] * R[7]) / det, (R[2] * R[7] - R[1] * R[8]) / det, (R[1] * R[5] - R[2] * R[4]) / det,
                         (R[5] * R[6] - R[3] * R[8]) / det, (R[0] * R[8] - R[2] * R[6]) / det, (R[2] * R[3] - R[0] * R[5]) / det,
                         (R[3] * R[7] - R[4] * R[6]) / det, (R[1] * R[6] - R[0] * R[7]) / det, (R[0] * R[4] - R[1] * R[3]) / det};
    for (int i = 0; i < 9; i++) Ri[i] = q[i];
    for (int r = 0; r < 3; r++) ti[r] = -(q[r * 3] * t[0] + q[r * 3 + 1] * t[1] + q[r * 3 + 2] * t[2]);
}
// depthExtrinsics.inverse() (PointCloud.h:88-90): rigid/affine 4x4 (column-major), inverted in fp64 and rounded once -> 3x3 row-major R^-1, t^-1
void invert_extrinsics(const float* extrinsics, float inv[12]) {
    double Ri[9], ti[3];
    invert_affine(extrinsics, Ri, ti);
    for (int i = 0; i < 9; i++) inv[i] = (float)Ri[i];
    for (int r = 0; r < 3; r++) inv[9 + r] = (float)ti[r];
}

bool depth_camera_ok(const icp_depth_camera* cam) {
    return cam && cam->width > 0 && cam->height > 0 && (long long)cam->width * cam->height <= 0x7FFFFFFFll &&
           std::isfinite(cam->fx) && std::isfinite(cam->fy) && std::isfinite(cam->cx) && std::isfinite(cam->cy);
}
int check_depth_args(icp_ctx* c, const icp_depth_camera* cam, const icp_depth_options* opt, const char* who) {
    if (!depth_camera_ok(cam) || !opt || opt->downsample_factor < 1 || std::isnan(opt->max_distance)) {
        c->err = std::string(who) + ": bad camera or options (width, height > 0, downsample_factor >= 1)"; return ICP_ERR_INVALID_ARG;
    }
    return ICP_OK;
}

// One depth frame [depth 4n | rgbx 4n] into upload slot `slot`: host -> page-locked block -> device, on stream s (the context's own stream,
// or depth_stream when the frame goes up while the previous one iterates); depth_up[slot] marks its arrival.  The only host-side wait is for
// the slot's previous copy to have left the page-locked block.
// The colour frame has n pixels unless n_color says otherwise (icp_depth_mesh's colour camera).
int stage_depth(icp_ctx* c, int slot, const float* depth, const uint8_t* rgbx, int n, hipStream_t s, int n_color = -1) {
    if (n_color < 0) n_color = n;
    if (!c->depth_up[slot]) HIPCK(c, hipEventCreateWithFlags(&c->depth_up[slot].e, hipEventDisableTiming));
    if (c->depth_pending[slot]) { HIPCK(c, hipEventSynchronize(c->depth_up[slot])); c->depth_pending[slot] = false; }
    const size_t bytes = (size_t)n * 4 + (rgbx ? (size_t)n_color * 4 : 0), cap = (size_t)n * 4 + (size_t)(n_color > n ? n_color : n) * 4;
    int rc;
    PinBuf& pin = c->depth_pin[slot];
    if ((rc = ensure_pin(c, pin, bytes, cap, 0))) return rc;      // (a block that has to grow becomes exactly cap >= bytes)
    if ((rc = ensure(c, c->depth_dev[slot], cap))) return rc;
    memcpy(pin.p, depth, (size_t)n * 4);
    if (rgbx) memcpy(pin.as<char>() + (size_t)n * 4, rgbx, (size_t)n_color * 4);
    HIPCK(c, hipMemcpyAsync(c->depth_dev[slot].p, pin.p, bytes, hipMemcpyHostToDevice, s));
    HIPCK(c, hipEventRecord(c->depth_up[slot], s)); c->depth_pending[slot] = true;
    return ICP_OK;
}

// PointCloud(depthMap, colorFrame, K, extrinsics, width, height, keepOriginalSize, downsampleFactor, maxDistance) (PointCloud.h:78-165) from
// the frame in upload slot `slot` straight into the SoA planes of `cl` (dev_depth.hpp): count -> scan -> scatter on the context's stream,
// then ONE 4-byte copy of the kept-point count back to the host (the cloud's size decides every launch after it).  Leaves the planes as
// upload_cloud leaves them for the same arrays (pad: +inf padding of a target).
int depth_to_cloud(icp_ctx* c, int slot, const icp_depth_camera& cam, const icp_depth_options& opt, bool with_colors, Cloud& cl, bool pad, int* n_out) {
    int rc;
    const int n = cam.width * cam.height, f = opt.downsample_factor;
    const int count = (int)(((long long)n + f - 1) / f);
    const int nb = (count + 255) / 256, cap = (count + 63) / 64 * 64;
    HIPCK(c, hipStreamWaitEvent(c->stream, c->depth_up[slot], 0));
    DepthFrame fr;
    fr.depth = c->depth_dev[slot].as<float>(); fr.rgbx = with_colors ? c->depth_dev[slot].as<uint8_t>() + (size_t)n * 4 : nullptr;
    fr.width = cam.width; fr.height = cam.height; fr.factor = f; fr.count = count;
    fr.fx = cam.fx; fr.fy = cam.fy; fr.cx = cam.cx; fr.cy = cam.cy; fr.max_distance_halved = opt.max_distance / 2.f;
    invert_extrinsics(cam.extrinsics, fr.inv);
    fr.keep_all = opt.keep_original_size ? 1 : 0; fr.fix_color_index = opt.fix_color_index ? 1 : 0;
    for (DevBuf* pl : {&cl.x, &cl.y, &cl.z, &cl.nx, &cl.ny, &cl.nz}) if ((rc = ensure(c, *pl, (size_t)cap * 4))) return rc;
    if (with_colors) { for (DevBuf* pl : {&cl.rgba, &cl.cr, &cl.cg, &cl.cb}) if ((rc = ensure(c, *pl, (size_t)cap * 4))) return rc; }
    else for (DevBuf* pl : {&cl.rgba, &cl.cr, &cl.cg, &cl.cb}) release(*pl);      // no colour planes of an earlier, differently sized cloud stay behind
    if ((rc = ensure(c, c->depth_blocks, (size_t)nb * 4))) return rc;
    if ((rc = ensure(c, c->d_count, 16))) return rc;
    DepthOut o;
    o.x = cl.x.as<float>(); o.y = cl.y.as<float>(); o.z = cl.z.as<float>(); o.nx = cl.nx.as<float>(); o.ny = cl.ny.as<float>(); o.nz = cl.nz.as<float>();
    o.cr = with_colors ? cl.cr.as<float>() : nullptr; o.cg = with_colors ? cl.cg.as<float>() : nullptr; o.cb = with_colors ? cl.cb.as<float>() : nullptr;
    o.rgba = with_colors ? cl.rgba.as<uint32_t>() : nullptr;
    hipLaunchKernelGGL(k_depth_count, dim3(nb), dim3(256), 0, c->stream, fr, c->depth_blocks.as<int>());
    hipLaunchKernelGGL(k_select_scan, dim3(1), dim3(1024), 0, c->stream, c->depth_blocks.as<int>(), nb, c->d_count.as<int>());
    hipLaunchKernelGGL(k_depth_scatter, dim3(nb), dim3(256), 0, c->stream, fr, (const int*)c->depth_blocks.as<int>(), (const int*)c->d_count.as<int>(), pad ? 1 : 0, o);
    HIPCK(c, hipGetLastError());
    int kept = 0;
    if ((rc = read_count(c, c->d_count.p, &kept))) return rc;
    cl.n = kept; cl.npad = pad ? (kept + 63) / 64 * 64 : kept;
    cl.has_normals = true; cl.has_colors = with_colors;
    *n_out = kept;
    return ICP_OK;
}

// ---- the ground-truth RMSE bracket of a tracked frame, shared by icp_track_depth_frames and icp_track_depth_model ----
// track_rmse: per tracked frame its initial and final RMSE; pin_track: two page-locked pose slots of their own (see track_rmse_at).
int track_rmse_prepare(icp_ctx* c, int n_frames) {
    int rc;
    if ((rc = ensure(c, c->track_rmse, (size_t)(n_frames - 1) * 8))) return rc;
    return ensure_pin(c, c->pin_track, 2 * sizeof(PoseState), 0, 0);
}
// The convergence reference of the frame: the resident source (its `kept` points) and the same points moved by g.
int track_reference(icp_ctx* c, int kept, const Pose16& g) {
    int rc;
    for (DevBuf* pl : {&c->conv_src.x, &c->conv_src.y, &c->conv_src.z, &c->conv_ref.x, &c->conv_ref.y, &c->conv_ref.z}) if ((rc = ensure(c, *pl, (size_t)kept * 4))) return rc;
    hipLaunchKernelGGL(k_conv_from_source, dim3((kept + 255) / 256), dim3(256), 0, c->stream, c->src.x.as<float>(), c->src.y.as<float>(), c->src.z.as<float>(), kept, g,
                       c->conv_src.x.as<float>(), c->conv_src.y.as<float>(), c->conv_src.z.as<float>(), c->conv_ref.x.as<float>(), c->conv_ref.y.as<float>(), c->conv_ref.z.as<float>());
    HIPCK(c, hipGetLastError());
    c->conv_n = kept;
    return ICP_OK;
}
// The RMSE of the reference under `pose` into d_out, enqueued; k = 0 before the frame's run, 1 after it.  The pose is staged in
// pin_track[k], not in `pinned`: run_loop's write_pose rewrites `pinned` right after the initial measure, while this copy may still wait
// behind the kernels in front of it.  pin_track[0] / [1] are rewritten only by the next frame, after its first count read (depth_to_cloud,
// set_target_tsdf) has synchronised the stream, i.e. after both copies have left them; the end of the call synchronises before the last
// ones matter.
int track_rmse_at(icp_ctx* c, int k, const float pose[16], float* d_out) {
    int rc;
    if ((rc = write_pose_via(c, c->pin_track.as<PoseState>() + k, pose))) return rc;
    return enqueue_rmse(c, d_out);
}
// After the stream has drained: the measures back, into the frames that `measured` says had both taken.
template <class Measured>
int track_rmse_finish(icp_ctx* c, int n_frames, icp_track_frame* out, Measured measured) {
    std::vector<float> h((size_t)(n_frames - 1) * 2);
    HIPCK(c, hipMemcpy(h.data(), c->track_rmse.p, h.size() * 4, hipMemcpyDeviceToHost));
    for (int k = 1; k < n_frames; k++) if (measured(out[k - 1])) { out[k - 1].initial_rmse = h[(size_t)(k - 1) * 2]; out[k - 1].final_rmse = h[(size_t)(k - 1) * 2 + 1]; }
    return ICP_OK;
}

static int set_cloud_depth(icp_ctx* c, bool target, const float* depth, const uint8_t* rgbx, const icp_depth_camera* cam, const icp_depth_options* opt, int32_t* n_points_out) {
    const char* who = target ? "icp_set_target_depth" : "icp_set_source_depth";
    if (!c) return ICP_ERR_INVALID_ARG;
    if (n_points_out) *n_points_out = 0;
    if (!depth) { c->err = std::string(who) + ": null depth frame"; return ICP_ERR_INVALID_ARG; }
    int rc;
    if ((rc = check_depth_args(c, cam, opt, who))) return rc;
    DrainOnError guard(c);
    if ((rc = set_device(c))) return rc;
    int kept = 0;
    if ((rc = stage_depth(c, 0, depth, rgbx, cam->width * cam->height, c->stream))) return rc;
    if ((rc = depth_to_cloud(c, 0, *cam, *opt, rgbx != nullptr, target ? c->tgt : c->src, target, &kept))) return rc;
    if (n_points_out) *n_points_out = kept;
    if (target) {
        if (kept == 0) { c->bvh.valid = false; c->bvh6.valid = false; c->err = "icp_set_target_depth: the frame keeps no points"; return guard.done(ICP_ERR_NO_TARGET); }
        if ((rc = finish_target(c, rgbx != nullptr))) return rc;
    } else {
        if ((rc = finish_source(c))) return rc;
        if (kept == 0) { c->err = "icp_set_source_depth: the frame keeps no points"; return guard.done(ICP_ERR_NO_SOURCE); }
    }
    HIPCK(c, hipStreamSynchronize(c->stream));
    return guard.done();
}
}  // namespace

int icp_backproject_depth(icp_ctx* c, const float* depth, const uint8_t* rgbx, float fx, float fy, float cx, float cy,
                          const float extrinsics[16], int32_t width, int32_t height, float max_distance, int32_t fix_color_index,
                          float* xyz_out, float* normals_out, uint8_t* rgba_out, uint8_t* valid_out) {
    if (!c || !depth || !extrinsics || !xyz_out || !normals_out || width <= 0 || height <= 0) { if (c) c->err = "icp_backproject_depth: bad argument"; return ICP_ERR_INVALID_ARG; }
    int rc;
    DrainOnError guard(c);
    if ((rc = set_device(c))) return rc;
    const size_t n = (size_t)width * height;
    float inv[12];
    invert_extrinsics(extrinsics, inv);
    // fixed layout, colour slots always reserved: [depth 4n | rgbx 4n | inverse 64 | xyz 12n | normals 12n | rgba 4n | valid n]
    const size_t bytes = n * 4 + n * 4 + 64 + n * 12 * 2 + n * 4 + n;
    if ((rc = ensure(c, c->staging, bytes + 256))) return rc;
    char* base = c->staging.as<char>();
    float* d_depth = (float*)base; uint8_t* d_rgbx = (uint8_t*)(base + n * 4); float* d_inv = (float*)(base + n * 8);
    float* d_xyz = (float*)(base + n * 8 + 64); float* d_nrm = d_xyz + n * 3; uint8_t* d_rgba = (uint8_t*)(d_nrm + n * 3); uint8_t* d_valid = d_rgba + n * 4;
    HIPCK(c, hipMemcpyAsync(d_depth, depth, n * 4, hipMemcpyHostToDevice, c->stream));
    if (rgbx) HIPCK(c, hipMemcpyAsync(d_rgbx, rgbx, n * 4, hipMemcpyHostToDevice, c->stream));
    HIPCK(c, hipMemcpyAsync(d_inv, inv, sizeof(inv), hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(k_backproject, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, d_depth, rgbx ? d_rgbx : nullptr, width, height, fx, fy, cx, cy, d_inv,
                       max_distance / 2.f, fix_color_index, d_xyz, d_nrm, (rgbx && rgba_out) ? d_rgba : nullptr, valid_out ? d_valid : nullptr);
    HIPCK(c, hipGetLastError());
    HIPCK(c, hipMemcpyAsync(xyz_out, d_xyz, n * 12, hipMemcpyDeviceToHost, c->stream));
    HIPCK(c, hipMemcpyAsync(normals_out, d_nrm, n * 12, hipMemcpyDeviceToHost, c->stream));
    if (rgbx && rgba_out) HIPCK(c, hipMemcpyAsync(rgba_out, d_rgba, n * 4, hipMemcpyDeviceToHost, c->stream));
    if (valid_out) HIPCK(c, hipMemcpyAsync(valid_out, d_valid, n, hipMemcpyDeviceToHost, c->stream));
    HIPCK(c, hipStreamSynchronize(c->stream));
    return guard.done();
}

int icp_set_target_depth(icp_ctx* c, const float* depth, const uint8_t* rgbx, const icp_depth_camera* cam, const icp_depth_options* opt, int32_t* n_points_out) {
    return set_cloud_depth(c, true, depth, rgbx, cam, opt, n_points_out);
}
int icp_set_source_depth(icp_ctx* c, const float* depth, const uint8_t* rgbx, const icp_depth_camera* cam, const icp_depth_options* opt, int32_t* n_points_out) {
    return set_cloud_depth(c, false, depth, rgbx, cam, opt, n_points_out);
}

int icp_track_depth_frames(icp_ctx* c, const float* depth_frames, const uint8_t* rgbx_frames, int32_t n_frames, const icp_depth_camera* cam,
                           const icp_depth_options* target_opt, const icp_depth_options* source_opt, const float* gt_frames, float pose_inout[16],
                           icp_track_frame* out) {
    if (!c) return ICP_ERR_INVALID_ARG;
    if (!depth_frames || n_frames < 1 || !pose_inout || (n_frames > 1 && !out)) { c->err = "icp_track_depth_frames: bad argument"; return ICP_ERR_INVALID_ARG; }
    int rc;
    if ((rc = check_depth_args(c, cam, target_opt, "icp_track_depth_frames")) || (rc = check_depth_args(c, cam, source_opt, "icp_track_depth_frames"))) return rc;
    const icp_params& p = c->prm;
    if (p.matching == ICP_MATCH_PROJECTIVE) {
        // the projective matcher indexes the target by pixel: the organised frame 0 (main.cpp:201-207) seen through the same camera
        if (!target_opt->keep_original_size || target_opt->downsample_factor != 1) { c->err = "icp_track_depth_frames: projective matching needs an organised target (keep_original_size = 1, factor 1)"; return ICP_ERR_INVALID_ARG; }
        if (p.fx != cam->fx || p.fy != cam->fy || p.cx != cam->cx || p.cy != cam->cy || p.width != cam->width || p.height != cam->height) {
            c->err = "icp_track_depth_frames: the camera of the params differs from the depth camera"; return ICP_ERR_INVALID_ARG;
        }
    }
    if (!rgbx_frames && ((p.matching == ICP_MATCH_KNN && p.color_icp) || p.weighting == ICP_WEIGHT_COLORS)) { c->err = "icp_track_depth_frames: colour ICP needs the colour frames"; return ICP_ERR_INVALID_ARG; }
    DrainOnError guard(c);
    if ((rc = set_device(c))) return rc;
    const int n = cam->width * cam->height;
    const size_t fbytes = (size_t)n * 4;
    auto frame_rgbx = [&](int k) { return rgbx_frames ? rgbx_frames + (size_t)k * fbytes : nullptr; };
    if (!c->depth_stream) HIPCK(c, hipStreamCreateWithFlags(&c->depth_stream.s, hipStreamNonBlocking));
    // frame 0 = the target, its index built once (main.cpp:200-207); frame 1 goes up meanwhile
    int kept = 0;
    if ((rc = stage_depth(c, 0, depth_frames, frame_rgbx(0), n, c->stream))) return rc;
    if ((rc = depth_to_cloud(c, 0, *cam, *target_opt, rgbx_frames != nullptr, c->tgt, true, &kept))) return rc;
    if (n_frames > 1 && (rc = stage_depth(c, 1, depth_frames + (size_t)n, frame_rgbx(1), n, c->depth_stream))) return rc;
    if (kept == 0) {
        c->bvh.valid = false; c->bvh6.valid = false;
        for (int k = 1; k < n_frames; k++) { icp_track_frame& r = out[k - 1]; memset(&r, 0, sizeof(r)); r.status = ICP_ERR_NO_TARGET; r.initial_rmse = r.final_rmse = -1.f; memcpy(r.pose, pose_inout, 64); }
        c->err = "icp_track_depth_frames: frame 0 keeps no points";
        HIPCK(c, hipStreamSynchronize(c->depth_stream));
        return guard.done(ICP_ERR_NO_TARGET);
    }
    if ((rc = finish_target(c, rgbx_frames != nullptr))) return rc;
    if (gt_frames && n_frames > 1 && (rc = track_rmse_prepare(c, n_frames))) return rc;
    int first_err = ICP_OK;
    for (int k = 1; k < n_frames; k++) {
        icp_track_frame& r = out[k - 1];
        memset(&r, 0, sizeof(r)); r.initial_rmse = r.final_rmse = -1.f;
        const int slot = k & 1;
        if ((rc = depth_to_cloud(c, slot, *cam, *source_opt, rgbx_frames != nullptr, c->src, false, &kept))) return rc;
        // frame k + 1 goes up on the second stream while frame k iterates (its slot was last read by frame k - 1, which has finished)
        if (k + 1 < n_frames && (rc = stage_depth(c, slot ^ 1, depth_frames + (size_t)(k + 1) * n, frame_rgbx(k + 1), n, c->depth_stream))) return rc;
        if ((rc = finish_source(c))) return rc;
        r.n_src = kept;
        if (kept == 0) {                                   // nothing to align: the pose is carried unchanged, tracking goes on
            r.status = ICP_ERR_NO_SOURCE; memcpy(r.pose, pose_inout, 64);
            if (first_err == ICP_OK) { first_err = ICP_ERR_NO_SOURCE; c->err = "icp_track_depth_frames: a frame keeps no points"; }
            continue;
        }
        float* d_rmse = gt_frames ? c->track_rmse.as<float>() + (size_t)(k - 1) * 2 : nullptr;
        if (gt_frames) {
            // ConvergenceMeasure(source, transformPoints(source, targetTrajectory * trajectory_k^-1)) (main.cpp:296-305), on the device
            Pose16 g; memcpy(g.m, gt_frames + (size_t)(k - 1) * 16, 64);
            if ((rc = track_reference(c, kept, g))) return rc;
            if ((rc = track_rmse_at(c, 0, pose_inout, d_rmse))) return rc;      // initial_rmse = rmseAlignmentError(currentCameraToWorld) (:305)
        }
        int32_t iters = 0;
        rc = run_loop(c, pose_inout, nullptr, 0, &iters, false, c->merge_loop);          // estimatePose(source, target, currentCameraToWorld) (:308)
        if (rc == ICP_ERR_HIP) return rc;
        r.iterations = iters; r.status = rc;
        memcpy(r.pose, pose_inout, 64);
        if (rc != ICP_OK && first_err == ICP_OK) first_err = rc;
        if (gt_frames && (rc = track_rmse_at(c, 1, pose_inout, d_rmse + 1))) return rc;      // final RMSE (:311)
    }
    HIPCK(c, hipStreamSynchronize(c->stream));
    if (gt_frames && n_frames > 1 && (rc = track_rmse_finish(c, n_frames, out, [](const icp_track_frame& r) { return r.n_src > 0; }))) return rc;
    guard.ok = true;
    return first_err;
}

// SimpleMesh(sensor, cameraPose, edgeThreshold) (SimpleMesh.h:36-119, dev_mesh.hpp).  The two matrices are composed on the host in fp64 and
// rounded once: M = P^-1 E^-1 (both affine) for the vertices, C = Kc Ec P for the colour re-projection.  Scratch: upload slot 0 of the
// depth frames, `staging` = [xyz 12n | rgba 4n | triangles 24 (w - 1)(h - 1)], the depth compaction's block counts and d_count.
int icp_depth_mesh(icp_ctx* c, const float* depth, const uint8_t* rgbx, const icp_depth_camera* cam, const icp_color_camera* color_cam,
                   const float camera_pose[16], float edge_threshold, float* vertices_out, uint8_t* colors_out, uint32_t* triangles_out,
                   int32_t* n_triangles_out) {
    if (!c) return ICP_ERR_INVALID_ARG;
    if (n_triangles_out) *n_triangles_out = 0;
    if (!depth || !camera_pose || !vertices_out || !triangles_out || !n_triangles_out || (colors_out && !rgbx) || !depth_camera_ok(cam) ||
        2 * (long long)(cam->width - 1) * (cam->height - 1) > 0x7FFFFFFFll ||
        (color_cam && (color_cam->width <= 0 || color_cam->height <= 0 || (long long)color_cam->width * color_cam->height > 0x7FFFFFFFll ||
                       !std::isfinite(color_cam->fx) || !std::isfinite(color_cam->fy) || !std::isfinite(color_cam->cx) || !std::isfinite(color_cam->cy)))) {
        c->err = "icp_depth_mesh: bad argument (null pointer, colours without a colour frame, or a bad camera)"; return ICP_ERR_INVALID_ARG;
    }
    int rc;
    DrainOnError guard(c);
    if ((rc = set_device(c))) return rc;
    const int w = cam->width, h = cam->height, n = w * h;
    const int nq = (w - 1) * (h - 1), nb = (nq + 255) / 256;
    MeshFrame f;
    f.width = w; f.height = h; f.fx = cam->fx; f.fy = cam->fy; f.cx = cam->cx; f.cy = cam->cy;
    f.color_width = color_cam ? color_cam->width : w; f.color_height = color_cam ? color_cam->height : h;
    {
        double Pi[9], pt[3], Ei[9], et[3];
        invert_affine(camera_pose, Pi, pt);
        invert_affine(cam->extrinsics, Ei, et);
        for (int r = 0; r < 3; r++) {
            for (int k = 0; k < 3; k++) f.m[r * 3 + k] = (float)((Pi[r * 3] * Ei[k] + Pi[r * 3 + 1] * Ei[3 + k]) + Pi[r * 3 + 2] * Ei[6 + k]);
            f.m[9 + r] = (float)(((Pi[r * 3] * et[0] + Pi[r * 3 + 1] * et[1]) + Pi[r * 3 + 2] * et[2]) + pt[r]);
        }
        static const float identity[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
        const float* Ec = color_cam ? color_cam->extrinsics : identity;
        const double K[9] = {color_cam ? color_cam->fx : cam->fx, 0, color_cam ? color_cam->cx : cam->cx,
                             0, color_cam ? color_cam->fy : cam->fy, color_cam ? color_cam->cy : cam->cy, 0, 0, 1};
        double A[12];                                    // rows 0..2 of Ec P (column-major 4x4 operands)
        for (int r = 0; r < 3; r++)
            for (int k = 0; k < 4; k++)
                A[r * 4 + k] = (((double)Ec[r] * camera_pose[k * 4] + (double)Ec[4 + r] * camera_pose[k * 4 + 1]) + (double)Ec[8 + r] * camera_pose[k * 4 + 2]) +
                               (double)Ec[12 + r] * camera_pose[k * 4 + 3];
        for (int r = 0; r < 3; r++)
            for (int k = 0; k < 4; k++) f.c[r * 4 + k] = (float)((K[r * 3] * A[k] + K[r * 3 + 1] * A[4 + k]) + K[r * 3 + 2] * A[8 + k]);
    }
    const bool with_colors = colors_out != nullptr;
    if ((rc = stage_depth(c, 0, depth, with_colors ? rgbx : nullptr, n, c->stream, f.color_width * f.color_height))) return rc;
    HIPCK(c, hipStreamWaitEvent(c->stream, c->depth_up[0], 0));
    f.depth = c->depth_dev[0].as<float>(); f.rgbx = with_colors ? c->depth_dev[0].as<uint8_t>() + (size_t)n * 4 : nullptr;
    if ((rc = ensure(c, c->staging, (size_t)n * 16 + (size_t)nq * 24))) return rc;
    float* d_xyz = c->staging.as<float>(); uint32_t* d_rgba = (uint32_t*)(d_xyz + (size_t)n * 3); uint32_t* d_tris = d_rgba + n;
    int* hn;
    if ((rc = count_slot(c, &hn))) return rc;
    *hn = 0;
    hipLaunchKernelGGL(k_mesh_vertices, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, f, d_xyz, with_colors ? d_rgba : nullptr);
    if (nq > 0) {
        if ((rc = ensure(c, c->depth_blocks, (size_t)nb * 4))) return rc;
        if ((rc = ensure(c, c->d_count, 16))) return rc;
        hipLaunchKernelGGL(k_mesh_count, dim3(nb), dim3(256), 0, c->stream, (const float*)d_xyz, w, nq, edge_threshold, c->depth_blocks.as<int>());
        hipLaunchKernelGGL(k_select_scan, dim3(1), dim3(1024), 0, c->stream, c->depth_blocks.as<int>(), nb, c->d_count.as<int>());
        hipLaunchKernelGGL(k_mesh_scatter, dim3(nb), dim3(256), 0, c->stream, (const float*)d_xyz, w, nq, edge_threshold, (const int*)c->depth_blocks.as<int>(), d_tris);
        HIPCK(c, hipMemcpyAsync(hn, c->d_count.p, 4, hipMemcpyDeviceToHost, c->stream));
    }
    HIPCK(c, hipGetLastError());
    HIPCK(c, hipMemcpyAsync(vertices_out, d_xyz, (size_t)n * 12, hipMemcpyDeviceToHost, c->stream));
    if (with_colors) HIPCK(c, hipMemcpyAsync(colors_out, d_rgba, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCK(c, hipStreamSynchronize(c->stream));
    const int nt = *hn;
    if (nt < 0 || nt > 2 * nq) { c->err = "icp_depth_mesh: triangle count out of range"; return ICP_ERR_HIP; }
    if (nt > 0) {
        HIPCK(c, hipMemcpyAsync(triangles_out, d_tris, (size_t)nt * 12, hipMemcpyDeviceToHost, c->stream));
        HIPCK(c, hipStreamSynchronize(c->stream));
    }
    *n_triangles_out = nt;
    return guard.done();
}
