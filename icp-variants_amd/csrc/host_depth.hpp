// host_depth.hpp -- depth frames as clouds: back-projection, icp_set_target_depth / icp_set_source_depth, the frame-to-reference tracker
// (icp_track_depth_frames), the per-frame mesh (icp_depth_mesh) and the bilateral depth filter in front of the calls that align a frame
// (icp_set_depth_filter_options, icp_filter_depth).  Part of icp_hip.hip (included from there, after host_multi.hpp).
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

// ---- the bilateral depth filter (dev_depth_filter.hpp; contract: include/icp_hip.h) ----
const char* depth_filter_options_error(const icp_depth_filter_options* o) {
    if (!o) return "null options";
    if (o->radius < 0 || o->radius > ICP_DEPTH_FILTER_MAX_RADIUS) return "radius must be in 0 .. 4";
    if (!(std::isfinite(o->sigma_space) && o->sigma_space > 0.f)) return "sigma_space must be finite and > 0";
    if (!(std::isfinite(o->sigma_range) && o->sigma_range > 0.f)) return "sigma_range must be finite and > 0";
    if (!std::isfinite((float)(256.0 / (9.0 * (double)o->sigma_range * (double)o->sigma_range)))) return "sigma_range is too small (256 / (9 sigma_range^2) is not finite in fp32)";
    return nullptr;
}
// The tables of checked options, each entry computed in fp64 and rounded once.
void depth_filter_tables(const icp_depth_filter_options& o, float* spatial, float* range, float* inv_bin) {
    const int r = o.radius, w = 2 * r + 1;
    const double two_ss = 2.0 * (double)o.sigma_space * (double)o.sigma_space;
    if (spatial && r > 0) for (int dy = -r; dy <= r; dy++) for (int dx = -r; dx <= r; dx++) spatial[(dy + r) * w + (dx + r)] = (float)exp(-(double)(dx * dx + dy * dy) / two_ss);
    if (range) for (int q = 0; q < ICP_DEPTH_FILTER_RANGE_BINS; q++) range[q] = (float)exp(-4.5 * ((double)q + 0.5) / 256.0);
    if (inv_bin) *inv_bin = (float)(256.0 / (9.0 * (double)o.sigma_range * (double)o.sigma_range));
}
// The device tables [spatial 81 | range 256] of `o`, uploaded on s and waited for (once per change of options, or per icp_filter_depth with
// options of its own, which leaves the context's tables stale).
int depth_filter_upload_tables(icp_ctx* c, const icp_depth_filter_options& o, hipStream_t s) {
    constexpr int NS = (2 * ICP_DEPTH_FILTER_MAX_RADIUS + 1) * (2 * ICP_DEPTH_FILTER_MAX_RADIUS + 1);
    float h[NS + ICP_DEPTH_FILTER_RANGE_BINS] = {0};
    depth_filter_tables(o, h, h + NS, &c->df_inv_bin);
    int rc;
    if ((rc = ensure(c, c->df_tables, sizeof(h)))) return rc;
    HIPCK(c, hipMemcpyAsync(c->df_tables.p, h, sizeof(h), hipMemcpyHostToDevice, s));
    HIPCK(c, hipStreamSynchronize(s));
    return ICP_OK;
}
// One launch of k_depth_filter<radius> on s: width x height floats at `in` -> `out`, with the device tables as they stand.
int depth_filter_launch(icp_ctx* c, int radius, const float* in, float* out, int width, int height, hipStream_t s) {
    constexpr int NS = (2 * ICP_DEPTH_FILTER_MAX_RADIUS + 1) * (2 * ICP_DEPTH_FILTER_MAX_RADIUS + 1);
    DepthFilterArgs a;
    a.in = in; a.out = out; a.spatial = c->df_tables.as<float>(); a.range = a.spatial + NS; a.width = width; a.height = height; a.inv_bin = c->df_inv_bin;
    const dim3 grid((width + DF_TW - 1) / DF_TW, (height + DF_TH - 1) / DF_TH), block(DF_TW, DF_TH);
    switch (radius) {
        case 1: hipLaunchKernelGGL(k_depth_filter<1>, grid, block, 0, s, a); break;
        case 2: hipLaunchKernelGGL(k_depth_filter<2>, grid, block, 0, s, a); break;
        case 3: hipLaunchKernelGGL(k_depth_filter<3>, grid, block, 0, s, a); break;
        case 4: hipLaunchKernelGGL(k_depth_filter<4>, grid, block, 0, s, a); break;
        default: c->err = "depth filter: no kernel for this radius"; return ICP_ERR_INVALID_ARG;
    }
    HIPCK(c, hipGetLastError());
    return ICP_OK;
}
// The depth frame of upload slot `slot` as the consumers that ALIGN a frame read it: the filtered copy where stage_depth made one, else the
// raw frame.  The consumers that fuse or export a frame, and every reader of the colour frame behind it, read depth_dev[slot] itself.
const float* aligned_depth(const icp_ctx* c, int slot) { return c->depth_filtered[slot] ? c->depth_filt[slot].as<float>() : c->depth_dev[slot].as<float>(); }

// One depth frame [depth 4n | rgbx 4n] into upload slot `slot`: host -> page-locked block -> device, on stream s (the context's own stream,
// or depth_stream when the frame goes up while the previous one iterates); depth_up[slot] marks its arrival.  The only host-side wait is for
// the slot's previous copy to have left the page-locked block.
// The colour frame has n pixels unless n_color says otherwise (icp_depth_mesh's colour camera).
// width > 0 (the callers whose frame is aligned): with the context's depth filter on, the frame is filtered on s right behind the copy, into
// depth_filt[slot], before depth_up[slot] is recorded -- every consumer waits for that event, and the slot's reuse is ordered for the
// filtered copy as it is for the raw one (its readers are the raw frame's readers).
int stage_depth(icp_ctx* c, int slot, const float* depth, const uint8_t* rgbx, int n, hipStream_t s, int n_color = -1, int width = 0) {
    if (n_color < 0) n_color = n;
    const bool filter = width > 0 && c->df_opt.radius > 0;
    c->depth_filtered[slot] = false;
    if (!c->depth_up[slot]) HIPCK(c, hipEventCreateWithFlags(&c->depth_up[slot].e, hipEventDisableTiming));
    if (c->depth_pending[slot]) { HIPCK(c, hipEventSynchronize(c->depth_up[slot])); c->depth_pending[slot] = false; }
    const size_t bytes = (size_t)n * 4 + (rgbx ? (size_t)n_color * 4 : 0), cap = (size_t)n * 4 + (size_t)(n_color > n ? n_color : n) * 4;
    int rc;
    PinBuf& pin = c->depth_pin[slot];
    if ((rc = ensure_pin(c, pin, bytes, cap, 0))) return rc;      // (a block that has to grow becomes exactly cap >= bytes)
    if ((rc = ensure(c, c->depth_dev[slot], cap))) return rc;
    memcpy(pin.p, depth, (size_t)n * 4);
    if (rgbx) memcpy(pin.as<char>() + (size_t)n * 4, rgbx, (size_t)n_color * 4);
    if (filter) {
        if ((rc = ensure(c, c->depth_filt[slot], (size_t)n * 4))) return rc;
        if (!c->df_tables_ok) { if ((rc = depth_filter_upload_tables(c, c->df_opt, s))) return rc; c->df_tables_ok = true; }
    }
    HIPCK(c, hipMemcpyAsync(c->depth_dev[slot].p, pin.p, bytes, hipMemcpyHostToDevice, s));
    if (filter) {
        if ((rc = depth_filter_launch(c, c->df_opt.radius, c->depth_dev[slot].as<float>(), c->depth_filt[slot].as<float>(), width, n / width, s))) return rc;
        c->depth_filtered[slot] = true;
    }
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
    fr.depth = aligned_depth(c, slot); fr.rgbx = with_colors ? c->depth_dev[slot].as<uint8_t>() + (size_t)n * 4 : nullptr;
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
    if ((rc = stage_depth(c, 0, depth, rgbx, cam->width * cam->height, c->stream, -1, cam->width))) return rc;
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
    if ((rc = stage_depth(c, 0, depth_frames, frame_rgbx(0), n, c->stream, -1, cam->width))) return rc;
    if ((rc = depth_to_cloud(c, 0, *cam, *target_opt, rgbx_frames != nullptr, c->tgt, true, &kept))) return rc;
    if (n_frames > 1 && (rc = stage_depth(c, 1, depth_frames + (size_t)n, frame_rgbx(1), n, c->depth_stream, -1, cam->width))) return rc;
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
        if (k + 1 < n_frames && (rc = stage_depth(c, slot ^ 1, depth_frames + (size_t)(k + 1) * n, frame_rgbx(k + 1), n, c->depth_stream, -1, cam->width))) return rc;
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

int icp_depth_filter_options_default(icp_depth_filter_options* o) {
    if (!o) return ICP_ERR_INVALID_ARG;
    o->radius = 0; o->sigma_space = 4.5f; o->sigma_range = 0.03f;
    return ICP_OK;
}
int icp_depth_filter_options_check(const icp_depth_filter_options* o) { return depth_filter_options_error(o) ? ICP_ERR_INVALID_ARG : ICP_OK; }
int icp_set_depth_filter_options(icp_ctx* c, const icp_depth_filter_options* o) {
    if (!c) return ICP_ERR_INVALID_ARG;
    icp_depth_filter_options v;
    if (o) v = *o; else icp_depth_filter_options_default(&v);
    if (const char* why = depth_filter_options_error(&v)) { c->err = std::string("icp_set_depth_filter_options: ") + why; return ICP_ERR_INVALID_ARG; }
    c->df_opt = v; c->df_tables_ok = false;      // (the device tables follow at the next frame that is filtered)
    return ICP_OK;
}
int icp_get_depth_filter_options(const icp_ctx* c, icp_depth_filter_options* o) { if (!c || !o) return ICP_ERR_INVALID_ARG; *o = c->df_opt; return ICP_OK; }
int icp_depth_filter_tables(const icp_depth_filter_options* o, float* spatial_out, float* range_out, float* inv_bin_out) {
    if (depth_filter_options_error(o)) return ICP_ERR_INVALID_ARG;
    depth_filter_tables(*o, spatial_out, range_out, inv_bin_out);
    return ICP_OK;
}

// Scratch: `staging` = [in 4n | out 4n]; the device tables are left stale for the context's own options when `opt` is given.
int icp_filter_depth(icp_ctx* c, const float* depth, int32_t width, int32_t height, const icp_depth_filter_options* opt, float* depth_out) {
    if (!c) return ICP_ERR_INVALID_ARG;
    if (!depth || !depth_out || width <= 0 || height <= 0 || (long long)width * height > 0x7FFFFFFFll) { c->err = "icp_filter_depth: bad argument (null frame, width, height > 0)"; return ICP_ERR_INVALID_ARG; }
    const icp_depth_filter_options o = opt ? *opt : c->df_opt;
    if (const char* why = depth_filter_options_error(&o)) { c->err = std::string("icp_filter_depth: ") + why; return ICP_ERR_INVALID_ARG; }
    const size_t n = (size_t)width * height;
    if (o.radius == 0) { if (depth_out != depth) memmove(depth_out, depth, n * 4); return ICP_OK; }
    int rc;
    DrainOnError guard(c);
    if ((rc = set_device(c))) return rc;
    if ((rc = ensure(c, c->staging, n * 8))) return rc;
    if (opt || !c->df_tables_ok) { if ((rc = depth_filter_upload_tables(c, o, c->stream))) return rc; c->df_tables_ok = !opt; }
    float* d_in = c->staging.as<float>(); float* d_out = d_in + n;
    HIPCK(c, hipMemcpyAsync(d_in, depth, n * 4, hipMemcpyHostToDevice, c->stream));
    if ((rc = depth_filter_launch(c, o.radius, d_in, d_out, width, height, c->stream))) return rc;
    HIPCK(c, hipMemcpyAsync(depth_out, d_out, n * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCK(c, hipStreamSynchronize(c->stream));
    return guard.done();
}

// Not part of icp_hip.h (tools/time_depth_filter.py): the device time of `reps` launches of the filter with the context's options (radius
// > 0) on a frame already on the device, between two events (which = 0), or of as many device-to-device copies of the frame (which = 1).
extern "C" int icp_debug_depth_filter_time(icp_ctx* c, int32_t which, const float* depth, int32_t width, int32_t height, int32_t reps, float* ms_out) {
    if (!c || !ms_out || !depth || which < 0 || which > 1 || width <= 0 || height <= 0 || reps < 1 || (which == 0 && c->df_opt.radius < 1)) return ICP_ERR_INVALID_ARG;
    int rc;
    DrainOnError guard(c);
    if ((rc = set_device(c))) return rc;
    if ((rc = ensure_events(c, 2))) return rc;
    const size_t n = (size_t)width * height;
    if ((rc = ensure(c, c->staging, n * 8))) return rc;
    if (!c->df_tables_ok && which == 0) { if ((rc = depth_filter_upload_tables(c, c->df_opt, c->stream))) return rc; c->df_tables_ok = true; }
    float* d_in = c->staging.as<float>(); float* d_out = d_in + n;
    HIPCK(c, hipMemcpyAsync(d_in, depth, n * 4, hipMemcpyHostToDevice, c->stream));
    for (int pass = 0; pass < 2; pass++) {               // (pass 0 warm: the first launch loads the code object)
        HIPCK(c, hipEventRecord(c->events[0], c->stream));
        for (int k = 0; k < (pass ? reps : 1); k++) {
            if (which == 0) { if ((rc = depth_filter_launch(c, c->df_opt.radius, d_in, d_out, width, height, c->stream))) return rc; }
            else HIPCK(c, hipMemcpyAsync(d_out, d_in, n * 4, hipMemcpyDeviceToDevice, c->stream));
        }
        HIPCK(c, hipEventRecord(c->events[1], c->stream));
        HIPCK(c, hipStreamSynchronize(c->stream));
    }
    HIPCK(c, hipEventElapsedTime(ms_out, c->events[0], c->events[1]));
    return guard.done();
}

// Not part of icp_hip.h (tests/test_gpu_depth_filter.py): the resident target (which = 0) or source (1) back on the host as it stands -- the
// first min(max_points, n) entries of the six planes x y z nx ny nz at planes_out + k * max_points and of the packed colours at rgba_out
// (either may be NULL); *n_out = n, *flags_out = has_normals | has_colors << 1.
extern "C" int icp_debug_get_cloud(icp_ctx* c, int32_t which, float* planes_out, uint32_t* rgba_out, int32_t max_points, int32_t* n_out, int32_t* flags_out) {
    if (!c || which < 0 || which > 1 || max_points < 0 || !n_out) return ICP_ERR_INVALID_ARG;
    const Cloud& cl = which ? c->src : c->tgt;
    *n_out = cl.n;
    if (flags_out) *flags_out = (cl.has_normals ? 1 : 0) | (cl.has_colors ? 2 : 0);
    const size_t m = (size_t)(cl.n < max_points ? cl.n : max_points);
    if (m == 0) return ICP_OK;
    DrainOnError guard(c);
    int rc;
    if ((rc = set_device(c))) return rc;
    HIPCK(c, hipStreamSynchronize(c->stream));
    const DevBuf* pl[6] = {&cl.x, &cl.y, &cl.z, &cl.nx, &cl.ny, &cl.nz};
    if (planes_out) for (int k = 0; k < (cl.has_normals ? 6 : 3); k++) HIPCK(c, hipMemcpy(planes_out + (size_t)k * max_points, pl[k]->p, m * 4, hipMemcpyDeviceToHost));
    if (rgba_out && cl.has_colors) HIPCK(c, hipMemcpy(rgba_out, cl.rgba.p, m * 4, hipMemcpyDeviceToHost));
    return guard.done();
}
