// host_sdf_color.hpp -- direct SDF tracking with the photometric term: the intensity field sampled at points (icp_tsdf_sample_color), the
// sums of one joint step (icp_tsdf_sdf_system_color), one frame aligned (icp_tsdf_align_depth_color) and the tracking loop
// (icp_track_depth_sdf_color), on the dense coloured volume or on a coloured hashed one (k_htsdf_sample_color, k_hsdf_accumulate_color:
// dev_tsdf_hash_color.hpp).  Kernels: dev_sdf_color.hpp; contract: include/icp_hip.h, DESIGN.md section 6r.  Part of icp_hip.hip
// (included from there, after host_sdf.hpp, whose checks, plan and staging it uses; the state, partials and record buffers are the same
// ones, sized for the larger records -- every call writes them before it reads them).
namespace {
const char* sdf_color_options_error(const icp_sdf_color_options* o) {
    if (!o) return "null colour options";
    if (!(std::isfinite(o->weight) && o->weight > 0.f)) return "the colour weight must be finite and > 0";
    if (!(std::isfinite(o->huber) && o->huber >= 0.f)) return "the colour huber must be finite and >= 0";
    return nullptr;
}
int sdf_color_check_call(icp_ctx* c, const float* depth, const uint8_t* rgbx, const icp_depth_camera* cam, const float* pose, const icp_sdf_options* opt,
                         const icp_sdf_color_options* copt, const char* who) {
    int rc;
    const bool hcol = tsdf_hashed_color(c);          // (either coloured storage: sdf_color_enqueue and sdf_color_integrate_slot choose the kernels)
    if ((rc = tsdf_check_call(c, cam, pose, who, hcol))) return rc;
    if (!hcol && (rc = tsdf_check_color(c, who))) return rc;
    if (!depth) { c->err = std::string(who) + ": null depth frame"; return ICP_ERR_INVALID_ARG; }
    if (!rgbx) { c->err = std::string(who) + ": null colour frame (rgbx)"; return ICP_ERR_INVALID_ARG; }
    if (const char* why = sdf_options_error(opt)) { c->err = std::string(who) + ": " + why; return ICP_ERR_INVALID_ARG; }
    if (const char* why = sdf_color_options_error(copt)) { c->err = std::string(who) + ": " + why; return ICP_ERR_INVALID_ARG; }
    return ICP_OK;
}
// sdf_plan, then the three buffers at the colour records' sizes.
int sdf_color_plan(icp_ctx* c, const icp_depth_camera& cam, const icp_sdf_options& opt, SdfPlan* pl) {
    int rc;
    if ((rc = sdf_plan(c, cam, opt, pl))) return rc;
    if ((rc = ensure(c, c->sdf_state, sizeof(SdfColorState)))) return rc;
    if ((rc = ensure(c, c->sdf_partials, (size_t)pl->n_blocks * (SDFC_NSUM * 8 + 3 * 4)))) return rc;
    if ((rc = ensure(c, c->sdf_rec, sizeof(icp_sdf_color_frame) + (size_t)opt.n_iterations * sizeof(icp_sdf_color_iter)))) return rc;
    return ICP_OK;
}
// sdf_enqueue with the coloured kernels: the slot holds the depth frame and, behind it, its colour frame (stage_depth).
int sdf_color_enqueue(icp_ctx* c, int slot, const SdfPlan& pl, const icp_sdf_options& opt, const icp_sdf_color_options& copt, const float pose[16], bool step, bool trace) {
    SdfFrame f = pl.f;
    f.depth = aligned_depth(c, slot);
    SdfColorFrame cf;
    const bool hashed = c->tsdf_hashed;
    cf.col = hashed ? c->th_cpool.as<float4>() : c->tsdf_col.as<float4>(); cf.rgbx = (const uint32_t*)(c->depth_dev[slot].as<float>() + (size_t)f.width * f.height); cf.weight = copt.weight; cf.huber = copt.huber;
    SdfColorState* st = c->sdf_state.as<SdfColorState>();
    icp_sdf_color_frame* rec = c->sdf_rec.as<icp_sdf_color_frame>();
    icp_sdf_color_iter* tr = (icp_sdf_color_iter*)(rec + 1);
    double* partials = c->sdf_partials.as<double>();
    int* counts = (int*)(partials + (size_t)SDFC_NSUM * pl.n_blocks);
    const TsdfVol v = tsdf_view(c);
    const HtVol hv = hashed ? htsdf_view(c) : HtVol();
    TsdfMat m; memcpy(m.m, pose, 64);
    HIPCK(c, hipStreamWaitEvent(c->stream, c->depth_up[slot], 0));
    if (trace) HIPCK(c, hipMemsetAsync(tr, 0, (size_t)opt.n_iterations * sizeof(icp_sdf_color_iter), c->stream));
    hipLaunchKernelGGL(k_sdf_init_color, dim3(1), dim3(64), 0, c->stream, st, m, rec);
    SdfColorSolve sp;
    sp.partials = partials; sp.counts = counts; sp.n_blocks = pl.n_blocks; sp.st = st; sp.rec = rec; sp.trace = trace ? tr : nullptr;
    sp.n_iterations = opt.n_iterations; sp.min_valid = opt.min_valid; sp.step = step ? 1 : 0;
    sp.stop_rotation = opt.stop_rotation; sp.stop_translation = opt.stop_translation;
    const int iterations = step ? opt.n_iterations : 1;
    for (int it = 0; it < iterations; it++) {
        if (hashed) hipLaunchKernelGGL(k_hsdf_accumulate_color, pl.grid, dim3(256), 0, c->stream, hv, f, cf, (const SdfColorState*)st, partials, counts);
        else hipLaunchKernelGGL(k_sdf_accumulate_color, pl.grid, dim3(256), 0, c->stream, v, f, cf, (const SdfColorState*)st, partials, counts);
        sp.iter = it;
        hipLaunchKernelGGL(k_sdf_solve_color, dim3(1), dim3(256), 0, c->stream, sp);
    }
    HIPCK(c, hipGetLastError());
    return ICP_OK;
}
// the coloured integrate on whichever storage the volume has (hashed: the touch's counters are read, one more host wait)
int sdf_color_integrate_slot(icp_ctx* c, int slot, const icp_depth_camera& cam, const float pose[16], const char* who) {
    return c->tsdf_hashed ? htsdf_integrate_slot(c, slot, cam, pose, nullptr, who, true) : tsdf_integrate_slot(c, slot, cam, pose, nullptr, true);
}
int sdf_color_read_record(icp_ctx* c, const icp_sdf_options& opt, icp_sdf_color_frame* rec_out, icp_sdf_color_iter* trace_out) {
    int rc;
    const size_t bytes = sizeof(icp_sdf_color_frame) + (trace_out ? (size_t)opt.n_iterations * sizeof(icp_sdf_color_iter) : 0);
    if ((rc = ensure_pinned(c, 2048 + bytes))) return rc;
    char* h = c->pinned.as<char>() + 2048;
    HIPCK(c, hipMemcpyAsync(h, c->sdf_rec.p, bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCK(c, hipStreamSynchronize(c->stream));
    memcpy(rec_out, h, sizeof(icp_sdf_color_frame));
    if (trace_out) memcpy(trace_out, h + sizeof(icp_sdf_color_frame), (size_t)opt.n_iterations * sizeof(icp_sdf_color_iter));
    return ICP_OK;
}
std::string sdf_color_failure(const char* who, const icp_sdf_color_frame& r, const icp_sdf_options& opt) {
    char buf[192];
    if (r.status == ICP_ERR_NO_SOURCE) snprintf(buf, sizeof(buf), "%s: the frame has no usable pixel", who);
    else snprintf(buf, sizeof(buf), "%s: step %d failed (%d valid pixels of %d usable, min_valid %d, or a non-finite solution)", who, r.iterations, r.n_valid_last, r.n_depth, opt.min_valid);
    return buf;
}
}  // namespace

int icp_sdf_color_options_default(icp_sdf_color_options* o) {
    if (!o) return ICP_ERR_INVALID_ARG;
    o->weight = 0.1f; o->huber = 0.f;
    return ICP_OK;
}
int icp_sdf_color_options_check(const icp_sdf_color_options* o) { return sdf_color_options_error(o) ? ICP_ERR_INVALID_ARG : ICP_OK; }

int icp_tsdf_sample_color(icp_ctx* c, const float* points, int32_t n, float* s_out, float* grad_out, uint8_t* valid_out) {
    if (!c) return ICP_ERR_INVALID_ARG;
    int rc;
    const bool hcol = tsdf_hashed_color(c);
    if (!hcol && (rc = tsdf_check_color(c, "icp_tsdf_sample_color"))) return rc;
    if (n < 0 || (n > 0 && !points)) { c->err = "icp_tsdf_sample_color: bad argument (n >= 0, points)"; return ICP_ERR_INVALID_ARG; }
    if (n == 0) return ICP_OK;
    DrainOnError guard(c);
    if ((rc = set_device(c))) return rc;
    if ((rc = ensure(c, c->staging, (size_t)n * 29))) return rc;      // [points 12n | S 4n | H 12n | valid n]
    float* d_pts = c->staging.as<float>(); float* d_s = d_pts + (size_t)n * 3; float* d_h = d_s + n; uint8_t* d_ok = (uint8_t*)(d_h + (size_t)n * 3);
    HIPCK(c, hipMemcpyAsync(d_pts, points, (size_t)n * 12, hipMemcpyHostToDevice, c->stream));
    if (hcol) hipLaunchKernelGGL(k_htsdf_sample_color, dim3((n + 255) / 256), dim3(256), 0, c->stream, htsdf_view(c), (const float4*)c->th_cpool.as<float4>(), (const float*)d_pts,
                                 (int)n, d_s, d_h, d_ok);
    else hipLaunchKernelGGL(k_tsdf_sample_color, dim3((n + 255) / 256), dim3(256), 0, c->stream, tsdf_view(c), (const float4*)c->tsdf_col.as<float4>(), (const float*)d_pts, (int)n,
                       d_s, d_h, d_ok);
    HIPCK(c, hipGetLastError());
    if (s_out) HIPCK(c, hipMemcpyAsync(s_out, d_s, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
    if (grad_out) HIPCK(c, hipMemcpyAsync(grad_out, d_h, (size_t)n * 12, hipMemcpyDeviceToHost, c->stream));
    if (valid_out) HIPCK(c, hipMemcpyAsync(valid_out, d_ok, (size_t)n, hipMemcpyDeviceToHost, c->stream));
    HIPCK(c, hipStreamSynchronize(c->stream));
    return guard.done();
}

int icp_tsdf_sdf_system_color(icp_ctx* c, const float* depth, const uint8_t* rgbx, const icp_depth_camera* cam, const float pose[16], const icp_sdf_options* opt,
                              const icp_sdf_color_options* copt, double* sums_out, int32_t* counts_out) {
    if (!c) return ICP_ERR_INVALID_ARG;
    int rc;
    if ((rc = sdf_color_check_call(c, depth, rgbx, cam, pose, opt, copt, "icp_tsdf_sdf_system_color"))) return rc;
    if (!sums_out || !counts_out) { c->err = "icp_tsdf_sdf_system_color: null output"; return ICP_ERR_INVALID_ARG; }
    DrainOnError guard(c);
    if ((rc = set_device(c))) return rc;
    SdfPlan pl;
    if ((rc = sdf_color_plan(c, *cam, *opt, &pl))) return rc;
    if ((rc = stage_depth(c, 0, depth, rgbx, cam->width * cam->height, c->stream, -1, cam->width))) return rc;
    if ((rc = sdf_color_enqueue(c, 0, pl, *opt, *copt, pose, false, false))) return rc;
    if ((rc = ensure_pinned(c, 2048 + sizeof(SdfColorState)))) return rc;
    SdfColorState* h = (SdfColorState*)(c->pinned.as<char>() + 2048);
    HIPCK(c, hipMemcpyAsync(h, c->sdf_state.p, sizeof(SdfColorState), hipMemcpyDeviceToHost, c->stream));
    HIPCK(c, hipStreamSynchronize(c->stream));
    memcpy(sums_out, h->sums, sizeof(h->sums));
    counts_out[0] = h->counts[0]; counts_out[1] = h->counts[1]; counts_out[2] = h->counts[2];
    return guard.done();
}

int icp_tsdf_align_depth_color(icp_ctx* c, const float* depth, const uint8_t* rgbx, const icp_depth_camera* cam, const icp_sdf_options* opt,
                               const icp_sdf_color_options* copt, float pose_inout[16], icp_sdf_color_frame* rec_out, icp_sdf_color_iter* trace_out) {
    if (!c) return ICP_ERR_INVALID_ARG;
    int rc;
    if ((rc = sdf_color_check_call(c, depth, rgbx, cam, pose_inout, opt, copt, "icp_tsdf_align_depth_color"))) return rc;
    DrainOnError guard(c);
    if ((rc = set_device(c))) return rc;
    SdfPlan pl;
    if ((rc = sdf_color_plan(c, *cam, *opt, &pl))) return rc;
    if ((rc = stage_depth(c, 0, depth, rgbx, cam->width * cam->height, c->stream, -1, cam->width))) return rc;
    if ((rc = sdf_color_enqueue(c, 0, pl, *opt, *copt, pose_inout, true, trace_out != nullptr))) return rc;
    icp_sdf_color_frame r;
    if ((rc = sdf_color_read_record(c, *opt, &r, trace_out))) return rc;
    if (rec_out) *rec_out = r;
    memcpy(pose_inout, r.pose, 64);
    if (r.status != ICP_OK) c->err = sdf_color_failure("icp_tsdf_align_depth_color", r, *opt);
    return guard.done(r.status);      // (synchronised by the record read)
}

// icp_track_depth_sdf's loop and staging: a slot's upload carries the depth frame and its colour frame in one copy, and the alignment waits
// for that slot's event, so frame k's colours are on the device before frame k iterates.
int icp_track_depth_sdf_color(icp_ctx* c, const float* depth_frames, const uint8_t* rgbx_frames, int32_t n_frames, const icp_depth_camera* cam,
                              const icp_sdf_options* opt, const icp_sdf_color_options* copt, float pose_inout[16], icp_sdf_color_frame* out) {
    if (!c) return ICP_ERR_INVALID_ARG;
    const char* who = "icp_track_depth_sdf_color";
    if (n_frames < 1 || (n_frames > 1 && !out)) { c->err = std::string(who) + ": bad argument"; return ICP_ERR_INVALID_ARG; }
    int rc;
    if ((rc = sdf_color_check_call(c, depth_frames, rgbx_frames, cam, pose_inout, opt, copt, who))) return rc;
    DrainOnError guard(c);
    if ((rc = set_device(c))) return rc;
    const int n = cam->width * cam->height;
    auto frame_rgbx = [&](int k) { return rgbx_frames + (size_t)k * n * 4; };
    SdfPlan pl;
    if ((rc = sdf_color_plan(c, *cam, *opt, &pl))) return rc;
    if (!c->depth_stream) HIPCK(c, hipStreamCreateWithFlags(&c->depth_stream.s, hipStreamNonBlocking));
    if (!c->sdf_ev) HIPCK(c, hipEventCreateWithFlags(&c->sdf_ev.e, hipEventDisableTiming));
    if ((rc = stage_depth(c, 0, depth_frames, frame_rgbx(0), n, c->stream, -1, cam->width))) return rc;
    if ((rc = sdf_color_integrate_slot(c, 0, *cam, pose_inout, who))) return rc;
    HIPCK(c, hipEventRecord(c->sdf_ev, c->stream));
    if (n_frames > 1 && (rc = stage_depth(c, 1, depth_frames + (size_t)n, frame_rgbx(1), n, c->depth_stream, -1, cam->width))) return rc;
    int first_err = ICP_OK;
    for (int k = 1; k < n_frames; k++) {
        const int slot = k & 1;
        if ((rc = sdf_color_enqueue(c, slot, pl, *opt, *copt, pose_inout, true, false))) return rc;
        if (k + 1 < n_frames) {                        // (the other slot was last read by the integration of frame k - 1: the copy waits for it on the device)
            HIPCK(c, hipStreamWaitEvent(c->depth_stream, c->sdf_ev, 0));
            if ((rc = stage_depth(c, slot ^ 1, depth_frames + (size_t)(k + 1) * n, frame_rgbx(k + 1), n, c->depth_stream, -1, cam->width))) return rc;
        }
        icp_sdf_color_frame& r = out[k - 1];
        if ((rc = sdf_color_read_record(c, *opt, &r, nullptr))) return rc;
        memcpy(pose_inout, r.pose, 64);
        if (r.status == ICP_OK) {
            if ((rc = sdf_color_integrate_slot(c, slot, *cam, pose_inout, who))) return rc;
            HIPCK(c, hipEventRecord(c->sdf_ev, c->stream));
        } else if (first_err == ICP_OK) { first_err = r.status; c->err = sdf_color_failure(who, r, *opt); }
    }
    HIPCK(c, hipStreamSynchronize(c->stream));
    HIPCK(c, hipStreamSynchronize(c->depth_stream));
    guard.ok = true;
    return first_err;
}

// Not part of icp_hip.h (tools/time_tsdf.py): icp_debug_sdf_time for ONE k_sdf_accumulate_color + k_sdf_solve_color pair.
extern "C" int icp_debug_sdf_color_time(icp_ctx* c, const float* depth, const uint8_t* rgbx, const icp_depth_camera* cam, const float pose[16], const icp_sdf_options* opt,
                                        const icp_sdf_color_options* copt, float* ms_out) {
    if (!c || !ms_out) return ICP_ERR_INVALID_ARG;
    int rc;
    if ((rc = sdf_color_check_call(c, depth, rgbx, cam, pose, opt, copt, "icp_debug_sdf_color_time"))) return rc;
    DrainOnError guard(c);
    if ((rc = set_device(c))) return rc;
    if ((rc = ensure_events(c, 2))) return rc;
    SdfPlan pl;
    if ((rc = sdf_color_plan(c, *cam, *opt, &pl))) return rc;
    if ((rc = stage_depth(c, 0, depth, rgbx, cam->width * cam->height, c->stream, -1, cam->width))) return rc;
    icp_sdf_options one = *opt; one.n_iterations = 1;
    if ((rc = sdf_color_enqueue(c, 0, pl, one, *copt, pose, true, false))) return rc;      // (warm: the first launch loads the code object)
    HIPCK(c, hipStreamSynchronize(c->stream));
    HIPCK(c, hipEventRecord(c->events[0], c->stream));
    if ((rc = sdf_color_enqueue(c, 0, pl, one, *copt, pose, true, false))) return rc;
    HIPCK(c, hipEventRecord(c->events[1], c->stream));
    HIPCK(c, hipStreamSynchronize(c->stream));
    HIPCK(c, hipEventElapsedTime(ms_out, c->events[0], c->events[1]));
    return guard.done();
}
