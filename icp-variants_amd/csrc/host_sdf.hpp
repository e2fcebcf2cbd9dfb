// host_sdf.hpp -- direct SDF tracking: the volume's field sampled at points (icp_tsdf_sample), the sums of one step (icp_tsdf_sdf_system),
// one frame aligned to the volume (icp_tsdf_align_depth) and the tracking loop over it (icp_track_depth_sdf).  Kernels: dev_sdf.hpp;
// contract: include/icp_hip.h, DESIGN.md section 6q.  Part of icp_hip.hip (included from there, after host_tsdf.hpp).
namespace {
const char* sdf_options_error(const icp_sdf_options* o) {
    if (!o) return "null options";
    if (o->stride < 1) return "stride must be >= 1";
    if (o->n_iterations < 1 || o->n_iterations > 1000) return "n_iterations must be in 1 .. 1000";
    if (o->min_valid < 6) return "min_valid must be >= 6";
    if (!(std::isfinite(o->huber) && o->huber >= 0.f)) return "huber must be finite and >= 0";
    if (!(std::isfinite(o->stop_rotation) && o->stop_rotation >= 0.f && std::isfinite(o->stop_translation) && o->stop_translation >= 0.f))
        return "stop_rotation and stop_translation must be finite and >= 0";
    return nullptr;
}
int sdf_check_call(icp_ctx* c, const float* depth, const icp_depth_camera* cam, const float* pose, const icp_sdf_options* opt, const char* who) {
    int rc;
    if ((rc = tsdf_check_call(c, cam, pose, who, true))) return rc;      // (either storage: sdf_enqueue and sdf_integrate_slot choose the kernels)
    if (!depth) { c->err = std::string(who) + ": null depth frame"; return ICP_ERR_INVALID_ARG; }
    if (const char* why = sdf_options_error(opt)) { c->err = std::string(who) + ": " + why; return ICP_ERR_INVALID_ARG; }
    return ICP_OK;
}

// What the launches of one frame share: the grid of 16 x 16 tiles of sampled pixels and the device blocks behind it.
struct SdfPlan { dim3 grid; int n_blocks; SdfFrame f; };
int sdf_plan(icp_ctx* c, const icp_depth_camera& cam, const icp_sdf_options& opt, SdfPlan* pl) {
    SdfFrame& f = pl->f;
    f.depth = nullptr; f.width = cam.width; f.height = cam.height; f.stride = opt.stride;
    f.ws = (cam.width + opt.stride - 1) / opt.stride; f.hs = (cam.height + opt.stride - 1) / opt.stride;
    f.fx = cam.fx; f.fy = cam.fy; f.cx = cam.cx; f.cy = cam.cy; f.huber = opt.huber;
    pl->grid = dim3((f.ws + 15) / 16, (f.hs + 15) / 16);
    pl->n_blocks = (int)(pl->grid.x * pl->grid.y);
    int rc;
    if ((rc = ensure(c, c->sdf_state, sizeof(SdfState)))) return rc;
    if ((rc = ensure(c, c->sdf_partials, (size_t)pl->n_blocks * (SDF_NSUM * 8 + 2 * 4)))) return rc;
    if ((rc = ensure(c, c->sdf_rec, sizeof(icp_sdf_frame) + (size_t)opt.n_iterations * sizeof(icp_sdf_iter)))) return rc;
    return ICP_OK;
}
// The frame in upload slot `slot` against the volume from `pose`, enqueued on the context's stream: the state, then `iterations` pairs of
// k_sdf_accumulate and k_sdf_solve (step = false: one pair that only folds).  Nothing here waits; the launches behind the frame's end drain.
int sdf_enqueue(icp_ctx* c, int slot, const SdfPlan& pl, const icp_sdf_options& opt, const float pose[16], bool step, bool trace) {
    SdfFrame f = pl.f;
    f.depth = aligned_depth(c, slot);
    SdfState* st = c->sdf_state.as<SdfState>();
    icp_sdf_frame* rec = c->sdf_rec.as<icp_sdf_frame>();
    icp_sdf_iter* tr = (icp_sdf_iter*)(rec + 1);
    double* partials = c->sdf_partials.as<double>();
    int* counts = (int*)(partials + (size_t)SDF_NSUM * pl.n_blocks);
    const bool hashed = c->tsdf_hashed;
    const TsdfVol v = tsdf_view(c);
    const HtVol hv = hashed ? htsdf_view(c) : HtVol();
    TsdfMat m; memcpy(m.m, pose, 64);
    HIPCK(c, hipStreamWaitEvent(c->stream, c->depth_up[slot], 0));
    if (trace) HIPCK(c, hipMemsetAsync(tr, 0, (size_t)opt.n_iterations * sizeof(icp_sdf_iter), c->stream));
    hipLaunchKernelGGL(k_sdf_init, dim3(1), dim3(64), 0, c->stream, st, m, rec);
    SdfSolve sp;
    sp.partials = partials; sp.counts = counts; sp.n_blocks = pl.n_blocks; sp.st = st; sp.rec = rec; sp.trace = trace ? tr : nullptr;
    sp.n_iterations = opt.n_iterations; sp.min_valid = opt.min_valid; sp.step = step ? 1 : 0;
    sp.stop_rotation = opt.stop_rotation; sp.stop_translation = opt.stop_translation;
    const int iterations = step ? opt.n_iterations : 1;
    for (int it = 0; it < iterations; it++) {
        if (hashed) hipLaunchKernelGGL(k_hsdf_accumulate, pl.grid, dim3(256), 0, c->stream, hv, f, (const SdfState*)st, partials, counts);
        else hipLaunchKernelGGL(k_sdf_accumulate, pl.grid, dim3(256), 0, c->stream, v, f, (const SdfState*)st, partials, counts);
        sp.iter = it;
        hipLaunchKernelGGL(k_sdf_solve, dim3(1), dim3(256), 0, c->stream, sp);
    }
    HIPCK(c, hipGetLastError());
    return ICP_OK;
}
// tsdf_integrate_slot on whichever storage the volume has (hashed: the touch's counters are read, one more host wait)
int sdf_integrate_slot(icp_ctx* c, int slot, const icp_depth_camera& cam, const float pose[16], bool color, const char* who) {
    return c->tsdf_hashed ? htsdf_integrate_slot(c, slot, cam, pose, nullptr, who, color) : tsdf_integrate_slot(c, slot, cam, pose, nullptr, color);
}
// The frame's record (and its trace) back through the page-locked block, waited for: the one host read of a frame.
int sdf_read_record(icp_ctx* c, const icp_sdf_options& opt, icp_sdf_frame* rec_out, icp_sdf_iter* trace_out) {
    int rc;
    const size_t bytes = sizeof(icp_sdf_frame) + (trace_out ? (size_t)opt.n_iterations * sizeof(icp_sdf_iter) : 0);
    if ((rc = ensure_pinned(c, 2048 + bytes))) return rc;
    char* h = c->pinned.as<char>() + 2048;
    HIPCK(c, hipMemcpyAsync(h, c->sdf_rec.p, bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCK(c, hipStreamSynchronize(c->stream));
    memcpy(rec_out, h, sizeof(icp_sdf_frame));
    if (trace_out) memcpy(trace_out, h + sizeof(icp_sdf_frame), (size_t)opt.n_iterations * sizeof(icp_sdf_iter));
    return ICP_OK;
}
std::string sdf_failure(const char* who, const icp_sdf_frame& r, const icp_sdf_options& opt) {
    char buf[192];
    if (r.status == ICP_ERR_NO_SOURCE) snprintf(buf, sizeof(buf), "%s: the frame has no usable pixel", who);
    else snprintf(buf, sizeof(buf), "%s: step %d failed (%d valid pixels of %d usable, min_valid %d, or a non-finite solution)", who, r.iterations, r.n_valid_last, r.n_depth, opt.min_valid);
    return buf;
}
}  // namespace

int icp_sdf_options_default(icp_sdf_options* o) {
    if (!o) return ICP_ERR_INVALID_ARG;
    o->stride = 1; o->n_iterations = 20; o->min_valid = 64; o->huber = 0.f; o->stop_rotation = 1e-5f; o->stop_translation = 1e-5f;
    return ICP_OK;
}
int icp_sdf_options_check(const icp_sdf_options* o) { return sdf_options_error(o) ? ICP_ERR_INVALID_ARG : ICP_OK; }

int icp_tsdf_sample(icp_ctx* c, const float* points, int32_t n, float* f_out, float* grad_out, uint8_t* valid_out) {
    if (!c) return ICP_ERR_INVALID_ARG;
    if (!c->tsdf_on) { c->err = "icp_tsdf_sample: no volume (icp_tsdf_create)"; return ICP_ERR_INVALID_ARG; }
    if (n < 0 || (n > 0 && !points)) { c->err = "icp_tsdf_sample: bad argument (n >= 0, points)"; return ICP_ERR_INVALID_ARG; }
    if (n == 0) return ICP_OK;
    int rc;
    DrainOnError guard(c);
    if ((rc = set_device(c))) return rc;
    if ((rc = ensure(c, c->staging, (size_t)n * 29))) return rc;      // [points 12n | F 4n | G 12n | valid n]
    float* d_pts = c->staging.as<float>(); float* d_f = d_pts + (size_t)n * 3; float* d_g = d_f + n; uint8_t* d_ok = (uint8_t*)(d_g + (size_t)n * 3);
    HIPCK(c, hipMemcpyAsync(d_pts, points, (size_t)n * 12, hipMemcpyHostToDevice, c->stream));
    if (c->tsdf_hashed) hipLaunchKernelGGL(k_htsdf_sample, dim3((n + 255) / 256), dim3(256), 0, c->stream, htsdf_view(c), (const float*)d_pts, (int)n, d_f, d_g, d_ok);
    else hipLaunchKernelGGL(k_tsdf_sample, dim3((n + 255) / 256), dim3(256), 0, c->stream, tsdf_view(c), (const float*)d_pts, (int)n, d_f, d_g, d_ok);
    HIPCK(c, hipGetLastError());
    if (f_out) HIPCK(c, hipMemcpyAsync(f_out, d_f, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
    if (grad_out) HIPCK(c, hipMemcpyAsync(grad_out, d_g, (size_t)n * 12, hipMemcpyDeviceToHost, c->stream));
    if (valid_out) HIPCK(c, hipMemcpyAsync(valid_out, d_ok, (size_t)n, hipMemcpyDeviceToHost, c->stream));
    HIPCK(c, hipStreamSynchronize(c->stream));
    return guard.done();
}

int icp_tsdf_sdf_system(icp_ctx* c, const float* depth, const icp_depth_camera* cam, const float pose[16], const icp_sdf_options* opt, double* sums_out,
                        int32_t* counts_out) {
    if (!c) return ICP_ERR_INVALID_ARG;
    int rc;
    if ((rc = sdf_check_call(c, depth, cam, pose, opt, "icp_tsdf_sdf_system"))) return rc;
    if (!sums_out || !counts_out) { c->err = "icp_tsdf_sdf_system: null output"; return ICP_ERR_INVALID_ARG; }
    DrainOnError guard(c);
    if ((rc = set_device(c))) return rc;
    SdfPlan pl;
    if ((rc = sdf_plan(c, *cam, *opt, &pl))) return rc;
    if ((rc = stage_depth(c, 0, depth, nullptr, cam->width * cam->height, c->stream, -1, cam->width))) return rc;
    if ((rc = sdf_enqueue(c, 0, pl, *opt, pose, false, false))) return rc;
    if ((rc = ensure_pinned(c, 2048 + sizeof(SdfState)))) return rc;
    SdfState* h = (SdfState*)(c->pinned.as<char>() + 2048);
    HIPCK(c, hipMemcpyAsync(h, c->sdf_state.p, sizeof(SdfState), hipMemcpyDeviceToHost, c->stream));
    HIPCK(c, hipStreamSynchronize(c->stream));
    memcpy(sums_out, h->sums, sizeof(h->sums));
    counts_out[0] = h->counts[0]; counts_out[1] = h->counts[1];
    return guard.done();
}

int icp_tsdf_align_depth(icp_ctx* c, const float* depth, const icp_depth_camera* cam, const icp_sdf_options* opt, float pose_inout[16], icp_sdf_frame* rec_out,
                         icp_sdf_iter* trace_out) {
    if (!c) return ICP_ERR_INVALID_ARG;
    int rc;
    if ((rc = sdf_check_call(c, depth, cam, pose_inout, opt, "icp_tsdf_align_depth"))) return rc;
    DrainOnError guard(c);
    if ((rc = set_device(c))) return rc;
    SdfPlan pl;
    if ((rc = sdf_plan(c, *cam, *opt, &pl))) return rc;
    if ((rc = stage_depth(c, 0, depth, nullptr, cam->width * cam->height, c->stream, -1, cam->width))) return rc;
    if ((rc = sdf_enqueue(c, 0, pl, *opt, pose_inout, true, trace_out != nullptr))) return rc;
    icp_sdf_frame r;
    if ((rc = sdf_read_record(c, *opt, &r, trace_out))) return rc;
    if (rec_out) *rec_out = r;
    memcpy(pose_inout, r.pose, 64);
    if (r.status != ICP_OK) c->err = sdf_failure("icp_tsdf_align_depth", r, *opt);
    return guard.done(r.status);      // (synchronised by the record read)
}

int icp_track_depth_sdf(icp_ctx* c, const float* depth_frames, const uint8_t* rgbx_frames, int32_t n_frames, const icp_depth_camera* cam, const icp_sdf_options* opt,
                        float pose_inout[16], icp_sdf_frame* out) {
    if (!c) return ICP_ERR_INVALID_ARG;
    const char* who = "icp_track_depth_sdf";
    if (n_frames < 1 || (n_frames > 1 && !out)) { c->err = std::string(who) + ": bad argument"; return ICP_ERR_INVALID_ARG; }
    int rc;
    if ((rc = sdf_check_call(c, depth_frames, cam, pose_inout, opt, who))) return rc;
    const bool color = rgbx_frames != nullptr;
    if (color && !tsdf_hashed_color(c) && (rc = tsdf_check_color(c, who))) return rc;      // (colour frames need colours: the dense array, or the blocks')
    DrainOnError guard(c);
    if ((rc = set_device(c))) return rc;
    const int n = cam->width * cam->height;
    auto frame_rgbx = [&](int k) { return color ? rgbx_frames + (size_t)k * n * 4 : nullptr; };
    SdfPlan pl;
    if ((rc = sdf_plan(c, *cam, *opt, &pl))) return rc;
    if (!c->depth_stream) HIPCK(c, hipStreamCreateWithFlags(&c->depth_stream.s, hipStreamNonBlocking));
    if (!c->sdf_ev) HIPCK(c, hipEventCreateWithFlags(&c->sdf_ev.e, hipEventDisableTiming));
    // frame 0 into the model at the incoming pose; frame 1 goes up meanwhile
    if ((rc = stage_depth(c, 0, depth_frames, frame_rgbx(0), n, c->stream, -1, cam->width))) return rc;
    if ((rc = sdf_integrate_slot(c, 0, *cam, pose_inout, color, who))) return rc;
    HIPCK(c, hipEventRecord(c->sdf_ev, c->stream));
    if (n_frames > 1 && (rc = stage_depth(c, 1, depth_frames + (size_t)n, frame_rgbx(1), n, c->depth_stream, -1, cam->width))) return rc;
    int first_err = ICP_OK;
    for (int k = 1; k < n_frames; k++) {
        const int slot = k & 1;
        if ((rc = sdf_enqueue(c, slot, pl, *opt, pose_inout, true, false))) return rc;
        // frame k + 1 goes up on the second stream while frame k iterates: its slot was last read by the integration of frame k - 1 (or an
        // earlier one), which may still be running -- the copy waits for it on the device, the host does not
        if (k + 1 < n_frames) {
            HIPCK(c, hipStreamWaitEvent(c->depth_stream, c->sdf_ev, 0));
            if ((rc = stage_depth(c, slot ^ 1, depth_frames + (size_t)(k + 1) * n, frame_rgbx(k + 1), n, c->depth_stream, -1, cam->width))) return rc;
        }
        icp_sdf_frame& r = out[k - 1];
        if ((rc = sdf_read_record(c, *opt, &r, nullptr))) return rc;
        memcpy(pose_inout, r.pose, 64);
        if (r.status == ICP_OK) {
            if ((rc = sdf_integrate_slot(c, slot, *cam, pose_inout, color, who))) return rc;      // (inverts the pose on the host: why the record is read)
            HIPCK(c, hipEventRecord(c->sdf_ev, c->stream));
        } else if (first_err == ICP_OK) { first_err = r.status; c->err = sdf_failure(who, r, *opt); }
    }
    HIPCK(c, hipStreamSynchronize(c->stream));
    HIPCK(c, hipStreamSynchronize(c->depth_stream));
    guard.ok = true;
    return first_err;
}

// Not part of icp_hip.h (tools/time_tsdf.py): the device time of ONE k_sdf_accumulate + k_sdf_solve pair at `pose` between two events on
// the context's stream, the frame staged outside the bracket.
extern "C" int icp_debug_sdf_time(icp_ctx* c, const float* depth, const icp_depth_camera* cam, const float pose[16], const icp_sdf_options* opt, float* ms_out) {
    if (!c || !ms_out) return ICP_ERR_INVALID_ARG;
    int rc;
    if ((rc = sdf_check_call(c, depth, cam, pose, opt, "icp_debug_sdf_time"))) return rc;
    DrainOnError guard(c);
    if ((rc = set_device(c))) return rc;
    if ((rc = ensure_events(c, 2))) return rc;
    SdfPlan pl;
    if ((rc = sdf_plan(c, *cam, *opt, &pl))) return rc;
    if ((rc = stage_depth(c, 0, depth, nullptr, cam->width * cam->height, c->stream, -1, cam->width))) return rc;
    icp_sdf_options one = *opt; one.n_iterations = 1;
    if ((rc = sdf_enqueue(c, 0, pl, one, pose, true, false))) return rc;      // (warm: the first launch loads the code object)
    HIPCK(c, hipStreamSynchronize(c->stream));
    HIPCK(c, hipEventRecord(c->events[0], c->stream));
    if ((rc = sdf_enqueue(c, 0, pl, one, pose, true, false))) return rc;
    HIPCK(c, hipEventRecord(c->events[1], c->stream));
    HIPCK(c, hipStreamSynchronize(c->stream));
    HIPCK(c, hipEventElapsedTime(ms_out, c->events[0], c->events[1]));
    return guard.done();
}
