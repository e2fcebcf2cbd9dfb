// host_sdf.hpp -- direct SDF tracking: the volume's field sampled at points (icp_tsdf_sample), the sums of one step (icp_tsdf_sdf_system),
// one frame aligned to the volume (icp_tsdf_align_depth) and the tracking loop over it (icp_track_depth_sdf) -- and, as templates over the
// record kind (SdfGeo here, SdfColor in host_sdf_color.hpp), the ONE host driver behind those calls and their coloured forms: buffers, plan,
// enqueue, record and state read-back, failure message, system, alignment, tracking loop, timed pair.  host_vgicp.hpp enqueues and reads
// back through the same driver with its own accumulate launch.  Kernels: dev_sdf.hpp; contract: include/icp_hip.h, DESIGN.md sections 6q
// and 6r-host.  Part of icp_hip.hip (included from there, after host_tsdf_hash_raycast.hpp).
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
    if ((rc = tsdf_check_call(c, cam, pose, who, true))) return rc;      // (either storage: SdfGeo's launches and sdf_integrate_slot choose the kernels)
    if (!depth) { c->err = std::string(who) + ": null depth frame"; return ICP_ERR_INVALID_ARG; }
    if (const char* why = sdf_options_error(opt)) { c->err = std::string(who) + ": " + why; return ICP_ERR_INVALID_ARG; }
    return ICP_OK;
}

// The two record kinds of direct SDF tracking, one traits struct each: SdfGeo (below) and SdfColor (host_sdf_color.hpp).  A kind names
// its state, frame record, iteration record and solve-parameter types, its NSUM sums and NCOUNT counts per block, the public options
// behind its extra per-frame kernel argument (Options -> Extra: nothing for geometry, SdfColorFrame for colour) and its three launches:
// init, accumulate on the dense or the hashed volume, solve.  The kernels stay restated per kind; everything the
// host does around them is written once below, over the kind.
struct SdfNone {};
struct SdfGeo {
    using State = SdfState; using Frame = icp_sdf_frame; using Iter = icp_sdf_iter; using Solve = SdfSolve; using Options = SdfNone; using Extra = SdfNone;
    static constexpr int NSUM = SDF_NSUM, NCOUNT = 2;
    static Extra extra(icp_ctx*, int, const SdfFrame&, const Options&) { return {}; }
    static void init(icp_ctx* c, State* st, const TsdfMat& m, Frame* rec) { hipLaunchKernelGGL(k_sdf_init, dim3(1), dim3(64), 0, c->stream, st, m, rec); }
    static void accumulate(icp_ctx* c, dim3 grid, const SdfFrame& f, const Extra&, const State* st, double* partials, int* counts) {
        if (c->tsdf_hashed) hipLaunchKernelGGL(k_hsdf_accumulate, grid, dim3(256), 0, c->stream, htsdf_view(c), f, st, partials, counts);
        else hipLaunchKernelGGL(k_sdf_accumulate, grid, dim3(256), 0, c->stream, tsdf_view(c), f, st, partials, counts);
    }
    static void solve(icp_ctx* c, const Solve& sp) { hipLaunchKernelGGL(k_sdf_solve, dim3(1), dim3(256), 0, c->stream, sp); }
};

// The three buffers every call of a kind writes before it reads: the state, partials[NSUM][blocks] + counts[NCOUNT][blocks], the frame
// record + trace.  They only grow, so the geometric and the coloured calls (and host_vgicp.hpp's) share them.
template <class K> int sdf_buffers(icp_ctx* c, int n_blocks, int n_iterations) {
    int rc;
    if ((rc = ensure(c, c->sdf_state, sizeof(typename K::State)))) return rc;
    if ((rc = ensure(c, c->sdf_partials, (size_t)n_blocks * (K::NSUM * 8 + K::NCOUNT * 4)))) return rc;
    if ((rc = ensure(c, c->sdf_rec, sizeof(typename K::Frame) + (size_t)n_iterations * sizeof(typename K::Iter)))) return rc;
    return ICP_OK;
}
// What the launches of one frame share: the grid of 16 x 16 tiles of sampled pixels and the device blocks behind it.
struct SdfPlan { dim3 grid; int n_blocks; SdfFrame f; };
template <class K> int sdf_plan(icp_ctx* c, const icp_depth_camera& cam, const icp_sdf_options& opt, SdfPlan* pl) {
    SdfFrame& f = pl->f;
    f.depth = nullptr; f.width = cam.width; f.height = cam.height; f.stride = opt.stride;
    f.ws = (cam.width + opt.stride - 1) / opt.stride; f.hs = (cam.height + opt.stride - 1) / opt.stride;
    f.fx = cam.fx; f.fy = cam.fy; f.cx = cam.cx; f.cy = cam.cy; f.huber = opt.huber;
    pl->grid = dim3((f.ws + 15) / 16, (f.hs + 15) / 16);
    pl->n_blocks = (int)(pl->grid.x * pl->grid.y);
    return sdf_buffers<K>(c, pl->n_blocks, opt.n_iterations);
}
// One alignment from `pose`, enqueued on the context's stream: the state, then `iterations` pairs of accumulate(st, partials, counts) over
// n_blocks blocks and the kind's solve (step = false: one pair that only folds).  Nothing here waits; the launches behind the end drain.
template <class K, class Acc>
int sdf_enqueue_pairs(icp_ctx* c, int n_blocks, const icp_sdf_options& opt, const float pose[16], bool step, bool trace, Acc&& accumulate) {
    typename K::State* st = c->sdf_state.as<typename K::State>();
    typename K::Frame* rec = c->sdf_rec.as<typename K::Frame>();
    typename K::Iter* tr = (typename K::Iter*)(rec + 1);
    double* partials = c->sdf_partials.as<double>();
    int* counts = (int*)(partials + (size_t)K::NSUM * n_blocks);
    TsdfMat m; memcpy(m.m, pose, 64);
    if (trace) HIPCK(c, hipMemsetAsync(tr, 0, (size_t)opt.n_iterations * sizeof(typename K::Iter), c->stream));
    K::init(c, st, m, rec);
    typename K::Solve sp;
    sp.partials = partials; sp.counts = counts; sp.n_blocks = n_blocks; sp.st = st; sp.rec = rec; sp.trace = trace ? tr : nullptr;
    sp.n_iterations = opt.n_iterations; sp.min_valid = opt.min_valid; sp.step = step ? 1 : 0;
    sp.stop_rotation = opt.stop_rotation; sp.stop_translation = opt.stop_translation;
    const int iterations = step ? opt.n_iterations : 1;
    for (int it = 0; it < iterations; it++) {
        accumulate((const typename K::State*)st, partials, counts);
        sp.iter = it;
        K::solve(c, sp);
    }
    HIPCK(c, hipGetLastError());
    return ICP_OK;
}
// The frame in upload slot `slot` (with the colour kind: the depth frame and, behind it, its colour frame) against the volume, dense or
// hashed: the stream waits for the slot's upload on the device, then sdf_enqueue_pairs.
template <class K>
int sdf_enqueue(icp_ctx* c, int slot, const SdfPlan& pl, const icp_sdf_options& opt, const typename K::Options& kopt, const float pose[16], bool step, bool trace) {
    SdfFrame f = pl.f;
    f.depth = aligned_depth(c, slot);
    const typename K::Extra x = K::extra(c, slot, f, kopt);
    HIPCK(c, hipStreamWaitEvent(c->stream, c->depth_up[slot], 0));
    return sdf_enqueue_pairs<K>(c, pl.n_blocks, opt, pose, step, trace,
                                [&](const typename K::State* st, double* partials, int* counts) { K::accumulate(c, pl.grid, f, x, st, partials, counts); });
}
// tsdf_integrate_slot on whichever storage the volume has (hashed: the touch's counters are read, one more host wait)
int sdf_integrate_slot(icp_ctx* c, int slot, const icp_depth_camera& cam, const float pose[16], bool color, const char* who) {
    return c->tsdf_hashed ? htsdf_integrate_slot(c, slot, cam, pose, nullptr, who, color) : tsdf_integrate_slot(c, slot, cam, pose, nullptr, color);
}
// The frame's record (and its trace) back through the page-locked block, waited for: the one host read of a frame.
template <class K> int sdf_read_record(icp_ctx* c, const icp_sdf_options& opt, typename K::Frame* rec_out, typename K::Iter* trace_out) {
    int rc;
    const size_t bytes = sizeof(typename K::Frame) + (trace_out ? (size_t)opt.n_iterations * sizeof(typename K::Iter) : 0);
    if ((rc = ensure_pinned(c, 2048 + bytes))) return rc;
    char* h = c->pinned.as<char>() + 2048;
    HIPCK(c, hipMemcpyAsync(h, c->sdf_rec.p, bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCK(c, hipStreamSynchronize(c->stream));
    memcpy(rec_out, h, sizeof(typename K::Frame));
    if (trace_out) memcpy(trace_out, h + sizeof(typename K::Frame), (size_t)opt.n_iterations * sizeof(typename K::Iter));
    return ICP_OK;
}
// The folded sums and counts of the last solve back through the same block, waited for: what the *_system calls return.
template <class K> int sdf_read_state(icp_ctx* c, double* sums_out, int32_t* counts_out) {
    int rc;
    if ((rc = ensure_pinned(c, 2048 + sizeof(typename K::State)))) return rc;
    typename K::State* h = (typename K::State*)(c->pinned.as<char>() + 2048);
    HIPCK(c, hipMemcpyAsync(h, c->sdf_state.p, sizeof(typename K::State), hipMemcpyDeviceToHost, c->stream));
    HIPCK(c, hipStreamSynchronize(c->stream));
    memcpy(sums_out, h->sums, sizeof(h->sums));
    for (int k = 0; k < K::NCOUNT; k++) counts_out[k] = h->counts[k];
    return ICP_OK;
}
template <class Frame> std::string sdf_failure(const char* who, const Frame& r, const icp_sdf_options& opt) {
    char buf[192];
    if (r.status == ICP_ERR_NO_SOURCE) snprintf(buf, sizeof(buf), "%s: the frame has no usable pixel", who);
    else snprintf(buf, sizeof(buf), "%s: step %d failed (%d valid pixels of %d usable, min_valid %d, or a non-finite solution)", who, r.iterations, r.n_valid_last, r.n_depth, opt.min_valid);
    return buf;
}

// ---- the bodies of the public calls, behind their checks (rgbx: null for the geometric kind)
// one frame staged in slot 0 and planned: what the system, the alignment and the timed pair start with
template <class K> int sdf_stage_one(icp_ctx* c, const float* depth, const uint8_t* rgbx, const icp_depth_camera& cam, const icp_sdf_options& opt, SdfPlan* pl) {
    int rc;
    if ((rc = set_device(c))) return rc;
    if ((rc = sdf_plan<K>(c, cam, opt, pl))) return rc;
    return stage_depth(c, 0, depth, rgbx, cam.width * cam.height, c->stream, -1, cam.width);
}
template <class K>
int sdf_system(icp_ctx* c, const float* depth, const uint8_t* rgbx, const icp_depth_camera& cam, const float pose[16], const icp_sdf_options& opt,
               const typename K::Options& kopt, double* sums_out, int32_t* counts_out) {
    int rc;
    DrainOnError guard(c);
    SdfPlan pl;
    if ((rc = sdf_stage_one<K>(c, depth, rgbx, cam, opt, &pl))) return rc;
    if ((rc = sdf_enqueue<K>(c, 0, pl, opt, kopt, pose, false, false))) return rc;
    if ((rc = sdf_read_state<K>(c, sums_out, counts_out))) return rc;
    return guard.done();
}
template <class K>
int sdf_align(icp_ctx* c, const float* depth, const uint8_t* rgbx, const icp_depth_camera& cam, const icp_sdf_options& opt, const typename K::Options& kopt,
              float pose_inout[16], typename K::Frame* rec_out, typename K::Iter* trace_out, const char* who) {
    int rc;
    DrainOnError guard(c);
    SdfPlan pl;
    if ((rc = sdf_stage_one<K>(c, depth, rgbx, cam, opt, &pl))) return rc;
    if ((rc = sdf_enqueue<K>(c, 0, pl, opt, kopt, pose_inout, true, trace_out != nullptr))) return rc;
    typename K::Frame r;
    if ((rc = sdf_read_record<K>(c, opt, &r, trace_out))) return rc;
    if (rec_out) *rec_out = r;
    memcpy(pose_inout, r.pose, 64);
    if (r.status != ICP_OK) c->err = sdf_failure(who, r, opt);
    return guard.done(r.status);      // (synchronised by the record read)
}
// The tracking loop.  rgbx_frames (optional with the geometric kind): every integrated frame's colours go into the volume as well; a
// slot's upload carries the depth frame and its colour frame in one copy, and the alignment waits for that slot's event.
template <class K>
int sdf_track(icp_ctx* c, const float* depth_frames, const uint8_t* rgbx_frames, int32_t n_frames, const icp_depth_camera& cam, const icp_sdf_options& opt,
              const typename K::Options& kopt, float pose_inout[16], typename K::Frame* out, const char* who) {
    int rc;
    const bool color = rgbx_frames != nullptr;
    DrainOnError guard(c);
    if ((rc = set_device(c))) return rc;
    const int n = cam.width * cam.height;
    auto frame_rgbx = [&](int k) { return color ? rgbx_frames + (size_t)k * n * 4 : nullptr; };
    SdfPlan pl;
    if ((rc = sdf_plan<K>(c, cam, opt, &pl))) return rc;
    if (!c->depth_stream) HIPCK(c, hipStreamCreateWithFlags(&c->depth_stream.s, hipStreamNonBlocking));
    if (!c->sdf_ev) HIPCK(c, hipEventCreateWithFlags(&c->sdf_ev.e, hipEventDisableTiming));
    // frame 0 into the model at the incoming pose; frame 1 goes up meanwhile
    if ((rc = stage_depth(c, 0, depth_frames, frame_rgbx(0), n, c->stream, -1, cam.width))) return rc;
    if ((rc = sdf_integrate_slot(c, 0, cam, pose_inout, color, who))) return rc;
    HIPCK(c, hipEventRecord(c->sdf_ev, c->stream));
    if (n_frames > 1 && (rc = stage_depth(c, 1, depth_frames + (size_t)n, frame_rgbx(1), n, c->depth_stream, -1, cam.width))) return rc;
    int first_err = ICP_OK;
    for (int k = 1; k < n_frames; k++) {
        const int slot = k & 1;
        if ((rc = sdf_enqueue<K>(c, slot, pl, opt, kopt, pose_inout, true, false))) return rc;
        // frame k + 1 goes up on the second stream while frame k iterates: its slot was last read by the integration of frame k - 1 (or an
        // earlier one), which may still be running -- the copy waits for it on the device, the host does not
        if (k + 1 < n_frames) {
            HIPCK(c, hipStreamWaitEvent(c->depth_stream, c->sdf_ev, 0));
            if ((rc = stage_depth(c, slot ^ 1, depth_frames + (size_t)(k + 1) * n, frame_rgbx(k + 1), n, c->depth_stream, -1, cam.width))) return rc;
        }
        typename K::Frame& r = out[k - 1];
        if ((rc = sdf_read_record<K>(c, opt, &r, nullptr))) return rc;
        memcpy(pose_inout, r.pose, 64);
        if (r.status == ICP_OK) {
            if ((rc = sdf_integrate_slot(c, slot, cam, pose_inout, color, who))) return rc;      // (inverts the pose on the host: why the record is read)
            HIPCK(c, hipEventRecord(c->sdf_ev, c->stream));
        } else if (first_err == ICP_OK) { first_err = r.status; c->err = sdf_failure(who, r, opt); }
    }
    HIPCK(c, hipStreamSynchronize(c->stream));
    HIPCK(c, hipStreamSynchronize(c->depth_stream));
    guard.ok = true;
    return first_err;
}
// The device time of ONE accumulate + solve pair at `pose` (timed_ms), the frame staged and the code warmed outside the bracket.
template <class K>
int sdf_time(icp_ctx* c, const float* depth, const uint8_t* rgbx, const icp_depth_camera& cam, const float pose[16], const icp_sdf_options& opt,
             const typename K::Options& kopt, float* ms_out) {
    int rc;
    DrainOnError guard(c);
    SdfPlan pl;
    if ((rc = sdf_stage_one<K>(c, depth, rgbx, cam, opt, &pl))) return rc;
    icp_sdf_options one = opt; one.n_iterations = 1;
    if ((rc = sdf_enqueue<K>(c, 0, pl, one, kopt, pose, true, false))) return rc;      // (warm: the first launch loads the code object)
    HIPCK(c, hipStreamSynchronize(c->stream));
    if ((rc = timed_ms(c, ms_out, [&] { return sdf_enqueue<K>(c, 0, pl, one, kopt, pose, true, false); }))) return rc;
    return guard.done();
}
// Both sample-to-host calls behind their checks: the points up, launch(points, field, gradient, valid), whatever the caller asked for back.
template <class Launch>
int tsdf_sample_to_host(icp_ctx* c, const float* points, int32_t n, float* f_out, float* grad_out, uint8_t* valid_out, const char* who, Launch&& launch) {
    if (n < 0 || (n > 0 && !points)) { c->err = std::string(who) + ": bad argument (n >= 0, points)"; return ICP_ERR_INVALID_ARG; }
    if (n == 0) return ICP_OK;
    int rc;
    DrainOnError guard(c);
    if ((rc = set_device(c))) return rc;
    if ((rc = ensure(c, c->staging, (size_t)n * 29))) return rc;      // [points 12n | field 4n | gradient 12n | valid n]
    float* d_pts = c->staging.as<float>(); float* d_f = d_pts + (size_t)n * 3; float* d_g = d_f + n; uint8_t* d_ok = (uint8_t*)(d_g + (size_t)n * 3);
    HIPCK(c, hipMemcpyAsync(d_pts, points, (size_t)n * 12, hipMemcpyHostToDevice, c->stream));
    launch((const float*)d_pts, d_f, d_g, d_ok);
    HIPCK(c, hipGetLastError());
    if (f_out) HIPCK(c, hipMemcpyAsync(f_out, d_f, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
    if (grad_out) HIPCK(c, hipMemcpyAsync(grad_out, d_g, (size_t)n * 12, hipMemcpyDeviceToHost, c->stream));
    if (valid_out) HIPCK(c, hipMemcpyAsync(valid_out, d_ok, (size_t)n, hipMemcpyDeviceToHost, c->stream));
    HIPCK(c, hipStreamSynchronize(c->stream));
    return guard.done();
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
    return tsdf_sample_to_host(c, points, n, f_out, grad_out, valid_out, "icp_tsdf_sample", [&](const float* d_pts, float* d_f, float* d_g, uint8_t* d_ok) {
        if (c->tsdf_hashed) hipLaunchKernelGGL(k_htsdf_sample, dim3((n + 255) / 256), dim3(256), 0, c->stream, htsdf_view(c), d_pts, (int)n, d_f, d_g, d_ok);
        else hipLaunchKernelGGL(k_tsdf_sample, dim3((n + 255) / 256), dim3(256), 0, c->stream, tsdf_view(c), d_pts, (int)n, d_f, d_g, d_ok);
    });
}

int icp_tsdf_sdf_system(icp_ctx* c, const float* depth, const icp_depth_camera* cam, const float pose[16], const icp_sdf_options* opt, double* sums_out,
                        int32_t* counts_out) {
    if (!c) return ICP_ERR_INVALID_ARG;
    int rc;
    if ((rc = sdf_check_call(c, depth, cam, pose, opt, "icp_tsdf_sdf_system"))) return rc;
    if (!sums_out || !counts_out) { c->err = "icp_tsdf_sdf_system: null output"; return ICP_ERR_INVALID_ARG; }
    return sdf_system<SdfGeo>(c, depth, nullptr, *cam, pose, *opt, {}, sums_out, counts_out);
}

int icp_tsdf_align_depth(icp_ctx* c, const float* depth, const icp_depth_camera* cam, const icp_sdf_options* opt, float pose_inout[16], icp_sdf_frame* rec_out,
                         icp_sdf_iter* trace_out) {
    if (!c) return ICP_ERR_INVALID_ARG;
    int rc;
    if ((rc = sdf_check_call(c, depth, cam, pose_inout, opt, "icp_tsdf_align_depth"))) return rc;
    return sdf_align<SdfGeo>(c, depth, nullptr, *cam, *opt, {}, pose_inout, rec_out, trace_out, "icp_tsdf_align_depth");
}

int icp_track_depth_sdf(icp_ctx* c, const float* depth_frames, const uint8_t* rgbx_frames, int32_t n_frames, const icp_depth_camera* cam, const icp_sdf_options* opt,
                        float pose_inout[16], icp_sdf_frame* out) {
    if (!c) return ICP_ERR_INVALID_ARG;
    const char* who = "icp_track_depth_sdf";
    if (n_frames < 1 || (n_frames > 1 && !out)) { c->err = std::string(who) + ": bad argument"; return ICP_ERR_INVALID_ARG; }
    int rc;
    if ((rc = sdf_check_call(c, depth_frames, cam, pose_inout, opt, who))) return rc;
    if (rgbx_frames && !tsdf_hashed_color(c) && (rc = tsdf_check_color(c, who))) return rc;      // (colour frames need colours: the dense array, or the blocks')
    return sdf_track<SdfGeo>(c, depth_frames, rgbx_frames, n_frames, *cam, *opt, {}, pose_inout, out, who);
}

// Not part of icp_hip.h (tools/time_tsdf.py): the device time of ONE k_sdf_accumulate + k_sdf_solve pair at `pose` between two events on
// the context's stream, the frame staged outside the bracket.
extern "C" int icp_debug_sdf_time(icp_ctx* c, const float* depth, const icp_depth_camera* cam, const float pose[16], const icp_sdf_options* opt, float* ms_out) {
    if (!c || !ms_out) return ICP_ERR_INVALID_ARG;
    int rc;
    if ((rc = sdf_check_call(c, depth, cam, pose, opt, "icp_debug_sdf_time"))) return rc;
    return sdf_time<SdfGeo>(c, depth, nullptr, *cam, pose, *opt, {}, ms_out);
}
