// host_sdf_cloud.hpp -- direct SDF tracking of a resident cloud (a laser scan in its sensor frame): the sums of one step
// (icp_tsdf_cloud_system), one alignment to the context's TSDF volume, dense or hashed (icp_tsdf_align_cloud), and the tracking loop that
// aligns every scan to the model built so far and fuses it there (icp_track_scans_sdf).  Kernels: dev_sdf_cloud.hpp, and dev_sdf.hpp's
// k_sdf_init / k_sdf_solve launched as they are, through host_sdf.hpp's shared driver (sdf_buffers, sdf_enqueue_pairs, sdf_read_state,
// sdf_read_record for the geometric kind) as host_vgicp.hpp does; the fuse inside the loop is host_tsdf_cloud.hpp's tsdf_cloud_run.
// icp_track_scans_sdf_color is the same loop with every scan uploaded with its colours and every fuse the coloured one.
// With the colour kind (SdfColor, host_sdf_color.hpp) the same plan, enqueue and loop run the photometric alignment of a coloured scan
// (icp_tsdf_cloud_system_color, icp_tsdf_align_cloud_color, icp_track_scans_sdf_photometric; kernels: dev_sdf_cloud_color.hpp, DESIGN.md
// section 6zj).  Contract: include/icp_hip.h, DESIGN.md section 6zf.  Part of icp_hip.hip (included from there, after host_tsdf_cloud.hpp).
namespace {
// The checks that need no device, in the order the header states them (pose_only: the loop has no resident cloud to ask for).
int sdf_cloud_check(icp_ctx* c, int32_t which, const float* pose, const icp_sdf_options* opt, const char* who, bool pose_only, const Cloud** cl_out) {
    if (!c->tsdf_on) { c->err = std::string(who) + ": no volume (icp_tsdf_create, icp_tsdf_create_hashed)"; return ICP_ERR_INVALID_ARG; }
    if (!pose_only && which != 0 && which != 1) { c->err = std::string(who) + ": bad argument (which 0 or 1)"; return ICP_ERR_INVALID_ARG; }
    if (!pose) { c->err = std::string(who) + ": null pose"; return ICP_ERR_INVALID_ARG; }
    for (int k = 0; k < 16; k++) if (!std::isfinite(pose[k])) { c->err = std::string(who) + ": the pose must be finite"; return ICP_ERR_INVALID_ARG; }
    if (const char* why = sdf_options_error(opt)) { c->err = std::string(who) + ": " + why; return ICP_ERR_INVALID_ARG; }
    if (opt->stride != 1) { c->err = std::string(who) + ": stride must be 1 (a resident cloud has no order to stride over)"; return ICP_ERR_INVALID_ARG; }
    if (pose_only) return ICP_OK;
    const Cloud& cl = which ? c->src : c->tgt;
    if (cl.n <= 0) {
        c->err = std::string(who) + (which ? ": no source cloud (icp_set_source)" : ": no target cloud (icp_set_target)");
        return which ? ICP_ERR_NO_SOURCE : ICP_ERR_NO_TARGET;
    }
    *cl_out = &cl;
    return ICP_OK;
}
// What the launches of one alignment share: the cloud's planes and the blocks of SC_POINTS_PER_LANE x 256 points behind them (the coloured
// accumulate has a constant of its own).
constexpr int sdf_cloud_per_block(const SdfNone*) { return 256 * SC_POINTS_PER_LANE; }
constexpr int sdf_cloud_per_block(const icp_sdf_color_options*) { return 256 * SCC_POINTS_PER_LANE; }
// (rgba: the cloud's packed colour plane, read by the colour kind alone.)
struct ScPlan { TcCloud cl; const uint32_t* rgba; int n_blocks; };
template <class K> int sdf_cloud_plan(icp_ctx* c, const Cloud& cl, const icp_sdf_options& opt, ScPlan* pl) {
    pl->cl.x = cl.x.as<float>(); pl->cl.y = cl.y.as<float>(); pl->cl.z = cl.z.as<float>(); pl->cl.n = cl.n;
    pl->rgba = cl.has_colors ? cl.rgba.as<uint32_t>() : nullptr;
    constexpr int per_block = sdf_cloud_per_block((const typename K::Options*)nullptr);
    pl->n_blocks = (cl.n + per_block - 1) / per_block;
    return sdf_buffers<K>(c, pl->n_blocks, opt.n_iterations);
}
// The cloud's accumulate of either kind on whichever storage the volume has.
void sdf_cloud_launch(icp_ctx* c, const ScPlan& pl, const icp_sdf_options& opt, const SdfNone&, const SdfState* st, double* partials, int* counts) {
    if (c->tsdf_hashed) hipLaunchKernelGGL(k_hsdf_accumulate_cloud, dim3(pl.n_blocks), dim3(256), 0, c->stream, htsdf_view(c), pl.cl, opt.huber, st, partials, counts);
    else hipLaunchKernelGGL(k_sdf_accumulate_cloud, dim3(pl.n_blocks), dim3(256), 0, c->stream, tsdf_view(c), pl.cl, opt.huber, st, partials, counts);
}
void sdf_cloud_launch(icp_ctx* c, const ScPlan& pl, const icp_sdf_options& opt, const icp_sdf_color_options& copt, const SdfColorState* st, double* partials, int* counts) {
    SdfColorFrame cf;      // (sdf_cloud_color_check: the volume and the cloud have colours)
    cf.col = c->tsdf_hashed ? c->th_cpool.as<float4>() : c->tsdf_col.as<float4>(); cf.rgbx = pl.rgba; cf.weight = copt.weight; cf.huber = copt.huber;
    if (c->tsdf_hashed) hipLaunchKernelGGL(k_hsdf_accumulate_cloud_color, dim3(pl.n_blocks), dim3(256), 0, c->stream, htsdf_view(c), pl.cl, cf, opt.huber, st, partials, counts);
    else hipLaunchKernelGGL(k_sdf_accumulate_cloud_color, dim3(pl.n_blocks), dim3(256), 0, c->stream, tsdf_view(c), pl.cl, cf, opt.huber, st, partials, counts);
}
// The cloud against the volume from `pose`, enqueued on the context's stream: sdf_enqueue_pairs for the kind with the cloud's accumulate
// of that kind.  No upload slot is waited for: the cloud is resident.  Nothing here waits.
template <class K>
int sdf_cloud_enqueue(icp_ctx* c, const ScPlan& pl, const icp_sdf_options& opt, const typename K::Options& kopt, const float pose[16], bool step, bool trace) {
    return sdf_enqueue_pairs<K>(c, pl.n_blocks, opt, pose, step, trace,
                                [&](const typename K::State* st, double* partials, int* counts) { sdf_cloud_launch(c, pl, opt, kopt, st, partials, counts); });
}
template <class Frame> std::string sdf_cloud_failure(const char* who, const Frame& r, const icp_sdf_options& opt) {
    char buf[224];
    if (r.status == ICP_ERR_NO_SOURCE) snprintf(buf, sizeof(buf), "%s: the cloud has no point with a finite position", who);
    else snprintf(buf, sizeof(buf), "%s: step %d failed (%d valid points of %d considered, min_valid %d, or a non-finite solution)", who, r.iterations, r.n_valid_last, r.n_depth, opt.min_valid);
    return buf;
}
// What the photometric calls check behind sdf_cloud_check: the colour options, a coloured volume, a coloured cloud (cl: NULL in the loop).
int sdf_cloud_color_check(icp_ctx* c, const Cloud* cl, const icp_sdf_color_options* copt, const char* who) {
    if (const char* why = sdf_color_options_error(copt)) { c->err = std::string(who) + ": " + why; return ICP_ERR_INVALID_ARG; }
    if (!tsdf_volume_colored(c)) {
        c->err = std::string(who) + ": the volume has no colours (icp_tsdf_color_create, icp_tsdf_create_color_hashed)";
        return ICP_ERR_INVALID_ARG;
    }
    if (cl && !cl->has_colors) { c->err = std::string(who) + ": the cloud has no colours (icp_set_target / icp_set_source with rgba)"; return ICP_ERR_INVALID_ARG; }
    return ICP_OK;
}
int sdf_cloud_color_check(icp_ctx*, const Cloud*, const SdfNone*, const char*) { return ICP_OK; }      // (the geometric kind has nothing to check)
// The bodies of the system and the alignment of either kind, behind their checks.
template <class K>
int sdf_cloud_system(icp_ctx* c, const Cloud& cl, const float pose[16], const icp_sdf_options& opt, const typename K::Options& kopt, double* sums_out, int32_t* counts_out) {
    int rc;
    DrainOnError guard(c);
    if ((rc = set_device(c))) return rc;
    ScPlan pl;
    if ((rc = sdf_cloud_plan<K>(c, cl, opt, &pl))) return rc;
    if ((rc = sdf_cloud_enqueue<K>(c, pl, opt, kopt, pose, false, false))) return rc;
    if ((rc = sdf_read_state<K>(c, sums_out, counts_out))) return rc;
    return guard.done();
}
template <class K>
int sdf_cloud_align(icp_ctx* c, const Cloud& cl, const icp_sdf_options& opt, const typename K::Options& kopt, float pose_inout[16], typename K::Frame* rec_out,
                    typename K::Iter* trace_out, const char* who) {
    int rc;
    DrainOnError guard(c);
    if ((rc = set_device(c))) return rc;
    ScPlan pl;
    if ((rc = sdf_cloud_plan<K>(c, cl, opt, &pl))) return rc;
    if ((rc = sdf_cloud_enqueue<K>(c, pl, opt, kopt, pose_inout, true, trace_out != nullptr))) return rc;
    typename K::Frame r;
    if ((rc = sdf_read_record<K>(c, opt, &r, trace_out))) return rc;
    if (rec_out) *rec_out = r;
    memcpy(pose_inout, r.pose, 64);
    if (r.status != ICP_OK) c->err = sdf_cloud_failure(who, r, opt);
    return guard.done(r.status);      // (synchronised by the record read)
}
// The timed pair of either kind (icp_debug_sdf_cloud_time, icp_debug_sdf_cloud_color_time).
template <class K>
int sdf_cloud_time(icp_ctx* c, const Cloud& cl, const float pose[16], const icp_sdf_options& opt, const typename K::Options& kopt, float* ms_out) {
    int rc;
    DrainOnError guard(c);
    if ((rc = set_device(c))) return rc;
    ScPlan pl;
    if ((rc = sdf_cloud_plan<K>(c, cl, opt, &pl))) return rc;
    icp_sdf_options one = opt; one.n_iterations = 1;
    if ((rc = sdf_cloud_enqueue<K>(c, pl, one, kopt, pose, true, false))) return rc;      // (warm: the first launch loads the code object)
    HIPCK(c, hipStreamSynchronize(c->stream));
    if ((rc = timed_ms(c, ms_out, [&] { return sdf_cloud_enqueue<K>(c, pl, one, kopt, pose, true, false); }))) return rc;
    return guard.done();
}
}  // namespace

int icp_tsdf_cloud_system(icp_ctx* c, int32_t which, const float pose[16], const icp_sdf_options* opt, double* sums_out, int32_t* counts_out) {
    if (!c) return ICP_ERR_INVALID_ARG;
    const char* who = "icp_tsdf_cloud_system";
    int rc;
    const Cloud* cl = nullptr;
    if ((rc = sdf_cloud_check(c, which, pose, opt, who, false, &cl))) return rc;
    if (!sums_out || !counts_out) { c->err = std::string(who) + ": null output"; return ICP_ERR_INVALID_ARG; }
    return sdf_cloud_system<SdfGeo>(c, *cl, pose, *opt, {}, sums_out, counts_out);
}
int icp_tsdf_cloud_system_color(icp_ctx* c, int32_t which, const float pose[16], const icp_sdf_options* opt, const icp_sdf_color_options* copt, double* sums_out,
                                int32_t* counts_out) {
    if (!c) return ICP_ERR_INVALID_ARG;
    const char* who = "icp_tsdf_cloud_system_color";
    int rc;
    const Cloud* cl = nullptr;
    if ((rc = sdf_cloud_check(c, which, pose, opt, who, false, &cl))) return rc;
    if ((rc = sdf_cloud_color_check(c, cl, copt, who))) return rc;
    if (!sums_out || !counts_out) { c->err = std::string(who) + ": null output"; return ICP_ERR_INVALID_ARG; }
    return sdf_cloud_system<SdfColor>(c, *cl, pose, *opt, *copt, sums_out, counts_out);
}

int icp_tsdf_align_cloud(icp_ctx* c, int32_t which, const icp_sdf_options* opt, float pose_inout[16], icp_sdf_frame* rec_out, icp_sdf_iter* trace_out) {
    if (!c) return ICP_ERR_INVALID_ARG;
    const char* who = "icp_tsdf_align_cloud";
    int rc;
    const Cloud* cl = nullptr;
    if ((rc = sdf_cloud_check(c, which, pose_inout, opt, who, false, &cl))) return rc;
    return sdf_cloud_align<SdfGeo>(c, *cl, *opt, {}, pose_inout, rec_out, trace_out, who);
}
int icp_tsdf_align_cloud_color(icp_ctx* c, int32_t which, const icp_sdf_options* opt, const icp_sdf_color_options* copt, float pose_inout[16], icp_sdf_color_frame* rec_out,
                               icp_sdf_color_iter* trace_out) {
    if (!c) return ICP_ERR_INVALID_ARG;
    const char* who = "icp_tsdf_align_cloud_color";
    int rc;
    const Cloud* cl = nullptr;
    if ((rc = sdf_cloud_check(c, which, pose_inout, opt, who, false, &cl))) return rc;
    if ((rc = sdf_cloud_color_check(c, cl, copt, who))) return rc;
    return sdf_cloud_align<SdfColor>(c, *cl, *opt, *copt, pose_inout, rec_out, trace_out, who);
}

namespace {
// The loop of icp_track_scans_sdf and, with color, of icp_track_scans_sdf_color: rgba[k] goes up with scan k and every fuse is coloured.
// With the colour kind (kopt: its options, color set) the alignment is the photometric one: icp_track_scans_sdf_photometric.
template <class K>
int track_scans_sdf_run(icp_ctx* c, const float* const* xyz, const uint8_t* const* rgba, const int32_t* n, int32_t n_scans, const icp_sdf_options* opt,
                        const typename K::Options* kopt, float pose_inout[16], typename K::Frame* out, icp_tsdf_cloud_info* infos_out, bool color, int32_t* n_colored_out,
                        const char* who) {
    int rc;
    if ((rc = sdf_cloud_check(c, 1, pose_inout, opt, who, true, nullptr))) return rc;
    if ((rc = sdf_cloud_color_check(c, nullptr, kopt, who))) return rc;
    if (n_scans > 1 && !out) { c->err = std::string(who) + ": null output (out: n_scans - 1 records)"; return ICP_ERR_INVALID_ARG; }
    if (n_scans < 1 || !xyz || !n) { c->err = std::string(who) + ": bad argument (n_scans >= 1, xyz, n)"; return ICP_ERR_INVALID_ARG; }
    for (int k = 0; k < n_scans; k++) if (!xyz[k] || n[k] <= 0) { c->err = std::string(who) + ": a scan has null points or n <= 0"; return ICP_ERR_INVALID_ARG; }
    { int J; if ((rc = tsdf_carve_steps(c, who, &J))) return rc; }      // (the fuses' carving: refused before any scan is uploaded)
    if (color) {
        if ((rc = tsdf_cloud_color_check(c, nullptr, who))) return rc;
        if (!rgba) { c->err = std::string(who) + ": null colours (rgba: one array per scan)"; return ICP_ERR_INVALID_ARG; }
        for (int k = 0; k < n_scans; k++) {
            if (!rgba[k]) { c->err = std::string(who) + ": a scan has null colours"; return ICP_ERR_INVALID_ARG; }
            if (n[k] > ICP_TSDF_CLOUD_COLOR_MAX_POINTS) { c->err = std::string(who) + ": a scan has more than 2^24 points (the colour sums are 32-bit)"; return ICP_ERR_INVALID_ARG; }
        }
        if (n_colored_out) memset(n_colored_out, 0, (size_t)n_scans * sizeof(int32_t));
    }
    if (infos_out) memset(infos_out, 0, (size_t)n_scans * sizeof(icp_tsdf_cloud_info));
    DrainOnError guard(c);
    if ((rc = set_device(c))) return rc;
    int first_err = ICP_OK;
    for (int k = 0; k < n_scans; k++) {
        // the scan becomes the source by icp_set_source's path, without its wait: the upload only waits for the previous scan to have left the staging block
        if ((rc = upload_cloud(c, c->src, xyz[k], nullptr, color ? rgba[k] : nullptr, n[k], false))) return rc;
        if ((rc = finish_source(c))) return rc;
        if (k > 0) {
            ScPlan pl;
            if ((rc = sdf_cloud_plan<K>(c, c->src, *opt, &pl))) return rc;
            if ((rc = sdf_cloud_enqueue<K>(c, pl, *opt, *kopt, pose_inout, true, false))) return rc;
            // the one host read of the alignment: the fuse takes its pose from the host
            typename K::Frame& r = out[k - 1];
            if ((rc = sdf_read_record<K>(c, *opt, &r, nullptr))) return rc;
            memcpy(pose_inout, r.pose, 64);
            if (r.status != ICP_OK) {
                if (first_err == ICP_OK) { first_err = r.status; c->err = sdf_cloud_failure(who, r, *opt); }
                continue;
            }
        }
        if ((rc = tsdf_cloud_run(c, c->src, pose_inout, nullptr, infos_out ? infos_out + k : nullptr, who, nullptr, color, n_colored_out ? n_colored_out + k : nullptr)))
            return rc;      // (waits: it reads its counters)
    }
    HIPCK(c, hipStreamSynchronize(c->stream));      // (a skipped last scan leaves its bookkeeping launches behind the record read)
    guard.ok = true;
    return first_err;
}
}  // namespace

int icp_track_scans_sdf(icp_ctx* c, const float* const* xyz, const int32_t* n, int32_t n_scans, const icp_sdf_options* opt, float pose_inout[16], icp_sdf_frame* out,
                        icp_tsdf_cloud_info* infos_out) {
    if (!c) return ICP_ERR_INVALID_ARG;
    const SdfNone none;
    return track_scans_sdf_run<SdfGeo>(c, xyz, nullptr, n, n_scans, opt, &none, pose_inout, out, infos_out, false, nullptr, "icp_track_scans_sdf");
}
int icp_track_scans_sdf_color(icp_ctx* c, const float* const* xyz, const uint8_t* const* rgba, const int32_t* n, int32_t n_scans, const icp_sdf_options* opt,
                              float pose_inout[16], icp_sdf_frame* out, icp_tsdf_cloud_info* infos_out, int32_t* n_colored_out) {
    if (!c) return ICP_ERR_INVALID_ARG;
    const SdfNone none;
    return track_scans_sdf_run<SdfGeo>(c, xyz, rgba, n, n_scans, opt, &none, pose_inout, out, infos_out, true, n_colored_out, "icp_track_scans_sdf_color");
}
int icp_track_scans_sdf_photometric(icp_ctx* c, const float* const* xyz, const uint8_t* const* rgba, const int32_t* n, int32_t n_scans, const icp_sdf_options* opt,
                                    const icp_sdf_color_options* copt, float pose_inout[16], icp_sdf_color_frame* out, icp_tsdf_cloud_info* infos_out,
                                    int32_t* n_colored_out) {
    if (!c) return ICP_ERR_INVALID_ARG;
    return track_scans_sdf_run<SdfColor>(c, xyz, rgba, n, n_scans, opt, copt, pose_inout, out, infos_out, true, n_colored_out, "icp_track_scans_sdf_photometric");
}

// Not part of icp_hip.h (tools/time_sdf_cloud.py): the device time of ONE cloud accumulate + k_sdf_solve pair at `pose` between two events
// on the context's stream, the cloud resident and the code warmed outside the bracket.
extern "C" int icp_debug_sdf_cloud_time(icp_ctx* c, int32_t which, const float pose[16], const icp_sdf_options* opt, float* ms_out) {
    if (!c || !ms_out) return ICP_ERR_INVALID_ARG;
    const char* who = "icp_debug_sdf_cloud_time";
    int rc;
    const Cloud* cl = nullptr;
    if ((rc = sdf_cloud_check(c, which, pose, opt, who, false, &cl))) return rc;
    return sdf_cloud_time<SdfGeo>(c, *cl, pose, *opt, {}, ms_out);
}
// The same for ONE coloured cloud accumulate + k_sdf_solve_color pair (tools/time_sdf_cloud_color.py).
extern "C" int icp_debug_sdf_cloud_color_time(icp_ctx* c, int32_t which, const float pose[16], const icp_sdf_options* opt, const icp_sdf_color_options* copt, float* ms_out) {
    if (!c || !ms_out) return ICP_ERR_INVALID_ARG;
    const char* who = "icp_debug_sdf_cloud_color_time";
    int rc;
    const Cloud* cl = nullptr;
    if ((rc = sdf_cloud_check(c, which, pose, opt, who, false, &cl))) return rc;
    if ((rc = sdf_cloud_color_check(c, cl, copt, who))) return rc;
    return sdf_cloud_time<SdfColor>(c, *cl, pose, *opt, *copt, ms_out);
}
