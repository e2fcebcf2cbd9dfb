// host_sdf_color.hpp -- direct SDF tracking with the photometric term: the intensity field sampled at points (icp_tsdf_sample_color), the
// sums of one joint step (icp_tsdf_sdf_system_color), one frame aligned (icp_tsdf_align_depth_color) and the tracking loop
// (icp_track_depth_sdf_color), on the dense coloured volume or on a coloured hashed one (k_htsdf_sample_color, k_hsdf_accumulate_color:
// dev_tsdf_hash_color.hpp).  Only what is about colour lives here: the colour options and checks, the colour
// kind's traits (SdfColor) and the thin public wrappers; the driver they instantiate -- plan, enqueue, read-backs, alignment, tracking
// loop, timed pair -- is host_sdf.hpp's, written once over the kind.  Kernels: dev_sdf_color.hpp; contract: include/icp_hip.h, DESIGN.md
// section 6r.  Part of icp_hip.hip (included from there, after host_sdf.hpp; the state, partials and record buffers are the same ones,
// sized for the larger records -- every call writes them before it reads them).
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
    const bool hcol = tsdf_hashed_color(c);          // (either coloured storage: SdfColor's launches and sdf_integrate_slot choose the kernels)
    if ((rc = tsdf_check_call(c, cam, pose, who, hcol))) return rc;
    if (!hcol && (rc = tsdf_check_color(c, who))) return rc;
    if (!depth) { c->err = std::string(who) + ": null depth frame"; return ICP_ERR_INVALID_ARG; }
    if (!rgbx) { c->err = std::string(who) + ": null colour frame (rgbx)"; return ICP_ERR_INVALID_ARG; }
    if (const char* why = sdf_options_error(opt)) { c->err = std::string(who) + ": " + why; return ICP_ERR_INVALID_ARG; }
    if (const char* why = sdf_color_options_error(copt)) { c->err = std::string(who) + ": " + why; return ICP_ERR_INVALID_ARG; }
    return ICP_OK;
}
// The colour kind of host_sdf.hpp's driver: the larger records, 29 sums and 3 counts, the coloured kernels, and SdfColorFrame as the extra
// per-frame argument -- the colours of the volume (the dense array, or the blocks' pool) and the slot's colour frame, which stage_depth
// puts behind the depth frame.
struct SdfColor {
    using State = SdfColorState; using Frame = icp_sdf_color_frame; using Iter = icp_sdf_color_iter; using Solve = SdfColorSolve;
    using Options = icp_sdf_color_options; using Extra = SdfColorFrame;
    static constexpr int NSUM = SDFC_NSUM, NCOUNT = 3;
    static Extra extra(icp_ctx* c, int slot, const SdfFrame& f, const Options& copt) {
        SdfColorFrame cf;
        cf.col = c->tsdf_hashed ? c->th_cpool.as<float4>() : c->tsdf_col.as<float4>(); cf.rgbx = (const uint32_t*)(c->depth_dev[slot].as<float>() + (size_t)f.width * f.height);
        cf.weight = copt.weight; cf.huber = copt.huber;
        return cf;
    }
    static void init(icp_ctx* c, State* st, const TsdfMat& m, Frame* rec) { hipLaunchKernelGGL(k_sdf_init_color, dim3(1), dim3(64), 0, c->stream, st, m, rec); }
    static void accumulate(icp_ctx* c, dim3 grid, const SdfFrame& f, const Extra& cf, const State* st, double* partials, int* counts) {
        if (c->tsdf_hashed) hipLaunchKernelGGL(k_hsdf_accumulate_color, grid, dim3(256), 0, c->stream, htsdf_view(c), f, cf, st, partials, counts);
        else hipLaunchKernelGGL(k_sdf_accumulate_color, grid, dim3(256), 0, c->stream, tsdf_view(c), f, cf, st, partials, counts);
    }
    static void solve(icp_ctx* c, const Solve& sp) { hipLaunchKernelGGL(k_sdf_solve_color, dim3(1), dim3(256), 0, c->stream, sp); }
};
static_assert(sizeof(SdfColorState) >= sizeof(SdfState) && sizeof(icp_sdf_color_frame) >= sizeof(icp_sdf_frame) && sizeof(icp_sdf_color_iter) >= sizeof(icp_sdf_iter),
              "the colour kind's buffers hold the geometric kind's");
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
    return tsdf_sample_to_host(c, points, n, s_out, grad_out, valid_out, "icp_tsdf_sample_color", [&](const float* d_pts, float* d_s, float* d_h, uint8_t* d_ok) {
        if (hcol) hipLaunchKernelGGL(k_htsdf_sample_color, dim3((n + 255) / 256), dim3(256), 0, c->stream, htsdf_view(c), (const float4*)c->th_cpool.as<float4>(), d_pts, (int)n, d_s, d_h, d_ok);
        else hipLaunchKernelGGL(k_tsdf_sample_color, dim3((n + 255) / 256), dim3(256), 0, c->stream, tsdf_view(c), (const float4*)c->tsdf_col.as<float4>(), d_pts, (int)n, d_s, d_h, d_ok);
    });
}

int icp_tsdf_sdf_system_color(icp_ctx* c, const float* depth, const uint8_t* rgbx, const icp_depth_camera* cam, const float pose[16], const icp_sdf_options* opt,
                              const icp_sdf_color_options* copt, double* sums_out, int32_t* counts_out) {
    if (!c) return ICP_ERR_INVALID_ARG;
    int rc;
    if ((rc = sdf_color_check_call(c, depth, rgbx, cam, pose, opt, copt, "icp_tsdf_sdf_system_color"))) return rc;
    if (!sums_out || !counts_out) { c->err = "icp_tsdf_sdf_system_color: null output"; return ICP_ERR_INVALID_ARG; }
    return sdf_system<SdfColor>(c, depth, rgbx, *cam, pose, *opt, *copt, sums_out, counts_out);
}

int icp_tsdf_align_depth_color(icp_ctx* c, const float* depth, const uint8_t* rgbx, const icp_depth_camera* cam, const icp_sdf_options* opt,
                               const icp_sdf_color_options* copt, float pose_inout[16], icp_sdf_color_frame* rec_out, icp_sdf_color_iter* trace_out) {
    if (!c) return ICP_ERR_INVALID_ARG;
    int rc;
    if ((rc = sdf_color_check_call(c, depth, rgbx, cam, pose_inout, opt, copt, "icp_tsdf_align_depth_color"))) return rc;
    return sdf_align<SdfColor>(c, depth, rgbx, *cam, *opt, *copt, pose_inout, rec_out, trace_out, "icp_tsdf_align_depth_color");
}

int icp_track_depth_sdf_color(icp_ctx* c, const float* depth_frames, const uint8_t* rgbx_frames, int32_t n_frames, const icp_depth_camera* cam,
                              const icp_sdf_options* opt, const icp_sdf_color_options* copt, float pose_inout[16], icp_sdf_color_frame* out) {
    if (!c) return ICP_ERR_INVALID_ARG;
    const char* who = "icp_track_depth_sdf_color";
    if (n_frames < 1 || (n_frames > 1 && !out)) { c->err = std::string(who) + ": bad argument"; return ICP_ERR_INVALID_ARG; }
    int rc;
    if ((rc = sdf_color_check_call(c, depth_frames, rgbx_frames, cam, pose_inout, opt, copt, who))) return rc;
    return sdf_track<SdfColor>(c, depth_frames, rgbx_frames, n_frames, *cam, *opt, *copt, pose_inout, out, who);
}

// Not part of icp_hip.h (tools/time_tsdf.py): icp_debug_sdf_time for ONE k_sdf_accumulate_color + k_sdf_solve_color pair.
extern "C" int icp_debug_sdf_color_time(icp_ctx* c, const float* depth, const uint8_t* rgbx, const icp_depth_camera* cam, const float pose[16], const icp_sdf_options* opt,
                                        const icp_sdf_color_options* copt, float* ms_out) {
    if (!c || !ms_out) return ICP_ERR_INVALID_ARG;
    int rc;
    if ((rc = sdf_color_check_call(c, depth, rgbx, cam, pose, opt, copt, "icp_debug_sdf_color_time"))) return rc;
    return sdf_time<SdfColor>(c, depth, rgbx, *cam, pose, *opt, *copt, ms_out);
}
