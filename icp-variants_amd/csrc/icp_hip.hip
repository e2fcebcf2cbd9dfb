// =====================================================================================
// icp_hip.hip -- C-ABI implementation (libicp_hip.so) over the gfx950 kernels in icp_device.hpp.
// Entry points and the reference interfaces they replace are documented in include/icp_hip.h.
// There is NO CPU fallback: every entry point needs a HIP device and fails with ICP_ERR_HIP /
// ICP_ERR_NO_DEVICE when none is usable.
// =====================================================================================
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstring>
#include <cstdio>
#include <cstdlib>
#include <cmath>
#include "icp_device.hpp"
#include <hip/hip_ext.h>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_select.hpp>
#include <rocprim/iterator/counting_iterator.hpp>
#include <rocprim/iterator/transform_iterator.hpp>
#include <map>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

// The host side in pieces, in dependency order (as icp_device.hpp includes dev_*.hpp): ONE translation unit, the device code compiled once.
// An entry point that include/icp_hip.h declares takes its C linkage from that declaration; only the hooks the header does not declare
// (icp_debug_*, icp_selftest_*, icp_internal_*) are written inside extern "C".
#include "host_ctx.hpp"
#include "host_index.hpp"
#include "host_launch.hpp"
#include "host_loop.hpp"
#include "host_multi.hpp"
#include "host_depth.hpp"
#include "host_tsdf.hpp"
#include "host_tsdf_hash.hpp"
#include "host_tsdf_hash_raycast.hpp"
#include "host_sdf.hpp"
#include "host_vgicp.hpp"
#include "host_hmap.hpp"
#include "host_vmap.hpp"
#include "host_vmap_prune.hpp"
#include "host_sdf_color.hpp"
#include "host_tsdf_mesh.hpp"
#include "host_tsdf_hash_mesh.hpp"
#include "host_mesh_cluster.hpp"
#include "host_tsdf_hash_evict.hpp"
#include "host_tsdf_cloud.hpp"
#include "host_sdf_cloud.hpp"
#include "host_global.hpp"
#include "host_debug.hpp"

// What stays here: context create / destroy, the option setters and getters, and the small one-shot entry points.
extern "C" {
const char* icp_version(void) { return "icp_hip gfx950 r2"; }

uint32_t icp_select_hash(uint32_t seed, uint32_t iteration, uint32_t index) { return select_hash(seed, iteration, index); }

int icp_params_default(icp_params* p) {
    if (!p) return ICP_ERR_INVALID_ARG;
    memset(p, 0, sizeof(*p));
    p->metric = 0; p->matching = 0; p->weighting = 0; p->rejection = 1; p->color_icp = 0; p->multires = 0;   // ICPOptimizer.h:29-31
    p->n_iterations = 20; p->max_distance = 0.0003f;
    p->knn_backend = ICP_KNN_BRUTE_FORCE; p->record_rmse = 0;
    p->knn_incremental = 1;
    p->selection = 0; p->selection_proba = 1.0f; p->selection_seed = 0u;      // setSelectionMethod(SELECT_ALL), proba default 1.0 (ICPOptimizer.h:58)
    return ICP_OK;
}

int icp_ctx_create_on_stream(int device, void* hip_stream, icp_ctx** out) {
    if (!out) return ICP_ERR_INVALID_ARG;
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return ICP_ERR_NO_DEVICE;
    if (device < 0 || device >= ndev) return ICP_ERR_INVALID_ARG;
    icp_ctx* c = new icp_ctx();
    c->device = device;
    icp_params_default(&c->prm);
    memset(&c->timing, 0, sizeof(c->timing));
    if (hipSetDevice(device) != hipSuccess) { delete c; return ICP_ERR_HIP; }
    { const char* e = getenv("ICP_HIP_MERGE"); if (e && e[0] == '0') c->merge_loop = false; }
    { const char* e = getenv("ICP_HIP_TRACE"); if (e && e[0] == '1') c->trace = true; }
    { const char* e = getenv("ICP_HIP_STAGE_EVENTS"); if (e && e[0] >= '0' && e[0] <= '9') c->stage_timing = atoi(e); }
    if (!hip_stream && hipStreamCreateWithFlags(&c->own_stream.s, hipStreamNonBlocking) != hipSuccess) { delete c; return ICP_ERR_HIP; }
    c->stream = hip_stream ? (hipStream_t)hip_stream : c->own_stream.s;
    c->cos_reject = compute_cos_reject();
    float ident[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    int rc = write_pose(c, ident);
    if (!rc && hipStreamSynchronize(c->stream) != hipSuccess) rc = ICP_ERR_HIP;
    if (rc) { icp_ctx_destroy(c); return rc; }
    *out = c;
    return ICP_OK;
}
int icp_ctx_create(int device, icp_ctx** out) { return icp_ctx_create_on_stream(device, nullptr, out); }

int icp_ctx_destroy(icp_ctx* c) {
    if (!c) return ICP_ERR_INVALID_ARG;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    if (c->depth_stream) (void)hipStreamSynchronize(c->depth_stream);
    delete c;                            // every buffer, page-locked block and event frees itself, the owned streams last (host_ctx.hpp)
    return ICP_OK;
}

const char* icp_last_error(const icp_ctx* c) { return c ? c->err.c_str() : "null context"; }

int icp_set_params(icp_ctx* c, const icp_params* p) {
    if (!c || !p) return ICP_ERR_INVALID_ARG;
    if (p->metric < 0 || p->metric > 4 || p->matching < 0 || p->matching > 1 || p->weighting < 0 || p->weighting > 3 || p->n_iterations < 0 || p->selection < ICP_SELECT_ALL || p->selection > ICP_SELECT_NORMAL_SPACE ||
        (p->knn_backend != ICP_KNN_BRUTE_FORCE && p->knn_backend != ICP_KNN_LBVH) || p->width < 0 || p->height < 0 || (long long)p->width * p->height > 0x7FFFFFFFll ||
        std::isnan(p->max_distance) || std::isnan(p->selection_proba) || !std::isfinite(p->fx) || !std::isfinite(p->fy) || !std::isfinite(p->cx) || !std::isfinite(p->cy)) {
        c->err = "icp_set_params: value out of range"; return ICP_ERR_INVALID_ARG;
    }
    c->prm = *p;
    return ICP_OK;
}
int icp_get_params(const icp_ctx* c, icp_params* p) { if (!c || !p) return ICP_ERR_INVALID_ARG; *p = c->prm; return ICP_OK; }

int icp_lm_options_default(icp_lm_options* o) {
    if (!o) return ICP_ERR_INVALID_ARG;
    memset(o, 0, sizeof(*o));
    o->initial_trust_region_radius = 1e4; o->max_trust_region_radius = 1e16; o->min_trust_region_radius = 1e-32;
    o->min_relative_decrease = 1e-3; o->min_lm_diagonal = 1e-6; o->max_lm_diagonal = 1e32;
    o->function_tolerance = 1e-6; o->gradient_tolerance = 1e-10; o->parameter_tolerance = 1e-8;
    o->max_num_iterations = 10;                            // configureSolver (ICPOptimizer.h:359)
    o->max_num_consecutive_invalid_steps = 5; o->jacobi_scaling = 1;
    return ICP_OK;
}

int icp_set_optimizer(icp_ctx* c, const icp_lm_options* o) {
    if (!c) return ICP_ERR_INVALID_ARG;
    if (!o) { c->lm_on = false; return ICP_OK; }
    const bool ok = o->max_num_iterations >= 0 && o->max_num_iterations <= 1000 && o->max_num_consecutive_invalid_steps >= 1 &&
                    o->min_trust_region_radius > 0 && o->min_trust_region_radius <= o->initial_trust_region_radius &&
                    o->initial_trust_region_radius <= o->max_trust_region_radius && std::isfinite(o->max_trust_region_radius) &&
                    o->min_lm_diagonal > 0 && o->min_lm_diagonal <= o->max_lm_diagonal && std::isfinite(o->max_lm_diagonal) &&
                    o->min_relative_decrease >= 0 && o->function_tolerance >= 0 && o->gradient_tolerance >= 0 && o->parameter_tolerance >= 0 &&
                    std::isfinite(o->min_relative_decrease) && std::isfinite(o->function_tolerance) && std::isfinite(o->gradient_tolerance) &&
                    std::isfinite(o->parameter_tolerance) && (o->jacobi_scaling == 0 || o->jacobi_scaling == 1);
    if (!ok) { c->err = "icp_set_optimizer: options out of range"; return ICP_ERR_INVALID_ARG; }
    c->lm_opt = *o; c->lm_on = true;
    return ICP_OK;
}

int icp_get_lm_summaries(const icp_ctx* c, icp_lm_summary* out, int32_t max, int32_t* count) {
    if (!c || !count || max < 0 || (max > 0 && !out)) return ICP_ERR_INVALID_ARG;
    const int32_t n = (int32_t)c->lm_last.size();
    for (int32_t i = 0; i < n && i < max; i++) out[i] = c->lm_last[(size_t)i];
    *count = n;
    return ICP_OK;
}

int icp_gicp_options_default(icp_gicp_options* o) {
    if (!o) return ICP_ERR_INVALID_ARG;
    o->epsilon = 1e-3f; o->covariance_k = 20;
    return ICP_OK;
}
int icp_set_gicp_options(icp_ctx* c, const icp_gicp_options* o) {
    if (!c) return ICP_ERR_INVALID_ARG;
    icp_gicp_options v;
    if (o) v = *o; else icp_gicp_options_default(&v);
    const int k = v.covariance_k;
    if (!(v.epsilon > 0.f && v.epsilon <= 1.f) || !(k == 0 || k == 5 || k == 10 || k == 20)) {
        c->err = "icp_set_gicp_options: need 0 < epsilon <= 1 and covariance_k in {0, 5, 10, 20}"; return ICP_ERR_INVALID_ARG;
    }
    c->gicp_opt = v;
    c->gicp_ready[0] = c->gicp_ready[1] = false; c->vg_ready = false;
    return ICP_OK;
}
int icp_get_gicp_options(const icp_ctx* c, icp_gicp_options* o) { if (!c || !o) return ICP_ERR_INVALID_ARG; *o = c->gicp_opt; return ICP_OK; }
int icp_colored_options_default(icp_colored_options* o) {
    if (!o) return ICP_ERR_INVALID_ARG;
    o->lambda_geometric = 0.968f; o->gradient_k = 20;
    return ICP_OK;
}
int icp_set_colored_options(icp_ctx* c, const icp_colored_options* o) {
    if (!c) return ICP_ERR_INVALID_ARG;
    icp_colored_options v;
    if (o) v = *o; else icp_colored_options_default(&v);
    const int k = v.gradient_k;
    if (!(v.lambda_geometric >= 0.f && v.lambda_geometric <= 1.f) || !(k == 5 || k == 10 || k == 20)) {
        c->err = "icp_set_colored_options: need 0 <= lambda_geometric <= 1 and gradient_k in {5, 10, 20}"; return ICP_ERR_INVALID_ARG;
    }
    c->col_opt = v;
    c->col_ready = false;
    return ICP_OK;
}
int icp_get_colored_options(const icp_ctx* c, icp_colored_options* o) { if (!c || !o) return ICP_ERR_INVALID_ARG; *o = c->col_opt; return ICP_OK; }

int icp_robust_options_default(icp_robust_options* o) {
    if (!o) return ICP_ERR_INVALID_ARG;
    o->kernel = ICP_ROBUST_NONE; o->tuning = 0.f; o->sigma = 0.f; o->overlap = 1.f;
    return ICP_OK;
}
int icp_set_robust_options(icp_ctx* c, const icp_robust_options* o) {
    if (!c) return ICP_ERR_INVALID_ARG;
    icp_robust_options v;
    if (o) v = *o; else icp_robust_options_default(&v);
    if (v.kernel < ICP_ROBUST_NONE || v.kernel > ICP_ROBUST_TUKEY) { c->err = "icp_set_robust_options: kernel must be one of ICP_ROBUST_NONE / HUBER / CAUCHY / TUKEY (0..3)"; return ICP_ERR_INVALID_ARG; }
    if (!(std::isfinite(v.tuning) && v.tuning >= 0.f) || !(std::isfinite(v.sigma) && v.sigma >= 0.f)) { c->err = "icp_set_robust_options: tuning and sigma must be finite and >= 0"; return ICP_ERR_INVALID_ARG; }
    if (!(v.overlap > 0.f && v.overlap <= 1.f)) { c->err = "icp_set_robust_options: need 0 < overlap <= 1"; return ICP_ERR_INVALID_ARG; }
    c->rob_opt = v;
    return ICP_OK;
}
int icp_get_robust_options(const icp_ctx* c, icp_robust_options* o) { if (!c || !o) return ICP_ERR_INVALID_ARG; *o = c->rob_opt; return ICP_OK; }
int icp_get_robust_stats(const icp_ctx* c, icp_robust_stats* out, int32_t max_out, int32_t* count_out) {
    if (!c || max_out < 0 || (!out && max_out > 0)) return ICP_ERR_INVALID_ARG;
    const int32_t n = (int32_t)c->rob_last.size();
    for (int32_t i = 0; i < n && i < max_out; i++) out[i] = c->rob_last[(size_t)i];
    if (count_out) *count_out = n;
    return ICP_OK;
}

int icp_reciprocal_options_default(icp_reciprocal_options* o) {
    if (!o) return ICP_ERR_INVALID_ARG;
    o->enabled = 0;
    return ICP_OK;
}
int icp_set_reciprocal_options(icp_ctx* c, const icp_reciprocal_options* o) {
    if (!c) return ICP_ERR_INVALID_ARG;
    icp_reciprocal_options v;
    if (o) v = *o; else icp_reciprocal_options_default(&v);
    if (v.enabled != 0 && v.enabled != 1) { c->err = "icp_set_reciprocal_options: enabled must be 0 or 1"; return ICP_ERR_INVALID_ARG; }
    c->rcp_opt = v;
    return ICP_OK;
}
int icp_get_reciprocal_options(const icp_ctx* c, icp_reciprocal_options* o) { if (!c || !o) return ICP_ERR_INVALID_ARG; *o = c->rcp_opt; return ICP_OK; }
int icp_get_reciprocal_stats(const icp_ctx* c, icp_reciprocal_stats* out, int32_t max_out, int32_t* count_out) {
    if (!c || max_out < 0 || (!out && max_out > 0)) return ICP_ERR_INVALID_ARG;
    const int32_t n = (int32_t)c->rcp_last.size();
    for (int32_t i = 0; i < n && i < max_out; i++) out[i] = c->rcp_last[(size_t)i];
    if (count_out) *count_out = n;
    return ICP_OK;
}

int icp_convergence_options_default(icp_convergence_options* o) {
    if (!o) return ICP_ERR_INVALID_ARG;
    o->enabled = 0; o->rotation_eps = 1e-6f; o->translation_eps = 1e-6f; o->min_iterations = 1; o->patience = 1;
    return ICP_OK;
}
int icp_set_convergence_options(icp_ctx* c, const icp_convergence_options* o) {
    if (!c) return ICP_ERR_INVALID_ARG;
    icp_convergence_options v;
    if (o) v = *o; else icp_convergence_options_default(&v);
    if (v.enabled != 0 && v.enabled != 1) { c->err = "icp_set_convergence_options: enabled must be 0 or 1"; return ICP_ERR_INVALID_ARG; }
    if (!(std::isfinite(v.rotation_eps) && v.rotation_eps > 0.f) || !(std::isfinite(v.translation_eps) && v.translation_eps > 0.f)) { c->err = "icp_set_convergence_options: rotation_eps and translation_eps must be finite and > 0"; return ICP_ERR_INVALID_ARG; }
    if (v.min_iterations < 1) { c->err = "icp_set_convergence_options: need min_iterations >= 1"; return ICP_ERR_INVALID_ARG; }
    if (v.patience < 1 || v.patience > 8) { c->err = "icp_set_convergence_options: need 1 <= patience <= 8"; return ICP_ERR_INVALID_ARG; }
    c->cvg_opt = v;
    return ICP_OK;
}
int icp_get_convergence_options(const icp_ctx* c, icp_convergence_options* o) { if (!c || !o) return ICP_ERR_INVALID_ARG; *o = c->cvg_opt; return ICP_OK; }
int icp_get_convergence(const icp_ctx* c, icp_convergence_result* out) { if (!c || !out) return ICP_ERR_INVALID_ARG; *out = c->cvg_last; return ICP_OK; }
int icp_get_convergence_trace(const icp_ctx* c, icp_convergence_step* out, int32_t max_out, int32_t* count_out) {
    if (!c || max_out < 0 || (!out && max_out > 0)) return ICP_ERR_INVALID_ARG;
    const int32_t n = (int32_t)c->cvg_trace.size();
    for (int32_t i = 0; i < n && i < max_out; i++) out[i] = c->cvg_trace[(size_t)i];
    if (count_out) *count_out = n;
    return ICP_OK;
}

int icp_nss_options_default(icp_nss_options* o) {
    if (!o) return ICP_ERR_INVALID_ARG;
    o->grid = 5; o->resample = 1;
    return ICP_OK;
}
int icp_set_nss_options(icp_ctx* c, const icp_nss_options* o) {
    if (!c) return ICP_ERR_INVALID_ARG;
    icp_nss_options v;
    if (o) v = *o; else icp_nss_options_default(&v);
    if (!(v.grid == 3 || v.grid == 5 || v.grid == 7) || !(v.resample == 0 || v.resample == 1)) {
        c->err = "icp_set_nss_options: need grid in {3, 5, 7} and resample in {0, 1}"; return ICP_ERR_INVALID_ARG;
    }
    c->nss_opt = v;
    c->nss_held_stale = true;                                // the bucket cache and the sorted levels follow the grid at their next use (nss_buckets)
    return ICP_OK;
}
int icp_get_nss_options(const icp_ctx* c, icp_nss_options* o) { if (!c || !o) return ICP_ERR_INVALID_ARG; *o = c->nss_opt; return ICP_OK; }
int icp_get_normal_buckets(icp_ctx* c, uint16_t* out, int32_t max_points, int32_t* n_out) {
    if (!c) return ICP_ERR_INVALID_ARG;
    if (max_points < 0 || (!out && max_points > 0)) { c->err = "icp_get_normal_buckets: bad argument (max_points >= 0)"; return ICP_ERR_INVALID_ARG; }
    int rc;
    DrainOnError guard(c);
    if ((rc = set_device(c))) return rc;
    if (c->src.n <= 0) { c->err = "no source cloud (icp_set_source)"; return ICP_ERR_NO_SOURCE; }
    if (!c->src.has_normals) { c->err = "icp_get_normal_buckets: the source has no normals"; return ICP_ERR_INVALID_ARG; }
    if ((rc = nss_buckets(c))) return rc;
    const int m = max_points < c->src.n ? max_points : c->src.n;
    if (n_out) *n_out = c->src.n;
    if (m > 0) HIPCK(c, hipMemcpyAsync(out, c->nss_bkt.p, (size_t)m * 2, hipMemcpyDeviceToHost, c->stream));
    HIPCK(c, hipStreamSynchronize(c->stream));
    return guard.done();
}
int icp_get_selection(icp_ctx* c, int32_t iteration, int32_t* out, int32_t max_out, int32_t* n_out) {
    if (!c) return ICP_ERR_INVALID_ARG;
    if (max_out < 0 || (!out && max_out > 0)) { c->err = "icp_get_selection: bad argument (max_out >= 0)"; return ICP_ERR_INVALID_ARG; }
    if (c->sel_last.empty()) { c->err = "icp_get_selection: the last run on this context made no selection (selection = 0, or no run since the source was set)"; return ICP_ERR_INVALID_ARG; }
    if (iteration < 0 || (size_t)iteration >= c->sel_last.size()) { c->err = "icp_get_selection: iteration out of range"; return ICP_ERR_INVALID_ARG; }
    int rc;
    DrainOnError guard(c);
    if ((rc = set_device(c))) return rc;
    const std::pair<const int*, int>& s = c->sel_last[(size_t)iteration];
    const int m = max_out < s.second ? max_out : s.second;
    if (n_out) *n_out = s.second;
    if (m > 0) HIPCK(c, hipMemcpyAsync(out, s.first, (size_t)m * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCK(c, hipStreamSynchronize(c->stream));
    return guard.done();
}

int icp_set_stage_timing(icp_ctx* c, int32_t every_nth) {
    if (!c || every_nth < 0) { if (c) c->err = "icp_set_stage_timing: bad argument"; return ICP_ERR_INVALID_ARG; }
    c->stage_timing = every_nth;
    return ICP_OK;
}

int icp_get_timing(const icp_ctx* c, icp_timing* out) { if (!c || !out) return ICP_ERR_INVALID_ARG; *out = c->timing; return ICP_OK; }

int icp_get_iteration_times(const icp_ctx* c, float* match_ms, float* weight_reject_build_ms, float* solve_ms, int32_t max_out, int32_t* count_out) {
    if (!c || !count_out || max_out < 0) return ICP_ERR_INVALID_ARG;
    const int n = (int)c->it_match_ms.size();
    for (int i = 0; i < n && i < max_out; i++) {
        if (match_ms) match_ms[i] = c->it_match_ms[(size_t)i];
        if (weight_reject_build_ms) weight_reject_build_ms[i] = c->it_post_ms[(size_t)i];
        if (solve_ms) solve_ms[i] = c->it_solve_ms[(size_t)i];
    }
    *count_out = n;
    return ICP_OK;
}

int icp_set_convergence_reference(icp_ctx* c, const float* src_xyz, const float* ref_xyz, int32_t n) {
    if (!c || !src_xyz || !ref_xyz || n <= 0) { if (c) c->err = "icp_set_convergence_reference: bad argument"; return ICP_ERR_INVALID_ARG; }
    int rc;
    DrainOnError guard(c);
    if ((rc = set_device(c))) return rc;
    if ((rc = upload3(c, src_xyz, n, n, 0.f, c->conv_src.x, c->conv_src.y, c->conv_src.z))) return rc;
    if ((rc = upload3(c, ref_xyz, n, n, 0.f, c->conv_ref.x, c->conv_ref.y, c->conv_ref.z))) return rc;
    c->conv_n = n;
    return guard.done();
}

// One convergence measure of the resident reference under a pose (icp_benchmark_error, icp_rmse).
static int measure_at(icp_ctx* c, const float pose[16], float* out, const char* no_reference, int (*enqueue)(icp_ctx*, float*)) {
    if (!c || !pose || !out) return ICP_ERR_INVALID_ARG;
    if (c->conv_n <= 0) { c->err = no_reference; return ICP_ERR_INVALID_ARG; }
    int rc;
    DrainOnError guard(c);
    if ((rc = set_device(c))) return rc;
    if ((rc = write_pose(c, pose))) return rc;
    if ((rc = ensure(c, c->rmse_out, 4))) return rc;
    if ((rc = enqueue(c, c->rmse_out.as<float>()))) return rc;
    HIPCK(c, hipMemcpyAsync(out, c->rmse_out.p, 4, hipMemcpyDeviceToHost, c->stream));
    HIPCK(c, hipStreamSynchronize(c->stream));
    return guard.done();
}
int icp_benchmark_error(icp_ctx* c, const float pose[16], float* error_out) { return measure_at(c, pose, error_out, "icp_benchmark_error: no convergence reference set", enqueue_fontana); }
int icp_rmse(icp_ctx* c, const float pose[16], float* rmse_out) { return measure_at(c, pose, rmse_out, "icp_rmse: no convergence reference set", enqueue_rmse); }

static int transform_common(icp_ctx* c, const float* in, int32_t n, const float pose[16], float* out, int normals) {
    if (!c || !in || !out || !pose || n <= 0) { if (c) c->err = "icp_transform: bad argument"; return ICP_ERR_INVALID_ARG; }
    int rc;
    DrainOnError guard(c);
    if ((rc = set_device(c))) return rc;
    if ((rc = write_pose(c, pose))) return rc;
    if ((rc = ensure(c, c->staging, (size_t)n * 24))) return rc;
    float* din = c->staging.as<float>(); float* dout = din + (size_t)n * 3;
    HIPCK(c, hipMemcpyAsync(din, in, (size_t)n * 12, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(k_transform_aos, dim3((n + 255) / 256), dim3(256), 0, c->stream, din, n, c->ps.as<PoseState>(), normals, dout);
    HIPCK(c, hipGetLastError());
    HIPCK(c, hipMemcpyAsync(out, dout, (size_t)n * 12, hipMemcpyDeviceToHost, c->stream));
    HIPCK(c, hipStreamSynchronize(c->stream));
    return guard.done();
}

int icp_transform_points(icp_ctx* c, const float* xyz, int32_t n, const float pose[16], float* out) { return transform_common(c, xyz, n, pose, out, 0); }
int icp_transform_normals(icp_ctx* c, const float* nrm, int32_t n, const float pose[16], float* out) { return transform_common(c, nrm, n, pose, out, 1); }
}  // extern "C"
