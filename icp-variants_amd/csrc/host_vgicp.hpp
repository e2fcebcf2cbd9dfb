// host_vgicp.hpp -- voxelized GICP: the target's voxel grid (icp_voxelize_target, icp_get_voxel_grid), the sums of one step
// (icp_vgicp_system) and one alignment of the resident source to the grid (icp_vgicp_align).  Kernels: dev_vgicp.hpp, and dev_sdf.hpp's
// k_sdf_init / k_sdf_solve launched as they are, through host_sdf.hpp's shared driver (sdf_enqueue_pairs, sdf_read_state, sdf_read_record
// for the geometric kind); contract: include/icp_hip.h, DESIGN.md section 6s.  Part of icp_hip.hip (included from there, after host_sdf.hpp:
// the pose state, the partials and the record are that file's buffers, free again whenever an entry point has returned).
namespace {
const char* vgicp_options_error(const icp_vgicp_options* o) {
    if (!o) return "null options";
    if (!(std::isfinite(o->voxel_size) && o->voxel_size > 0.f)) return "voxel_size must be finite and > 0";
    if (o->min_points < 1) return "min_points must be >= 1";
    if (o->n_iterations < 1 || o->n_iterations > 1000) return "n_iterations must be in 1 .. 1000";
    if (o->min_valid < 6) return "min_valid must be >= 6";
    if (!(std::isfinite(o->stop_rotation) && o->stop_rotation >= 0.f && std::isfinite(o->stop_translation) && o->stop_translation >= 0.f))
        return "stop_rotation and stop_translation must be finite and >= 0";
    return nullptr;
}
constexpr long long VG_MAX_CELLS = 1ll << 24;

// The cached GICP normals of a cloud as the kernels read them (gicp_normals has made them current): its own with covariance_k = 0.
void vg_normals(icp_ctx* c, int which, const float** nx, const float** ny, const float** nz) {
    const Cloud& cl = which ? c->src : c->tgt;
    const bool own = c->gicp_opt.covariance_k == 0;
    *nx = own ? cl.nx.as<float>() : c->gicp_n[which][0].as<float>();
    *ny = own ? cl.ny.as<float>() : c->gicp_n[which][1].as<float>();
    *nz = own ? cl.nz.as<float>() : c->gicp_n[which][2].as<float>();
}
VgGrid vg_view(const icp_ctx* c, int min_points) {
    VgGrid g;
    for (int a = 0; a < 3; a++) { g.lo[a] = c->vg_info.lo[a]; g.dims[a] = c->vg_info.dims[a]; }
    g.vs = c->vg_voxel; g.min_points = min_points;
    return g;
}
// The grid of the resident target at voxel size vs, unless it is current: bounds, one host read of them (the extent decides the
// allocation), the integer sums, the records, one host read of the occupied count.
int vg_build(icp_ctx* c, float vs, const char* who) {
    if (c->vg_ready && c->vg_voxel == vs) return ICP_OK;
    c->vg_ready = false;
    if (c->tgt.n <= 0) { c->err = std::string(who) + ": no target cloud (icp_set_target)"; return ICP_ERR_NO_TARGET; }
    int rc;
    if ((rc = gicp_normals(c, 0))) { c->err = std::string(who) + ": " + c->err; return rc; }
    VgTarget t;
    t.x = c->tgt.x.as<float>(); t.y = c->tgt.y.as<float>(); t.z = c->tgt.z.as<float>(); t.n = c->tgt.n; t.vs = vs;
    vg_normals(c, 0, &t.nx, &t.ny, &t.nz);
    if ((rc = ensure(c, c->vg_box, sizeof(VgBox)))) return rc;
    VgBox* box = c->vg_box.as<VgBox>();
    const dim3 grid((t.n + 255) / 256), block(256);
    hipLaunchKernelGGL(k_vg_box_init, dim3(1), dim3(64), 0, c->stream, box);
    hipLaunchKernelGGL(k_vg_bounds, grid, block, 0, c->stream, t, box);
    HIPCK(c, hipGetLastError());
    VgBox h;
    if ((rc = read_count(c, box, (int*)&h, (int)(sizeof(VgBox) / 4)))) return rc;
    if (h.lo[0] > h.hi[0]) { c->err = std::string(who) + ": no target point with a finite position and a finite GICP normal"; return ICP_ERR_NO_TARGET; }
    long long cells = 1;
    icp_voxel_grid_info info;
    for (int a = 0; a < 3; a++) {
        const long long d = (long long)h.hi[a] - (long long)h.lo[a] + 1;
        cells = (cells > VG_MAX_CELLS || d > VG_MAX_CELLS) ? VG_MAX_CELLS + 1 : cells * d;
        info.lo[a] = h.lo[a]; info.dims[a] = (int32_t)(d > INT_MAX ? INT_MAX : d);
    }
    if (cells > VG_MAX_CELLS) {
        char buf[224];
        snprintf(buf, sizeof(buf), "%s: voxel_size %g gives a grid of more than 2^24 cells over the target's extent (the grid is dense: choose a larger voxel_size)", who, (double)vs);
        c->err = buf; return ICP_ERR_INVALID_ARG;
    }
    const int n_cells = (int)cells;
    if ((rc = ensure(c, c->vg_count, (size_t)n_cells * 4))) return rc;
    if ((rc = ensure(c, c->vg_sums, (size_t)n_cells * VG_NSUM * 8))) return rc;
    if ((rc = ensure(c, c->vg_cells, (size_t)n_cells * 40))) return rc;
    HIPCK(c, hipMemsetAsync(c->vg_count.p, 0, (size_t)n_cells * 4, c->stream));
    HIPCK(c, hipMemsetAsync(c->vg_sums.p, 0, (size_t)n_cells * VG_NSUM * 8, c->stream));
    info.n_occupied = 0; info.n_points = 0;
    c->vg_info = info; c->vg_voxel = vs;
    const VgGrid g = vg_view(c, 1);
    hipLaunchKernelGGL(k_vg_cells_add, grid, block, 0, c->stream, t, g, c->vg_count.as<int>(), c->vg_sums.as<unsigned long long>());
    hipLaunchKernelGGL(k_vg_finalise, dim3((n_cells + 255) / 256), block, 0, c->stream, g, n_cells, (const int*)c->vg_count.as<int>(),
                       (const long long*)c->vg_sums.as<long long>(), c->vg_cells.as<float2>(), box);
    HIPCK(c, hipGetLastError());
    int tail[2];      // n_enter, n_occupied
    if ((rc = read_count(c, &box->n_enter, tail, 2))) return rc;
    c->vg_info.n_points = tail[0]; c->vg_info.n_occupied = tail[1];
    c->vg_ready = true;
    return ICP_OK;
}

int vgicp_check_call(icp_ctx* c, const icp_vgicp_options* opt, const float* pose, const char* who) {
    if (const char* why = vgicp_options_error(opt)) { c->err = std::string(who) + ": " + why; return ICP_ERR_INVALID_ARG; }
    if (!pose) { c->err = std::string(who) + ": null pose"; return ICP_ERR_INVALID_ARG; }
    if (c->tgt.n <= 0) { c->err = std::string(who) + ": no target cloud (icp_set_target)"; return ICP_ERR_NO_TARGET; }
    if (c->src.n <= 0) { c->err = std::string(who) + ": no source cloud (icp_set_source)"; return ICP_ERR_NO_SOURCE; }
    return ICP_OK;
}
// What the launches of one alignment share: the grid (built when it is not current), both clouds' GICP normals, the blocks of 256 source
// points and the device blocks behind them.
struct VgPlan { VgGrid g; const float2* cells; VgSource s; int n_blocks; icp_sdf_options so; HmTable h = {nullptr, 0, 0.f, 0}; };      // (h.keys set: the cells are a hashed voxel map's, host_hmap.hpp)
// (the source's half: what the voxel map's alignment shares, host_vmap.hpp; the caller has set pl->g and pl->cells)
int vgicp_plan_source(icp_ctx* c, const icp_vgicp_options& opt, const char* who, VgPlan* pl) {
    int rc;
    if ((rc = gicp_normals(c, 1))) { c->err = std::string(who) + ": " + c->err; return rc; }
    VgSource& s = pl->s;
    s.x = c->src.x.as<float>(); s.y = c->src.y.as<float>(); s.z = c->src.z.as<float>(); s.n = c->src.n;
    vg_normals(c, 1, &s.nx, &s.ny, &s.nz);
    s.one_minus_eps = 1.0 - (double)c->gicp_opt.epsilon;
    pl->n_blocks = (s.n + 256 * VG_POINTS_PER_LANE - 1) / (256 * VG_POINTS_PER_LANE);
    pl->so.stride = 1; pl->so.n_iterations = opt.n_iterations; pl->so.min_valid = opt.min_valid; pl->so.huber = 0.f;
    pl->so.stop_rotation = opt.stop_rotation; pl->so.stop_translation = opt.stop_translation;
    return sdf_buffers<SdfGeo>(c, pl->n_blocks, opt.n_iterations);
}
int vgicp_plan(icp_ctx* c, const icp_vgicp_options& opt, const char* who, VgPlan* pl) {
    int rc;
    if ((rc = vg_build(c, opt.voxel_size, who))) return rc;
    pl->g = vg_view(c, opt.min_points); pl->cells = c->vg_cells.as<float2>();
    return vgicp_plan_source(c, opt, who, pl);
}
// The source against the grid from `pose`, enqueued on the context's stream: host_sdf.hpp's sdf_enqueue_pairs for the geometric kind with
// k_vgicp_accumulate (or, on a hashed voxel map's cells, k_hmap_accumulate) as the accumulate.  No upload slot is waited for: the source
// is resident.  Nothing here waits; the launches behind the alignment's end drain.
int vgicp_enqueue(icp_ctx* c, const VgPlan& pl, const float pose[16], bool step, bool trace) {
    return sdf_enqueue_pairs<SdfGeo>(c, pl.n_blocks, pl.so, pose, step, trace, [&](const SdfState* st, double* partials, int* counts) {
        if (pl.h.keys) hipLaunchKernelGGL(k_hmap_accumulate, dim3(pl.n_blocks), dim3(256), 0, c->stream, pl.h, pl.cells, pl.s, st, partials, counts);
        else hipLaunchKernelGGL(k_vgicp_accumulate, dim3(pl.n_blocks), dim3(256), 0, c->stream, pl.g, pl.cells, pl.s, st, partials, counts);
    });
}
// One fold at `pose` and the state read back: what icp_vgicp_system does behind its plan.
int vgicp_system_run(icp_ctx* c, const VgPlan& pl, const float pose[16], double* sums_out, int32_t* counts_out) {
    int rc;
    if ((rc = vgicp_enqueue(c, pl, pose, false, false))) return rc;
    return sdf_read_state<SdfGeo>(c, sums_out, counts_out);
}
std::string vgicp_failure(const char* who, const icp_sdf_frame& r, int min_valid) {
    char buf[224];
    if (r.status == ICP_ERR_NO_SOURCE) snprintf(buf, sizeof(buf), "%s: the source has no point with a finite position", who);
    else snprintf(buf, sizeof(buf), "%s: step %d failed (%d valid points of %d considered, min_valid %d, or a non-finite solution)", who, r.iterations, r.n_valid_last, r.n_depth, min_valid);
    return buf;
}
// The alignment behind its plan: enqueued at once, ONE record read (with the trace when asked for); returns the record's status.
int vgicp_align_run(icp_ctx* c, const VgPlan& pl, const icp_vgicp_options& opt, float pose_inout[16], icp_vgicp_record* rec_out, icp_vgicp_iter* trace_out, int32_t max_trace,
                    const char* who, icp_sdf_frame* r) {
    int rc;
    const bool trace = trace_out && max_trace > 0;
    if ((rc = vgicp_enqueue(c, pl, pose_inout, true, trace))) return rc;
    std::vector<icp_sdf_iter> tr(trace ? (size_t)opt.n_iterations : 0);
    if ((rc = sdf_read_record<SdfGeo>(c, pl.so, r, trace ? tr.data() : nullptr))) return rc;
    if (trace) memcpy(trace_out, tr.data(), (size_t)(max_trace < opt.n_iterations ? max_trace : opt.n_iterations) * sizeof(icp_sdf_iter));
    if (rec_out) *rec_out = *r;
    memcpy(pose_inout, r->pose, 64);
    if (r->status != ICP_OK) c->err = vgicp_failure(who, *r, opt.min_valid);
    return ICP_OK;
}
// A grid's three arrays to the host (icp_get_voxel_grid, icp_get_voxel_map): any pointer may be null; waits for the stream.
int vg_download(icp_ctx* c, size_t n_cells, const DevBuf& count, const DevBuf& sums, const DevBuf& cells, int32_t* counts_out, int64_t* sums_out, float* cells_out) {
    if (counts_out) HIPCK(c, hipMemcpyAsync(counts_out, count.p, n_cells * 4, hipMemcpyDeviceToHost, c->stream));
    if (sums_out) HIPCK(c, hipMemcpyAsync(sums_out, sums.p, n_cells * VG_NSUM * 8, hipMemcpyDeviceToHost, c->stream));
    if (cells_out) {
        // the records without their count word: nine floats per cell
        std::vector<float> h(n_cells * 10);
        HIPCK(c, hipMemcpyAsync(h.data(), cells.p, n_cells * 40, hipMemcpyDeviceToHost, c->stream));
        HIPCK(c, hipStreamSynchronize(c->stream));
        for (size_t i = 0; i < n_cells; i++) memcpy(cells_out + i * 9, h.data() + i * 10, 36);
    }
    HIPCK(c, hipStreamSynchronize(c->stream));
    return ICP_OK;
}
}  // namespace

int icp_vgicp_options_default(icp_vgicp_options* o) {
    if (!o) return ICP_ERR_INVALID_ARG;
    o->voxel_size = 0.25f; o->min_points = 1; o->n_iterations = 30; o->min_valid = 64; o->stop_rotation = 1e-5f; o->stop_translation = 1e-5f;
    return ICP_OK;
}
int icp_vgicp_options_check(const icp_vgicp_options* o) { return vgicp_options_error(o) ? ICP_ERR_INVALID_ARG : ICP_OK; }

int icp_voxelize_target(icp_ctx* c, const icp_vgicp_options* opt, icp_voxel_grid_info* info_out) {
    if (!c) return ICP_ERR_INVALID_ARG;
    if (const char* why = vgicp_options_error(opt)) { c->err = std::string("icp_voxelize_target: ") + why; return ICP_ERR_INVALID_ARG; }
    int rc;
    DrainOnError guard(c);
    if ((rc = set_device(c))) return rc;
    if ((rc = vg_build(c, opt->voxel_size, "icp_voxelize_target"))) return rc;
    if (info_out) *info_out = c->vg_info;
    return guard.done();      // (synchronised by the read of the occupied count, or nothing was enqueued)
}

int icp_get_voxel_grid(icp_ctx* c, int32_t* counts_out, int64_t* sums_out, float* cells_out) {
    if (!c) return ICP_ERR_INVALID_ARG;
    if (!c->vg_ready) { c->err = "icp_get_voxel_grid: no voxel grid (icp_voxelize_target)"; return ICP_ERR_INVALID_ARG; }
    int rc;
    DrainOnError guard(c);
    if ((rc = set_device(c))) return rc;
    const size_t n_cells = (size_t)c->vg_info.dims[0] * c->vg_info.dims[1] * c->vg_info.dims[2];
    if ((rc = vg_download(c, n_cells, c->vg_count, c->vg_sums, c->vg_cells, counts_out, sums_out, cells_out))) return rc;
    return guard.done();
}

int icp_vgicp_system(icp_ctx* c, const float pose[16], const icp_vgicp_options* opt, double* sums_out, int32_t* counts_out) {
    if (!c) return ICP_ERR_INVALID_ARG;
    int rc;
    if ((rc = vgicp_check_call(c, opt, pose, "icp_vgicp_system"))) return rc;
    if (!sums_out || !counts_out) { c->err = "icp_vgicp_system: null output"; return ICP_ERR_INVALID_ARG; }
    DrainOnError guard(c);
    if ((rc = set_device(c))) return rc;
    VgPlan pl;
    if ((rc = vgicp_plan(c, *opt, "icp_vgicp_system", &pl))) return rc;
    if ((rc = vgicp_system_run(c, pl, pose, sums_out, counts_out))) return rc;
    return guard.done();
}

int icp_vgicp_align(icp_ctx* c, const icp_vgicp_options* opt, float pose_inout[16], icp_vgicp_record* rec_out, icp_vgicp_iter* trace_out, int32_t max_trace) {
    if (!c) return ICP_ERR_INVALID_ARG;
    int rc;
    if ((rc = vgicp_check_call(c, opt, pose_inout, "icp_vgicp_align"))) return rc;
    if (max_trace < 0 || (max_trace > 0 && !trace_out)) { c->err = "icp_vgicp_align: bad argument (max_trace >= 0, trace_out)"; return ICP_ERR_INVALID_ARG; }
    DrainOnError guard(c);
    if ((rc = set_device(c))) return rc;
    VgPlan pl;
    if ((rc = vgicp_plan(c, *opt, "icp_vgicp_align", &pl))) return rc;
    icp_sdf_frame r;
    if ((rc = vgicp_align_run(c, pl, *opt, pose_inout, rec_out, trace_out, max_trace, "icp_vgicp_align", &r))) return rc;
    return guard.done(r.status);      // (synchronised by the record read)
}

// Not part of icp_hip.h (tools/time_vgicp.py): the device time of ONE k_vgicp_accumulate + k_sdf_solve pair at `pose`, and of one grid
// build from a cold grid (its two host reads included), each between two events on the context's stream; next to them the event time of
// the target's last index build (build_bvh's own bracket), 0 when none has run.
extern "C" int icp_debug_vgicp_time(icp_ctx* c, const float pose[16], const icp_vgicp_options* opt, float* iter_ms_out, float* build_ms_out, float* index_ms_out) {
    if (!c || !iter_ms_out || !build_ms_out || !index_ms_out) return ICP_ERR_INVALID_ARG;
    *index_ms_out = (float)c->bvh.build_ms;
    int rc;
    if ((rc = vgicp_check_call(c, opt, pose, "icp_debug_vgicp_time"))) return rc;
    DrainOnError guard(c);
    if ((rc = set_device(c))) return rc;
    if ((rc = vg_build(c, opt->voxel_size, "icp_debug_vgicp_time"))) return rc;      // (warm: normals cached, buffers allocated, code loaded)
    c->vg_ready = false;
    if ((rc = timed_ms(c, build_ms_out, [&] { return vg_build(c, opt->voxel_size, "icp_debug_vgicp_time"); }))) return rc;
    VgPlan pl;
    if ((rc = vgicp_plan(c, *opt, "icp_debug_vgicp_time", &pl))) return rc;
    pl.so.n_iterations = 1;
    if ((rc = vgicp_enqueue(c, pl, pose, true, false))) return rc;
    HIPCK(c, hipStreamSynchronize(c->stream));
    if ((rc = timed_ms(c, iter_ms_out, [&] { return vgicp_enqueue(c, pl, pose, true, false); }))) return rc;
    return guard.done();
}
