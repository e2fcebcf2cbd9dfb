// host_vmap.hpp -- scan-to-map laser tracking: the persistent voxel map (icp_voxel_map_create / destroy / insert / upload, icp_get_voxel_map),
// the sums of one step and one alignment of the resident source against it (icp_voxel_map_system, icp_voxel_map_align), and the tracking
// loop over a sequence of scans (icp_track_scans_vmap).  Kernels: dev_vmap.hpp for the insert; the alignment launches host_vgicp.hpp's
// k_vgicp_accumulate and k_sdf_solve as they are, with the map's cells in the plan.  Contract: include/icp_hip.h, DESIGN.md section 6t.
// Part of icp_hip.hip (included from there, after host_vgicp.hpp).
namespace {
const char* vmap_options_error(const icp_voxel_map_options* o) {
    if (!o) return "null options";
    if (!(std::isfinite(o->voxel_size) && o->voxel_size > 0.f)) return "voxel_size must be finite and > 0";
    long long cells = 1;
    for (int a = 0; a < 3; a++) {
        if (o->dims[a] < 1) return "dims must be >= 1 on every axis";
        if (o->lo[a] < -VG_CLAMP || o->lo[a] > VG_CLAMP) return "lo must lie within +-2^30 cells";
        cells = (cells > VG_MAX_CELLS || o->dims[a] > VG_MAX_CELLS) ? VG_MAX_CELLS + 1 : cells * o->dims[a];
    }
    if (cells > VG_MAX_CELLS) return "the map is dense: dims_x dims_y dims_z must be at most 2^24 cells";
    return nullptr;
}
size_t vm_cells(const icp_ctx* c) { return (size_t)c->vm_opt.dims[0] * c->vm_opt.dims[1] * c->vm_opt.dims[2]; }
VgGrid vm_view(const icp_ctx* c, int min_points) {
    VgGrid g;
    for (int a = 0; a < 3; a++) { g.lo[a] = c->vm_opt.lo[a]; g.dims[a] = c->vm_opt.dims[a]; }
    g.vs = c->vm_opt.voxel_size; g.min_points = min_points;
    return g;
}
int vmap_check(icp_ctx* c, const char* who) {
    if (!c->vm_on) { c->err = std::string(who) + ": no voxel map (icp_voxel_map_create)"; return ICP_ERR_INVALID_ARG; }
    return ICP_OK;
}
// One cloud into the map at `pose`, enqueued: the five counters of the insert cleared, k_vmap_insert over the points, k_vmap_records over
// as many lanes as the list can be long.  Nothing here waits or reads.
int vmap_insert_enqueue(icp_ctx* c, int which, const float pose[16], const char* who) {
    const Cloud& cl = which ? c->src : c->tgt;
    if (cl.n <= 0) {
        c->err = std::string(who) + (which ? ": no source cloud (icp_set_source)" : ": no target cloud (icp_set_target)");
        return which ? ICP_ERR_NO_SOURCE : ICP_ERR_NO_TARGET;
    }
    int rc;
    if ((rc = gicp_normals(c, which))) { c->err = std::string(who) + ": " + c->err; return rc; }
    if (c->vm_hashed) return hmap_insert_enqueue(c, which, pose, who);
    const size_t n_cells = vm_cells(c);
    if (c->vm_serial == INT_MAX) {                     // the serial numbers have run out: every stamp back to "never"
        HIPCK(c, hipMemsetAsync(c->vm_stamp.p, 0, n_cells * 4, c->stream));
        c->vm_serial = 0;
    }
    const int serial = ++c->vm_serial;
    VmCloud t;
    t.x = cl.x.as<float>(); t.y = cl.y.as<float>(); t.z = cl.z.as<float>(); t.n = cl.n;
    vg_normals(c, which, &t.nx, &t.ny, &t.nz);
    const int list_cap = (size_t)cl.n < n_cells ? cl.n : (int)n_cells;
    if ((rc = ensure(c, c->vm_list, (size_t)list_cap * 4))) return rc;
    int* ctr = c->vm_ctr.as<int>();
    HIPCK(c, hipMemsetAsync(ctr, 0, VM_OCCUPIED * 4, c->stream));
    const VgGrid g = vm_view(c, 1);
    TsdfMat m; memcpy(m.m, pose, 64);
    hipLaunchKernelGGL(k_vmap_insert, dim3((cl.n + 255) / 256), dim3(256), 0, c->stream, t, g, m, serial, list_cap, c->vm_count.as<int>(),
                       c->vm_sums.as<unsigned long long>(), c->vm_stamp.as<int>(), c->vm_list.as<int>(), ctr);
    hipLaunchKernelGGL(k_vmap_records, dim3((list_cap + 255) / 256), dim3(256), 0, c->stream, g, list_cap, (const int*)ctr, (const int*)c->vm_list.as<int>(),
                       (const int*)c->vm_count.as<int>(), (const long long*)c->vm_sums.as<long long>(), c->vm_cells.as<float2>());
    HIPCK(c, hipGetLastError());
    return ICP_OK;
}
// The plan of an alignment against the map: its cells and extent, then the source's half of host_vgicp.hpp's plan.
int vmap_plan(icp_ctx* c, const icp_vgicp_options* opt, const float* pose, const char* who, VgPlan* pl) {
    if (const char* why = vgicp_options_error(opt)) { c->err = std::string(who) + ": " + why; return ICP_ERR_INVALID_ARG; }
    if (!pose) { c->err = std::string(who) + ": null pose"; return ICP_ERR_INVALID_ARG; }
    int rc;
    if ((rc = vmap_check(c, who))) return rc;
    if (opt->voxel_size != c->vm_opt.voxel_size) {
        char buf[192];
        snprintf(buf, sizeof(buf), "%s: voxel_size %g is not the map's (%g)", who, (double)opt->voxel_size, (double)c->vm_opt.voxel_size);
        c->err = buf; return ICP_ERR_INVALID_ARG;
    }
    if (c->src.n <= 0) { c->err = std::string(who) + ": no source cloud (icp_set_source)"; return ICP_ERR_NO_SOURCE; }
    pl->g = vm_view(c, opt->min_points); pl->cells = c->vm_cells.as<float2>();
    if (c->vm_hashed) hmap_plan(c, opt->min_points, pl);
    return vgicp_plan_source(c, *opt, who, pl);
}
}  // namespace

int icp_voxel_map_options_check(const icp_voxel_map_options* o) { return vmap_options_error(o) ? ICP_ERR_INVALID_ARG : ICP_OK; }

int icp_voxel_map_create(icp_ctx* c, const icp_voxel_map_options* opt) {
    if (!c) return ICP_ERR_INVALID_ARG;
    if (const char* why = vmap_options_error(opt)) { c->err = std::string("icp_voxel_map_create: ") + why; return ICP_ERR_INVALID_ARG; }
    int rc;
    DrainOnError guard(c);
    if ((rc = set_device(c))) return rc;
    c->vm_on = false;
    if (c->vm_hashed) { HIPCK(c, hipStreamSynchronize(c->stream)); release(c->vh_keys); c->vm_hashed = false; c->vh_vac = false; c->vh_vac_bound = 0; }
    c->vm_opt = *opt;
    const size_t n = vm_cells(c);
    if ((rc = ensure(c, c->vm_count, n * 4))) return rc;
    if ((rc = ensure(c, c->vm_sums, n * VG_NSUM * 8))) return rc;
    if ((rc = ensure(c, c->vm_cells, n * 40))) return rc;
    if ((rc = ensure(c, c->vm_stamp, n * 4))) return rc;
    if ((rc = ensure(c, c->vm_ctr, VM_CTR_WORDS * 4))) return rc;
    if ((rc = ensure(c, c->vm_box, sizeof(VgBox)))) return rc;
    HIPCK(c, hipMemsetAsync(c->vm_count.p, 0, n * 4, c->stream));
    HIPCK(c, hipMemsetAsync(c->vm_sums.p, 0, n * VG_NSUM * 8, c->stream));
    HIPCK(c, hipMemsetAsync(c->vm_cells.p, 0, n * 40, c->stream));
    HIPCK(c, hipMemsetAsync(c->vm_stamp.p, 0, n * 4, c->stream));
    HIPCK(c, hipMemsetAsync(c->vm_ctr.p, 0, VM_NCTR * 4, c->stream));
    HIPCK(c, hipStreamSynchronize(c->stream));
    c->vm_serial = 0; c->vm_on = true;
    return guard.done();
}

int icp_voxel_map_destroy(icp_ctx* c) {
    if (!c) return ICP_ERR_INVALID_ARG;
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    for (DevBuf* b : {&c->vm_count, &c->vm_sums, &c->vm_cells, &c->vm_stamp, &c->vm_list, &c->vm_ctr, &c->vm_box, &c->vh_keys}) release(*b);
    c->vm_on = false; c->vm_hashed = false;
    return ICP_OK;
}

int icp_voxel_map_insert(icp_ctx* c, int32_t which, const float pose[16], icp_voxel_map_insert_info* info_out) {
    if (!c) return ICP_ERR_INVALID_ARG;
    const char* who = "icp_voxel_map_insert";
    int rc;
    if ((rc = vmap_check(c, who))) return rc;
    if ((which != 0 && which != 1) || !pose) { c->err = std::string(who) + ": bad argument (which 0 or 1, pose)"; return ICP_ERR_INVALID_ARG; }
    DrainOnError guard(c);
    if ((rc = set_device(c))) return rc;
    if ((rc = vmap_insert_enqueue(c, which, pose, who))) return rc;
    if (c->vm_hashed) { if ((rc = hmap_read_counters(c, (int*)info_out, who))) return rc; }      // (the counter that must stay 0 is read with the info)
    else if (info_out) { if ((rc = read_count(c, c->vm_ctr.p, (int*)info_out, 6))) return rc; }
    else HIPCK(c, hipStreamSynchronize(c->stream));
    return guard.done();
}

int icp_get_voxel_map(icp_ctx* c, icp_voxel_map_info* info_out, int32_t* counts_out, int64_t* sums_out, float* cells_out) {
    if (!c) return ICP_ERR_INVALID_ARG;
    int rc;
    if ((rc = vmap_check(c, "icp_get_voxel_map"))) return rc;
    if (c->vm_hashed) { c->err = "icp_get_voxel_map: the voxel map is hashed: use icp_get_voxel_map_hashed"; return ICP_ERR_INVALID_ARG; }
    DrainOnError guard(c);
    if ((rc = set_device(c))) return rc;
    if (info_out) {
        info_out->voxel_size = c->vm_opt.voxel_size;
        for (int a = 0; a < 3; a++) { info_out->lo[a] = c->vm_opt.lo[a]; info_out->dims[a] = c->vm_opt.dims[a]; }
        if ((rc = read_count(c, c->vm_ctr.as<int>() + VM_OCCUPIED, &info_out->n_occupied))) return rc;
    }
    if ((rc = vg_download(c, vm_cells(c), c->vm_count, c->vm_sums, c->vm_cells, counts_out, sums_out, cells_out))) return rc;
    return guard.done();
}

int icp_voxel_map_upload(icp_ctx* c, const int32_t* counts, const int64_t* sums) {
    if (!c) return ICP_ERR_INVALID_ARG;
    const char* who = "icp_voxel_map_upload";
    int rc;
    if ((rc = vmap_check(c, who))) return rc;
    if (c->vm_hashed) { c->err = std::string(who) + ": the voxel map is hashed: use icp_voxel_map_upload_hashed"; return ICP_ERR_INVALID_ARG; }
    if (!counts || !sums) { c->err = std::string(who) + ": null counts or sums"; return ICP_ERR_INVALID_ARG; }
    const size_t n = vm_cells(c);
    for (size_t i = 0; i < n; i++) if (counts[i] < 0) { c->err = std::string(who) + ": a count is negative"; return ICP_ERR_INVALID_ARG; }
    DrainOnError guard(c);
    if ((rc = set_device(c))) return rc;
    HIPCK(c, hipMemcpyAsync(c->vm_count.p, counts, n * 4, hipMemcpyHostToDevice, c->stream));
    HIPCK(c, hipMemcpyAsync(c->vm_sums.p, sums, n * VG_NSUM * 8, hipMemcpyHostToDevice, c->stream));
    // a full sweep: k_vg_finalise as the target's grid runs it, its occupied count into the map's running total
    VgBox* box = c->vm_box.as<VgBox>();
    hipLaunchKernelGGL(k_vg_box_init, dim3(1), dim3(64), 0, c->stream, box);
    hipLaunchKernelGGL(k_vg_finalise, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, vm_view(c, 1), (int)n, (const int*)c->vm_count.as<int>(),
                       (const long long*)c->vm_sums.as<long long>(), c->vm_cells.as<float2>(), box);
    HIPCK(c, hipGetLastError());
    HIPCK(c, hipMemcpyAsync(c->vm_ctr.as<int>() + VM_OCCUPIED, &box->n_occupied, 4, hipMemcpyDeviceToDevice, c->stream));
    HIPCK(c, hipStreamSynchronize(c->stream));
    return guard.done();
}

int icp_voxel_map_system(icp_ctx* c, const float pose[16], const icp_vgicp_options* opt, double* sums_out, int32_t* counts_out) {
    if (!c) return ICP_ERR_INVALID_ARG;
    const char* who = "icp_voxel_map_system";
    if (!sums_out || !counts_out) { c->err = std::string(who) + ": null output"; return ICP_ERR_INVALID_ARG; }
    int rc;
    DrainOnError guard(c);
    if ((rc = set_device(c))) return rc;
    VgPlan pl;
    if ((rc = vmap_plan(c, opt, pose, who, &pl))) return rc;
    if ((rc = vgicp_system_run(c, pl, pose, sums_out, counts_out))) return rc;
    return guard.done();
}

int icp_voxel_map_align(icp_ctx* c, const icp_vgicp_options* opt, float pose_inout[16], icp_vgicp_record* rec_out, icp_vgicp_iter* trace_out, int32_t max_trace) {
    if (!c) return ICP_ERR_INVALID_ARG;
    const char* who = "icp_voxel_map_align";
    if (max_trace < 0 || (max_trace > 0 && !trace_out)) { c->err = std::string(who) + ": bad argument (max_trace >= 0, trace_out)"; return ICP_ERR_INVALID_ARG; }
    int rc;
    DrainOnError guard(c);
    if ((rc = set_device(c))) return rc;
    VgPlan pl;
    if ((rc = vmap_plan(c, opt, pose_inout, who, &pl))) return rc;
    icp_sdf_frame r;
    if ((rc = vgicp_align_run(c, pl, *opt, pose_inout, rec_out, trace_out, max_trace, who, &r))) return rc;
    return guard.done(r.status);      // (synchronised by the record read)
}

int icp_track_scans_vmap(icp_ctx* c, const float* const* xyz, const float* const* normals, const int32_t* n, int32_t n_scans, const icp_vgicp_options* opt,
                         float pose_inout[16], icp_vgicp_record* out) {
    if (!c) return ICP_ERR_INVALID_ARG;
    const char* who = "icp_track_scans_vmap";
    if (n_scans < 1 || !xyz || !n || (n_scans > 1 && !out)) { c->err = std::string(who) + ": bad argument (n_scans >= 1, xyz, n, out)"; return ICP_ERR_INVALID_ARG; }
    if (const char* why = vgicp_options_error(opt)) { c->err = std::string(who) + ": " + why; return ICP_ERR_INVALID_ARG; }
    if (!pose_inout) { c->err = std::string(who) + ": null pose"; return ICP_ERR_INVALID_ARG; }
    int rc;
    if ((rc = vmap_check(c, who))) return rc;
    if (opt->voxel_size != c->vm_opt.voxel_size) { c->err = std::string(who) + ": voxel_size is not the map's"; return ICP_ERR_INVALID_ARG; }
    const bool own = c->gicp_opt.covariance_k == 0;
    for (int k = 0; k < n_scans; k++) {
        if (!xyz[k] || n[k] <= 0) { c->err = std::string(who) + ": a scan has null points or n <= 0"; return ICP_ERR_INVALID_ARG; }
        if (own && (!normals || !normals[k])) { c->err = std::string(who) + ": covariance_k = 0 needs normals on every scan"; return ICP_ERR_INVALID_ARG; }
    }
    DrainOnError guard(c);
    if ((rc = set_device(c))) return rc;
    int first_err = ICP_OK;
    for (int k = 0; k < n_scans; k++) {
        // the scan becomes the source by icp_set_source's path, without its wait: the upload only waits for the previous scan to have left the staging block
        if ((rc = upload_cloud(c, c->src, xyz[k], normals ? normals[k] : nullptr, nullptr, n[k], false))) return rc;
        if ((rc = finish_source(c))) return rc;
        if (k > 0) {
            VgPlan pl;
            if ((rc = vmap_plan(c, opt, pose_inout, who, &pl))) return rc;
            icp_sdf_frame& r = out[k - 1];
            if ((rc = vgicp_enqueue(c, pl, pose_inout, true, false))) return rc;
            // the one host read of the scan: the insert takes its pose from the host (a hashed map's occupied count comes with it)
            if ((rc = c->vm_hashed ? hmap_read_record(c, pl.so, &r, who) : sdf_read_record<SdfGeo>(c, pl.so, &r, nullptr))) return rc;
            memcpy(pose_inout, r.pose, 64);
            if (r.status != ICP_OK) {
                if (first_err == ICP_OK) { first_err = r.status; c->err = vgicp_failure(who, r, opt->min_valid); }
                continue;
            }
        }
        if ((rc = vmap_insert_enqueue(c, 1, pose_inout, who))) return rc;
    }
    if (c->vm_hashed) { if ((rc = hmap_read_counters(c, nullptr, who))) return rc; }
    else HIPCK(c, hipStreamSynchronize(c->stream));
    guard.ok = true;
    return first_err;
}

// Not part of icp_hip.h (tools/time_vmap.py): the device time of ONE insert of the resident cloud `which` at `pose` (both kernels and the
// counters' clear) and of k_vmap_records alone over the list that insert left, each between two events on the context's stream, after a
// warm insert.  Every call adds the cloud to the map twice: a tool's map, not a user's.
extern "C" int icp_debug_vmap_time(icp_ctx* c, int32_t which, const float pose[16], float* insert_ms_out, float* records_ms_out) {
    if (!c || !pose || !insert_ms_out || !records_ms_out || (which != 0 && which != 1)) return ICP_ERR_INVALID_ARG;
    const char* who = "icp_debug_vmap_time";
    int rc;
    if ((rc = vmap_check(c, who))) return rc;
    DrainOnError guard(c);
    if ((rc = set_device(c))) return rc;
    if (c->vm_hashed) {
        if ((rc = gicp_normals(c, which))) return rc;
        if ((rc = hmap_debug_time(c, which, pose, insert_ms_out, records_ms_out, who))) return rc;
        return guard.done();
    }
    if ((rc = vmap_insert_enqueue(c, which, pose, who))) return rc;
    HIPCK(c, hipStreamSynchronize(c->stream));
    if ((rc = timed_ms(c, insert_ms_out, [&] { return vmap_insert_enqueue(c, which, pose, who); }))) return rc;
    const Cloud& cl = which ? c->src : c->tgt;
    const size_t n_cells = vm_cells(c);
    const int list_cap = (size_t)cl.n < n_cells ? cl.n : (int)n_cells;
    rc = timed_ms(c, records_ms_out, [&] {
        hipLaunchKernelGGL(k_vmap_records, dim3((list_cap + 255) / 256), dim3(256), 0, c->stream, vm_view(c, 1), list_cap, (const int*)c->vm_ctr.as<int>(),
                           (const int*)c->vm_list.as<int>(), (const int*)c->vm_count.as<int>(), (const long long*)c->vm_sums.as<long long>(), c->vm_cells.as<float2>());
        return ICP_OK;
    });
    if (rc) return rc;
    return guard.done();
}

// Not part of icp_hip.h (tools/time_hmap.py): the device time of ONE accumulate launch of the resident source against the map at `pose`
// (k_vgicp_accumulate for a dense map, k_hmap_accumulate for a hashed one), the mean over `reps` launches between two events, after a
// fold at that pose that leaves the state's stop word clear.
extern "C" int icp_debug_vmap_accumulate_time(icp_ctx* c, const float pose[16], const icp_vgicp_options* opt, int32_t reps, float* ms_out) {
    if (!c || !ms_out || reps < 1) return ICP_ERR_INVALID_ARG;
    const char* who = "icp_debug_vmap_accumulate_time";
    int rc;
    DrainOnError guard(c);
    if ((rc = set_device(c))) return rc;
    VgPlan pl;
    if ((rc = vmap_plan(c, opt, pose, who, &pl))) return rc;
    if ((rc = vgicp_enqueue(c, pl, pose, false, false))) return rc;
    HIPCK(c, hipStreamSynchronize(c->stream));
    double* partials = c->sdf_partials.as<double>();
    int* counts = (int*)(partials + (size_t)SDF_NSUM * pl.n_blocks);
    const SdfState* st = c->sdf_state.as<SdfState>();
    float ms = 0.f;
    rc = timed_ms(c, &ms, [&] {
        for (int r = 0; r < reps; r++) {
            if (pl.h.keys) hipLaunchKernelGGL(k_hmap_accumulate, dim3(pl.n_blocks), dim3(256), 0, c->stream, pl.h, pl.cells, pl.s, st, partials, counts);
            else hipLaunchKernelGGL(k_vgicp_accumulate, dim3(pl.n_blocks), dim3(256), 0, c->stream, pl.g, pl.cells, pl.s, st, partials, counts);
        }
        return ICP_OK;
    });
    if (rc) return rc;
    *ms_out = ms / (float)reps;
    return guard.done();
}
