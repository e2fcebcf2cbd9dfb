// host_vmap_prune.hpp -- a local voxel map: icp_voxel_map_prune (cells beyond a radius go back to the cleared state), icp_voxel_map_compact, and
// icp_track_scans_vmap_local, the tracking loop that prunes about the sensor after every insert.  Kernels: dev_vmap_prune.hpp; the hashed
// map's room rule and compaction: host_hmap.hpp.  Contract: include/icp_hip.h, DESIGN.md section 6v.  Part of icp_hip.hip (included from
// there, after host_vmap.hpp).
namespace {
// One prune, enqueued: the counters of a prune cleared (16 bytes), then one launch over the cells or the slots.  Nothing here waits.
int vmap_prune_enqueue(icp_ctx* c, const float centre[3], float r2) {
    int* ctr = c->vm_ctr.as<int>();
    VmPruneCtr* pc = (VmPruneCtr*)(ctr + VM_PRUNE_AT);
    HIPCK(c, hipMemsetAsync(pc, 0, sizeof(VmPruneCtr), c->stream));
    const VmSphere s = {centre[0], centre[1], centre[2], r2, c->vm_opt.voxel_size};
    if (c->vm_hashed) {
        const int cap = (int)hm_cap(c);
        hipLaunchKernelGGL(k_hmap_prune, dim3((cap + 255) / 256), dim3(256), 0, c->stream, (const unsigned long long*)c->vh_keys.as<unsigned long long>(), cap, s, c->vm_count.as<int>(),
                           c->vm_sums.as<long long>(), c->vm_cells.as<float2>(), c->vm_stamp.as<int>(), ctr, pc);
        c->vh_vac = true; c->vh_vac_bound += c->vh_bound;      // (until the counters are read: every occupied cell may have gone)
    } else {
        const int n = (int)vm_cells(c);
        hipLaunchKernelGGL(k_vmap_prune, dim3((n + 255) / 256), dim3(256), 0, c->stream, vm_view(c, 1), s, n, c->vm_count.as<int>(), c->vm_sums.as<long long>(),
                           c->vm_cells.as<float2>(), c->vm_stamp.as<int>(), ctr, pc);
    }
    HIPCK(c, hipGetLastError());
    return ICP_OK;
}
// what the host knows of a prune's info when it enqueues it
void vmap_prune_host_info(const icp_ctx* c, icp_voxel_map_prune_info* o) {
    memset(o, 0, sizeof(*o));
    o->n_compacted = c->vm_hashed ? c->vh_compacted : 0;
    o->capacity = c->vm_hashed ? (int32_t)hm_cap(c) : (int32_t)vm_cells(c);
}
// The seven words behind VM_OCCUPIED as one copy brought them (occupied, unplaced, vacated; removed, -, removed points): the rest of the
// info, and for a hashed map the host's counts made exact and the counter that must stay 0.
int vmap_prune_take(icp_ctx* c, const int* h, icp_voxel_map_prune_info* o, const char* who) {
    if (o) {
        o->n_removed = h[3]; o->n_occupied = h[0]; o->n_vacated = c->vm_hashed ? h[2] : 0;
        memcpy(&o->n_points_removed, h + 5, 8);
    }
    if (!c->vm_hashed) return ICP_OK;
    c->vh_bound = h[0]; c->vh_vac_bound = h[2]; c->vh_vac = h[2] > 0;
    return hmap_unplaced_error(c, h[1], who);
}
constexpr int VM_TAIL_WORDS = VM_CTR_WORDS - VM_OCCUPIED;
// sdf_read_record with those seven words read in the SAME wait (hmap_read_record's way, 32 bytes in front of the record's place)
int vmap_read_record_local(icp_ctx* c, const icp_sdf_options& so, icp_sdf_frame* r, icp_voxel_map_prune_info* pending, const char* who) {
    int rc;
    if ((rc = ensure_pinned(c, 4096 + sizeof(icp_sdf_frame)))) return rc;
    int* h = (int*)(c->pinned.as<char>() + 2016);
    HIPCK(c, hipMemcpyAsync(h, c->vm_ctr.as<int>() + VM_OCCUPIED, VM_TAIL_WORDS * 4, hipMemcpyDeviceToHost, c->stream));
    if ((rc = sdf_read_record<SdfGeo>(c, so, r, nullptr))) return rc;
    return vmap_prune_take(c, h, pending, who);
}
int vmap_read_prune(icp_ctx* c, icp_voxel_map_prune_info* o, const char* who) {
    int h[VM_TAIL_WORDS], rc;
    if ((rc = read_count(c, c->vm_ctr.as<int>() + VM_OCCUPIED, h, VM_TAIL_WORDS))) return rc;
    return vmap_prune_take(c, h, o, who);
}
}  // namespace

int icp_voxel_map_prune(icp_ctx* c, const float centre[3], float radius, icp_voxel_map_prune_info* info_out) {
    if (!c) return ICP_ERR_INVALID_ARG;
    const char* who = "icp_voxel_map_prune";
    int rc;
    if ((rc = vmap_check(c, who))) return rc;
    if (!centre || !(std::isfinite(centre[0]) && std::isfinite(centre[1]) && std::isfinite(centre[2]))) { c->err = std::string(who) + ": centre must be three finite numbers"; return ICP_ERR_INVALID_ARG; }
    if (!(std::isfinite(radius) && radius >= 0.f)) { c->err = std::string(who) + ": radius must be finite and >= 0"; return ICP_ERR_INVALID_ARG; }
    DrainOnError guard(c);
    if ((rc = set_device(c))) return rc;
    if ((rc = vmap_prune_enqueue(c, centre, radius * radius))) return rc;
    if (info_out) {
        vmap_prune_host_info(c, info_out);
        if ((rc = vmap_read_prune(c, info_out, who))) return rc;
    }
    return guard.done();
}

int icp_voxel_map_compact(icp_ctx* c) {
    if (!c) return ICP_ERR_INVALID_ARG;
    const char* who = "icp_voxel_map_compact";
    int rc;
    if ((rc = hmap_check(c, who))) return rc;
    if (!c->vh_vac) return ICP_OK;
    DrainOnError guard(c);
    if ((rc = set_device(c))) return rc;
    if ((rc = hmap_read_vacated(c))) return rc;
    if (c->vh_vac) {
        if ((rc = hmap_rehash(c, c->vh_log2cap, true))) return rc;
        if ((rc = hmap_read_counters(c, nullptr, who))) return rc;
    }
    return guard.done();
}

int icp_track_scans_vmap_local(icp_ctx* c, const float* const* xyz, const float* const* normals, const int32_t* n, int32_t n_scans, const icp_vgicp_options* opt,
                               float keep_radius, float pose_inout[16], icp_vgicp_record* out, icp_voxel_map_prune_info* prune_out) {
    if (!c) return ICP_ERR_INVALID_ARG;
    const char* who = "icp_track_scans_vmap_local";
    if (n_scans < 1 || !xyz || !n || (n_scans > 1 && !out)) { c->err = std::string(who) + ": bad argument (n_scans >= 1, xyz, n, out)"; return ICP_ERR_INVALID_ARG; }
    if (const char* why = vgicp_options_error(opt)) { c->err = std::string(who) + ": " + why; return ICP_ERR_INVALID_ARG; }
    if (!pose_inout) { c->err = std::string(who) + ": null pose"; return ICP_ERR_INVALID_ARG; }
    if (!(std::isfinite(keep_radius) && keep_radius > 0.f)) { c->err = std::string(who) + ": keep_radius must be finite and > 0"; return ICP_ERR_INVALID_ARG; }
    if (!(std::isfinite(pose_inout[12]) && std::isfinite(pose_inout[13]) && std::isfinite(pose_inout[14]))) { c->err = std::string(who) + ": the pose's translation must be finite"; return ICP_ERR_INVALID_ARG; }
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
    if (prune_out) memset(prune_out, 0, (size_t)n_scans * sizeof(*prune_out));
    const float r2 = keep_radius * keep_radius;
    int first_err = ICP_OK, pending = -1;              // pending: the scan whose prune's counters are still on the device
    for (int k = 0; k < n_scans; k++) {
        if ((rc = upload_cloud(c, c->src, xyz[k], normals ? normals[k] : nullptr, nullptr, n[k], false))) return rc;
        if ((rc = finish_source(c))) return rc;
        if (k > 0) {
            VgPlan pl;
            if ((rc = vmap_plan(c, opt, pose_inout, who, &pl))) return rc;
            icp_sdf_frame& r = out[k - 1];
            if ((rc = vgicp_enqueue(c, pl, pose_inout, true, false))) return rc;
            // the one host read of the scan: its record, and with it what the previous prune left (the next insert's room rule uses it)
            if ((rc = vmap_read_record_local(c, pl.so, &r, prune_out && pending >= 0 ? &prune_out[pending] : nullptr, who))) return rc;
            pending = -1;
            memcpy(pose_inout, r.pose, 64);
            if (r.status != ICP_OK) {
                if (first_err == ICP_OK) { first_err = r.status; c->err = vgicp_failure(who, r, opt->min_valid); }
                continue;
            }
        }
        if ((rc = vmap_insert_enqueue(c, 1, pose_inout, who))) return rc;
        if ((rc = vmap_prune_enqueue(c, pose_inout + 12, r2))) return rc;
        if (prune_out) vmap_prune_host_info(c, &prune_out[k]);
        pending = k;
    }
    if ((rc = vmap_read_prune(c, prune_out && pending >= 0 ? &prune_out[pending] : nullptr, who))) return rc;
    guard.ok = true;
    return first_err;
}

// Not part of icp_hip.h (tools/time_vmap_prune.py): the device time of ONE prune of the map about `centre` between two events (with a
// radius that removes nothing the map is left as it was), and of one compaction of a hashed map into a table of the same size.
extern "C" int icp_debug_vmap_prune_time(icp_ctx* c, const float centre[3], float radius, float* ms_out) {
    if (!c || !centre || !ms_out) return ICP_ERR_INVALID_ARG;
    int rc;
    if ((rc = vmap_check(c, "icp_debug_vmap_prune_time"))) return rc;
    DrainOnError guard(c);
    if ((rc = set_device(c))) return rc;
    HIPCK(c, hipStreamSynchronize(c->stream));
    if ((rc = timed_ms(c, ms_out, [&] { return vmap_prune_enqueue(c, centre, radius * radius); }))) return rc;
    return guard.done();
}
extern "C" int icp_debug_hmap_compact_time(icp_ctx* c, float* ms_out) {
    if (!c || !ms_out) return ICP_ERR_INVALID_ARG;
    int rc;
    if ((rc = hmap_check(c, "icp_debug_hmap_compact_time"))) return rc;
    DrainOnError guard(c);
    if ((rc = set_device(c))) return rc;
    HIPCK(c, hipStreamSynchronize(c->stream));
    if ((rc = timed_ms(c, ms_out, [&] { return hmap_rehash(c, c->vh_log2cap, true); }))) return rc;
    return guard.done();
}
