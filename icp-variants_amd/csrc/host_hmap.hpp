// host_hmap.hpp -- the hashed storage of the voxel map: icp_voxel_map_create_hashed / reserve / upload_hashed, icp_get_voxel_map_hashed, and
// what host_vmap.hpp's entry points call when the context's map is hashed (the insert with its room rule, the plan of an alignment, the
// growth).  Kernels: dev_hmap.hpp.  Contract: include/icp_hip.h, DESIGN.md section 6u.  Part of icp_hip.hip (included from there, after
// host_vgicp.hpp and before host_vmap.hpp).
namespace {
constexpr int HM_MIN_LOG2 = 8, HM_MAX_LOG2 = 26;
// log2 of the smallest table of at least `capacity` slots (2^8 at least), or -1 beyond 2^26
int hm_log2_for(long long capacity) {
    int l = HM_MIN_LOG2;
    while (l <= HM_MAX_LOG2 && (1ll << l) < capacity) l++;
    return l <= HM_MAX_LOG2 ? l : -1;
}
const char* hmap_create_error(float voxel_size, int32_t capacity) {
    if (!(std::isfinite(voxel_size) && voxel_size > 0.f)) return "voxel_size must be finite and > 0";
    if (capacity < 1) return "capacity must be >= 1";
    if (capacity > (1 << HM_MAX_LOG2)) return "capacity must be at most 2^26 slots";
    return nullptr;
}
int hmap_check(icp_ctx* c, const char* who) {
    if (!c->vm_on) { c->err = std::string(who) + ": no voxel map (icp_voxel_map_create_hashed)"; return ICP_ERR_INVALID_ARG; }
    if (!c->vm_hashed) { c->err = std::string(who) + ": the voxel map is dense (icp_voxel_map_create): use icp_get_voxel_map / icp_voxel_map_upload"; return ICP_ERR_INVALID_ARG; }
    return ICP_OK;
}
size_t hm_cap(const icp_ctx* c) { return (size_t)1 << c->vh_log2cap; }
struct HmBufs { DevBuf keys, count, sums, cells, stamp; };
// a cleared table of 2^log2cap slots: every key empty, every count, sum, record and stamp 0 (enqueued)
int hmap_alloc(icp_ctx* c, int log2cap, HmBufs& b) {
    const size_t n = (size_t)1 << log2cap;
    int rc;
    if ((rc = ensure(c, b.keys, n * 8))) return rc;
    if ((rc = ensure(c, b.count, n * 4))) return rc;
    if ((rc = ensure(c, b.sums, n * VG_NSUM * 8))) return rc;
    if ((rc = ensure(c, b.cells, n * 40))) return rc;
    if ((rc = ensure(c, b.stamp, n * 4))) return rc;
    HIPCK(c, hipMemsetAsync(b.keys.p, 0xFF, n * 8, c->stream));
    HIPCK(c, hipMemsetAsync(b.count.p, 0, n * 4, c->stream));
    HIPCK(c, hipMemsetAsync(b.sums.p, 0, n * VG_NSUM * 8, c->stream));
    HIPCK(c, hipMemsetAsync(b.cells.p, 0, n * 40, c->stream));
    HIPCK(c, hipMemsetAsync(b.stamp.p, 0, n * 4, c->stream));
    return ICP_OK;
}
void hmap_adopt(icp_ctx* c, int log2cap, HmBufs& b) {
    c->vh_keys = std::move(b.keys); c->vm_count = std::move(b.count); c->vm_sums = std::move(b.sums); c->vm_cells = std::move(b.cells); c->vm_stamp = std::move(b.stamp);
    c->vh_log2cap = log2cap;
}
// Growth: a cleared table of 2^log2cap slots, k_hmap_rehash over the old one, and the old one freed once the kernel has finished.
// compact: k_hmap_compact in its place, which leaves the slots without points behind (section 6v); the vacated count goes back to 0.
int hmap_rehash(icp_ctx* c, int log2cap, bool compact = false) {
    int rc;
    HmBufs b;
    if ((rc = hmap_alloc(c, log2cap, b))) return rc;
    const int old_cap = (int)hm_cap(c);
    if (compact) {
        hipLaunchKernelGGL(k_hmap_compact, dim3((old_cap + 255) / 256), dim3(256), 0, c->stream, old_cap, (const unsigned long long*)c->vh_keys.as<unsigned long long>(),
                           (const int*)c->vm_count.as<int>(), (const long long*)c->vm_sums.as<long long>(), (const float2*)c->vm_cells.as<float2>(),
                           b.keys.as<unsigned long long>(), log2cap, b.count.as<int>(), b.sums.as<long long>(), b.cells.as<float2>(), c->vm_ctr.as<int>());
        HIPCK(c, hipGetLastError());
        HIPCK(c, hipMemsetAsync(c->vm_ctr.as<int>() + VM_VACATED, 0, 4, c->stream));
        HIPCK(c, hipStreamSynchronize(c->stream));
        if (log2cap > c->vh_log2cap) c->vh_grown++;
        hmap_adopt(c, log2cap, b);
        c->vh_compacted++; c->vh_vac = false; c->vh_vac_bound = 0;
        return ICP_OK;
    }
    hipLaunchKernelGGL(k_hmap_rehash, dim3((old_cap + 255) / 256), dim3(256), 0, c->stream, old_cap, (const unsigned long long*)c->vh_keys.as<unsigned long long>(),
                       (const int*)c->vm_count.as<int>(), (const long long*)c->vm_sums.as<long long>(), (const float2*)c->vm_cells.as<float2>(),
                       b.keys.as<unsigned long long>(), log2cap, b.count.as<int>(), b.sums.as<long long>(), b.cells.as<float2>(), c->vm_ctr.as<int>());
    HIPCK(c, hipGetLastError());
    HIPCK(c, hipStreamSynchronize(c->stream));
    hmap_adopt(c, log2cap, b);
    c->vh_grown++;
    return ICP_OK;
}
// The room rule: capacity >= 2 (occupied + vacated + n) before n points (or entries) go in.  `occupied` and `vacated` are the host's bounds
// (vacated is 0 on a map that was never pruned, and then this is the rule of section 6u, read for read); when the bounds fail the true
// counts are read in one copy, and when those fail too the table is doubled until it holds (nothing vacated) or compacted into the smallest
// table of at least this capacity with 2 (occupied + n) <= 0.75 capacity (section 6v).  Past 2^26: refused, nothing modified.
int hmap_read_vacated(icp_ctx* c) {
    int t[3], rc;
    if ((rc = read_count(c, c->vm_ctr.as<int>() + VM_OCCUPIED, t, 3))) return rc;
    c->vh_bound = t[0]; c->vh_vac_bound = t[2]; c->vh_vac = t[2] > 0;
    return ICP_OK;
}
int hmap_room(icp_ctx* c, long long n, const char* who) {
    int rc;
    if (2 * (c->vh_bound + c->vh_vac_bound + n) > (long long)hm_cap(c)) {
        if (c->vh_vac) { if ((rc = hmap_read_vacated(c))) return rc; }
        else {
            int occ = 0;
            if ((rc = read_count(c, c->vm_ctr.as<int>() + VM_OCCUPIED, &occ))) return rc;
            c->vh_bound = occ;
        }
    }
    if (2 * (c->vh_bound + c->vh_vac_bound + n) <= (long long)hm_cap(c)) return ICP_OK;
    const long long need = 2 * (c->vh_bound + n);
    int l = hm_log2_for(need);
    if (c->vh_vac_bound > 0) {                         // (exact by now) compaction, with hysteresis
        l = c->vh_log2cap;
        while (l <= HM_MAX_LOG2 && 4 * need > 3 * (1ll << l)) l++;
        if (l > HM_MAX_LOG2) l = -1;
    }
    if (l < 0) {
        char buf[224];
        snprintf(buf, sizeof(buf), "%s: %lld occupied cells and %lld more points need a table of more than 2^26 slots (capacity >= 2 (occupied + points))", who, c->vh_bound, n);
        c->err = buf; return ICP_ERR_INVALID_ARG;
    }
    return hmap_rehash(c, l, c->vh_vac_bound > 0);
}
// the counter that must stay 0
int hmap_unplaced_error(icp_ctx* c, int n_unplaced, const char* who) {
    if (n_unplaced == 0) return ICP_OK;
    char buf[160];
    snprintf(buf, sizeof(buf), "%s: %d points found no slot in the hashed voxel map (the room rule was broken)", who, n_unplaced);
    c->err = buf; return ICP_ERR_HIP;
}
// vmap_insert_enqueue for a hashed map: the room rule (which may read 4 bytes and may grow the table), then the two launches.
int hmap_insert_enqueue(icp_ctx* c, int which, const float pose[16], const char* who) {
    const Cloud& cl = which ? c->src : c->tgt;
    int rc;
    if ((rc = hmap_room(c, cl.n, who))) return rc;
    const size_t cap = hm_cap(c);
    if (c->vm_serial == INT_MAX) {
        HIPCK(c, hipMemsetAsync(c->vm_stamp.p, 0, cap * 4, c->stream));
        c->vm_serial = 0;
    }
    const int serial = ++c->vm_serial;
    VmCloud t;
    t.x = cl.x.as<float>(); t.y = cl.y.as<float>(); t.z = cl.z.as<float>(); t.n = cl.n;
    vg_normals(c, which, &t.nx, &t.ny, &t.nz);
    const int list_cap = (size_t)cl.n < cap ? cl.n : (int)cap;
    if ((rc = ensure(c, c->vm_list, (size_t)list_cap * 4))) return rc;
    int* ctr = c->vm_ctr.as<int>();
    HIPCK(c, hipMemsetAsync(ctr, 0, VM_OCCUPIED * 4, c->stream));
    TsdfMat m; memcpy(m.m, pose, 64);
    const float vs = c->vm_opt.voxel_size;
    hipLaunchKernelGGL(k_hmap_insert, dim3((cl.n + 255) / 256), dim3(256), 0, c->stream, t, c->vh_keys.as<unsigned long long>(), c->vh_log2cap, vs, m, serial, list_cap,
                       c->vm_count.as<int>(), c->vm_sums.as<unsigned long long>(), c->vm_stamp.as<int>(), c->vm_list.as<int>(), ctr);
    hipLaunchKernelGGL(k_hmap_records, dim3((list_cap + 255) / 256), dim3(256), 0, c->stream, (const unsigned long long*)c->vh_keys.as<unsigned long long>(), vs, list_cap,
                       (const int*)ctr, (const int*)c->vm_list.as<int>(), (const int*)c->vm_count.as<int>(), (const long long*)c->vm_sums.as<long long>(), c->vm_cells.as<float2>());
    HIPCK(c, hipGetLastError());
    c->vh_bound += cl.n;
    return ICP_OK;
}
// what vmap_plan sets for a hashed map in place of the extent
void hmap_plan(const icp_ctx* c, int min_points, VgPlan* pl) {
    pl->h.keys = c->vh_keys.as<unsigned long long>(); pl->h.log2cap = c->vh_log2cap; pl->h.vs = c->vm_opt.voxel_size; pl->h.min_points = min_points;
}
// The occupied and the unplaced counters (7 words of the map's counters are read; the first six are the last insert's info): waits.
int hmap_read_counters(icp_ctx* c, int* info6, const char* who) {
    int h[7], rc;
    if ((rc = read_count(c, c->vm_ctr.p, h, 7))) return rc;
    if (info6) memcpy(info6, h, 24);
    c->vh_bound = h[VM_OCCUPIED];
    return hmap_unplaced_error(c, h[VM_UNPLACED], who);
}
// sdf_read_record with the map's occupied and unplaced counters read in the SAME wait (icp_track_scans_vmap on a hashed map: the previous
// insert has finished by then, so the count is exact and the next insert's room rule needs no wait of its own).
int hmap_read_record(icp_ctx* c, const icp_sdf_options& so, icp_sdf_frame* r, const char* who) {
    int rc;
    if ((rc = ensure_pinned(c, 4096 + sizeof(icp_sdf_frame)))) return rc;      // (sdf_read_record's block, grown first: it must not move under the copy below)
    int* h = (int*)(c->pinned.as<char>() + 2032);      // (the 16 bytes in front of the record's place)
    HIPCK(c, hipMemcpyAsync(h, c->vm_ctr.as<int>() + VM_OCCUPIED, 8, hipMemcpyDeviceToHost, c->stream));
    if ((rc = sdf_read_record<SdfGeo>(c, so, r, nullptr))) return rc;
    c->vh_bound = h[0];
    return hmap_unplaced_error(c, h[1], who);
}
}  // namespace

int icp_voxel_map_create_hashed(icp_ctx* c, float voxel_size, int32_t capacity) {
    if (!c) return ICP_ERR_INVALID_ARG;
    if (const char* why = hmap_create_error(voxel_size, capacity)) { c->err = std::string("icp_voxel_map_create_hashed: ") + why; return ICP_ERR_INVALID_ARG; }
    int rc;
    DrainOnError guard(c);
    if ((rc = set_device(c))) return rc;
    c->vm_on = false;
    HIPCK(c, hipStreamSynchronize(c->stream));
    const int l = hm_log2_for(capacity);
    HmBufs b;
    if ((rc = hmap_alloc(c, l, b))) return rc;
    if ((rc = ensure(c, c->vm_ctr, VM_CTR_WORDS * 4))) return rc;
    HIPCK(c, hipMemsetAsync(c->vm_ctr.p, 0, VM_NCTR * 4, c->stream));
    HIPCK(c, hipStreamSynchronize(c->stream));
    hmap_adopt(c, l, b);
    c->vm_opt.voxel_size = voxel_size;
    for (int a = 0; a < 3; a++) { c->vm_opt.lo[a] = 0; c->vm_opt.dims[a] = 0; }
    c->vm_serial = 0; c->vh_grown = 0; c->vh_bound = 0; c->vh_vac = false; c->vh_compacted = 0; c->vh_vac_bound = 0; c->vm_hashed = true; c->vm_on = true;
    return guard.done();
}

int icp_voxel_map_reserve(icp_ctx* c, int32_t capacity) {
    if (!c) return ICP_ERR_INVALID_ARG;
    const char* who = "icp_voxel_map_reserve";
    int rc;
    if ((rc = hmap_check(c, who))) return rc;
    if (capacity < 1 || capacity > (1 << HM_MAX_LOG2)) { c->err = std::string(who) + ": capacity must be in 1 .. 2^26"; return ICP_ERR_INVALID_ARG; }
    const int l = hm_log2_for(capacity);
    if (l <= c->vh_log2cap) return ICP_OK;
    DrainOnError guard(c);
    if ((rc = set_device(c))) return rc;
    if (c->vh_vac && (rc = hmap_read_vacated(c))) return rc;      // (a pruned map: compacted on the way when slots are vacated)
    if ((rc = hmap_rehash(c, l, c->vh_vac))) return rc;
    if ((rc = hmap_read_counters(c, nullptr, who))) return rc;
    return guard.done();
}

int icp_get_voxel_map_hashed(icp_ctx* c, icp_voxel_hash_map_info* info_out, int32_t max_entries, int32_t* coords_out, int32_t* counts_out, int64_t* sums_out, float* cells_out) {
    if (!c) return ICP_ERR_INVALID_ARG;
    const char* who = "icp_get_voxel_map_hashed";
    int rc;
    if ((rc = hmap_check(c, who))) return rc;
    DrainOnError guard(c);
    if ((rc = set_device(c))) return rc;
    int tail[2];
    if ((rc = read_count(c, c->vm_ctr.as<int>() + VM_OCCUPIED, tail, 2))) return rc;
    c->vh_bound = tail[0];
    if (info_out) {
        memset(info_out, 0, sizeof(*info_out));
        info_out->voxel_size = c->vm_opt.voxel_size; info_out->capacity = (int32_t)hm_cap(c); info_out->n_occupied = tail[0]; info_out->n_grown = c->vh_grown; info_out->n_unplaced = tail[1];
    }
    if (!coords_out && !counts_out && !sums_out && !cells_out) return guard.done();
    if (max_entries < tail[0]) {
        char buf[160];
        snprintf(buf, sizeof(buf), "%s: max_entries %d is below the %d occupied cells", who, max_entries, tail[0]);
        c->err = buf; return ICP_ERR_INVALID_ARG;
    }
    // a save path: the slots to the host, then compacted and sorted by key
    const size_t cap = hm_cap(c);
    std::vector<unsigned long long> keys(cap);
    const bool want_cnt = counts_out || c->vh_vac;      // (a vacated slot has a key and no points: it is no entry)
    std::vector<int32_t> cnt(want_cnt ? cap : 0);
    std::vector<int64_t> sm(sums_out ? cap * VG_NSUM : 0);
    std::vector<float> rec(cells_out ? cap * 10 : 0);
    HIPCK(c, hipMemcpyAsync(keys.data(), c->vh_keys.p, cap * 8, hipMemcpyDeviceToHost, c->stream));
    if (want_cnt) HIPCK(c, hipMemcpyAsync(cnt.data(), c->vm_count.p, cap * 4, hipMemcpyDeviceToHost, c->stream));
    if (sums_out) HIPCK(c, hipMemcpyAsync(sm.data(), c->vm_sums.p, cap * VG_NSUM * 8, hipMemcpyDeviceToHost, c->stream));
    if (cells_out) HIPCK(c, hipMemcpyAsync(rec.data(), c->vm_cells.p, cap * 40, hipMemcpyDeviceToHost, c->stream));
    HIPCK(c, hipStreamSynchronize(c->stream));
    std::vector<std::pair<unsigned long long, uint32_t>> occ;
    occ.reserve((size_t)tail[0]);
    for (size_t i = 0; i < cap; i++) if (keys[i] != HM_EMPTY && (!c->vh_vac || cnt[i] > 0)) occ.emplace_back(keys[i], (uint32_t)i);
    if (occ.size() != (size_t)tail[0]) { c->err = std::string(who) + ": the table's keys and its occupied count disagree"; return ICP_ERR_HIP; }
    std::sort(occ.begin(), occ.end());
    for (size_t e = 0; e < occ.size(); e++) {
        const unsigned long long k = occ[e].first; const size_t i = occ[e].second;
        if (coords_out) for (int a = 0; a < 3; a++) coords_out[3 * e + a] = (int32_t)((k >> (21 * a)) & 0x1FFFFFull) - HM_RANGE;
        if (counts_out) counts_out[e] = cnt[i];
        if (sums_out) memcpy(sums_out + e * VG_NSUM, sm.data() + i * VG_NSUM, VG_NSUM * 8);
        if (cells_out) memcpy(cells_out + e * 9, rec.data() + i * 10, 36);
    }
    return guard.done();
}

int icp_voxel_map_upload_hashed(icp_ctx* c, int32_t n, const int32_t* coords, const int32_t* counts, const int64_t* sums) {
    if (!c) return ICP_ERR_INVALID_ARG;
    const char* who = "icp_voxel_map_upload_hashed";
    int rc;
    if ((rc = hmap_check(c, who))) return rc;
    if (n < 0 || (n > 0 && (!coords || !counts || !sums))) { c->err = std::string(who) + ": bad argument (n >= 0, coords, counts, sums)"; return ICP_ERR_INVALID_ARG; }
    std::vector<unsigned long long> keys((size_t)n);
    for (int i = 0; i < n; i++) {
        if (counts[i] < 0) { c->err = std::string(who) + ": a count is negative"; return ICP_ERR_INVALID_ARG; }
        unsigned long long k = 0;
        for (int a = 0; a < 3; a++) {
            const int32_t v = coords[3 * (size_t)i + a];
            if (v < -HM_RANGE || v >= HM_RANGE) { c->err = std::string(who) + ": a coordinate is not storable (-2^20 <= c < 2^20)"; return ICP_ERR_INVALID_ARG; }
            k |= (unsigned long long)(uint32_t)(v + HM_RANGE) << (21 * a);
        }
        keys[(size_t)i] = k;
    }
    std::sort(keys.begin(), keys.end());
    if (std::adjacent_find(keys.begin(), keys.end()) != keys.end()) { c->err = std::string(who) + ": a coordinate occurs twice"; return ICP_ERR_INVALID_ARG; }
    const int l = hm_log2_for(2ll * n);
    if (l < 0) { c->err = std::string(who) + ": n entries need a table of more than 2^26 slots (capacity >= 2 n)"; return ICP_ERR_INVALID_ARG; }
    DrainOnError guard(c);
    if ((rc = set_device(c))) return rc;
    // the state is REPLACED: the table cleared, grown where 2 n slots need it, then the entries placed
    HIPCK(c, hipStreamSynchronize(c->stream));
    HmBufs b;
    const int log2cap = l > c->vh_log2cap ? l : c->vh_log2cap;
    if (log2cap > c->vh_log2cap) c->vh_grown++;
    if ((rc = hmap_alloc(c, log2cap, b))) return rc;
    HIPCK(c, hipMemsetAsync(c->vm_ctr.p, 0, VM_NCTR * 4, c->stream));
    HIPCK(c, hipStreamSynchronize(c->stream));
    hmap_adopt(c, log2cap, b);
    c->vm_serial = 0; c->vh_bound = n; c->vh_vac = false; c->vh_vac_bound = 0;
    if (n > 0) {
        DevBuf up;
        const size_t b_xyz = (size_t)n * 12, b_cnt = (size_t)n * 4, b_sum = (size_t)n * VG_NSUM * 8;
        if ((rc = ensure(c, up, b_sum + b_xyz + b_cnt))) return rc;
        char* d = up.as<char>();
        HIPCK(c, hipMemcpyAsync(d, sums, b_sum, hipMemcpyHostToDevice, c->stream));
        HIPCK(c, hipMemcpyAsync(d + b_sum, coords, b_xyz, hipMemcpyHostToDevice, c->stream));
        HIPCK(c, hipMemcpyAsync(d + b_sum + b_xyz, counts, b_cnt, hipMemcpyHostToDevice, c->stream));
        hipLaunchKernelGGL(k_hmap_place, dim3((n + 255) / 256), dim3(256), 0, c->stream, n, (const int*)(d + b_sum), (const int*)(d + b_sum + b_xyz), (const long long*)d,
                           c->vm_opt.voxel_size, c->vh_keys.as<unsigned long long>(), c->vh_log2cap, c->vm_count.as<int>(), c->vm_sums.as<long long>(), c->vm_cells.as<float2>(),
                           c->vm_ctr.as<int>());
        HIPCK(c, hipGetLastError());
        if ((rc = hmap_read_counters(c, nullptr, who))) return rc;      // (waits: `up` is free to go)
    }
    return guard.done();
}

// Not part of icp_hip.h (tools/time_hmap.py): icp_debug_vmap_time's two figures for whichever storage the map has (host_vmap.hpp calls
// this for a hashed map), and the device time of one rehash of the map into a table of the same size (a tool's map: n_grown goes up).
static int hmap_debug_time(icp_ctx* c, int32_t which, const float pose[16], float* insert_ms_out, float* records_ms_out, const char* who) {
    int rc;
    if ((rc = hmap_insert_enqueue(c, which, pose, who))) return rc;
    HIPCK(c, hipStreamSynchronize(c->stream));
    if ((rc = hmap_room(c, (which ? c->src : c->tgt).n, who))) return rc;      // (so that the timed insert neither reads nor grows)
    if ((rc = timed_ms(c, insert_ms_out, [&] { return hmap_insert_enqueue(c, which, pose, who); }))) return rc;
    const Cloud& cl = which ? c->src : c->tgt;
    const size_t cap = hm_cap(c);
    const int list_cap = (size_t)cl.n < cap ? cl.n : (int)cap;
    return timed_ms(c, records_ms_out, [&] {
        hipLaunchKernelGGL(k_hmap_records, dim3((list_cap + 255) / 256), dim3(256), 0, c->stream, (const unsigned long long*)c->vh_keys.as<unsigned long long>(), c->vm_opt.voxel_size, list_cap,
                           (const int*)c->vm_ctr.as<int>(), (const int*)c->vm_list.as<int>(), (const int*)c->vm_count.as<int>(), (const long long*)c->vm_sums.as<long long>(), c->vm_cells.as<float2>());
        return ICP_OK;
    });
}
extern "C" int icp_debug_hmap_rehash_time(icp_ctx* c, float* rehash_ms_out) {
    if (!c || !rehash_ms_out) return ICP_ERR_INVALID_ARG;
    int rc;
    if ((rc = hmap_check(c, "icp_debug_hmap_rehash_time"))) return rc;
    DrainOnError guard(c);
    if ((rc = set_device(c))) return rc;
    HIPCK(c, hipStreamSynchronize(c->stream));
    if ((rc = timed_ms(c, rehash_ms_out, [&] { return hmap_rehash(c, c->vh_log2cap); }))) return rc;
    return guard.done();
}
