// host_tsdf_hash_evict.hpp -- streaming the hashed TSDF volume: icp_tsdf_evict_blocks (the blocks beyond a radius leave the pool, into an
// outbox the host fetches with icp_tsdf_evicted_blocks) and icp_tsdf_insert_blocks (blocks from the host join the resident ones).
// Kernels: dev_tsdf_hash_evict.hpp; the room rule, the rehash and the save path: host_tsdf_hash.hpp.  Contract: include/icp_hip.h,
// DESIGN.md section 6za; a coloured hashed volume streams its colour pool by the same plan (icp_tsdf_evicted_blocks_color,
// icp_tsdf_insert_blocks_color: section 6zb).  Part of icp_hip.hip (included from there, after host_tsdf_hash.hpp).
namespace {
// An evict's working set in ONE buffer: the counters (a 256-byte line of their own), the lists of evicted blocks, holes and movers (n ints
// each), the keep flags (n bytes).
struct HeWork { int* ec; int* evicted; int* holes; int* movers; uint8_t* keep; };
int htsdf_evict_work(icp_ctx* c, int n, HeWork& w) {
    int rc;
    if ((rc = ensure(c, c->te_work, 256 + (size_t)n * 13))) return rc;
    char* p = c->te_work.as<char>();
    w.ec = (int*)p; w.evicted = (int*)(p + 256); w.holes = w.evicted + n; w.movers = w.holes + n; w.keep = (uint8_t*)(w.movers + n);
    return ICP_OK;
}
void htsdf_stream_info(const icp_ctx* c, icp_tsdf_stream_info* o) {
    memset(o, 0, sizeof(*o));
    o->n_blocks = c->th_nblk; o->capacity = c->th_pool_cap; o->n_held = c->te_held; o->n_grown = c->th_grown;
}
}  // namespace

int icp_tsdf_evict_blocks(icp_ctx* c, const float centre[3], float radius, int32_t hold, icp_tsdf_stream_info* info_out) {
    if (!c) return ICP_ERR_INVALID_ARG;
    const char* who = "icp_tsdf_evict_blocks";
    int rc;
    if ((rc = htsdf_check(c, who))) return rc;
    if (!centre || !(std::isfinite(centre[0]) && std::isfinite(centre[1]) && std::isfinite(centre[2]))) { c->err = std::string(who) + ": centre must be three finite numbers"; return ICP_ERR_INVALID_ARG; }
    if (!(std::isfinite(radius) && radius >= 0.f)) { c->err = std::string(who) + ": radius must be finite and >= 0"; return ICP_ERR_INVALID_ARG; }
    DrainOnError guard(c);
    if ((rc = set_device(c))) return rc;
    c->te_held = 0;                                    // (the previous evict's outbox ends here)
    if (info_out) htsdf_stream_info(c, info_out);
    const int n = c->th_nblk;
    if (n == 0) return guard.done();
    HeWork w;
    if ((rc = htsdf_evict_work(c, n, w))) return rc;
    const icp_tsdf_options& o = c->tsdf_opt;
    const HtSphere q = {centre[0], centre[1], centre[2], radius * radius, o.origin[0], o.origin[1], o.origin[2], o.voxel_size};
    HIPCK(c, hipMemsetAsync(w.ec, 0, HE_NCTR * 4, c->stream));
    hipLaunchKernelGGL(k_htsdf_evict_mark, dim3((n + 255) / 256), dim3(256), 0, c->stream, n, (const unsigned long long*)c->th_pkey.as<unsigned long long>(), q, w.keep, w.evicted, w.ec);
    HIPCK(c, hipGetLastError());
    // the one read that decides everything else: the launch sizes, the tail clear, and the early return
    int h[2];
    if ((rc = read_count(c, w.ec, h, 2))) return rc;
    const int n_keep = h[HE_KEEP], n_ev = h[HE_EVICT];
    if (n_keep + n_ev != n) { c->err = std::string(who) + ": the mark's counters do not add up"; return ICP_ERR_HIP; }
    if (n_ev == 0) return guard.done();               // nothing leaves: nothing at all is modified
    float2* pool = c->th_pool.as<float2>();
    unsigned long long* pkey = c->th_pkey.as<unsigned long long>();
    int* h_moved = nullptr;
    if ((rc = count_slot(c, &h_moved))) return rc;      // (everything that can fail for want of memory comes before the first store)
    if (hold) {
        if ((rc = ensure(c, c->te_out_pool, (size_t)n_ev * 4096))) return rc;
        if ((rc = ensure(c, c->te_out_key, (size_t)n_ev * 8))) return rc;
        if (c->th_color && (rc = ensure(c, c->te_out_cpool, (size_t)n_ev * 8192))) return rc;
        hipLaunchKernelGGL(k_htsdf_evict_out, dim3(n_ev), dim3(512), 0, c->stream, (const float2*)pool, (const unsigned long long*)pkey, (const int*)w.evicted,
                           c->te_out_pool.as<float2>(), c->te_out_key.as<unsigned long long>());
        if (c->th_color) hipLaunchKernelGGL(k_htsdf_evict_out_color, dim3(n_ev), dim3(512), 0, c->stream, (const float4*)c->th_cpool.as<float4>(), (const int*)w.evicted,
                                            c->te_out_cpool.as<float4>());
        HIPCK(c, hipGetLastError());
    }
    // compaction by minimal move: the kept blocks at or above n_keep into the holes below it (as many of the one as of the other)
    const int n_bound = n_keep < n_ev ? n_keep : n_ev;
    *h_moved = 0;
    if (n_bound > 0) {
        hipLaunchKernelGGL(k_htsdf_evict_plan, dim3((n + 255) / 256), dim3(256), 0, c->stream, n, n_keep, (const uint8_t*)w.keep, w.holes, w.movers, w.ec);
        hipLaunchKernelGGL(k_htsdf_evict_move, dim3(n_bound), dim3(512), 0, c->stream, pool, pkey, (const int*)w.holes, (const int*)w.movers, (const int*)w.ec);
        if (c->th_color) hipLaunchKernelGGL(k_htsdf_evict_move_color, dim3(n_bound), dim3(512), 0, c->stream, c->th_cpool.as<float4>(), (const int*)w.holes, (const int*)w.movers,
                                            (const int*)w.ec);      // (a mover's colours into the hole its geometry went into)
        HIPCK(c, hipGetLastError());
        HIPCK(c, hipMemcpyAsync(h_moved, w.ec + HE_MOVERS, 4, hipMemcpyDeviceToHost, c->stream));
    }
    // the tail as htsdf_alloc leaves it, so that a later touch hands out fresh blocks; the table cleared and rebuilt over the kept blocks
    HIPCK(c, hipMemsetAsync(c->th_pool.as<char>() + (size_t)n_keep * 4096, 0, (size_t)n_ev * 4096, c->stream));
    HIPCK(c, hipMemsetAsync(pkey + n_keep, 0xFF, (size_t)n_ev * 8, c->stream));
    if (c->th_color) HIPCK(c, hipMemsetAsync(c->th_cpool.as<char>() + (size_t)n_keep * 8192, 0, (size_t)n_ev * 8192, c->stream));
    const size_t slots = (size_t)1 << c->th_log2cap;
    HIPCK(c, hipMemsetAsync(c->th_keys.p, 0xFF, slots * 8, c->stream));
    HIPCK(c, hipMemsetAsync(c->th_vals.p, 0xFF, slots * 4, c->stream));
    if ((rc = htsdf_rehash_launch(c, n_keep, c->th_keys.as<unsigned long long>(), c->th_vals.as<int>(), (const unsigned long long*)pkey, c->th_log2cap))) return rc;
    if ((rc = htsdf_set_counters(c, n_keep))) return rc;      // (the second wait; n_moved comes with it)
    c->th_nblk = n_keep; c->th_unplaced = 0;
    if (hold) c->te_held = n_ev;
    if (info_out) {
        info_out->n_evicted = n_ev; info_out->n_blocks = n_keep; info_out->n_moved = *h_moved; info_out->n_held = c->te_held;
    }
    return guard.done();
}

namespace {
int htsdf_evicted(icp_ctx* c, int32_t max_blocks, int32_t* coords_out, float* tsdf_out, float* weight_out, float* rgb_out, float* cweight_out, const char* who);
int htsdf_insert(icp_ctx* c, int32_t n, const int32_t* coords, const float* tsdf, const float* weight, const float* rgb, const float* cweight, icp_tsdf_stream_info* info_out,
                 const char* who);
}  // namespace
int icp_tsdf_evicted_blocks(icp_ctx* c, int32_t max_blocks, int32_t* coords_out, float* tsdf_out, float* weight_out) {
    if (!c) return ICP_ERR_INVALID_ARG;
    int rc;
    if ((rc = htsdf_check(c, "icp_tsdf_evicted_blocks"))) return rc;
    return htsdf_evicted(c, max_blocks, coords_out, tsdf_out, weight_out, nullptr, nullptr, "icp_tsdf_evicted_blocks");      // (a coloured volume: the outbox's geometry)
}
int icp_tsdf_evicted_blocks_color(icp_ctx* c, int32_t max_blocks, int32_t* coords_out, float* tsdf_out, float* weight_out, float* rgb_out, float* cweight_out) {
    if (!c) return ICP_ERR_INVALID_ARG;
    int rc;
    if ((rc = htsdf_check_color(c, "icp_tsdf_evicted_blocks_color"))) return rc;
    return htsdf_evicted(c, max_blocks, coords_out, tsdf_out, weight_out, rgb_out, cweight_out, "icp_tsdf_evicted_blocks_color");
}
namespace {
int htsdf_evicted(icp_ctx* c, int32_t max_blocks, int32_t* coords_out, float* tsdf_out, float* weight_out, float* rgb_out, float* cweight_out, const char* who) {
    int rc;
    const int n = c->te_held;
    if (!coords_out && !tsdf_out && !weight_out && !rgb_out && !cweight_out) return ICP_OK;
    if (max_blocks < n) {
        char buf[160];
        snprintf(buf, sizeof(buf), "%s: max_blocks %d is below the %d held blocks", who, max_blocks, n);
        c->err = buf; return ICP_ERR_INVALID_ARG;
    }
    if (n == 0) return ICP_OK;
    if ((rc = set_device(c))) return rc;
    return htsdf_download_sorted(c, n, c->te_out_key.p, c->te_out_pool.p, coords_out, tsdf_out, weight_out, c->th_color ? c->te_out_cpool.p : nullptr, rgb_out, cweight_out);
}
}  // namespace

int icp_tsdf_insert_blocks(icp_ctx* c, int32_t n, const int32_t* coords, const float* tsdf, const float* weight, icp_tsdf_stream_info* info_out) {
    if (!c) return ICP_ERR_INVALID_ARG;
    const char* who = "icp_tsdf_insert_blocks";
    int rc;
    if ((rc = htsdf_check(c, who))) return rc;
    if (info_out) htsdf_stream_info(c, info_out);
    if (n < 0 || (n > 0 && (!coords || !tsdf || !weight))) { c->err = std::string(who) + ": bad argument (n >= 0, coords, tsdf, weight)"; return ICP_ERR_INVALID_ARG; }
    return htsdf_insert(c, n, coords, tsdf, weight, nullptr, nullptr, info_out, who);      // (a coloured volume: the new blocks uncoloured, the pool's tail is clear)
}
int icp_tsdf_insert_blocks_color(icp_ctx* c, int32_t n, const int32_t* coords, const float* tsdf, const float* weight, const float* rgb, const float* cweight,
                                 icp_tsdf_stream_info* info_out) {
    if (!c) return ICP_ERR_INVALID_ARG;
    const char* who = "icp_tsdf_insert_blocks_color";
    int rc;
    if ((rc = htsdf_check_color(c, who))) return rc;
    if (info_out) htsdf_stream_info(c, info_out);
    if (n < 0 || (n > 0 && (!coords || !tsdf || !weight || !rgb || !cweight))) { c->err = std::string(who) + ": bad argument (n >= 0, coords, tsdf, weight, rgb, cweight)"; return ICP_ERR_INVALID_ARG; }
    return htsdf_insert(c, n, coords, tsdf, weight, rgb, cweight, info_out, who);
}
namespace {
int htsdf_insert(icp_ctx* c, int32_t n, const int32_t* coords, const float* tsdf, const float* weight, const float* rgb, const float* cweight, icp_tsdf_stream_info* info_out,
                 const char* who) {
    int rc;
    if ((rc = htsdf_check_coords(c, n, coords, who))) return rc;
    if (!htsdf_keys_distinct(n, coords)) { c->err = std::string(who) + ": a block coordinate occurs twice"; return ICP_ERR_INVALID_ARG; }
    if (n == 0) return ICP_OK;
    DrainOnError guard(c);
    if ((rc = set_device(c))) return rc;
    // the keys that are resident already, counted on the device: one of them refuses the call before anything is modified
    DevBuf d_coords;
    if ((rc = ensure(c, d_coords, (size_t)n * 12))) return rc;
    HIPCK(c, hipMemcpyAsync(d_coords.p, coords, (size_t)n * 12, hipMemcpyHostToDevice, c->stream));
    int* d_present = c->tsdf_cnt.as<int>();
    HIPCK(c, hipMemsetAsync(d_present, 0, 4, c->stream));
    hipLaunchKernelGGL(k_htsdf_present, dim3((n + 255) / 256), dim3(256), 0, c->stream, htsdf_view(c), (int)n, (const int*)d_coords.as<int>(), d_present);
    HIPCK(c, hipGetLastError());
    int n_present = 0;
    if ((rc = read_count(c, d_present, &n_present))) return rc;
    if (n_present > 0) {
        if (info_out) info_out->n_present = n_present;
        char buf[192];
        snprintf(buf, sizeof(buf), "%s: %d of the %d blocks are resident already: nothing modified (icp_tsdf_upload_hashed replaces the state)", who, n_present, (int)n);
        c->err = buf; return ICP_ERR_INVALID_ARG;
    }
    if ((rc = htsdf_allocate(c, n, coords, d_coords, who))) return rc;
    if ((rc = htsdf_place_blocks(c, n, d_coords, tsdf, weight))) return rc;
    if (rgb && (rc = htsdf_place_colors(c, n, d_coords, rgb, cweight))) return rc;
    if (info_out) { htsdf_stream_info(c, info_out); info_out->n_inserted = n; }
    return guard.done();
}
}  // namespace

// Not part of icp_hip.h (tools/time_htsdf_evict.py): ONE icp_tsdf_evict_blocks / icp_tsdf_insert_blocks between two events on the
// context's stream -- the device's time from the call's first command to its last, the host's waits in between included.
extern "C" int icp_debug_htsdf_evict_time(icp_ctx* c, const float centre[3], float radius, int32_t hold, icp_tsdf_stream_info* info_out, float* ms_out) {
    if (!c || !ms_out) return ICP_ERR_INVALID_ARG;
    int rc;
    if ((rc = htsdf_check(c, "icp_debug_htsdf_evict_time"))) return rc;
    DrainOnError guard(c);
    if ((rc = set_device(c))) return rc;
    HIPCK(c, hipStreamSynchronize(c->stream));
    if ((rc = timed_ms(c, ms_out, [&] { return icp_tsdf_evict_blocks(c, centre, radius, hold, info_out); }))) return rc;
    return guard.done();
}
extern "C" int icp_debug_htsdf_insert_time(icp_ctx* c, int32_t n, const int32_t* coords, const float* tsdf, const float* weight, icp_tsdf_stream_info* info_out, float* ms_out) {
    if (!c || !ms_out) return ICP_ERR_INVALID_ARG;
    int rc;
    if ((rc = htsdf_check(c, "icp_debug_htsdf_insert_time"))) return rc;
    DrainOnError guard(c);
    if ((rc = set_device(c))) return rc;
    HIPCK(c, hipStreamSynchronize(c->stream));
    if ((rc = timed_ms(c, ms_out, [&] { return icp_tsdf_insert_blocks(c, n, coords, tsdf, weight, info_out); }))) return rc;
    return guard.done();
}
