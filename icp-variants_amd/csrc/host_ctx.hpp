// host_ctx.hpp -- the context behind the C ABI (icp_ctx) and what every entry point leans on: device buffers, the resident clouds, levels
// and trees as host-side records, page-locked staging, cloud uploads, the finite filter and compaction, the pose upload, readiness checks.
// Part of icp_hip.hip (included from there, first); the pieces after it are host_index, host_launch, host_loop, host_multi, host_depth, host_tsdf, host_tsdf_hash, host_tsdf_hash_raycast, host_sdf, host_vgicp, host_hmap, host_vmap, host_vmap_prune, host_sdf_color, host_tsdf_mesh, host_tsdf_hash_mesh, host_mesh_cluster, host_tsdf_hash_evict, host_tsdf_cloud, host_sdf_cloud, host_global, host_debug.
using namespace icpdev;

#define HIPCK(ctx, expr)                                                                        \
    do {                                                                                        \
        hipError_t e__ = (expr);                                                                \
        if (e__ != hipSuccess) {                                                                \
            char buf__[256];                                                                    \
            snprintf(buf__, sizeof(buf__), "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e__), __FILE__, __LINE__); \
            (ctx)->err = buf__;                                                                 \
            return ICP_ERR_HIP;                                                                 \
        }                                                                                       \
    } while (0)

namespace {
// Device bytes held through ensure / release by every context of the process (views not counted): icp_debug_live_bytes.
std::atomic<long long> g_live_bytes{0};

// What a context owns frees itself: a device buffer, a page-locked host block, an event, a stream.  All move-only, so a record made of them
// (Cloud, Level, Bvh, NssLevel, NssHeld, FpfhCache, icp_ctx itself) needs no destructor and no list of its members anywhere.
struct DevBuf {
    void* p = nullptr; size_t cap = 0;
    bool view = false;                   // part of another allocation (a plane of a packed level, a section of the search-state pack): never freed on its own
    DevBuf() = default;
    DevBuf(DevBuf&& o) noexcept : p(o.p), cap(o.cap), view(o.view) { o.p = nullptr; o.cap = 0; o.view = false; }      // (a view stays a view)
    DevBuf& operator=(DevBuf&& o) noexcept { if (this != &o) { reset(); p = o.p; cap = o.cap; view = o.view; o.p = nullptr; o.cap = 0; o.view = false; } return *this; }
    ~DevBuf() { reset(); }
    void reset() { if (p && !view) { (void)hipFree(p); g_live_bytes -= (long long)cap; } p = nullptr; cap = 0; view = false; }
    template <class T> T* as() const { return (T*)p; }
};
static_assert(!std::is_copy_constructible<DevBuf>::value && !std::is_copy_assignable<DevBuf>::value, "a copied DevBuf would be freed twice");
struct PinBuf {                          // page-locked host block (ensure_pin); dev: the address the device writes it at
    void* p = nullptr; size_t cap = 0; void* dev = nullptr;
    PinBuf() = default; PinBuf(const PinBuf&) = delete; PinBuf& operator=(const PinBuf&) = delete;
    ~PinBuf() { if (p) (void)hipHostFree(p); }
    template <class T> T* as() const { return (T*)p; }
};
struct Event {                           // created where it is first needed (&ev.e); passes for the hipEvent_t it holds
    hipEvent_t e = nullptr;
    Event() = default; Event(Event&& o) noexcept : e(o.e) { o.e = nullptr; } Event& operator=(Event&& o) noexcept { std::swap(e, o.e); return *this; }
    ~Event() { if (e) (void)hipEventDestroy(e); }
    operator hipEvent_t() const { return e; }
};
struct Stream {                          // created where it is first needed (&st.s); passes for the hipStream_t it holds
    hipStream_t s = nullptr;
    Stream() = default; Stream(const Stream&) = delete; Stream& operator=(const Stream&) = delete;
    ~Stream() { if (s) (void)hipStreamDestroy(s); }
    operator hipStream_t() const { return s; }
};

struct Cloud {
    int n = 0, npad = 0;
    DevBuf x, y, z, nx, ny, nz, cr, cg, cb, rgba;
    bool has_normals = false, has_colors = false;
};

// One resolution level of the source: the selection (original indices, increasing), and -- for the BVH matcher -- a physical
// copy of the selected points in Morton order, so that everything the ICP loop touches per query (source planes, search
// state, matches) is indexed by the same sorted position and streams coalesced.  factor 0 = the whole cloud, unfiltered.
struct Level { DevBuf idx; DevBuf order; DevBuf sorted_idx; DevBuf pack; Cloud sorted; bool sorted_valid = false; int n = 0; };   // pack: the sorted copy's planes in ONE allocation (x y z nx ny nz cr cg cb rgba, a fixed stride apart)

// Normal-space sampling (dev_nss.hpp).  NssLevel: a level's candidates sorted by bucket (cand), the segment starts (seg: nb + 1 ints), its long
// segments (longs: one NssLongs); max_long / max_chunks: host-side bounds of their number and of their chunks, from the level's size alone.
// NssHeld: the draw a run with resample = 0 holds for a decimation factor, as a level of its own; word = the iteration it was drawn for.
struct NssLevel { DevBuf cand, seg, longs; int n_base = 0, max_long = 0, max_chunks = 0; };
struct NssHeld { Level lv; uint32_t word = 0; };

// Global registration (dev_fpfh.hpp): the features of one resident cloud -- per point the neighbour list (idx, d2: n x k) and the SPFH
// (counts n x 33, pairs n), per keypoint the FPFH rows (feat: nk x 33) -- for the (k, stride) they were computed with.
struct FpfhCache { DevBuf nb_idx, nb_d2, counts, pairs, feat; bool ready = false; int k = 0, stride = 0, n = 0, nk = 0; };

// LBVH over the target (buildIndex): device buffers + the host-side facts needed to launch the build.
struct Bvh {
    bool valid = false;
    int n_valid = 0, n_leaves = 0, Lp = 1;
    DevBuf keys, keys2, vals, vals2, temp, leaves, recs, nodes, qnodes, pos_of;
    DevBuf axl[12], side, scanr, axis_of_node;      // presorted-axes build: DIM index lists (ping-pong), side flag per point id, scan result, widest axis per node
    int n_ids = 0;                                   // size of the id space the lists index (points of the cloud the tree is built over)
    const Cloud* attrs = nullptr;                     // cloud whose normals / colours go into the records (nullptr: none)
    int Lq = 0;                                       // 4-wide levels
    const int* d_finite = nullptr;                    // device list of the finite points' indices, increasing (owned by the context)
    double build_ms = 0.0;
};
}  // namespace

struct icp_ctx {
    int device = 0;
    Stream own_stream, depth_stream;     // declared first: destroyed after every buffer, block and event below.  depth_stream: the second stream of the depth frames' uploads
    hipStream_t stream = nullptr;        // own_stream, or the caller's (icp_ctx_create_on_stream), which is left alone
    int stage_timing = 1;                // icp_set_stage_timing: 0 none, 1 every iteration, N > 1 every Nth iteration (scaled)
    unsigned timing_phase = 0;           // rotates the sampled iterations from run to run
    double wall_ticks_per_ms = 0;        // rate of the device's wall clock (hipDeviceAttributeWallClockRate, kHz), asked for by the first merged run
    PinBuf pinned;                       // page-locked host staging: pose upload, stats + pose download (truly asynchronous copies)
    bool trace = false;                  // ICP_HIP_TRACE=1: per-iteration stage times on stderr
    bool merge_loop = true;              // point-to-plane loop through the fused BVH matcher: reduce + solve ride in front of the next matcher launch (ICP_HIP_MERGE=0: separate k_reduce_solve launches)
    int merged_runs = 0, merged_fallbacks = 0;   // runs that took the merged loop / that had to be repeated with the separate launches (icp_debug_counters)
    bool lm_on = false; icp_lm_options lm_opt;   // icp_set_optimizer: the non-linear optimiser (k_lm_eval / k_lm_step) instead of the linear solve
    DevBuf lm_state, lm_partials, lm_sums;       // its minimiser state, eval partials, per-iteration records of the run in flight
    std::vector<icp_lm_summary> lm_last;         // the records of the last run (icp_get_lm_summaries)
    DevBuf ms_ps, ms_nn, ms_st, ms_st2, ms_rec, ms_d2, ms_partials, ms_totals, ms_stats, ms_score, ms_res;   // icp_run_multistart: one slice per start (dev_multi.hpp)
    icp_gicp_options gicp_opt = {1e-3f, 20};     // icp_set_gicp_options
    DevBuf gicp_n[2][3], gicp_flag;              // GICP normals of the target [0] / source [1] (SoA, original order), finite flags of their scratch tree
    bool gicp_ready[2] = {false, false};         // the cache is current (dropped by every call that replaces the cloud and by new options)
    icp_colored_options col_opt = {0.968f, 20};  // icp_set_colored_options
    DevBuf col_grad[3];                          // colour gradients of the target (SoA, original order, dev_colored.hpp)
    bool col_ready = false;                      // the cache is current (dropped by every call that replaces the target and by new options)
    icp_robust_options rob_opt = {ICP_ROBUST_NONE, 0.f, 0.f, 1.f};   // icp_set_robust_options
    DevBuf rob_keys, rob_state, rob_stats;      // trimmed / robust mode (dev_robust.hpp): r^2 keys per query, the chain's state, per-iteration records
    std::vector<icp_robust_stats> rob_last;      // the records of the last call (icp_get_robust_stats)
    icp_reciprocal_options rcp_opt = {0};        // icp_set_reciprocal_options: mutual nearest-neighbour rejection (dev_reciprocal.hpp)
    Bvh src_bvh; DevBuf src_rflag, src_finite;   // its reverse index: the BVH over the resident source (built on first use, dropped with the source), finite flags and list
    DevBuf rcp_stats;                            // per-iteration records of the run in flight
    bool rcp_naive = false; DevBuf rcp_q[3], rcp_nn;   // icp_debug_reciprocal_naive (tools/time_reciprocal.py): the reverse test as a full search of a written-out query cloud
    std::vector<icp_reciprocal_stats> rcp_last;  // the records of the last call (icp_get_reciprocal_stats)
    icp_convergence_options cvg_opt = {0, 1e-6f, 1e-6f, 1, 1};      // icp_set_convergence_options: stopping on a converged pose
    icp_convergence_result cvg_last = {0, 0, 0, -1.f, -1.f};        // the last run (icp_get_convergence) ...
    std::vector<icp_convergence_step> cvg_trace;                    // ... and its trace, one step per iteration that ran (icp_get_convergence_trace)
    icp_global_options glob_opt = {20, 1, 1, 4096, 0.9f, 0.005f, 0u, 16};   // icp_set_global_options
    FpfhCache fpfh[2];                           // features of the target [0] / source [1] (dropped by every call that replaces the cloud and by new options)
    DevBuf gm_best[2], gm_fwd, gm_keep, gm_list, gm_idx, gm_pts, gm_hyp;   // matcher results (forward / backward), kept flags and list, the pairs' indices and points, the hypotheses
    std::vector<icp_global_hypothesis> glob_last;                          // the hypotheses of the last icp_register_global
    icp_params prm;
    Cloud tgt, src, qry;                 // qry: scratch cloud of icp_query_matches
    Cloud nrm_cloud; Bvh nrm_bvh;        // scratch of icp_estimate_normals
    Bvh bvh, bvh6;                       // exact kd-ordered BVH of the target over xyz / over xyz+rgb (knn_backend == ICP_KNN_LBVH)
    DevBuf src_flag, src_box;            // per source point: finite point && finite normal (PointCloud.h:334); bounding box of the finite points (ordered bits)
    DevBuf tgt_flag, tgt_finite, nrm_finite, sel_temp, d_count;   // finite filters of the index builds, compaction scratch
    PinBuf pin_up; Event up_ev; bool up_pending = false;   // page-locked upload staging + "copy has left it" event
    DevBuf okeys, okeys2, ovals, otemp;  // scratch of the Morton sort of the queries
    std::map<int, Level> levels;         // multires selections by decimation factor
    DevBuf sel_lists, sel_counts, sel_blocks;            // RANDOM_SAMPLING / normal-space sampling: per-iteration index lists, their sizes, scan scratch
    icp_nss_options nss_opt = {5, 1};                    // icp_set_nss_options
    DevBuf nss_bkt; int nss_bkt_grid = 0;                // bucket of every source point for grid nss_bkt_grid (0: none computed for this source)
    std::map<int, NssLevel> nss_levels;                  // by decimation factor, for nss_bkt_grid
    std::map<int, NssHeld> nss_held;                     // by decimation factor, drawn for (nss_opt, nss_held_proba, nss_held_seed)
    float nss_held_proba = 0.f; uint32_t nss_held_seed = 0u; bool nss_held_stale = false;   // stale: the options changed; dropped at the next loop start
    DevBuf nss_table, nss_quota, nss_thr, nss_state, nss_hist, nss_total;   // scratch: the level sort's count table; per draw the quotas, thresholds, long-segment select state and histograms (left cleared)
    std::vector<std::pair<const int*, int>> sel_last;    // icp_get_selection: the query set (device list, size) of every iteration of the last run with selection != 0
    DevBuf qpack; size_t q_cap = 0;                      // nn_raw | qstate | qstate2 (views below), q_cap elements each
    DevBuf qstate, qstate2;                              // incremental k-NN: per-query anchor + bound on the other targets; bound on the targets outside the neighbour's leaf
    DevBuf dbg_steps;                    // development builds only (ICP_DEBUG_STEPS)
    DevBuf ps, matches, d2, best64, nn_raw, partials, partials2, ring, totals, sums, stats, staging, rmse_partials, rmse_out, fontana_partials;
    DevBuf block_t1;                     // merged loop: the matcher blocks' end stamps, two buffers that alternate like partials / partials2 (RingStamps, dev_solve.hpp)
    Cloud conv_src, conv_ref; int conv_n = 0;
    // depth frames (icp_set_*_depth, icp_track_depth_frames): two upload slots, each a page-locked staging block + a device copy of
    // [depth 4n | rgbx 4n]; the next frame of a sequence goes up on depth_stream while the current one iterates
    PinBuf depth_pin[2]; DevBuf depth_dev[2]; Event depth_up[2]; bool depth_pending[2] = {false, false};
    // the bilateral depth filter (icp_set_depth_filter_options, host_depth.hpp): its options, the device tables [spatial 81 | range 256] and
    // whether they are current; per upload slot the filtered copy of the depth frame and whether the slot's last frame was filtered
    icp_depth_filter_options df_opt = {0, 4.5f, 0.03f}; DevBuf df_tables; bool df_tables_ok = false; float df_inv_bin = 0.f;
    DevBuf depth_filt[2]; bool depth_filtered[2] = {false, false};
    DevBuf depth_blocks, track_rmse;     // block counts / offsets of the depth compaction; per-frame initial + final RMSE of a tracked sequence
    PinBuf pin_track;                    // page-locked pose staging of a tracked frame's initial / final RMSE: two slots of its own, apart from `pinned`
    DevBuf tsdf_vox, tsdf_cnt; bool tsdf_on = false; icp_tsdf_options tsdf_opt;   // the TSDF volume of frame-to-model tracking (host_tsdf.hpp): (tsdf, weight) per voxel, the update / hit counter, its options (ray_step resolved)
    DevBuf tsdf_col; bool tsdf_col_on = false;   // its optional colour array (icp_tsdf_color_create): one float4 (R, G, B, Wc) per voxel, 16 bytes, the indexing of tsdf_vox
    DevBuf th_keys, th_vals, th_pool, th_pkey, th_ctr;   // the hashed storage of the volume (host_tsdf_hash.hpp): the table's keys and pool indices, the pool of 4 KiB blocks, every block's key, the counters
    bool tsdf_hashed = false; int th_log2cap = 0, th_pool_cap = 0, th_nblk = 0, th_grown = 0, th_unplaced = 0, th_max_log2 = 22; long long th_oor = 0;   // the volume is hashed (icp_tsdf_create_hashed); table of 2^th_log2cap slots, pool of th_pool_cap blocks; allocated blocks (exact after every call); growths; the last touch's unplaced claims; log2 of the largest pool growth may reach (2^22 blocks; lowered by icp_debug_htsdf_max_blocks alone); samples out of range so far
    DevBuf th_cpool; bool th_color = false;   // the colours of the hashed volume (icp_tsdf_create_color_hashed): a second pool, one float4 (R, G, B, Wc) per voxel, 8 KiB per block, by the same pool index
    DevBuf te_out_cpool;                 // the colours of the outbox (a coloured hashed volume evicted with hold)
    DevBuf te_work, te_out_pool, te_out_key; int te_held = 0;   // streaming the hashed volume (host_tsdf_hash_evict.hpp): an evict's flags, lists and counters; the outbox (evicted blocks and their keys) and the blocks it holds
    DevBuf tc_acc, tc_ctr; size_t tc_voxels = 0;   // icp_tsdf_integrate_cloud (host_tsdf_cloud.hpp): the integer accumulators [S 8 bytes | N 4 bytes] per voxel of the box or the pool, the call's 64-bit counters; the voxels the accumulators are laid out for and all zero over (0: to be made and cleared)
    DevBuf tcc_acc; size_t tcc_voxels = 0;   // icp_tsdf_integrate_cloud_color (host_tsdf_cloud.hpp): the colour accumulators [SR | SG | SB | NC], 16 bytes per voxel of the box or the pool, made at the first coloured call; the voxels they are laid out for and all zero over (0: to be made and cleared)
    icp_tsdf_carve_options tcv_opt = {0.f, 0.f}; icp_tsdf_carve_info tcv_info = {0, 0, 0, 0};   // free-space carving of the cloud integrate (icp_set_tsdf_carve_options, host_tsdf_cloud.hpp): the options, which outlive clouds, volumes and resets, and the stats of the last cloud fuse
    DevBuf tm_bits, tm_mask, tm_base, tm_blk, tm_out;   // icp_tsdf_mesh (host_tsdf_mesh.hpp): the three bitmaps, the edge-mask bytes, the run bases, the block tables + totals, the staged mesh
    DevBuf tm_nbr, tm_ord;               // icp_tsdf_mesh_hashed (host_tsdf_hash_mesh.hpp), which also uses the five above: the 27 neighbour ranks of every block; order[rank] -> pool index, then rank_of[pool index]
    DevBuf mc_tab, mc_vtx, mc_tri, mc_acc, mc_in, mc_out; bool mc_combine = true;   // vertex clustering (host_mesh_cluster.hpp): the cell table [keys | first members | referenced flag, then rank + 1]; per vertex its slot and per rank the cluster's slot, the leader block table, the counters; per triangle the canonical triple and its slot, the triangle table, the survivor block table; the accumulators by rank; the uploaded input of icp_mesh_cluster; the staged clustered mesh; the accumulate combines neighbouring lanes
    DevBuf sdf_state, sdf_partials, sdf_rec; Event sdf_ev;  // direct SDF tracking (host_sdf.hpp's driver, for the record kinds SdfGeo and SdfColor, and host_vgicp.hpp through it): the kind's pose / stop state, partials[NSUM][blocks] + counts[NCOUNT][blocks] (28 + 2 or 29 + 3), the frame record + trace; they only grow, every call writes them before it reads them; "the last integration has left its upload slot"
    DevBuf vg_box, vg_count, vg_sums, vg_cells;   // voxelized GICP (host_vgicp.hpp): the target's voxel grid -- bounds + counters, per cell the count, the nine int64 sums, the 40-byte record
    bool vg_ready = false; float vg_voxel = 0.f; icp_voxel_grid_info vg_info = {{0, 0, 0}, {0, 0, 0}, 0, 0};   // the grid is current for vg_voxel (dropped with the target's GICP normal cache); its extent
    DevBuf vm_count, vm_sums, vm_cells, vm_stamp, vm_list, vm_ctr, vm_box;   // the voxel map (host_vmap.hpp): per cell the count, the nine int64 sums, the 40-byte record and the stamp of the last insert that touched it; the list of the cells an insert touched, the counters, the scratch counters of a full sweep
    bool vm_on = false; icp_voxel_map_options vm_opt = {0.f, {0, 0, 0}, {0, 0, 0}}; int vm_serial = 0;   // the map exists (icp_voxel_map_create); its voxel size and extent; the serial number of the last insert
    DevBuf vh_keys;                      // the hashed storage of the map (host_hmap.hpp): one 8-byte key per slot; vm_count .. vm_stamp are then indexed by slot
    bool vm_hashed = false; int vh_log2cap = 0, vh_grown = 0; long long vh_bound = 0;   // the map is hashed (icp_voxel_map_create_hashed; vm_opt holds its voxel size alone); capacity = 2^vh_log2cap; rehashes so far; the host's upper bound on the occupied count
    bool vh_vac = false; int vh_compacted = 0; long long vh_vac_bound = 0;   // local maps (host_vmap_prune.hpp): a prune has been enqueued since the last compaction, so slots may be vacated (false: none is, and every hashed call does what it did before prunes existed); compactions so far; the host's upper bound on the vacated count
    float cos_reject = 0.5f;
    std::vector<Event> events;
    Event build_ev[2];                   // index-build bracket (build_bvh)
    icp_timing timing;
    std::vector<float> it_match_ms, it_post_ms, it_solve_ms;   // per iteration of the last run; -1 where the iteration was not bracketed
    std::string err;
};

namespace {
constexpr int POST_BLOCKS = 512;

int ensure(icp_ctx* c, DevBuf& b, size_t bytes) {
    if (bytes <= b.cap && b.p) return ICP_OK;
    if (b.view) { b.p = nullptr; b.cap = 0; b.view = false; }      // outgrown: becomes an allocation of its own
    if (b.p) { HIPCK(c, hipFree(b.p)); g_live_bytes -= (long long)b.cap; b.p = nullptr; b.cap = 0; }
    size_t want = bytes < 256 ? 256 : bytes;
    HIPCK(c, hipMalloc(&b.p, want));
    b.cap = want; g_live_bytes += (long long)want;
    return ICP_OK;
}
// A page-locked block of at least `bytes`; one that has to grow becomes max(min_bytes, bytes + bytes / slack_div) (slack_div 0: no slack).
int ensure_pin(icp_ctx* c, PinBuf& b, size_t bytes, size_t min_bytes, size_t slack_div) {
    if (bytes <= b.cap && b.p) return ICP_OK;
    if (b.p) { HIPCK(c, hipHostFree(b.p)); b.p = nullptr; b.cap = 0; b.dev = nullptr; }
    const size_t want = bytes < min_bytes ? min_bytes : bytes + (slack_div ? bytes / slack_div : 0);
    HIPCK(c, hipHostMalloc(&b.p, want, hipHostMallocDefault));
    b.cap = want;
    HIPCK(c, hipHostGetDevicePointer(&b.dev, b.p, 0));
    return ICP_OK;
}
int ensure_pinned(icp_ctx* c, size_t bytes) { return ensure_pin(c, c->pinned, bytes, 4096, 0); }
void release(DevBuf& b) { b.reset(); }
void set_view(DevBuf& b, void* p, size_t bytes) { release(b); b.p = p; b.cap = bytes; b.view = true; }
// (these also run outside destroy, where the record lives on: a dropped level or draw must not look valid)
void release(Cloud& c) { release(c.x); release(c.y); release(c.z); release(c.nx); release(c.ny); release(c.nz); release(c.cr); release(c.cg); release(c.cb); release(c.rgba); }
void release(Level& lv) { release(lv.idx); release(lv.order); release(lv.sorted_idx); release(lv.sorted); release(lv.pack); lv.sorted_valid = false; }
void release(NssLevel& nl) { release(nl.cand); release(nl.seg); release(nl.longs); }
// the normal-space sampling caches that belong to the resident source (held: only the held draws, which also depend on the options)
void drop_nss(icp_ctx* c, bool held_only);

// Largest float c with (double)acosf(c) > 60*pi/180 on THIS host's libm: the device rejection test
// `c <= cos_reject` is then bit-identical to the reference's `acos(c) > threshold` (ICPOptimizer.h:161,170)
// as evaluated by the host the reference would run on (acosf is monotone on [0.25, 0.75]).
float compute_cos_reject() {
    const double threshold = 60 * 3.141592653589793238462643383279502884 / 180.0;
    uint32_t lo, hi; float flo = 0.25f, fhi = 0.75f;
    memcpy(&lo, &flo, 4); memcpy(&hi, &fhi, 4);       // predicate true at lo, false at hi
    while (hi - lo > 1) {
        uint32_t mid = lo + (hi - lo) / 2; float fm; memcpy(&fm, &mid, 4);
        if ((double)acosf(fm) > threshold) lo = mid; else hi = mid;
    }
    float r; memcpy(&r, &lo, 4);
    return r;
}

int set_device(icp_ctx* c) { HIPCK(c, hipSetDevice(c->device)); return ICP_OK; }

// Every entry point that enqueues work synchronises the stream before it returns (write_pose's contract: the page-locked staging
// area and the scratch buffers are free again by the next call).  On the success paths that is the entry point's own final
// hipStreamSynchronize; this guard covers the error returns in between.
struct DrainOnError {
    icp_ctx* c; bool ok = false;
    explicit DrainOnError(icp_ctx* ctx) : c(ctx) {}
    ~DrainOnError() { if (!ok && c && c->stream) (void)hipStreamSynchronize(c->stream); }
    int done(int rc = ICP_OK) { ok = (rc == ICP_OK); return rc; }
};

// Host clouds -> device SoA planes.  The whole cloud (points, normals, colours) goes through ONE page-locked staging buffer and
// ONE asynchronous copy, the AoS -> SoA kernels follow on the stream, and nothing here waits for the device: the only host-side
// wait is for the previous upload to have left the staging buffer.  (Round 1: pageable copies + one synchronisation per plane.)
int ensure_pin_up(icp_ctx* c, size_t bytes) {
    if (c->up_pending) { HIPCK(c, hipEventSynchronize(c->up_ev)); c->up_pending = false; }
    int rc;
    if ((rc = ensure_pin(c, c->pin_up, bytes, 65536, 8))) return rc;
    if (!c->up_ev) HIPCK(c, hipEventCreateWithFlags(&c->up_ev.e, hipEventDisableTiming));
    return ICP_OK;
}
int upload_cloud(icp_ctx* c, Cloud& cl, const float* xyz, const float* nrm, const uint8_t* rgba, int n, bool pad_inf) {
    const int npad = pad_inf ? ((n + 63) / 64) * 64 : n;
    const size_t b_xyz = (size_t)n * 12, b_nrm = nrm ? (size_t)n * 12 : 0, b_col = rgba ? (size_t)n * 4 : 0, total = b_xyz + b_nrm + b_col;
    int rc;
    if ((rc = ensure_pin_up(c, total))) return rc;
    if ((rc = ensure(c, c->staging, total))) return rc;
    char* h = c->pin_up.as<char>();
    memcpy(h, xyz, b_xyz);
    if (nrm) memcpy(h + b_xyz, nrm, b_nrm);
    if (rgba) memcpy(h + b_xyz + b_nrm, rgba, b_col);
    HIPCK(c, hipMemcpyAsync(c->staging.p, h, total, hipMemcpyHostToDevice, c->stream));
    HIPCK(c, hipEventRecord(c->up_ev, c->stream)); c->up_pending = true;
    const char* d = c->staging.as<char>();
    const dim3 g((npad + 255) / 256), b(256);
    for (DevBuf* pl : {&cl.x, &cl.y, &cl.z}) if ((rc = ensure(c, *pl, (size_t)npad * 4))) return rc;
    hipLaunchKernelGGL(k_deinterleave3, g, b, 0, c->stream, (const float*)d, n, npad, INFINITY, cl.x.as<float>(), cl.y.as<float>(), cl.z.as<float>());
    cl.has_normals = nrm != nullptr;
    if (nrm) {
        for (DevBuf* pl : {&cl.nx, &cl.ny, &cl.nz}) if ((rc = ensure(c, *pl, (size_t)n * 4))) return rc;
        hipLaunchKernelGGL(k_deinterleave3, dim3((n + 255) / 256), b, 0, c->stream, (const float*)(d + b_xyz), n, n, 0.f, cl.nx.as<float>(), cl.ny.as<float>(), cl.nz.as<float>());
    }
    cl.has_colors = rgba != nullptr;
    if (rgba) {
        for (DevBuf* pl : {&cl.rgba, &cl.cr, &cl.cg, &cl.cb}) if ((rc = ensure(c, *pl, (size_t)npad * 4))) return rc;
        hipLaunchKernelGGL(k_colors, g, b, 0, c->stream, (const uint8_t*)(d + b_xyz + b_nrm), n, npad, cl.rgba.as<uint32_t>(), cl.cr.as<float>(), cl.cg.as<float>(), cl.cb.as<float>());
    }
    HIPCK(c, hipGetLastError());
    cl.n = n; cl.npad = npad;
    return ICP_OK;
}
// one plane triple through the same staging path (convergence reference)
int upload3(icp_ctx* c, const float* aos, int n, int npad, float pad_value, DevBuf& x, DevBuf& y, DevBuf& z) {
    int rc;
    if ((rc = ensure_pin_up(c, (size_t)n * 12))) return rc;
    if ((rc = ensure(c, c->staging, (size_t)n * 12))) return rc;
    for (DevBuf* pl : {&x, &y, &z}) if ((rc = ensure(c, *pl, (size_t)npad * 4))) return rc;
    memcpy(c->pin_up.p, aos, (size_t)n * 12);
    HIPCK(c, hipMemcpyAsync(c->staging.p, c->pin_up.p, (size_t)n * 12, hipMemcpyHostToDevice, c->stream));
    HIPCK(c, hipEventRecord(c->up_ev, c->stream)); c->up_pending = true;
    hipLaunchKernelGGL(k_deinterleave3, dim3((npad + 255) / 256), dim3(256), 0, c->stream, c->staging.as<float>(), n, npad, pad_value, x.as<float>(), y.as<float>(), z.as<float>());
    HIPCK(c, hipGetLastError());
    HIPCK(c, hipStreamSynchronize(c->stream));      // staging is reused by the caller's next plane
    return ICP_OK;
}

// Small counts the device has produced come back through one slot of the page-locked block, at 2048 (the first bytes of the block stage
// the pose): n_words 4-byte words.  read_count: one count, copied and waited for.  Where the copy has to go out among others, count_slot
// gives the slot and the caller enqueues the copy and waits itself.
int count_slot(icp_ctx* c, int** slot) {
    int rc;
    if ((rc = ensure_pinned(c, 4096))) return rc;
    *slot = (int*)(c->pinned.as<char>() + 2048);
    return ICP_OK;
}
int read_count(icp_ctx* c, const void* d_count, int* out, int n_words = 1) {
    int rc; int* h;
    if ((rc = count_slot(c, &h))) return rc;
    HIPCK(c, hipMemcpyAsync(h, d_count, (size_t)n_words * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCK(c, hipStreamSynchronize(c->stream));
    memcpy(out, h, (size_t)n_words * 4);
    return ICP_OK;
}

// Indices j * factor (j = 0 .. count - 1) whose flag is set, in increasing order, compacted on the device (rocPRIM select); one
// 4-byte copy returns how many there are.  flags: one byte per j.
int compact_flagged(icp_ctx* c, const uint8_t* d_flags, int count, int factor, DevBuf& out, int* n_out) {
    int rc;
    if ((rc = ensure(c, out, (size_t)(count > 0 ? count : 1) * 4))) return rc;
    if ((rc = ensure(c, c->d_count, 16))) return rc;
    *n_out = 0;
    if (count <= 0) return ICP_OK;
    auto in = rocprim::make_transform_iterator(rocprim::counting_iterator<int>(0), MulBy{factor});
    size_t tb = 0;
    HIPCK(c, rocprim::select(nullptr, tb, in, d_flags, out.as<int>(), c->d_count.as<int>(), (size_t)count, c->stream));
    if ((rc = ensure(c, c->sel_temp, tb))) return rc;
    HIPCK(c, rocprim::select(c->sel_temp.p, tb, in, d_flags, out.as<int>(), c->d_count.as<int>(), (size_t)count, c->stream));
    return read_count(c, c->d_count.p, n_out);
}
// finite filter of a cloud that is already on the device -> flag bytes + compacted index list
int finite_list(icp_ctx* c, const Cloud& cl, bool with_normals, DevBuf& flag, DevBuf& list, int* n_out) {
    int rc;
    if ((rc = ensure(c, flag, (size_t)cl.n))) return rc;
    const bool nrm = with_normals && cl.has_normals;
    hipLaunchKernelGGL(k_mark_finite, dim3((cl.n + 255) / 256), dim3(256), 0, c->stream, cl.x.as<float>(), cl.y.as<float>(), cl.z.as<float>(),
                       nrm ? cl.nx.as<float>() : nullptr, nrm ? cl.ny.as<float>() : nullptr, nrm ? cl.nz.as<float>() : nullptr, cl.n, flag.as<uint8_t>());
    HIPCK(c, hipGetLastError());
    return compact_flagged(c, flag.as<uint8_t>(), cl.n, 1, list, n_out);
}

// Upload the pose state.  Staged through the context's page-locked buffer: no synchronisation here -- every entry point
// that uses the pose synchronises the stream before it returns, so the staging area is free again by the next call.
// write_pose_via: the same through a page-locked PoseState h the caller owns (and keeps untouched until the stream has passed the copy).
void make_pose_state(const float pose[16], PoseState* h) {      // the state of a pose nothing has iterated on yet: the pose, its normal matrix, the rest zero
    memset(h, 0, sizeof(*h));
    memcpy(h->pose, pose, 64);
    normal_matrix_from_pose(h->pose, h->nmat);
}
int write_pose_via(icp_ctx* c, PoseState* h, const float pose[16]) {
    int rc;
    make_pose_state(pose, h);
    if ((rc = ensure(c, c->ps, sizeof(PoseState)))) return rc;
    HIPCK(c, hipMemcpyAsync(c->ps.p, h, sizeof(*h), hipMemcpyHostToDevice, c->stream));
    return ICP_OK;
}
int write_pose(icp_ctx* c, const float pose[16]) {
    int rc;
    if ((rc = ensure_pinned(c, sizeof(PoseState)))) return rc;
    return write_pose_via(c, c->pinned.as<PoseState>(), pose);
}

int check_ready(icp_ctx* c, bool need_source, bool full_pipeline) {
    const icp_params& p = c->prm;
    if (c->tgt.n <= 0) { c->err = "target index needs to be built before querying (icp_set_target)"; return ICP_ERR_NO_TARGET; }
    if (need_source && c->src.n <= 0) { c->err = "no source cloud (icp_set_source)"; return ICP_ERR_NO_SOURCE; }
    if (p.matching == ICP_MATCH_PROJECTIVE) {
        if (p.height <= 0 || p.width <= 0) { c->err = "set camera params before querying any matches"; return ICP_ERR_NO_CAMERA; }
        if ((long long)p.width * p.height != c->tgt.n) { c->err = "invalid size of target points (must be width*height)"; return ICP_ERR_TARGET_SIZE; }
    } else if (p.color_icp) {
        if (!c->tgt.has_colors || (need_source && !c->src.has_colors)) { c->err = "colour ICP needs colours on target and source"; return ICP_ERR_COLOR_MISMATCH; }
    }
    if (full_pipeline) {
        if (!c->tgt.has_normals || !c->src.has_normals) { c->err = "normals required on source and target"; return ICP_ERR_INVALID_ARG; }
        if (p.weighting == ICP_WEIGHT_COLORS && (!c->tgt.has_colors || !c->src.has_colors)) { c->err = "colour weighting needs colours"; return ICP_ERR_COLOR_MISMATCH; }
    }
    return ICP_OK;
}

int ensure_events(icp_ctx* c, size_t count) {
    while (c->events.size() < count) { Event e; HIPCK(c, hipEventCreate(&e.e)); c->events.push_back(std::move(e)); }
    return ICP_OK;
}
// The one timed bracket of the icp_debug_*_time functions: the device time, in milliseconds, of what `enqueue` puts on the context's
// stream, between two events.  What is staged or warmed outside the bracket is the caller's, in front of this call.
template <class Enqueue> int timed_ms(icp_ctx* c, float* ms_out, Enqueue&& enqueue) {
    int rc;
    if ((rc = ensure_events(c, 2))) return rc;
    HIPCK(c, hipEventRecord(c->events[0], c->stream));
    if ((rc = enqueue())) return rc;
    HIPCK(c, hipEventRecord(c->events[1], c->stream));
    HIPCK(c, hipStreamSynchronize(c->stream));
    HIPCK(c, hipEventElapsedTime(ms_out, c->events[0], c->events[1]));
    return ICP_OK;
}
}  // namespace
