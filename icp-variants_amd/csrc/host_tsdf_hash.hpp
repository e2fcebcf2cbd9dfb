// host_tsdf_hash.hpp -- the hashed storage of the TSDF volume: icp_tsdf_create_hashed / reserve_blocks / allocate_blocks / upload_hashed,
// icp_get_tsdf_hashed, and what host_tsdf.hpp's and host_sdf.hpp's entry points call when the context's volume is hashed (the touch with
// its room rule in front of an integrate, the growth, reset and release).  Kernels: dev_tsdf_hash.hpp.  Contract: include/icp_hip.h,
// DESIGN.md section 6x; the colour pool of a coloured hashed volume (icp_tsdf_create_color_hashed, icp_get_tsdf_color_hashed,
// icp_tsdf_upload_color_hashed; kernels: dev_tsdf_hash_color.hpp): section 6zb.  Part of icp_hip.hip (included from there, after host_tsdf.hpp, which declares what it calls, and before host_sdf.hpp).
namespace {
constexpr int HT_MAX_POOL_LOG2 = 22;                // 2^22 blocks of 4 KiB: 16 GiB
constexpr int HT_MAX_STEPS = 1024;                  // samples along a ray's truncation band: 2 truncation / voxel_size
// log2 of the smallest pool of at least `blocks` blocks, or -1 beyond 2^22
int ht_log2_for(long long blocks) {
    int l = 0;
    while (l <= HT_MAX_POOL_LOG2 && (1ll << l) < blocks) l++;
    return l <= HT_MAX_POOL_LOG2 ? l : -1;
}
int htsdf_check(icp_ctx* c, const char* who) {
    if (!c->tsdf_on) { c->err = std::string(who) + ": no volume (icp_tsdf_create_hashed)"; return ICP_ERR_INVALID_ARG; }
    if (!c->tsdf_hashed) { c->err = std::string(who) + ": the volume is dense (icp_tsdf_create): use icp_tsdf_download / icp_tsdf_upload"; return ICP_ERR_INVALID_ARG; }
    return ICP_OK;
}
// the calls that need the colour pool
int htsdf_check_color(icp_ctx* c, const char* who) {
    int rc;
    if ((rc = htsdf_check(c, who))) return rc;
    if (!c->th_color) { c->err = std::string(who) + ": the hashed volume has no colours (icp_tsdf_create_color_hashed)"; return ICP_ERR_INVALID_ARG; }
    return ICP_OK;
}
struct HtBufs { DevBuf keys, vals, pool, pkey, cpool; };
// a cleared table of 2^(pool_log2 + 1) slots and a cleared pool of 2^pool_log2 blocks (enqueued)
int htsdf_alloc(icp_ctx* c, int pool_log2, HtBufs& b) {
    const size_t blocks = (size_t)1 << pool_log2, slots = 2 * blocks;
    int rc;
    if ((rc = ensure(c, b.keys, slots * 8))) return rc;
    if ((rc = ensure(c, b.vals, slots * 4))) return rc;
    if ((rc = ensure(c, b.pool, blocks * 4096))) return rc;
    if ((rc = ensure(c, b.pkey, blocks * 8))) return rc;
    HIPCK(c, hipMemsetAsync(b.keys.p, 0xFF, slots * 8, c->stream));
    HIPCK(c, hipMemsetAsync(b.vals.p, 0xFF, slots * 4, c->stream));      // HT_NONE
    HIPCK(c, hipMemsetAsync(b.pool.p, 0, blocks * 4096, c->stream));      // tsdf 0, weight 0
    HIPCK(c, hipMemsetAsync(b.pkey.p, 0xFF, blocks * 8, c->stream));
    if (c->th_color) {                                 // the colour pool of a coloured volume: (0, 0, 0, 0), uncoloured
        if ((rc = ensure(c, b.cpool, blocks * 8192))) return rc;
        HIPCK(c, hipMemsetAsync(b.cpool.p, 0, blocks * 8192, c->stream));
    }
    return ICP_OK;
}
void htsdf_adopt(icp_ctx* c, int pool_log2, HtBufs& b) {
    c->th_keys = std::move(b.keys); c->th_vals = std::move(b.vals); c->th_pool = std::move(b.pool); c->th_pkey = std::move(b.pkey);
    if (c->th_color) c->th_cpool = std::move(b.cpool);
    c->th_log2cap = pool_log2 + 1; c->th_pool_cap = 1 << pool_log2;
}
HtTable htsdf_table(const icp_ctx* c) {
    HtTable t;
    t.keys = c->th_keys.as<unsigned long long>(); t.vals = c->th_vals.as<int>(); t.pool_key = c->th_pkey.as<unsigned long long>();
    t.log2cap = c->th_log2cap; t.pool_cap = c->th_pool_cap;
    return t;
}
HtVol htsdf_view(const icp_ctx* c) {
    const icp_tsdf_options& o = c->tsdf_opt;
    HtVol v;
    v.keys = c->th_keys.as<unsigned long long>(); v.vals = c->th_vals.as<int>(); v.pool = c->th_pool.as<float2>(); v.pool_key = c->th_pkey.as<unsigned long long>();
    v.log2cap = c->th_log2cap; v.pool_cap = c->th_pool_cap;
    v.ox = o.origin[0]; v.oy = o.origin[1]; v.oz = o.origin[2]; v.s = o.voxel_size;
    v.trunc = o.truncation; v.max_w = o.max_weight; v.max_d = o.max_depth;
    return v;
}
// the counter of handed-out blocks set to n, the unplaced counter to 0 (enqueued; waited for before the words leave scope)
int htsdf_set_counters(icp_ctx* c, int n_blocks) {
    const int h[2] = {n_blocks, 0};
    HIPCK(c, hipMemcpyAsync(c->th_ctr.p, h, 8, hipMemcpyHostToDevice, c->stream));
    HIPCK(c, hipStreamSynchronize(c->stream));
    return ICP_OK;
}
int htsdf_rehash_launch(icp_ctx* c, int n_live, unsigned long long* keys, int* vals, const unsigned long long* pkey, int log2cap) {
    if (n_live > 0) {
        hipLaunchKernelGGL(k_htsdf_rehash, dim3((n_live + 255) / 256), dim3(256), 0, c->stream, n_live, pkey, keys, vals, log2cap, c->th_ctr.as<int>());
        HIPCK(c, hipGetLastError());
    }
    return ICP_OK;
}
// Growth: a cleared table and pool of 2^pool_log2 blocks, the first n_live blocks and their keys copied over, their keys entered into the
// new table; the old buffers are freed once all that has finished.  Claims that failed leave nothing behind: their keys are in no pool entry.
int htsdf_regrow(icp_ctx* c, int pool_log2, int n_live) {
    int rc;
    HtBufs b;
    if ((rc = htsdf_alloc(c, pool_log2, b))) return rc;
    if (n_live > 0) {
        HIPCK(c, hipMemcpyAsync(b.pool.p, c->th_pool.p, (size_t)n_live * 4096, hipMemcpyDeviceToDevice, c->stream));
        HIPCK(c, hipMemcpyAsync(b.pkey.p, c->th_pkey.p, (size_t)n_live * 8, hipMemcpyDeviceToDevice, c->stream));
        if (c->th_color) HIPCK(c, hipMemcpyAsync(b.cpool.p, c->th_cpool.p, (size_t)n_live * 8192, hipMemcpyDeviceToDevice, c->stream));
    }
    if ((rc = htsdf_rehash_launch(c, n_live, b.keys.as<unsigned long long>(), b.vals.as<int>(), (const unsigned long long*)b.pkey.as<unsigned long long>(), pool_log2 + 1))) return rc;
    if ((rc = htsdf_set_counters(c, n_live))) return rc;      // (waits)
    htsdf_adopt(c, pool_log2, b);
    c->th_nblk = n_live; c->th_grown++;
    return ICP_OK;
}
// The room rule around a launch that claims blocks (the touch of a frame, an explicit allocation): launch, read the three counters,
// and while anything was unplaced double table and pool and launch again (the launch is idempotent).  Past 2^22 blocks the call is
// refused and the volume put back as it was: the table rebuilt from the blocks it had before (the blocks added since are still all zero).
template <class Launch>
int htsdf_claim(icp_ctx* c, Launch launch, const char* who, long long* oor_out) {
    const int n_before = c->th_nblk;
    int rc;
    for (;;) {
        int* ctr = c->th_ctr.as<int>();
        HIPCK(c, hipMemsetAsync(ctr + HT_UNPLACED, 0, 8, c->stream));      // unplaced, out of range
        if ((rc = launch())) return rc;
        HIPCK(c, hipGetLastError());
        int h[3];
        if ((rc = read_count(c, ctr, h, 3))) return rc;
        c->th_unplaced = h[HT_UNPLACED];
        if (h[HT_UNPLACED] == 0) { c->th_nblk = h[HT_NBLK]; if (oor_out) *oor_out = h[HT_OOR]; return ICP_OK; }
        const int live = h[HT_NBLK] < c->th_pool_cap ? h[HT_NBLK] : c->th_pool_cap;
        const int pool_log2 = c->th_log2cap - 1;
        if (pool_log2 + 1 > c->th_max_log2) {
            const size_t slots = (size_t)1 << c->th_log2cap;
            HIPCK(c, hipMemsetAsync(c->th_keys.p, 0xFF, slots * 8, c->stream));
            HIPCK(c, hipMemsetAsync(c->th_vals.p, 0xFF, slots * 4, c->stream));
            if ((rc = htsdf_rehash_launch(c, n_before, c->th_keys.as<unsigned long long>(), c->th_vals.as<int>(), (const unsigned long long*)c->th_pkey.as<unsigned long long>(), c->th_log2cap))) return rc;
            if ((rc = htsdf_set_counters(c, n_before))) return rc;
            c->th_nblk = n_before;
            char buf[192];
            snprintf(buf, sizeof(buf), "%s: the hashed volume would need more than 2^%d blocks (%d allocated): not grown, nothing modified", who, c->th_max_log2, n_before);
            c->err = buf; return ICP_ERR_INVALID_ARG;
        }
        if ((rc = htsdf_regrow(c, pool_log2 + 1, live))) return rc;
    }
}
// tsdf_integrate_slot for a hashed volume: the touch under the room rule (one host wait, more when the volume grows), then the integrate
// over the pool, enqueued; d_count (optional): zeroed, then the number of voxels written.  color (a coloured volume only): the slot's colour
// frame goes into the colour pool as well, k_htsdf_integrate_color in place of k_htsdf_integrate (d_count[1]: the voxels coloured).
int htsdf_integrate_slot(icp_ctx* c, int slot, const icp_depth_camera& cam, const float pose[16], int* d_count, const char* who, bool color) {
    const icp_tsdf_options& o = c->tsdf_opt;
    TsdfMat m; memset(&m, 0, sizeof(m));
    invert_extrinsics(pose, m.m);
    TsdfMat P; memcpy(P.m, pose, 64);
    const int n_steps = (int)std::ceil(2.0 * (double)o.truncation / (double)o.voxel_size);
    const float* depth = c->depth_dev[slot].as<float>();
    HIPCK(c, hipStreamWaitEvent(c->stream, c->depth_up[slot], 0));
    int rc;
    long long oor = 0;
    const dim3 grid((cam.width + 15) / 16, (cam.height + 15) / 16);
    auto touch = [&]() {
        hipLaunchKernelGGL(k_htsdf_touch, grid, dim3(256), 0, c->stream, htsdf_table(c), tsdf_cam(cam), P, depth, o.origin[0], o.origin[1], o.origin[2], o.voxel_size,
                           o.truncation, o.max_depth, n_steps, c->th_ctr.as<int>());
        return (int)ICP_OK;
    };
    if ((rc = htsdf_claim(c, touch, who, &oor))) return rc;
    c->th_oor += oor;
    if (d_count) HIPCK(c, hipMemsetAsync(d_count, 0, color ? 8 : 4, c->stream));
    if (c->th_nblk > 0) {
        if (color) hipLaunchKernelGGL(k_htsdf_integrate_color, dim3(c->th_nblk), dim3(512), 0, c->stream, htsdf_view(c), tsdf_cam(cam), m, depth, d_count,
                                      (const uint32_t*)(depth + (size_t)cam.width * cam.height), c->th_cpool.as<float4>(), d_count ? d_count + 1 : nullptr);
        else hipLaunchKernelGGL(k_htsdf_integrate, dim3(c->th_nblk), dim3(512), 0, c->stream, htsdf_view(c), tsdf_cam(cam), m, depth, d_count);
        HIPCK(c, hipGetLastError());
    }
    return ICP_OK;
}
// icp_tsdf_reset on a hashed volume: every block forgotten, the capacity kept
int htsdf_reset(icp_ctx* c) {
    const size_t blocks = (size_t)c->th_pool_cap, slots = (size_t)1 << c->th_log2cap;
    HIPCK(c, hipMemsetAsync(c->th_keys.p, 0xFF, slots * 8, c->stream));
    HIPCK(c, hipMemsetAsync(c->th_vals.p, 0xFF, slots * 4, c->stream));
    HIPCK(c, hipMemsetAsync(c->th_pool.p, 0, blocks * 4096, c->stream));
    HIPCK(c, hipMemsetAsync(c->th_pkey.p, 0xFF, blocks * 8, c->stream));
    if (c->th_color) HIPCK(c, hipMemsetAsync(c->th_cpool.p, 0, blocks * 8192, c->stream));
    HIPCK(c, hipMemsetAsync(c->th_ctr.p, 0, HT_NCTR * 4, c->stream));
    HIPCK(c, hipStreamSynchronize(c->stream));
    c->th_nblk = 0; c->th_unplaced = 0; c->th_oor = 0; c->te_held = 0;
    return ICP_OK;
}
void htsdf_drop(icp_ctx* c) {
    for (DevBuf* d : {&c->th_keys, &c->th_vals, &c->th_pool, &c->th_pkey, &c->th_ctr, &c->te_work, &c->te_out_pool, &c->te_out_key, &c->th_cpool, &c->te_out_cpool}) release(*d);
    c->te_held = 0; c->th_color = false;
    c->tsdf_hashed = false; c->th_log2cap = 0; c->th_pool_cap = 0; c->th_nblk = 0;
}
// block coordinates from the caller: every one storable, or a message
int htsdf_check_coords(icp_ctx* c, int32_t n, const int32_t* coords, const char* who) {
    for (size_t i = 0; i < (size_t)n * 3; i++)
        if (coords[i] < -HM_RANGE || coords[i] >= HM_RANGE) { c->err = std::string(who) + ": a block coordinate is not storable (-2^20 <= b < 2^20)"; return ICP_ERR_INVALID_ARG; }
    return ICP_OK;
}
// n block coordinates (checked) on the device in `d_coords`, allocated under the room rule
int htsdf_allocate(icp_ctx* c, int32_t n, const int32_t* coords, DevBuf& d_coords, const char* who) {
    int rc;
    if ((rc = ensure(c, d_coords, (size_t)n * 12))) return rc;
    HIPCK(c, hipMemcpyAsync(d_coords.p, coords, (size_t)n * 12, hipMemcpyHostToDevice, c->stream));
    auto alloc = [&]() {
        hipLaunchKernelGGL(k_htsdf_alloc, dim3((n + 255) / 256), dim3(256), 0, c->stream, htsdf_table(c), (int)n, (const int*)d_coords.as<int>(), c->th_ctr.as<int>());
        return (int)ICP_OK;
    };
    return htsdf_claim(c, alloc, who, nullptr);
}
// A save path: n blocks of a pool (this volume's, or the outbox of an evict) to the host SORTED BY KEY -- the keys first, sorted on the host;
// then the blocks, a slab of at most 4096 (16 MiB) at a time.  Any output may be null.
// d_cpool with rgb_out (n x 512 x 3) and cweight_out (n x 512): the colour pool's blocks in the same order, a slab of at most 2048 (16 MiB).
int htsdf_download_sorted(icp_ctx* c, int n, const void* d_pkey, const void* d_pool, int32_t* coords_out, float* tsdf_out, float* weight_out,
                          const void* d_cpool = nullptr, float* rgb_out = nullptr, float* cweight_out = nullptr) {
    HIPCK(c, hipStreamSynchronize(c->stream));
    std::vector<unsigned long long> keys((size_t)n);
    HIPCK(c, hipMemcpy(keys.data(), d_pkey, (size_t)n * 8, hipMemcpyDeviceToHost));
    std::vector<std::pair<unsigned long long, int>> order((size_t)n);
    for (int i = 0; i < n; i++) order[(size_t)i] = {keys[(size_t)i], i};
    std::sort(order.begin(), order.end());
    std::vector<int> place((size_t)n);                 // pool index -> position in the sorted output
    for (int e = 0; e < n; e++) {
        place[(size_t)order[(size_t)e].second] = e;
        if (coords_out) for (int a = 0; a < 3; a++) coords_out[3 * (size_t)e + a] = (int32_t)((order[(size_t)e].first >> (21 * a)) & 0x1FFFFFull) - HM_RANGE;
    }
    const int slab = 4096, cslab = 2048;              // 16 MiB either way: 4 KiB of geometry, 8 KiB of colour per block
    std::vector<float> h((size_t)(n < cslab ? n : cslab) * 2048);
    if (d_cpool && (rgb_out || cweight_out)) {
        for (int at = 0; at < n; at += cslab) {
            const int m = n - at < cslab ? n - at : cslab;
            HIPCK(c, hipMemcpy(h.data(), (const char*)d_cpool + (size_t)at * 8192, (size_t)m * 8192, hipMemcpyDeviceToHost));
            for (int i = 0; i < m; i++) {
                const size_t e = (size_t)place[(size_t)(at + i)];
                const float* src = h.data() + (size_t)i * 2048;
                if (rgb_out) for (int q = 0; q < 512; q++) for (int a = 0; a < 3; a++) rgb_out[(e * 512 + q) * 3 + a] = src[4 * q + a];
                if (cweight_out) for (int q = 0; q < 512; q++) cweight_out[e * 512 + q] = src[4 * q + 3];
            }
        }
    }
    if (!tsdf_out && !weight_out) return ICP_OK;
    for (int at = 0; at < n; at += slab) {
        const int m = n - at < slab ? n - at : slab;
        HIPCK(c, hipMemcpy(h.data(), (const char*)d_pool + (size_t)at * 4096, (size_t)m * 4096, hipMemcpyDeviceToHost));
        for (int i = 0; i < m; i++) {
            const size_t e = (size_t)place[(size_t)(at + i)];
            const float* src = h.data() + (size_t)i * 1024;
            if (tsdf_out) for (int q = 0; q < 512; q++) tsdf_out[e * 512 + q] = src[2 * q];
            if (weight_out) for (int q = 0; q < 512; q++) weight_out[e * 512 + q] = src[2 * q + 1];
        }
    }
    return ICP_OK;
}
// n block coordinates as sorted keys; false when one occurs twice
bool htsdf_keys_distinct(int32_t n, const int32_t* coords) {
    std::vector<unsigned long long> keys((size_t)n);
    for (int i = 0; i < n; i++) {
        unsigned long long k = 0;
        for (int a = 0; a < 3; a++) k |= (unsigned long long)(uint32_t)(coords[3 * (size_t)i + a] + HM_RANGE) << (21 * a);
        keys[(size_t)i] = k;
    }
    std::sort(keys.begin(), keys.end());
    return std::adjacent_find(keys.begin(), keys.end()) == keys.end();
}
// n blocks in icp_get_tsdf_hashed's layout (their coordinates on the device in d_coords, allocated) placed where they sit in the pool, a
// slab of at most 4096 at a time (waits per slab: the host block and the staging buffer are reused)
int htsdf_place_blocks(icp_ctx* c, int32_t n, const DevBuf& d_coords, const float* tsdf, const float* weight) {
    int rc;
    DevBuf d_in;
    const int slab = 4096;
    const int m_max = n < slab ? n : slab;
    std::vector<float2> h((size_t)m_max * 512);
    if ((rc = ensure(c, d_in, (size_t)m_max * 4096))) return rc;
    for (int at = 0; at < n; at += slab) {
        const int m = n - at < slab ? n - at : slab;
        for (size_t q = 0; q < (size_t)m * 512; q++) h[q] = make_float2(tsdf[(size_t)at * 512 + q], weight[(size_t)at * 512 + q]);
        HIPCK(c, hipMemcpyAsync(d_in.p, h.data(), (size_t)m * 4096, hipMemcpyHostToDevice, c->stream));
        hipLaunchKernelGGL(k_htsdf_place, dim3(m), dim3(512), 0, c->stream, htsdf_view(c), (const int*)(d_coords.as<int>() + 3 * (size_t)at), (const float2*)d_in.as<float2>());
        HIPCK(c, hipGetLastError());
        HIPCK(c, hipStreamSynchronize(c->stream));      // (the host block and d_in are reused by the next slab)
    }
    return ICP_OK;
}
// htsdf_place_blocks for the colour pool: rgb n x 512 x 3 and cweight n x 512, a slab of at most 2048 (16 MiB) at a time.
int htsdf_place_colors(icp_ctx* c, int32_t n, const DevBuf& d_coords, const float* rgb, const float* cweight) {
    int rc;
    DevBuf d_in;
    const int slab = 2048;
    const int m_max = n < slab ? n : slab;
    std::vector<float4> h((size_t)m_max * 512);
    if ((rc = ensure(c, d_in, (size_t)m_max * 8192))) return rc;
    for (int at = 0; at < n; at += slab) {
        const int m = n - at < slab ? n - at : slab;
        for (size_t q = 0; q < (size_t)m * 512; q++) {
            const float* s3 = rgb + ((size_t)at * 512 + q) * 3;
            h[q] = make_float4(s3[0], s3[1], s3[2], cweight[(size_t)at * 512 + q]);
        }
        HIPCK(c, hipMemcpyAsync(d_in.p, h.data(), (size_t)m * 8192, hipMemcpyHostToDevice, c->stream));
        hipLaunchKernelGGL(k_htsdf_place_color, dim3(m), dim3(512), 0, c->stream, htsdf_view(c), c->th_cpool.as<float4>(), (const int*)(d_coords.as<int>() + 3 * (size_t)at),
                           (const float4*)d_in.as<float4>());
        HIPCK(c, hipGetLastError());
        HIPCK(c, hipStreamSynchronize(c->stream));      // (the host block and d_in are reused by the next slab)
    }
    return ICP_OK;
}
// icp_tsdf_create_hashed and icp_tsdf_create_color_hashed: the second adds the colour pool
int htsdf_create(icp_ctx* c, const icp_tsdf_options* opt, int32_t block_capacity, bool color, const char* who);
int htsdf_get(icp_ctx* c, icp_tsdf_hashed_info* info_out, int32_t max_blocks, int32_t* coords_out, float* tsdf_out, float* weight_out, float* rgb_out, float* cweight_out,
              const char* who);
int htsdf_upload(icp_ctx* c, int32_t n, const int32_t* coords, const float* tsdf, const float* weight, const float* rgb, const float* cweight, const char* who);
}  // namespace

int icp_tsdf_create_hashed(icp_ctx* c, const icp_tsdf_options* opt, int32_t block_capacity) {
    if (!c) return ICP_ERR_INVALID_ARG;
    return htsdf_create(c, opt, block_capacity, false, "icp_tsdf_create_hashed");
}
int icp_tsdf_create_color_hashed(icp_ctx* c, const icp_tsdf_options* opt, int32_t block_capacity) {
    if (!c) return ICP_ERR_INVALID_ARG;
    return htsdf_create(c, opt, block_capacity, true, "icp_tsdf_create_color_hashed");
}
int icp_tsdf_hashed_has_color(icp_ctx* c, int32_t* has_out) {
    if (!c) return ICP_ERR_INVALID_ARG;
    int rc;
    if ((rc = htsdf_check(c, "icp_tsdf_hashed_has_color"))) return rc;
    if (has_out) *has_out = c->th_color ? 1 : 0;
    return ICP_OK;
}

namespace {
int htsdf_create(icp_ctx* c, const icp_tsdf_options* opt, int32_t block_capacity, bool color, const char* who) {
    if (!opt) { c->err = std::string(who) + ": null options"; return ICP_ERR_INVALID_ARG; }
    icp_tsdf_options o = *opt;
    o.dims[0] = o.dims[1] = o.dims[2] = 2;             // (ignored: a hashed volume has no extent)
    if (const char* why = tsdf_options_error(&o)) { c->err = std::string(who) + ": " + why; return ICP_ERR_INVALID_ARG; }
    if (!(2.0 * (double)o.truncation / (double)o.voxel_size <= (double)HT_MAX_STEPS)) { c->err = std::string(who) + ": 2 truncation / voxel_size must not exceed 1024"; return ICP_ERR_INVALID_ARG; }
    if (block_capacity < 1 || block_capacity > (1 << HT_MAX_POOL_LOG2)) { c->err = std::string(who) + ": block_capacity must be in 1 .. 2^22"; return ICP_ERR_INVALID_ARG; }
    int rc;
    DrainOnError guard(c);
    if ((rc = set_device(c))) return rc;
    if (c->tsdf_on) { if ((rc = icp_tsdf_release(c))) return rc; }
    o.dims[0] = o.dims[1] = o.dims[2] = 0;
    if (o.ray_step == 0.f) o.ray_step = o.truncation / 2.f;
    c->tsdf_opt = o;
    c->th_color = color;                               // (htsdf_alloc and htsdf_adopt look at it; cleared again if the allocation fails)
    struct Undo { icp_ctx* c; bool armed; ~Undo() { if (armed) { release(c->th_cpool); c->th_color = false; } } } undo{c, true};
    HtBufs b;
    const int l = ht_log2_for(block_capacity);
    if ((rc = htsdf_alloc(c, l, b))) return rc;
    if ((rc = ensure(c, c->th_ctr, HT_NCTR * 4))) return rc;
    if ((rc = ensure(c, c->tsdf_cnt, 16))) return rc;
    HIPCK(c, hipMemsetAsync(c->th_ctr.p, 0, HT_NCTR * 4, c->stream));
    HIPCK(c, hipStreamSynchronize(c->stream));
    htsdf_adopt(c, l, b);
    c->th_nblk = 0; c->th_grown = 0; c->th_unplaced = 0; c->th_oor = 0;
    c->tsdf_hashed = true; c->tsdf_on = true;
    undo.armed = false;
    return guard.done();
}
}  // namespace

int icp_tsdf_reserve_blocks(icp_ctx* c, int32_t block_capacity) {
    if (!c) return ICP_ERR_INVALID_ARG;
    const char* who = "icp_tsdf_reserve_blocks";
    int rc;
    if ((rc = htsdf_check(c, who))) return rc;
    if (block_capacity < 1 || block_capacity > (1 << HT_MAX_POOL_LOG2)) { c->err = std::string(who) + ": block_capacity must be in 1 .. 2^22"; return ICP_ERR_INVALID_ARG; }
    const int l = ht_log2_for(block_capacity);
    if (l + 1 <= c->th_log2cap) return ICP_OK;
    DrainOnError guard(c);
    if ((rc = set_device(c))) return rc;
    HIPCK(c, hipStreamSynchronize(c->stream));
    if ((rc = htsdf_regrow(c, l, c->th_nblk))) return rc;
    return guard.done();
}

int icp_tsdf_allocate_blocks(icp_ctx* c, int32_t n, const int32_t* coords) {
    if (!c) return ICP_ERR_INVALID_ARG;
    const char* who = "icp_tsdf_allocate_blocks";
    int rc;
    if ((rc = htsdf_check(c, who))) return rc;
    if (n < 0 || (n > 0 && !coords)) { c->err = std::string(who) + ": bad argument (n >= 0, coords)"; return ICP_ERR_INVALID_ARG; }
    if ((rc = htsdf_check_coords(c, n, coords, who))) return rc;
    if (n == 0) return ICP_OK;
    DrainOnError guard(c);
    if ((rc = set_device(c))) return rc;
    DevBuf d_coords;
    if ((rc = htsdf_allocate(c, n, coords, d_coords, who))) return rc;      // (waits: d_coords is free to go)
    return guard.done();
}

int icp_get_tsdf_hashed(icp_ctx* c, icp_tsdf_hashed_info* info_out, int32_t max_blocks, int32_t* coords_out, float* tsdf_out, float* weight_out) {
    if (!c) return ICP_ERR_INVALID_ARG;
    int rc;
    if ((rc = htsdf_check(c, "icp_get_tsdf_hashed"))) return rc;
    return htsdf_get(c, info_out, max_blocks, coords_out, tsdf_out, weight_out, nullptr, nullptr, "icp_get_tsdf_hashed");
}
int icp_get_tsdf_color_hashed(icp_ctx* c, icp_tsdf_hashed_info* info_out, int32_t max_blocks, int32_t* coords_out, float* tsdf_out, float* weight_out, float* rgb_out,
                              float* cweight_out) {
    if (!c) return ICP_ERR_INVALID_ARG;
    int rc;
    if ((rc = htsdf_check_color(c, "icp_get_tsdf_color_hashed"))) return rc;
    return htsdf_get(c, info_out, max_blocks, coords_out, tsdf_out, weight_out, rgb_out, cweight_out, "icp_get_tsdf_color_hashed");
}
namespace {
int htsdf_get(icp_ctx* c, icp_tsdf_hashed_info* info_out, int32_t max_blocks, int32_t* coords_out, float* tsdf_out, float* weight_out, float* rgb_out, float* cweight_out,
              const char* who) {
    int rc;
    const int n = c->th_nblk;
    if (info_out) {
        memset(info_out, 0, sizeof(*info_out));
        info_out->n_blocks = n; info_out->capacity = c->th_pool_cap; info_out->n_grown = c->th_grown; info_out->n_unplaced = c->th_unplaced; info_out->n_out_of_range = c->th_oor;
    }
    if (!coords_out && !tsdf_out && !weight_out && !rgb_out && !cweight_out) return ICP_OK;
    if (max_blocks < n) {
        char buf[160];
        snprintf(buf, sizeof(buf), "%s: max_blocks %d is below the %d allocated blocks", who, max_blocks, n);
        c->err = buf; return ICP_ERR_INVALID_ARG;
    }
    if (n == 0) return ICP_OK;
    if ((rc = set_device(c))) return rc;
    return htsdf_download_sorted(c, n, c->th_pkey.p, c->th_pool.p, coords_out, tsdf_out, weight_out, c->th_color ? c->th_cpool.p : nullptr, rgb_out, cweight_out);
}
}  // namespace

int icp_tsdf_upload_hashed(icp_ctx* c, int32_t n, const int32_t* coords, const float* tsdf, const float* weight) {
    if (!c) return ICP_ERR_INVALID_ARG;
    const char* who = "icp_tsdf_upload_hashed";
    int rc;
    if ((rc = htsdf_check(c, who))) return rc;
    if (n < 0 || (n > 0 && (!coords || !tsdf || !weight))) { c->err = std::string(who) + ": bad argument (n >= 0, coords, tsdf, weight)"; return ICP_ERR_INVALID_ARG; }
    return htsdf_upload(c, n, coords, tsdf, weight, nullptr, nullptr, who);      // (a coloured volume: every block uncoloured)
}
int icp_tsdf_upload_color_hashed(icp_ctx* c, int32_t n, const int32_t* coords, const float* tsdf, const float* weight, const float* rgb, const float* cweight) {
    if (!c) return ICP_ERR_INVALID_ARG;
    const char* who = "icp_tsdf_upload_color_hashed";
    int rc;
    if ((rc = htsdf_check_color(c, who))) return rc;
    if (n < 0 || (n > 0 && (!coords || !tsdf || !weight || !rgb || !cweight))) { c->err = std::string(who) + ": bad argument (n >= 0, coords, tsdf, weight, rgb, cweight)"; return ICP_ERR_INVALID_ARG; }
    return htsdf_upload(c, n, coords, tsdf, weight, rgb, cweight, who);
}
namespace {
int htsdf_upload(icp_ctx* c, int32_t n, const int32_t* coords, const float* tsdf, const float* weight, const float* rgb, const float* cweight, const char* who) {
    int rc;
    if ((rc = htsdf_check_coords(c, n, coords, who))) return rc;
    if (!htsdf_keys_distinct(n, coords)) { c->err = std::string(who) + ": a block coordinate occurs twice"; return ICP_ERR_INVALID_ARG; }
    const int l = ht_log2_for(n);
    if (l < 0) { c->err = std::string(who) + ": more than 2^22 blocks"; return ICP_ERR_INVALID_ARG; }
    DrainOnError guard(c);
    if ((rc = set_device(c))) return rc;
    HIPCK(c, hipStreamSynchronize(c->stream));
    // the state is REPLACED: everything forgotten, the pool grown where n blocks need it, the blocks allocated, their voxels placed
    if ((rc = htsdf_reset(c))) return rc;
    if (n > c->th_pool_cap && (rc = htsdf_regrow(c, l, 0))) return rc;
    if (n > 0) {
        DevBuf d_coords;
        if ((rc = htsdf_allocate(c, n, coords, d_coords, who))) return rc;
        if ((rc = htsdf_place_blocks(c, n, d_coords, tsdf, weight))) return rc;
        if (rgb && (rc = htsdf_place_colors(c, n, d_coords, rgb, cweight))) return rc;
    }
    return guard.done();
}
}  // namespace

// Not part of icp_hip.h (tests/test_gpu_htsdf.py): lowers the pool size at which this context's hashed volume refuses to grow from 2^22 blocks
// to 2^log2_blocks, so that the refusal and the restoring of the table can be tested without 16 GiB.
extern "C" int icp_debug_htsdf_max_blocks(icp_ctx* c, int32_t log2_blocks) {
    if (!c || log2_blocks < 0 || log2_blocks > HT_MAX_POOL_LOG2) return ICP_ERR_INVALID_ARG;
    c->th_max_log2 = log2_blocks;
    return ICP_OK;
}

// Not part of icp_hip.h (tools/time_htsdf.py): the device time of ONE touch launch and of ONE integrate launch on the hashed volume between
// events on the context's stream, the frame staged and its blocks allocated outside the brackets (the timed touch claims nothing new).
extern "C" int icp_debug_htsdf_time(icp_ctx* c, const float* depth, const icp_depth_camera* cam, const float pose[16], float* touch_ms_out, float* integrate_ms_out) {
    if (!c || !touch_ms_out || !integrate_ms_out || !depth) return ICP_ERR_INVALID_ARG;
    const char* who = "icp_debug_htsdf_time";
    int rc;
    if ((rc = htsdf_check(c, who))) return rc;
    if ((rc = tsdf_check_call(c, cam, pose, who, true))) return rc;
    DrainOnError guard(c);
    if ((rc = set_device(c))) return rc;
    if ((rc = ensure_events(c, 3))) return rc;
    if ((rc = stage_depth(c, 0, depth, nullptr, cam->width * cam->height, c->stream))) return rc;
    if ((rc = htsdf_integrate_slot(c, 0, *cam, pose, nullptr, who))) return rc;      // (warm; allocates)
    HIPCK(c, hipStreamSynchronize(c->stream));
    const icp_tsdf_options& o = c->tsdf_opt;
    TsdfMat m; memset(&m, 0, sizeof(m));
    invert_extrinsics(pose, m.m);
    TsdfMat P; memcpy(P.m, pose, 64);
    const int n_steps = (int)std::ceil(2.0 * (double)o.truncation / (double)o.voxel_size);
    const float* d = c->depth_dev[0].as<float>();
    HIPCK(c, hipEventRecord(c->events[0], c->stream));
    hipLaunchKernelGGL(k_htsdf_touch, dim3((cam->width + 15) / 16, (cam->height + 15) / 16), dim3(256), 0, c->stream, htsdf_table(c), tsdf_cam(*cam), P, d, o.origin[0], o.origin[1],
                       o.origin[2], o.voxel_size, o.truncation, o.max_depth, n_steps, c->th_ctr.as<int>());
    HIPCK(c, hipEventRecord(c->events[1], c->stream));
    if (c->th_nblk > 0) hipLaunchKernelGGL(k_htsdf_integrate, dim3(c->th_nblk), dim3(512), 0, c->stream, htsdf_view(c), tsdf_cam(*cam), m, d, c->tsdf_cnt.as<int>());
    HIPCK(c, hipEventRecord(c->events[2], c->stream));
    HIPCK(c, hipGetLastError());
    HIPCK(c, hipStreamSynchronize(c->stream));
    HIPCK(c, hipEventElapsedTime(touch_ms_out, c->events[0], c->events[1]));
    HIPCK(c, hipEventElapsedTime(integrate_ms_out, c->events[1], c->events[2]));
    HIPCK(c, hipMemsetAsync(c->th_ctr.as<int>() + HT_UNPLACED, 0, 8, c->stream));      // (the timed touch counted its samples out of range again)
    HIPCK(c, hipStreamSynchronize(c->stream));
    return guard.done();
}

// Not part of icp_hip.h (tools/time_htsdf_color.py): icp_debug_htsdf_time's integrate figure for ONE k_htsdf_integrate_color launch on a
// coloured hashed volume, the frames staged and their blocks allocated outside the bracket.
extern "C" int icp_debug_htsdf_color_time(icp_ctx* c, const float* depth, const uint8_t* rgbx, const icp_depth_camera* cam, const float pose[16], float* integrate_ms_out) {
    if (!c || !integrate_ms_out || !depth || !rgbx) return ICP_ERR_INVALID_ARG;
    const char* who = "icp_debug_htsdf_color_time";
    int rc;
    if ((rc = htsdf_check_color(c, who))) return rc;
    if ((rc = tsdf_check_call(c, cam, pose, who, true))) return rc;
    DrainOnError guard(c);
    if ((rc = set_device(c))) return rc;
    if ((rc = ensure_events(c, 2))) return rc;
    if ((rc = stage_depth(c, 0, depth, rgbx, cam->width * cam->height, c->stream))) return rc;
    if ((rc = htsdf_integrate_slot(c, 0, *cam, pose, nullptr, who, true))) return rc;      // (warm; allocates)
    HIPCK(c, hipStreamSynchronize(c->stream));
    *integrate_ms_out = 0.f;
    if (c->th_nblk > 0) {
        TsdfMat m; memset(&m, 0, sizeof(m));
        invert_extrinsics(pose, m.m);
        const float* d = c->depth_dev[0].as<float>();
        HIPCK(c, hipEventRecord(c->events[0], c->stream));
        hipLaunchKernelGGL(k_htsdf_integrate_color, dim3(c->th_nblk), dim3(512), 0, c->stream, htsdf_view(c), tsdf_cam(*cam), m, d, c->tsdf_cnt.as<int>(),
                           (const uint32_t*)(d + (size_t)cam->width * cam->height), c->th_cpool.as<float4>(), c->tsdf_cnt.as<int>() + 1);
        HIPCK(c, hipEventRecord(c->events[1], c->stream));
        HIPCK(c, hipGetLastError());
        HIPCK(c, hipStreamSynchronize(c->stream));
        HIPCK(c, hipEventElapsedTime(integrate_ms_out, c->events[0], c->events[1]));
    }
    return guard.done();
}
