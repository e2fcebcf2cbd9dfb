// dev_tsdf_cloud.hpp -- an unorganised cloud (a laser scan) fused into the TSDF volume, dense or hashed (icp_tsdf_integrate_cloud): every
// usable point is a ray from the sensor centre, walked through the truncation band in steps of one voxel; each sample observes its
// NEAREST voxel.  Contract: include/icp_hip.h; tests/tsdf_cloud_restatement.py states the same arithmetic in numpy.
// Part of icp_device.hpp (included from there, inside namespace icpdev, after dev_tsdf_hash.hpp).
// ------------------------------------------------------------------------------------------------
// Many rays of one scan reach the same voxel, in an order nobody fixes: the scan is therefore accumulated per voxel in INTEGERS -- S, the
// sum of the observations quantised to 1/32768 (64-bit), and N, their number (32-bit), two plain arrays by the voxel's storage index --
// and folded into the float2 once per voxel, so nothing depends on the order of the points or on a race.  The fold zeroes what it read:
// the accumulators are all zero outside a call.  Integer atomics and vector stores only; every fp32 operation in the contract's order.
constexpr float HT_VOX_LO = -8388608.f, HT_VOX_HI = 8388607.f;      // voxels whose block is storable: -2^23 <= g <= 2^23 - 1
constexpr float TC_SCALE = 32768.f;
constexpr int TC_RAYS = 0, TC_SAMPLES = 1, TC_OUTSIDE = 2, TC_UPDATED = 3, TC_NCTR = 4;      // 64-bit counters of one call
struct TcCloud { const float* x; const float* y; const float* z; int n; };
struct TcGrid { float ox, oy, oz, s, trunc, max_d; int n_steps; };
struct TcRay { float cx, cy, cz, ux, uy, uz, r; bool usable; };

// The ray of point i at `pose` (column-major) from the sensor origin e (scan frame): centre, unit direction, range.
__device__ __forceinline__ TcRay tc_ray(const TcCloud& cl, int i, const float* __restrict__ P, float ex, float ey, float ez, float max_d) {
    TcRay q;
    q.cx = (P[0] * ex + (P[4] * ey + P[8] * ez)) + P[12];
    q.cy = (P[1] * ex + (P[5] * ey + P[9] * ez)) + P[13];
    q.cz = (P[2] * ex + (P[6] * ey + P[10] * ez)) + P[14];
    q.ux = q.uy = q.uz = 0.f; q.r = 0.f; q.usable = false;
    if (i < cl.n) {
        const float px = cl.x[i], py = cl.y[i], pz = cl.z[i];
        if (isfinite(px) && isfinite(py) && isfinite(pz)) {
            const float wx = (P[0] * px + (P[4] * py + P[8] * pz)) + P[12];
            const float wy = (P[1] * px + (P[5] * py + P[9] * pz)) + P[13];
            const float wz = (P[2] * px + (P[6] * py + P[10] * pz)) + P[14];
            const float dx = wx - q.cx, dy = wy - q.cy, dz = wz - q.cz;
            const float r2 = dx * dx + (dy * dy + dz * dz);
            const float r = sqrtf(r2);
            if (isfinite(r) && r > 0.f && r <= max_d) { q.usable = true; q.r = r; q.ux = dx / r; q.uy = dy / r; q.uz = dz / r; }
        }
    }
    return q;
}
// Sample m of the ray: false when the ray has none there (unusable, or t_m <= 0); else the nearest voxel as three floats (integers, or
// what the range test will refuse: NaN never passes it).
__device__ __forceinline__ bool tc_sample(const TcRay& q, const TcGrid& g, int m, float& gx, float& gy, float& gz) {
    const float t = fminf((q.r - g.trunc) + (float)m * g.s, q.r + g.trunc);
    if (!(q.usable && t > 0.f)) return false;
    const float x = q.cx + t * q.ux, y = q.cy + t * q.uy, z = q.cz + t * q.uz;
    gx = floorf(((x - g.ox) / g.s) + 0.5f); gy = floorf(((y - g.oy) / g.s) + 0.5f); gz = floorf(((z - g.oz) / g.s) + 0.5f);
    return true;
}
// The observation of voxel g by the ray: false when the voxel lies further than the truncation behind the point; else k.
__device__ __forceinline__ bool tc_observe(const TcRay& q, const TcGrid& g, float gx, float gy, float gz, int& k) {
    const float x = g.ox + gx * g.s, y = g.oy + gy * g.s, z = g.oz + gz * g.s;      // (gx is (float)g already)
    const float ex = x - q.cx, ey = y - q.cy, ez = z - q.cz;
    const float proj = ex * q.ux + (ey * q.uy + ez * q.uz);
    const float sdf = q.r - proj;
    if (sdf < -g.trunc) return false;
    const float f = fminf(1.f, sdf / g.trunc);
    k = (int)rintf(f * TC_SCALE);
    return true;
}
// a wave's sum of v into ctr[which], one atomic (every lane of the wave calls)
__device__ __forceinline__ void tc_count(unsigned long long* __restrict__ ctr, int which, int v, int lane) {
    if (!__ballot(v != 0)) return;                     // (uniform)
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, WAVE);
    if (lane == 0) atomicAdd(&ctr[which], (unsigned long long)v);
}

// Allocation in front of the accumulate, from the cloud and the pose alone: one ray per lane, k_htsdf_touch's shape without the eight
// corners.  The walk is uniform (every lane takes all n_steps + 1 steps), so the shuffle is legal.
__global__ __launch_bounds__(256) void k_htsdf_touch_cloud(const HtTable t, const TcCloud cl, const TsdfMat pose, float ex, float ey, float ez, const TcGrid g,
                                                           int* __restrict__ ctr) {
    const int lane = threadIdx.x & 63;
    const TcRay q = tc_ray(cl, blockIdx.x * 256 + threadIdx.x, pose.m, ex, ey, ez, g.max_d);
    unsigned long long prev = HM_EMPTY;
    for (int m = 0; m <= g.n_steps; m++) {
        float gx = 0.f, gy = 0.f, gz = 0.f;
        bool active = tc_sample(q, g, m, gx, gy, gz);
        active = active && gx >= HT_VOX_LO && gx <= HT_VOX_HI && gy >= HT_VOX_LO && gy <= HT_VOX_HI && gz >= HT_VOX_LO && gz <= HT_VOX_HI;      // in float, before the cast
        const unsigned long long key = active ? hm_key((int)gx >> 3, (int)gy >> 3, (int)gz >> 3) : HM_EMPTY;
        const unsigned long long left = __shfl_up(key, 1, WAVE);
        if (key != HM_EMPTY) {
            if (key != prev && !(lane > 0 && left == key)) ht_touch_block(t, key, ctr);
            prev = key;
        }
    }
}

// The accumulate: the same walk; HASHED: the sample's block by lookup, remembered per lane while the key repeats; else the box index.
// Two integer atomics per observation.
template <bool HASHED>
__device__ __forceinline__ void tc_accumulate_body(const HtVol& v, int nx, int ny, int nz, const TcCloud& cl, const TsdfMat& pose, float ex, float ey, float ez, const TcGrid& g,
                                                   unsigned long long* __restrict__ S, int* __restrict__ N, unsigned long long* __restrict__ ctr) {
    const int lane = threadIdx.x & 63;
    const TcRay q = tc_ray(cl, blockIdx.x * 256 + threadIdx.x, pose.m, ex, ey, ez, g.max_d);
    unsigned long long prev_key = HM_EMPTY;
    int prev_blk = -1, n_samples = 0, n_outside = 0;
    float pgx = 0.f, pgy = 0.f, pgz = 0.f;
    bool have_prev = false;
    const float hx = (float)(nx - 1), hy = (float)(ny - 1), hz = (float)(nz - 1);
    for (int m = 0; m <= g.n_steps; m++) {
        float gx = 0.f, gy = 0.f, gz = 0.f;
        if (!tc_sample(q, g, m, gx, gy, gz)) continue;
        const bool in = HASHED ? (gx >= HT_VOX_LO && gx <= HT_VOX_HI && gy >= HT_VOX_LO && gy <= HT_VOX_HI && gz >= HT_VOX_LO && gz <= HT_VOX_HI)
                               : (gx >= 0.f && gx <= hx && gy >= 0.f && gy <= hy && gz >= 0.f && gz <= hz);      // in float, before the cast: NaN is outside
        if (!in) { n_outside++; continue; }
        if (have_prev && gx == pgx && gy == pgy && gz == pgz) continue;
        have_prev = true; pgx = gx; pgy = gy; pgz = gz;
        n_samples++;
        int k;
        if (!tc_observe(q, g, gx, gy, gz, k)) continue;
        const int ix = (int)gx, iy = (int)gy, iz = (int)gz;
        size_t at;
        if (HASHED) {
            const unsigned long long key = hm_key(ix >> 3, iy >> 3, iz >> 3);
            if (key != prev_key) { prev_key = key; prev_blk = ht_lookup(v, ix >> 3, iy >> 3, iz >> 3); }
            if (prev_blk < 0 || prev_blk >= v.pool_cap) continue;      // (the touch is exact: cannot happen)
            at = (size_t)prev_blk * 512 + (size_t)((iz & 7) * 64 + (iy & 7) * 8 + (ix & 7));
        } else at = ((size_t)iz * ny + (size_t)iy) * nx + (size_t)ix;
        atomicAdd(&S[at], (unsigned long long)(long long)k);
        atomicAdd(&N[at], 1);
    }
    tc_count(ctr, TC_RAYS, q.usable ? 1 : 0, lane);
    tc_count(ctr, TC_SAMPLES, n_samples, lane);
    tc_count(ctr, TC_OUTSIDE, n_outside, lane);
}
__global__ __launch_bounds__(256) void k_htsdf_accumulate_cloud(const HtVol v, const TcCloud cl, const TsdfMat pose, float ex, float ey, float ez, const TcGrid g,
                                                                unsigned long long* __restrict__ S, int* __restrict__ N, unsigned long long* __restrict__ ctr) {
    tc_accumulate_body<true>(v, 0, 0, 0, cl, pose, ex, ey, ez, g, S, N, ctr);
}
__global__ __launch_bounds__(256) void k_tsdf_accumulate_cloud(int nx, int ny, int nz, const TcCloud cl, const TsdfMat pose, float ex, float ey, float ez, const TcGrid g,
                                                               unsigned long long* __restrict__ S, int* __restrict__ N, unsigned long long* __restrict__ ctr) {
    HtVol none = {};
    tc_accumulate_body<false>(none, nx, ny, nz, cl, pose, ex, ey, ez, g, S, N, ctr);
}

// The fold of one voxel: D <- (W D + fbar) / (W + 1), W <- min(W + 1, max_weight) where the scan observed it; the accumulators back to zero.
__device__ __forceinline__ bool tc_fold_voxel(float2* __restrict__ vox, unsigned long long* __restrict__ S, int* __restrict__ N, size_t at, float max_w) {
    const int n = N[at];
    if (n <= 0) return false;
    const long long s = (long long)S[at];
    const float fbar = (float)((double)s / ((double)n * 32768.0));
    const float2 o = vox[at];
    float2 r;
    r.x = (o.y * o.x + fbar) / (o.y + 1.f);
    r.y = fminf(o.y + 1.f, max_w);
    vox[at] = r;
    S[at] = 0ull; N[at] = 0;
    return true;
}
// Hashed: one work-group per pool block, a lane per voxel.
__global__ __launch_bounds__(512) void k_htsdf_fold_cloud(float2* __restrict__ pool, float max_w, unsigned long long* __restrict__ S, int* __restrict__ N,
                                                          unsigned long long* __restrict__ ctr) {
    __shared__ int red[8];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const bool upd = tc_fold_voxel(pool, S, N, (size_t)blockIdx.x * 512 + tid, max_w);
    const unsigned long long bu = __ballot(upd);
    if (lane == 0) red[wave] = __popcll(bu);
    __syncthreads();
    if (tid == 0) {
        const int t = ((red[0] + red[1]) + (red[2] + red[3])) + ((red[4] + red[5]) + (red[6] + red[7]));
        if (t) atomicAdd(&ctr[TC_UPDATED], (unsigned long long)t);
    }
}
// Dense: k_tsdf_integrate's tiling, one thread per (i, j) walks TSDF_KCHUNK voxels along k.
__global__ __launch_bounds__(256) void k_tsdf_fold_cloud(float2* __restrict__ vox, int nx, int ny, int nz, float max_w, unsigned long long* __restrict__ S, int* __restrict__ N,
                                                         unsigned long long* __restrict__ ctr) {
    __shared__ int red[4];
    const int i = blockIdx.x * 64 + threadIdx.x, j = blockIdx.y * 4 + threadIdx.y;
    const bool in = i < nx && j < ny;
    const int k0 = blockIdx.z * TSDF_KCHUNK, k1 = min(k0 + TSDF_KCHUNK, nz);
    const size_t plane = (size_t)nx * ny;
    size_t idx = (size_t)k0 * plane + (size_t)j * nx + i;
    int cnt = 0;
    for (int k = k0; k < k1; k++, idx += plane) {
        const bool upd = in && tc_fold_voxel(vox, S, N, idx, max_w);
        cnt += __popcll(__ballot(upd));
    }
    if (threadIdx.x == 0) red[threadIdx.y] = cnt;
    __syncthreads();
    if (threadIdx.x == 0 && threadIdx.y == 0) {
        const int t = (red[0] + red[1]) + (red[2] + red[3]);
        if (t) atomicAdd(&ctr[TC_UPDATED], (unsigned long long)t);
    }
}
