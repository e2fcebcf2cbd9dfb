// dev_tsdf_cloud_color.hpp -- the colours of a cloud (a laser scan) fused into the COLOURED TSDF volume, dense or hashed, with its geometry
// (icp_tsdf_integrate_cloud_color): a second walk of every usable ray through the band, m = 0 .. M, behind the geometry accumulate -- the
// plain one or the carving one, which it does not depend on -- and a second fold.  Contract: include/icp_hip.h, DESIGN.md section 6zh;
// tests/tsdf_cloud_color_restatement.py states the same arithmetic in numpy.  Part of icp_device.hpp (included from there, inside
// namespace icpdev, after dev_tsdf_carve.hpp).
// ------------------------------------------------------------------------------------------------
// A band sample colours its voxel iff its observation is not skipped and !(sdf > truncation): icp_tsdf_integrate_color's band rule.  The
// point's three bytes are summed per voxel in INTEGERS -- four 32-bit words (SR, SG, SB, NC), 16 bytes by the voxel's storage index -- and
// folded into the float4 (R, G, B, Wc) once per voxel, so nothing depends on the order of the points or on a race.  A ray meets a voxel
// at most once and a cloud has at most 2^24 points: NC <= 2^24, every sum <= 255 2^24 < 2^32.  The fold zeroes what it read.
// Two things decide the cost of the accumulate.  Each is a constant of the build, so that a library with either form of each can be built
// and timed (tools/time_tsdf_cloud_color.py; DESIGN.md section 6zh has the table); integers: every form gives the same bits.
//   PACK     the four words as two 64-bit atomics, SR | SG << 32 and SB | NC << 32: no field can carry into its neighbour.
//   COMBINE  runs of neighbouring lanes with the same storage index summed with dev_tsdf_carve.hpp's segmented shuffle sum, the four
//            values in one 64-bit word of 16-bit fields (64 lanes x 255 < 2^16); the run's head issues the atomics.
// Integer atomics and vector stores only; every fp32 operation of the contract in the contract's order.
#ifndef ICP_TSDF_COLOR_PACK
#define ICP_TSDF_COLOR_PACK 1         // measured: 1.8 x the four 32-bit atomics on a 370 k-point scan, hashed and dense
#endif
#ifndef ICP_TSDF_COLOR_COMBINE
#define ICP_TSDF_COLOR_COMBINE 1      // measured: 2.5 to 2.8 x on top of either form of the atomics
#endif
constexpr bool TCC_PACK = ICP_TSDF_COLOR_PACK != 0, TCC_COMBINE = ICP_TSDF_COLOR_COMBINE != 0;
constexpr int TCC_COLORED = 5, TCC_NCTR = 6;      // the sixth 64-bit counter of a coloured call: the voxels the colour fold wrote

// tc_observe with the distance kept: false when the voxel lies further than the truncation behind the point; else sdf.
__device__ __forceinline__ bool tcc_observe(const TcRay& q, const TcGrid& g, float gx, float gy, float gz, float& sdf) {
    const float x = g.ox + gx * g.s, y = g.oy + gy * g.s, z = g.oz + gz * g.s;
    const float ex = x - q.cx, ey = y - q.cy, ez = z - q.cz;
    const float proj = ex * q.ux + (ey * q.uy + ez * q.uz);
    sdf = q.r - proj;
    return !(sdf < -g.trunc);
}
// (r, g, b, n) into the voxel's four words
template <bool PACK>
__device__ __forceinline__ void tcc_add(uint32_t* __restrict__ acc, unsigned long long at, uint32_t r, uint32_t g, uint32_t b, uint32_t n) {
    if (PACK) {
        unsigned long long* a = (unsigned long long*)(acc + 4ull * at);
        atomicAdd(a, (unsigned long long)r | ((unsigned long long)g << 32));
        atomicAdd(a + 1, (unsigned long long)b | ((unsigned long long)n << 32));
    } else {
        uint32_t* a = acc + 4ull * at;
        atomicAdd(a, r); atomicAdd(a + 1, g); atomicAdd(a + 2, b); atomicAdd(a + 3, n);
    }
}
// One step's colours of a wave (every lane of the wave calls; at == TCV_NONE: the lane has none): tcv_run_add with the packed word.
template <bool PACK>
__device__ __forceinline__ void tcc_run_add(int lane, unsigned long long at, uint32_t c, uint32_t* __restrict__ acc) {
    if (!__ballot(at != TCV_NONE)) return;             // (uniform)
    unsigned long long w = (unsigned long long)(c & 255u) | ((unsigned long long)((c >> 8) & 255u) << 16) | ((unsigned long long)((c >> 16) & 255u) << 32) | (1ull << 48);
    const unsigned long long left = __shfl_up(at, 1, WAVE);
    const bool head = lane == 0 || left != at;
    const unsigned long long heads = __ballot(head);
    if (heads != ~0ull) {                              // (uniform)
        const int run = __popcll(heads & (~0ull >> (63 - lane)));
        for (int off = 1; off < WAVE; off <<= 1) {
            const bool same = __shfl_down(run, off, WAVE) == run && lane + off < WAVE;
            const unsigned long long ow = __shfl_down(w, off, WAVE);
            if (same) w += ow;
        }
    }
    if (head && at != TCV_NONE) tcc_add<PACK>(acc, at, (uint32_t)(w & 0xffffull), (uint32_t)((w >> 16) & 0xffffull), (uint32_t)((w >> 32) & 0xffffull), (uint32_t)(w >> 48));
}

// The colour walk: tc_accumulate_body's samples, ranges and rule about repeated voxels, whatever the carve options are; no counters.
template <bool HASHED, bool PACK, bool COMBINE>
__device__ __forceinline__ void tcc_body(const HtVol& v, int nx, int ny, int nz, const TcCloud& cl, const uint32_t* __restrict__ rgba, const TsdfMat& pose, float ex, float ey,
                                         float ez, const TcGrid& g, uint32_t* __restrict__ acc) {
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * 256 + threadIdx.x;
    const TcRay q = tc_ray(cl, i, pose.m, ex, ey, ez, g.max_d);
    const uint32_t c = q.usable ? rgba[i] : 0u;      // (usable: i < cl.n)
    unsigned long long prev_key = HM_EMPTY;
    int prev_blk = -1;
    float pgx = 0.f, pgy = 0.f, pgz = 0.f;
    bool have_prev = false;
    const float hx = (float)(nx - 1), hy = (float)(ny - 1), hz = (float)(nz - 1);
    for (int m = 0; m <= g.n_steps; m++) {             // (uniform: the shuffles of COMBINE are legal)
        unsigned long long at = TCV_NONE;
        float gx = 0.f, gy = 0.f, gz = 0.f;
        if (tc_sample(q, g, m, gx, gy, gz)) {
            const bool in = HASHED ? (gx >= HT_VOX_LO && gx <= HT_VOX_HI && gy >= HT_VOX_LO && gy <= HT_VOX_HI && gz >= HT_VOX_LO && gz <= HT_VOX_HI)
                                   : (gx >= 0.f && gx <= hx && gy >= 0.f && gy <= hy && gz >= 0.f && gz <= hz);      // in float, before the cast: NaN is outside
            if (in && !(have_prev && gx == pgx && gy == pgy && gz == pgz)) {
                have_prev = true; pgx = gx; pgy = gy; pgz = gz;
                float sdf;
                if (tcc_observe(q, g, gx, gy, gz, sdf) && !(sdf > g.trunc)) {
                    const int ix = (int)gx, iy = (int)gy, iz = (int)gz;
                    if (HASHED) {
                        const unsigned long long key = hm_key(ix >> 3, iy >> 3, iz >> 3);
                        if (key != prev_key) { prev_key = key; prev_blk = ht_lookup(v, ix >> 3, iy >> 3, iz >> 3); }
                        if (prev_blk >= 0 && prev_blk < v.pool_cap)      // (the touch is exact: always)
                            at = (unsigned long long)prev_blk * 512ull + (unsigned long long)((iz & 7) * 64 + (iy & 7) * 8 + (ix & 7));
                    } else at = ((unsigned long long)iz * (unsigned long long)ny + (unsigned long long)iy) * (unsigned long long)nx + (unsigned long long)ix;
                }
            }
        }
        if (COMBINE) tcc_run_add<PACK>(lane, at, c, acc);
        else if (at != TCV_NONE) tcc_add<PACK>(acc, at, c & 255u, (c >> 8) & 255u, (c >> 16) & 255u, 1u);
    }
}
__global__ __launch_bounds__(256) void k_htsdf_accumulate_cloud_color(const HtVol v, const TcCloud cl, const uint32_t* __restrict__ rgba, const TsdfMat pose, float ex, float ey,
                                                                      float ez, const TcGrid g, uint32_t* __restrict__ acc) {
    tcc_body<true, TCC_PACK, TCC_COMBINE>(v, 0, 0, 0, cl, rgba, pose, ex, ey, ez, g, acc);
}
__global__ __launch_bounds__(256) void k_tsdf_accumulate_cloud_color(int nx, int ny, int nz, const TcCloud cl, const uint32_t* __restrict__ rgba, const TsdfMat pose, float ex,
                                                                     float ey, float ez, const TcGrid g, uint32_t* __restrict__ acc) {
    HtVol none = {};
    tcc_body<false, TCC_PACK, TCC_COMBINE>(none, nx, ny, nz, cl, rgba, pose, ex, ey, ez, g, acc);
}

// The fold of one voxel: C <- (Wc C + cbar) / (Wc + 1) per channel, Wc <- min(Wc + 1, max_weight) where the scan coloured it; one 16-byte
// load of the accumulators, one 16-byte load and store of the colour, the accumulators back to zero with one 16-byte store.
__device__ __forceinline__ bool tcc_fold_voxel(float4* __restrict__ col, uint4* __restrict__ acc, size_t at, float max_w) {
    const uint4 a = acc[at];
    if (a.w == 0u) return false;
    const double n = (double)a.w;
    const float cr = (float)((double)a.x / n), cg = (float)((double)a.y / n), cb = (float)((double)a.z / n);
    const float4 o = col[at];
    float4 r;
    r.x = (o.w * o.x + cr) / (o.w + 1.f);
    r.y = (o.w * o.y + cg) / (o.w + 1.f);
    r.z = (o.w * o.z + cb) / (o.w + 1.f);
    r.w = fminf(o.w + 1.f, max_w);
    col[at] = r;
    acc[at] = make_uint4(0u, 0u, 0u, 0u);
    return true;
}
// Hashed: k_htsdf_fold_cloud's shape, one work-group per pool block, a lane per voxel.
__global__ __launch_bounds__(512) void k_htsdf_fold_cloud_color(float4* __restrict__ cpool, float max_w, uint4* __restrict__ acc, unsigned long long* __restrict__ ctr) {
    __shared__ int red[8];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const bool upd = tcc_fold_voxel(cpool, acc, (size_t)blockIdx.x * 512 + tid, max_w);
    const unsigned long long bu = __ballot(upd);
    if (lane == 0) red[wave] = __popcll(bu);
    __syncthreads();
    if (tid == 0) {
        const int t = ((red[0] + red[1]) + (red[2] + red[3])) + ((red[4] + red[5]) + (red[6] + red[7]));
        if (t) atomicAdd(&ctr[TCC_COLORED], (unsigned long long)t);
    }
}
// Dense: k_tsdf_fold_cloud's tiling, one thread per (i, j) walks TSDF_KCHUNK voxels along k.
__global__ __launch_bounds__(256) void k_tsdf_fold_cloud_color(float4* __restrict__ col, int nx, int ny, int nz, float max_w, uint4* __restrict__ acc,
                                                               unsigned long long* __restrict__ ctr) {
    __shared__ int red[4];
    const int i = blockIdx.x * 64 + threadIdx.x, j = blockIdx.y * 4 + threadIdx.y;
    const bool in = i < nx && j < ny;
    const int k0 = blockIdx.z * TSDF_KCHUNK, k1 = min(k0 + TSDF_KCHUNK, nz);
    const size_t plane = (size_t)nx * ny;
    size_t idx = (size_t)k0 * plane + (size_t)j * nx + i;
    int cnt = 0;
    for (int k = k0; k < k1; k++, idx += plane) {
        const bool upd = in && tcc_fold_voxel(col, acc, idx, max_w);
        cnt += __popcll(__ballot(upd));
    }
    if (threadIdx.x == 0) red[threadIdx.y] = cnt;
    __syncthreads();
    if (threadIdx.x == 0 && threadIdx.y == 0) {
        const int t = (red[0] + red[1]) + (red[2] + red[3]);
        if (t) atomicAdd(&ctr[TCC_COLORED], (unsigned long long)t);
    }
}
