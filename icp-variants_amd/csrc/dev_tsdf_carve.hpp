// dev_tsdf_carve.hpp -- free space carved while a cloud is fused into the TSDF volume (icp_set_tsdf_carve_options): the accumulate of
// dev_tsdf_cloud.hpp with its walk started J steps in front of the band, m = -J .. M.  A sample with m < 0 observes its nearest voxel with
// the band's own observation wherever the voxel HAS STORAGE (dense: in the box; hashed: its block resident after the call's touch) and does
// nothing and counts nowhere else.  Contract: include/icp_hip.h; tests/tsdf_carve_restatement.py states the same
// arithmetic in numpy.  Part of icp_device.hpp (included from there, inside namespace icpdev, after dev_tsdf_cloud.hpp).
// ------------------------------------------------------------------------------------------------
// With carving on these kernels REPLACE the accumulate launch (touch and fold are dev_tsdf_cloud.hpp's, unchanged).  Two things decide the
// cost.  Each is a constant of the build, so that a library with either form of each can be built and timed (tools/time_tsdf_carve.py;
// DESIGN.md section 6zg has the table): the product combines and does not jump.
//   COMBINE  near the sensor whole waves share a voxel: runs of neighbouring lanes with the same storage index are summed with a segmented
//            shuffle sum (k_vmap_insert's) and the run's head issues the two atomics.  Integers: any combining is exact.
//   SKIP     a sample without storage says where the next one with storage can be: hashed, the first sample that may lie outside the
//            missing block; dense, the first that may lie inside the box.  Every skip is VERIFIED, not trusted: each axis of the voxel
//            sequence g_a(m) is monotone in m in fp32 itself (t_m is non-decreasing in m; t u_a, c_a + ., (. - o_a) / s, . + 0.5f and floorf
//            are monotone), so when the LAST skipped sample lies in the same block as the first (or outside the box on the same side of
//            the same axis) every sample between them does too.  The estimate only has to be good, the check makes it legal.
// The same monotony is why a ray never returns to a voxel it left, and why the rule about repeated voxels needs no memory beyond the last
// voxel seen: dropping samples without storage from the walk cannot change which observations are applied.
// Integer atomics and vector stores only; every fp32 operation of the contract in the contract's order.
#ifndef ICP_TSDF_CARVE_COMBINE
#define ICP_TSDF_CARVE_COMBINE 1      // measured: 2.2 to 2.9 x the plain atomics on a 370 k-point scan, hashed and dense
#endif
#ifndef ICP_TSDF_CARVE_SKIP
#define ICP_TSDF_CARVE_SKIP 0         // measured: within the spread of the repeats in a room, where space without storage is short
#endif
constexpr bool TCV_COMBINE = ICP_TSDF_CARVE_COMBINE != 0, TCV_SKIP = ICP_TSDF_CARVE_SKIP != 0;
constexpr int TC_CARVED = 4, TCV_NCTR = 5;      // the fifth 64-bit counter of a call: the applied m < 0 observations
constexpr unsigned long long TCV_NONE = ~0ull;
struct TcCarve { int j_steps; float min_range; };

__device__ __forceinline__ float tcv_t(const TcRay& q, const TcGrid& g, int m) { return fminf((q.r - g.trunc) + (float)m * g.s, q.r + g.trunc); }
// tc_sample's voxel at t, and p: the arguments of its floorf (the position in voxels, + 0.5)
__device__ __forceinline__ void tcv_voxel(const TcRay& q, const TcGrid& g, float t, float (&p)[3], float& gx, float& gy, float& gz) {
    const float x = q.cx + t * q.ux, y = q.cy + t * q.uy, z = q.cz + t * q.uz;
    p[0] = ((x - g.ox) / g.s) + 0.5f; p[1] = ((y - g.oy) / g.s) + 0.5f; p[2] = ((z - g.oz) / g.s) + 0.5f;
    gx = floorf(p[0]); gy = floorf(p[1]); gz = floorf(p[2]);
}
// The lane's first m: the smallest m >= -J whose t_m > min_range, or 0 (the band's own test is t_m > 0), or M + 1 for a ray that is not
// usable.  An estimate, then exact steps either way: t_m is non-decreasing in m.
__device__ __forceinline__ int tcv_first(const TcRay& q, const TcGrid& g, const TcCarve& cv) {
    if (!q.usable) return g.n_steps + 1;
    const float est = floorf((cv.min_range - (q.r - g.trunc)) / g.s);
    int m = !(est < 0.f) ? 0 : (est <= -(float)cv.j_steps ? -cv.j_steps : (int)est);
    while (m > -cv.j_steps && tcv_t(q, g, m - 1) > cv.min_range) m--;
    while (m < 0 && !(tcv_t(q, g, m) > cv.min_range)) m++;
    return m;
}
// Sample `cur` (< 0) lies in block (bx, by, bz), which is not resident: the next m to look at.  cur + n with every sample cur .. cur + n - 1
// in that block (verified on the last), else cur + 1.
__device__ __forceinline__ int tcv_leave_block(const TcRay& q, const TcGrid& g, int cur, const float (&p)[3], int bx, int by, int bz) {
    const float u[3] = {q.ux, q.uy, q.uz};
    const int b[3] = {bx, by, bz};
    float steps = 1.0e9f;
#pragma unroll
    for (int a = 0; a < 3; a++) {
        const float lo = (float)(b[a] * 8);
        if (u[a] > 0.f) steps = fminf(steps, ((lo + 8.f) - p[a]) / u[a]);
        else if (u[a] < 0.f) steps = fminf(steps, (p[a] - lo) / -u[a]);
    }
    const int n = steps >= (float)(-cur) ? -cur : (int)steps;      // (never past m = -1: the band is the existing walk)
    if (n < 2) return cur + 1;
    float pp[3], gx, gy, gz;
    tcv_voxel(q, g, tcv_t(q, g, cur + n - 1), pp, gx, gy, gz);
    const bool in = gx >= HT_VOX_LO && gx <= HT_VOX_HI && gy >= HT_VOX_LO && gy <= HT_VOX_HI && gz >= HT_VOX_LO && gz <= HT_VOX_HI;
    if (in && ((int)gx >> 3) == bx && ((int)gy >> 3) == by && ((int)gz >> 3) == bz) return cur + n;
    return cur + 1;
}
// Sample `cur` (< 0) lies outside the box: the next m to look at.  On an axis where the ray is outside and does not move towards the box
// no m < 0 sample can be inside: 0.  Else cur + n with the last skipped sample still outside on the same side of the axis that takes the
// ray longest to reach (verified), else cur + 1.
__device__ __forceinline__ int tcv_enter_box(const TcRay& q, const TcGrid& g, int cur, const float (&p)[3], float gx, float gy, float gz, float hx, float hy, float hz) {
    const float u[3] = {q.ux, q.uy, q.uz}, gv[3] = {gx, gy, gz}, h[3] = {hx, hy, hz};
    float steps = 0.f, bound = 0.f;
    int axis = -1, side = 0;
#pragma unroll
    for (int a = 0; a < 3; a++) {
        if (gv[a] < 0.f) {
            if (!(u[a] > 0.f)) return 0;
            const float sa = (0.f - p[a]) / u[a];
            if (axis < 0 || sa > steps) { steps = sa; axis = a; side = -1; bound = 0.f; }
        } else if (gv[a] > h[a]) {
            if (!(u[a] < 0.f)) return 0;
            const float sa = (p[a] - (h[a] + 1.f)) / -u[a];
            if (axis < 0 || sa > steps) { steps = sa; axis = a; side = 1; bound = h[a]; }
        }
    }
    if (axis < 0) return cur + 1;                      // (NaN coordinates: nothing to reason from)
    const int n = steps >= (float)(-cur) ? -cur : (int)steps;
    if (n < 2) return cur + 1;
    float pp[3], vx, vy, vz;
    tcv_voxel(q, g, tcv_t(q, g, cur + n - 1), pp, vx, vy, vz);
    const float w = axis == 0 ? vx : (axis == 1 ? vy : vz);
    if (side < 0 ? w < 0.f : w > bound) return cur + n;
    return cur + 1;
}
// One step's observations of a wave into the accumulators (every lane of the wave calls; at == TCV_NONE: the lane has none).  Runs of
// neighbouring lanes with one storage index are summed into their head: vm_run_sum's segmented shuffle sum with one value, the run's
// length read off the ballot of heads.  A wave whose indices all differ from their left neighbour's pays one shuffle and one ballot.
__device__ __forceinline__ void tcv_run_add(int lane, unsigned long long at, int k, unsigned long long* __restrict__ S, int* __restrict__ N) {
    if (!__ballot(at != TCV_NONE)) return;             // (uniform)
    const unsigned long long left = __shfl_up(at, 1, WAVE);
    const bool head = lane == 0 || left != at;
    const unsigned long long heads = __ballot(head);
    int cnt = 1;
    if (heads != ~0ull) {                              // (uniform)
        const int run = __popcll(heads & (~0ull >> (63 - lane)));
        for (int off = 1; off < WAVE; off <<= 1) {
            const bool same = __shfl_down(run, off, WAVE) == run && lane + off < WAVE;
            const int ok = __shfl_down(k, off, WAVE);
            if (same) k += ok;
        }
        const unsigned long long rest = lane < 63 ? heads >> (lane + 1) : 0ull;      // the heads to the right of the lane
        cnt = rest ? __ffsll((long long)rest) : WAVE - lane;
    }
    if (head && at != TCV_NONE) {
        atomicAdd(&S[at], (unsigned long long)(long long)k);
        atomicAdd(&N[at], cnt);
    }
}

// The walk m = -J .. M of one ray per lane, every lane from its own first m.  The band (m >= 0) is tc_accumulate_body's, count for count.
template <bool HASHED, bool COMBINE, bool SKIP>
__device__ __forceinline__ void tcv_body(const HtVol& v, int nx, int ny, int nz, const TcCloud& cl, const TsdfMat& pose, float ex, float ey, float ez, const TcGrid& g,
                                         const TcCarve& cv, unsigned long long* __restrict__ S, int* __restrict__ N, unsigned long long* __restrict__ ctr) {
    const int lane = threadIdx.x & 63;
    const TcRay q = tc_ray(cl, blockIdx.x * 256 + threadIdx.x, pose.m, ex, ey, ez, g.max_d);
    const int M = g.n_steps;
    unsigned long long prev_key = HM_EMPTY;
    int prev_blk = -1, n_samples = 0, n_outside = 0, n_carved = 0;
    float pgx = 0.f, pgy = 0.f, pgz = 0.f;
    bool have_prev = false;
    const float hx = (float)(nx - 1), hy = (float)(ny - 1), hz = (float)(nz - 1);
    int m = tcv_first(q, g, cv);
    while (COMBINE ? __ballot(m <= M) != 0ull : m <= M) {
        unsigned long long at = TCV_NONE;
        int k = 0;
        if (m <= M) {
            const int cur = m;
            m = cur + 1;
            const float t = tcv_t(q, g, cur);
            if (cur >= 0 ? t > 0.f : t > cv.min_range) {
                float p[3], gx, gy, gz;
                tcv_voxel(q, g, t, p, gx, gy, gz);
                const bool in = HASHED ? (gx >= HT_VOX_LO && gx <= HT_VOX_HI && gy >= HT_VOX_LO && gy <= HT_VOX_HI && gz >= HT_VOX_LO && gz <= HT_VOX_HI)
                                       : (gx >= 0.f && gx <= hx && gy >= 0.f && gy <= hy && gz >= 0.f && gz <= hz);      // in float, before the cast: NaN is outside
                if (!in) {
                    if (cur >= 0) n_outside++;
                    else if (SKIP && !HASHED) m = tcv_enter_box(q, g, cur, p, gx, gy, gz, hx, hy, hz);
                } else if (!(have_prev && gx == pgx && gy == pgy && gz == pgz)) {
                    have_prev = true; pgx = gx; pgy = gy; pgz = gz;
                    if (cur >= 0) n_samples++;
                    const int ix = (int)gx, iy = (int)gy, iz = (int)gz;
                    bool stored = true;
                    unsigned long long a2 = 0ull;
                    if (HASHED) {
                        const unsigned long long key = hm_key(ix >> 3, iy >> 3, iz >> 3);
                        if (key != prev_key) { prev_key = key; prev_blk = ht_lookup(v, ix >> 3, iy >> 3, iz >> 3); }
                        if (prev_blk < 0 || prev_blk >= v.pool_cap) {      // (m >= 0: the touch is exact, cannot happen)
                            stored = false;
                            if (SKIP && cur < 0) m = tcv_leave_block(q, g, cur, p, ix >> 3, iy >> 3, iz >> 3);
                        } else a2 = (unsigned long long)prev_blk * 512ull + (unsigned long long)((iz & 7) * 64 + (iy & 7) * 8 + (ix & 7));
                    } else a2 = ((unsigned long long)iz * (unsigned long long)ny + (unsigned long long)iy) * (unsigned long long)nx + (unsigned long long)ix;
                    int kk;
                    if (stored && tc_observe(q, g, gx, gy, gz, kk)) {
                        at = a2; k = kk;
                        if (cur < 0) n_carved++;
                    }
                }
            }
        }
        if (COMBINE) tcv_run_add(lane, at, k, S, N);
        else if (at != TCV_NONE) {
            atomicAdd(&S[at], (unsigned long long)(long long)k);
            atomicAdd(&N[at], 1);
        }
    }
    tc_count(ctr, TC_RAYS, q.usable ? 1 : 0, lane);
    tc_count(ctr, TC_SAMPLES, n_samples, lane);
    tc_count(ctr, TC_OUTSIDE, n_outside, lane);
    tc_count(ctr, TC_CARVED, n_carved, lane);
}
__global__ __launch_bounds__(256) void k_htsdf_carve_cloud(const HtVol v, const TcCloud cl, const TsdfMat pose, float ex, float ey, float ez, const TcGrid g, const TcCarve cv,
                                                           unsigned long long* __restrict__ S, int* __restrict__ N, unsigned long long* __restrict__ ctr) {
    tcv_body<true, TCV_COMBINE, TCV_SKIP>(v, 0, 0, 0, cl, pose, ex, ey, ez, g, cv, S, N, ctr);
}
__global__ __launch_bounds__(256) void k_tsdf_carve_cloud(int nx, int ny, int nz, const TcCloud cl, const TsdfMat pose, float ex, float ey, float ez, const TcGrid g,
                                                          const TcCarve cv, unsigned long long* __restrict__ S, int* __restrict__ N, unsigned long long* __restrict__ ctr) {
    HtVol none = {};
    tcv_body<false, TCV_COMBINE, TCV_SKIP>(none, nx, ny, nz, cl, pose, ex, ey, ez, g, cv, S, N, ctr);
}
