// dev_tsdf_hash.hpp -- the HASHED storage of the TSDF volume: dev_tsdf.hpp's per-voxel state (one float2 (tsdf, weight)) in blocks of
// 8 x 8 x 8 voxels that a hash table addresses by BLOCK coordinates (Niessner, Zollhoefer, Izadi, Stamminger, SIGGRAPH Asia 2013), so the
// volume has no extent and costs memory only around the surface.  Contract: include/icp_hip.h, DESIGN.md section 6x;
// tests/htsdf_restatement.py states the same arithmetic in numpy.  Part of icp_device.hpp (included from there, inside namespace icpdev,
// after dev_sdf.hpp and dev_hmap.hpp, whose key, home, find and claim helpers address the table: 21 bits per axis of block coordinate).
// ------------------------------------------------------------------------------------------------
// Layout: `keys` (8 bytes per slot, empty = ~0) and `vals` (4 bytes per slot: the block's index in the pool, HT_NONE while the slot has
// none) are the table; `pool` holds the blocks, 512 float2 each, x fastest (4 KiB; one z-layer is a 512-byte run); `pool_key` records the
// key of every pool block, so a kernel over the blocks 0 .. n_blocks - 1 never scans the table.  The kernels here only ever append blocks
// (dev_tsdf_hash_evict.hpp takes blocks out and leaves the pool compact, its tail cleared), and the
// pool is cleared when it is allocated: a fresh block reads (0, 0), unobserved.  Where a block sits in the pool may depend on a race
// between two claims; what it holds does not.  Integer atomics and vector stores only.
constexpr int HT_NONE = -1, HT_TAKEN = -2;          // vals: no block yet; a claim is deciding (or has found the pool full)
constexpr int HT_NBLK = 0, HT_UNPLACED = 1, HT_OOR = 2, HT_NCTR = 4;      // counters: blocks handed out, claims without storage, samples out of range
constexpr float HT_CELL_LO = -8388608.f, HT_CELL_HI = 8388606.f;          // cells whose eight corners have storable blocks: -2^23 <= f <= 2^23 - 2
struct HtVol {
    const unsigned long long* keys; const int* vals; float2* pool; const unsigned long long* pool_key;
    int log2cap, pool_cap;
    float ox, oy, oz, s;
    float trunc, max_w, max_d;
};
struct HtTable { unsigned long long* keys; int* vals; unsigned long long* pool_key; int log2cap, pool_cap; };

// The pool index of block `key`, or -1: plain loads (the table was written by earlier launches).
__device__ __forceinline__ int ht_lookup(const HtVol& v, int bx, int by, int bz) {
    const unsigned long long key = hm_key(bx, by, bz);
    const int slot = hm_find_from(v.keys, v.log2cap, key, hm_home(key, v.log2cap), 0);
    return slot < 0 ? -1 : v.vals[slot];
}

// Storage for block `key`, decided once per key however many lanes ask: the key's slot is claimed (hm_claim), and the lane that turns the
// slot's value from HT_NONE to HT_TAKEN takes the next pool index.  A claim that finds no slot or no pool block is counted in
// ctr[HT_UNPLACED] and its key gets no storage: the host then grows table and pool and runs the launch again.  Once the pool is full no
// further key is entered into the table (a lane only looks its key up), so the table never fills beyond the pool and every probe stays short.
__device__ __forceinline__ void ht_touch_block(const HtTable& t, unsigned long long key, int* __restrict__ ctr) {
    if (__hip_atomic_load(&ctr[HT_NBLK], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= t.pool_cap) {
        const unsigned mask = (1u << t.log2cap) - 1u;
        unsigned slot = hm_home(key, t.log2cap);
        bool found = false;
        for (unsigned i = 0; i <= mask; i++) {
            const unsigned long long k = __hip_atomic_load(&t.keys[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (k == key) { found = __hip_atomic_load(&t.vals[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != HT_NONE; break; }
            if (k == HM_EMPTY) break;
            slot = (slot + 1u) & mask;
        }
        if (!found) atomicAdd(&ctr[HT_UNPLACED], 1);      // (a key found HT_TAKEN was counted by the lane that took it, if it got no block)
        return;
    }
    const int slot = hm_claim(t.keys, t.log2cap, key);
    if (slot < 0) { atomicAdd(&ctr[HT_UNPLACED], 1); return; }
    if (__hip_atomic_load(&t.vals[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != HT_NONE) return;
    if (atomicCAS(&t.vals[slot], HT_NONE, HT_TAKEN) != HT_NONE) return;
    const int idx = atomicAdd(&ctr[HT_NBLK], 1);
    if (idx < t.pool_cap) {
        t.pool_key[idx] = key;
        __hip_atomic_store(&t.vals[slot], idx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    } else atomicAdd(&ctr[HT_UNPLACED], 1);
}

// Allocation in front of an integrate, from the depth frame and the pose alone: one pixel per lane, an 8 x 8 tile of pixels per wave.  The
// lane walks its ray through the truncation band in steps of one voxel, sample m at z_m = min((d - truncation) + m s, d + truncation),
// and asks for the blocks of the eight corners of every sample's cell.  Most of what it asks for it has asked for before: a key equal to
// the lane's previous one is skipped, and so is a key the lane to the left asks for in the same step (that lane, or one further left,
// makes the claim).  The walk is uniform (every lane takes all n_steps + 1 steps, idle ones with nothing to ask), so the shuffle is legal.
__global__ __launch_bounds__(256) void k_htsdf_touch(const HtTable t, const TsdfCam cam, const TsdfMat pose, const float* __restrict__ depth, float ox, float oy, float oz,
                                                     float s, float trunc, float max_d, int n_steps, int* __restrict__ ctr) {
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int u = blockIdx.x * 16 + (wave & 1) * 8 + (lane & 7), w = blockIdx.y * 16 + (wave >> 1) * 8 + (lane >> 3);
    const float* __restrict__ P = pose.m;
    float d = 0.f;
    bool usable = false;
    if (u < cam.width && w < cam.height) {
        d = depth[(size_t)w * cam.width + u];
        usable = isfinite(d) && d > 0.f && d <= max_d;
    }
    const float a = ((float)u - cam.cx) / cam.fx, b = ((float)w - cam.cy) / cam.fy;
    const float z_lo = d - trunc, z_hi = d + trunc;
    unsigned long long prev = HM_EMPTY;
    int n_oor = 0;
    for (int m = 0; m <= n_steps; m++) {
        const float z = fminf(z_lo + (float)m * s, z_hi);
        bool active = usable && z > 0.f;
        int cx = 0, cy = 0, cz = 0;
        if (active) {
            const float x = a * z, y = b * z;
            const float q0 = (P[0] * x + (P[4] * y + P[8] * z)) + P[12];
            const float q1 = (P[1] * x + (P[5] * y + P[9] * z)) + P[13];
            const float q2 = (P[2] * x + (P[6] * y + P[10] * z)) + P[14];
            const float f0 = floorf((q0 - ox) / s), f1 = floorf((q1 - oy) / s), f2 = floorf((q2 - oz) / s);
            if (f0 >= HT_CELL_LO && f0 <= HT_CELL_HI && f1 >= HT_CELL_LO && f1 <= HT_CELL_HI && f2 >= HT_CELL_LO && f2 <= HT_CELL_HI) {      // in float, before the cast: NaN skips
                cx = (int)f0; cy = (int)f1; cz = (int)f2;
            } else { active = false; n_oor++; }
        }
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const int dx = k & 1, dy = (k >> 1) & 1, dz = k >> 2;
            const int bx = (cx + dx) >> 3, by = (cy + dy) >> 3, bz = (cz + dz) >> 3;
            // a corner whose block is that of the corner one step back along an axis repeats a key already asked for in this sample
            const bool distinct = (!dx || bx != (cx >> 3)) && (!dy || by != (cy >> 3)) && (!dz || bz != (cz >> 3));
            const unsigned long long key = active && distinct ? hm_key(bx, by, bz) : HM_EMPTY;
            const unsigned long long left = __shfl_up(key, 1, WAVE);
            if (key != HM_EMPTY) {
                if (key != prev && !(lane > 0 && left == key)) ht_touch_block(t, key, ctr);
                prev = key;
            }
        }
    }
    const unsigned long long bo = __ballot(n_oor > 0);
    if (bo) {                                          // (uniform; rare)
        for (int off = 32; off > 0; off >>= 1) n_oor += __shfl_down(n_oor, off, WAVE);
        if (lane == 0) atomicAdd(&ctr[HT_OOR], n_oor);
    }
}

// Explicit allocation (icp_tsdf_allocate_blocks, and the blocks of an upload): one block coordinate per lane, storable by the host's check.
__global__ __launch_bounds__(256) void k_htsdf_alloc(const HtTable t, int n, const int* __restrict__ coords, int* __restrict__ ctr) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    ht_touch_block(t, hm_key(coords[3 * (size_t)i], coords[3 * (size_t)i + 1], coords[3 * (size_t)i + 2]), ctr);
}

// Growth: one LIVE pool block per lane enters its key into the new table (CAS: two blocks never share a key, but two lanes may want one
// slot) with its pool index as the value; the blocks themselves are copied by the host's device-to-device copy.  The new table is larger
// than twice the pool: a block that finds no slot cannot happen and is counted.
__global__ __launch_bounds__(256) void k_htsdf_rehash(int n_live, const unsigned long long* __restrict__ pool_key, unsigned long long* __restrict__ keys, int* __restrict__ vals,
                                                      int log2cap, int* __restrict__ ctr) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_live) return;
    const int slot = hm_claim(keys, log2cap, pool_key[i]);
    if (slot < 0) { atomicAdd(&ctr[HT_UNPLACED], 1); return; }
    vals[slot] = i;
}

// Upload: one work-group per uploaded block (its coordinates allocated by k_htsdf_alloc before) copies the block's 512 voxels from the
// staged (tsdf, weight) pairs to wherever the block sits in the pool.
__global__ __launch_bounds__(512) void k_htsdf_place(const HtVol v, const int* __restrict__ coords, const float2* __restrict__ in) {
    const int e = blockIdx.x;
    const int blk = ht_lookup(v, coords[3 * (size_t)e], coords[3 * (size_t)e + 1], coords[3 * (size_t)e + 2]);      // (uniform)
    if (blk < 0) return;
    v.pool[(size_t)blk * 512 + threadIdx.x] = in[(size_t)e * 512 + threadIdx.x];
}

// k_tsdf_integrate over the pool: one work-group per block, one wave per z-layer, a lane per (x, y) of the layer -- every access of a
// wave is one 512-byte run.  Per voxel the arithmetic is tsdf_integrate_body's, operation for operation, with the signed global voxel
// coordinate g = 8 b + local in place of the box index; whether a voxel is updated is decided from the depth frame alone.
__global__ __launch_bounds__(512) void k_htsdf_integrate(const HtVol v, const TsdfCam cam, const TsdfMat mat, const float* __restrict__ depth, int* __restrict__ n_updated) {
    __shared__ int red[8];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    int b[3];
    hm_unkey(v.pool_key[blockIdx.x], b);
    const int gi = b[0] * 8 + (lane & 7), gj = b[1] * 8 + (lane >> 3), gk = b[2] * 8 + wave;
    const float* __restrict__ M = mat.m;
    const float px = v.ox + (float)gi * v.s, py = v.oy + (float)gj * v.s, pz = v.oz + (float)gk * v.s;
    const float ax = M[0] * px, ay = M[3] * px, az = M[6] * px;
    const float bx = M[1] * py, by = M[4] * py, bz = M[7] * py;
    const float wf = (float)cam.width, hf = (float)cam.height;
    bool upd = false;
    float f = 0.f;
    const float zc = (az + (bz + M[8] * pz)) + M[11];
    if (zc > 0.f) {
        const float xc = (ax + (bx + M[2] * pz)) + M[9];
        const float yc = (ay + (by + M[5] * pz)) + M[10];
        const float u = floorf((cam.fx * (xc / zc) + cam.cx) + 0.5f), w = floorf((cam.fy * (yc / zc) + cam.cy) + 0.5f);
        if (u >= 0.f && u < wf && w >= 0.f && w < hf) {          // in float, before the cast: NaN skips
            const float d = depth[(int)w * cam.width + (int)u];
            if (isfinite(d) && d > 0.f && d <= v.max_d) {
                const float sdf = d - zc;
                if (!(sdf < -v.trunc)) { f = fminf(1.f, sdf / v.trunc); upd = true; }
            }
        }
    }
    if (upd) {
        float2* __restrict__ p = v.pool + ((size_t)blockIdx.x * 512 + tid);
        const float2 o = *p;
        float2 r;
        r.x = (o.y * o.x + f) / (o.y + 1.f);
        r.y = fminf(o.y + 1.f, v.max_w);
        *p = r;
    }
    if (n_updated) {
        const unsigned long long bu = __ballot(upd);
        if (lane == 0) red[wave] = __popcll(bu);
        __syncthreads();
        if (tid == 0) {
            const int t = ((red[0] + red[1]) + (red[2] + red[3])) + ((red[4] + red[5]) + (red[6] + red[7]));
            if (t) atomicAdd(n_updated, t);
        }
    }
}

// tsdf_cell on the hashed volume: the same g, floor and fractions, the corners c[dx + 2 dy + 4 dz].  A cell that lies inside one block
// (local coordinates <= 6 on every axis: 343 of 512) costs one lookup and eight loads issued together; a cell across a face, an edge or
// a corner looks up each of its 2, 4 or 8 distinct blocks once.  false when the cell is not storable (tested in float: NaN and
// out-of-range coordinates never reach a cast), when a corner's block does not exist, or when a corner is unobserved.
__device__ __forceinline__ bool htsdf_cell(const HtVol& v, float qx, float qy, float qz, float (&c)[8], float& tx, float& ty, float& tz) {
    const float gx = (qx - v.ox) / v.s, gy = (qy - v.oy) / v.s, gz = (qz - v.oz) / v.s;
    const float fx = floorf(gx), fy = floorf(gy), fz = floorf(gz);
    if (!(fx >= HT_CELL_LO && fx <= HT_CELL_HI && fy >= HT_CELL_LO && fy <= HT_CELL_HI && fz >= HT_CELL_LO && fz <= HT_CELL_HI)) return false;
    tx = gx - fx; ty = gy - fy; tz = gz - fz;
    const int ix = (int)fx, iy = (int)fy, iz = (int)fz;
    const int bx = ix >> 3, by = iy >> 3, bz = iz >> 3, lx = ix & 7, ly = iy & 7, lz = iz & 7;
    if (lx <= 6 && ly <= 6 && lz <= 6) {
        const int blk = ht_lookup(v, bx, by, bz);
        if (blk < 0) return false;
        const float2* __restrict__ p = v.pool + ((size_t)blk * 512 + (size_t)(lz * 64 + ly * 8 + lx));
        const float2 a0 = p[0], a1 = p[1], a2 = p[8], a3 = p[9], a4 = p[64], a5 = p[65], a6 = p[72], a7 = p[73];
        c[0] = a0.x; c[1] = a1.x; c[2] = a2.x; c[3] = a3.x; c[4] = a4.x; c[5] = a5.x; c[6] = a6.x; c[7] = a7.x;
        return a0.y > 0.f && a1.y > 0.f && a2.y > 0.f && a3.y > 0.f && a4.y > 0.f && a5.y > 0.f && a6.y > 0.f && a7.y > 0.f;
    }
    const int cross = (lx == 7 ? 1 : 0) | (ly == 7 ? 2 : 0) | (lz == 7 ? 4 : 0);      // the axes along which the cell leaves its block
    int pb[8];
    bool all = true;
#pragma unroll
    for (int j = 0; j < 8; j++) {
        pb[j] = -1;
        if ((j & ~cross) == 0) { pb[j] = ht_lookup(v, bx + (j & 1), by + ((j >> 1) & 1), bz + (j >> 2)); all = all && pb[j] >= 0; }
    }
    if (!all) return false;
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 8; k++) {
        const int j = k & cross;
        int blk = pb[0];
#pragma unroll
        for (int q = 1; q < 8; q++) blk = j == q ? pb[q] : blk;      // (a chain of selects: no register array is indexed)
        const int off = (((lz + (k >> 2)) & 7) * 64 + ((ly + ((k >> 1) & 1)) & 7) * 8) + ((lx + (k & 1)) & 7);
        const float2 a = v.pool[(size_t)blk * 512 + (size_t)off];
        c[k] = a.x;
        ok = ok && a.y > 0.f;
    }
    return ok;
}

// k_tsdf_sample with htsdf_cell.
__global__ __launch_bounds__(256) void k_htsdf_sample(const HtVol v, const float* __restrict__ pts, int n, float* __restrict__ f_out, float* __restrict__ g_out,
                                                      uint8_t* __restrict__ valid_out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float c[8], tx, ty, tz, F = 0.f, gx = 0.f, gy = 0.f, gz = 0.f;
    const bool ok = htsdf_cell(v, pts[(size_t)i * 3], pts[(size_t)i * 3 + 1], pts[(size_t)i * 3 + 2], c, tx, ty, tz);
    if (ok) { F = sdf_field(c, tx, ty, tz); sdf_gradient(c, tx, ty, tz, gx, gy, gz); }
    f_out[i] = sdf_canonical(F);
    g_out[(size_t)i * 3] = sdf_canonical(gx); g_out[(size_t)i * 3 + 1] = sdf_canonical(gy); g_out[(size_t)i * 3 + 2] = sdf_canonical(gz);
    valid_out[i] = ok ? 1 : 0;
}

// k_sdf_accumulate with htsdf_cell: that kernel's text (sharing it through a body template would have to leave its instructions as they
// are), the same per-lane terms, the same block_reduce_wide fold and partials layout, so k_sdf_init and k_sdf_solve run around it as they are.
__global__ __launch_bounds__(256) void k_hsdf_accumulate(const HtVol v, const SdfFrame f, const SdfState* __restrict__ st, double* __restrict__ partials,
                                                         int* __restrict__ counts) {
    __shared__ double lds[4 * SDF_NSUM * 17];
    __shared__ int red[8];
    if (st->stop) return;                              // (uniform) the frame has ended: nothing of this launch is needed
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int su = blockIdx.x * 16 + (wave & 1) * 8 + (lane & 7), sv = blockIdx.y * 16 + (wave >> 1) * 8 + (lane >> 3);
    const float* __restrict__ P = st->pose;
    double acc[SDF_NSUM];
#pragma unroll
    for (int a = 0; a < SDF_NSUM; a++) acc[a] = 0.0;
    bool usable = false, valid = false;
    if (su < f.ws && sv < f.hs) {
        const int u = su * f.stride, w = sv * f.stride;
        const float d = f.depth[(size_t)w * f.width + u];
        usable = isfinite(d) && d > 0.f && d <= v.max_d;
        if (usable) {
            const float a = ((float)u - f.cx) / f.fx, b = ((float)w - f.cy) / f.fy;
            const float x = a * d, y = b * d;
            const float q0 = (P[0] * x + (P[4] * y + P[8] * d)) + P[12];
            const float q1 = (P[1] * x + (P[5] * y + P[9] * d)) + P[13];
            const float q2 = (P[2] * x + (P[6] * y + P[10] * d)) + P[14];
            float c[8], tx, ty, tz;
            if (htsdf_cell(v, q0, q1, q2, c, tx, ty, tz)) {
                const float F = sdf_field(c, tx, ty, tz);
                if (fabsf(F) < 1.f) {                  // (a NaN drops out; a sample clamped at the free-space value carries no gradient)
                    valid = true;
                    float gx, gy, gz;
                    sdf_gradient(c, tx, ty, tz, gx, gy, gz);
                    const double r = (double)F * (double)v.trunc, sc = (double)v.trunc / (double)v.s;
                    const double g0 = (double)gx * sc, g1 = (double)gy * sc, g2 = (double)gz * sc;
                    const double p0 = (double)q0, p1 = (double)q1, p2 = (double)q2;
                    const double J[6] = {p1 * g2 - p2 * g1, p2 * g0 - p0 * g2, p0 * g1 - p1 * g0, g0, g1, g2};
                    double wt = 1.0;
                    if (f.huber > 0.f) { const double ar = fabs(r), h = (double)f.huber; wt = ar <= h ? 1.0 : h / ar; }
                    int k = 0;
#pragma unroll
                    for (int i = 0; i < 6; i++) {
                        const double wj = wt * J[i];
#pragma unroll
                        for (int j = i; j < 6; j++) acc[k++] = wj * J[j];
                        acc[21 + i] = -(wj * r);
                    }
                    acc[27] = (wt * r) * r;
                }
            }
        }
    }
    const unsigned long long bu = __ballot(usable), bv = __ballot(valid);
    if (lane == 0) { red[2 * wave] = __popcll(bu); red[2 * wave + 1] = __popcll(bv); }
    const double tot = block_reduce_wide<SDF_NSUM, 4>(acc, lds);      // (its barrier also covers red)
    const int nb = gridDim.x * gridDim.y, blk = blockIdx.y * gridDim.x + blockIdx.x;
    if (tid < SDF_NSUM) partials[(size_t)tid * nb + blk] = tot;
    if (tid >= 64 && tid < 66) { const int q = tid - 64; counts[(size_t)q * nb + blk] = (red[q] + red[2 + q]) + (red[4 + q] + red[6 + q]); }
}
