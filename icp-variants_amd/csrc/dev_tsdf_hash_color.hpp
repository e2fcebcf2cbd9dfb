// dev_tsdf_hash_color.hpp -- the colours of the HASHED TSDF volume: a second pool, one fp32 float4 (R, G, B, Wc) per voxel, 512 per block
// (8 KiB), x fastest, indexed by the pool index of the geometry block and kept in a buffer of its own -- every geometry-only kernel keeps
// its instructions and its bytes per block.  Contract: include/icp_hip.h; tests/htsdf_color_restatement.py states
// the same arithmetic in numpy.  Part of icp_device.hpp (included from there, inside namespace icpdev, after dev_tsdf_hash_evict.hpp and
// dev_sdf_color.hpp).
// ------------------------------------------------------------------------------------------------
// The kernels of dev_tsdf_hash.hpp and dev_tsdf_hash_evict.hpp are restated here, not shared through a body template: they keep their
// instructions (DESIGN.md sections 6p, 6r and 6x did the same).  The colour pool is cleared when it is allocated and wherever the geometry
// pool is: a fresh block reads (0, 0, 0, 0), uncoloured.  Integer atomics and vector stores only.

// k_htsdf_integrate with tsdf_integrate_body<true>'s colour: one work-group per block, one wave per z-layer, a lane per (x, y) -- a wave's
// geometry access is one 512-byte run, its colour access one 1 KiB run of 16-byte loads and stores.  Per voxel the geometry is
// k_htsdf_integrate's arithmetic, operation for operation; the voxel is painted iff it is updated AND !(sdf > truncation), from the pixel
// the geometry used, and a voxel that is not painted has its float4 neither read nor written.
__global__ __launch_bounds__(512) void k_htsdf_integrate_color(const HtVol v, const TsdfCam cam, const TsdfMat mat, const float* __restrict__ depth, int* __restrict__ n_updated,
                                                               const uint32_t* __restrict__ rgbx, float4* __restrict__ cpool, int* __restrict__ n_colored) {
    __shared__ int red[16];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    int b[3];
    hm_unkey(v.pool_key[blockIdx.x], b);
    const int gi = b[0] * 8 + (lane & 7), gj = b[1] * 8 + (lane >> 3), gk = b[2] * 8 + wave;
    const float* __restrict__ M = mat.m;
    const float px = v.ox + (float)gi * v.s, py = v.oy + (float)gj * v.s, pz = v.oz + (float)gk * v.s;
    const float ax = M[0] * px, ay = M[3] * px, az = M[6] * px;
    const float bx = M[1] * py, by = M[4] * py, bz = M[7] * py;
    const float wf = (float)cam.width, hf = (float)cam.height;
    bool upd = false, paint = false;
    float f = 0.f;
    int pix = 0;
    const float zc = (az + (bz + M[8] * pz)) + M[11];
    if (zc > 0.f) {
        const float xc = (ax + (bx + M[2] * pz)) + M[9];
        const float yc = (ay + (by + M[5] * pz)) + M[10];
        const float u = floorf((cam.fx * (xc / zc) + cam.cx) + 0.5f), w = floorf((cam.fy * (yc / zc) + cam.cy) + 0.5f);
        if (u >= 0.f && u < wf && w >= 0.f && w < hf) {          // in float, before the cast: NaN skips
            pix = (int)w * cam.width + (int)u;
            const float d = depth[pix];
            if (isfinite(d) && d > 0.f && d <= v.max_d) {
                const float sdf = d - zc;
                if (!(sdf < -v.trunc)) { f = fminf(1.f, sdf / v.trunc); upd = true; }
                paint = upd && !(sdf > v.trunc);
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
    if (paint) {
        const uint32_t c = rgbx[pix];
        float4* __restrict__ p = cpool + ((size_t)blockIdx.x * 512 + tid);
        const float4 o = *p;
        float4 r;
        r.x = (o.w * o.x + (float)(int)(c & 0xFFu)) / (o.w + 1.f);
        r.y = (o.w * o.y + (float)(int)((c >> 8) & 0xFFu)) / (o.w + 1.f);
        r.z = (o.w * o.z + (float)(int)((c >> 16) & 0xFFu)) / (o.w + 1.f);
        r.w = fminf(o.w + 1.f, v.max_w);
        *p = r;
    }
    if (n_updated || n_colored) {                      // (uniform) both counts through one barrier
        const unsigned long long bu = __ballot(upd), bp = __ballot(paint);
        if (lane == 0) { red[wave] = __popcll(bu); red[8 + wave] = __popcll(bp); }
        __syncthreads();
        if (tid < 2) {
            const int* r = red + 8 * tid;
            const int t = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
            int* out = tid ? n_colored : n_updated;
            if (t && out) atomicAdd(out, t);
        }
    }
}

// k_htsdf_place for the colour pool: one work-group per uploaded block copies its 512 staged float4 to wherever the block sits.
__global__ __launch_bounds__(512) void k_htsdf_place_color(const HtVol v, float4* __restrict__ cpool, const int* __restrict__ coords, const float4* __restrict__ in) {
    const int e = blockIdx.x;
    const int blk = ht_lookup(v, coords[3 * (size_t)e], coords[3 * (size_t)e + 1], coords[3 * (size_t)e + 2]);      // (uniform)
    if (blk < 0) return;
    cpool[(size_t)blk * 512 + threadIdx.x] = in[(size_t)e * 512 + threadIdx.x];
}

// k_htsdf_evict_out and k_htsdf_evict_move for the colour pool, by the SAME lists: an evicted block's colours take its place in the
// outbox, a mover's colours go into the hole its geometry goes into.  Sources lie at or above n_keep, destinations below: one launch.
__global__ __launch_bounds__(512) void k_htsdf_evict_out_color(const float4* __restrict__ cpool, const int* __restrict__ evicted, float4* __restrict__ out_cpool) {
    const int e = blockIdx.x, src = evicted[e];        // (uniform)
    out_cpool[(size_t)e * 512 + threadIdx.x] = cpool[(size_t)src * 512 + threadIdx.x];
}
__global__ __launch_bounds__(512) void k_htsdf_evict_move_color(float4* __restrict__ cpool, const int* __restrict__ holes, const int* __restrict__ movers,
                                                                const int* __restrict__ ec) {
    const int j = blockIdx.x;
    if (j >= ec[HE_MOVERS]) return;                    // (uniform)
    const int src = movers[j], dst = holes[j];
    cpool[(size_t)dst * 512 + threadIdx.x] = cpool[(size_t)src * 512 + threadIdx.x];
}

// The colour cell of world point q on the hashed volume: htsdf_cell's addressing (the same g, floor and fractions, one lookup for a cell
// inside one block, one per distinct block for a cell across a face, an edge or a corner; a chain of selects picks among the looked-up
// blocks, no register array is indexed), reading the colour pool: s_k = (R_k + G_k) + B_k per corner.  false when the cell is not storable
// (tested in float, before any cast), when a corner's block does not exist, or when a corner has Wc == 0.  The geometry's weights play no part.
__device__ __forceinline__ bool htsdf_color_cell(const HtVol& v, const float4* __restrict__ cpool, float qx, float qy, float qz, float (&s)[8], float& tx, float& ty,
                                                 float& tz) {
    const float gx = (qx - v.ox) / v.s, gy = (qy - v.oy) / v.s, gz = (qz - v.oz) / v.s;
    const float fx = floorf(gx), fy = floorf(gy), fz = floorf(gz);
    if (!(fx >= HT_CELL_LO && fx <= HT_CELL_HI && fy >= HT_CELL_LO && fy <= HT_CELL_HI && fz >= HT_CELL_LO && fz <= HT_CELL_HI)) return false;
    tx = gx - fx; ty = gy - fy; tz = gz - fz;
    const int ix = (int)fx, iy = (int)fy, iz = (int)fz;
    const int bx = ix >> 3, by = iy >> 3, bz = iz >> 3, lx = ix & 7, ly = iy & 7, lz = iz & 7;
    if (lx <= 6 && ly <= 6 && lz <= 6) {
        const int blk = ht_lookup(v, bx, by, bz);
        if (blk < 0) return false;
        const float4* __restrict__ p = cpool + ((size_t)blk * 512 + (size_t)(lz * 64 + ly * 8 + lx));
        const float4 a0 = p[0], a1 = p[1], a2 = p[8], a3 = p[9], a4 = p[64], a5 = p[65], a6 = p[72], a7 = p[73];
        s[0] = (a0.x + a0.y) + a0.z; s[1] = (a1.x + a1.y) + a1.z; s[2] = (a2.x + a2.y) + a2.z; s[3] = (a3.x + a3.y) + a3.z;
        s[4] = (a4.x + a4.y) + a4.z; s[5] = (a5.x + a5.y) + a5.z; s[6] = (a6.x + a6.y) + a6.z; s[7] = (a7.x + a7.y) + a7.z;
        return a0.w > 0.f && a1.w > 0.f && a2.w > 0.f && a3.w > 0.f && a4.w > 0.f && a5.w > 0.f && a6.w > 0.f && a7.w > 0.f;
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
        const float4 a = cpool[(size_t)blk * 512 + (size_t)off];
        s[k] = (a.x + a.y) + a.z;
        ok = ok && a.w > 0.f;
    }
    return ok;
}

// k_tsdf_sample_color with htsdf_color_cell.
__global__ __launch_bounds__(256) void k_htsdf_sample_color(const HtVol v, const float4* __restrict__ cpool, const float* __restrict__ pts, int n, float* __restrict__ s_out,
                                                            float* __restrict__ h_out, uint8_t* __restrict__ valid_out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float s[8], tx, ty, tz, S = 0.f, hx = 0.f, hy = 0.f, hz = 0.f;
    const bool ok = htsdf_color_cell(v, cpool, pts[(size_t)i * 3], pts[(size_t)i * 3 + 1], pts[(size_t)i * 3 + 2], s, tx, ty, tz);
    if (ok) { S = sdf_field(s, tx, ty, tz); sdf_gradient(s, tx, ty, tz, hx, hy, hz); }
    s_out[i] = sdf_canonical(S);
    h_out[(size_t)i * 3] = sdf_canonical(hx); h_out[(size_t)i * 3 + 1] = sdf_canonical(hy); h_out[(size_t)i * 3 + 2] = sdf_canonical(hz);
    valid_out[i] = ok ? 1 : 0;
}

// htsdf_cell restated to read BOTH pools through what its lookups found, so the colour read costs no second table probe: the one pool
// index of an interior cell (343 of 512 cells: its eight float2 and eight float4 loads are issued together), the up to eight indices of a
// crossing cell (the chain of selects picks one per corner for both loads).  Returns htsdf_cell's verdict on the geometry (c, tx, ty, tz as
// there); s_k = (R_k + G_k) + B_k per corner and all8 = every corner has Wc > 0 are meaningful where it returns true.
__device__ __forceinline__ bool htsdf_cell_both(const HtVol& v, const float4* __restrict__ cpool, float qx, float qy, float qz, float (&c)[8], float (&s)[8], float& tx,
                                                float& ty, float& tz, bool& all8) {
    const float gx = (qx - v.ox) / v.s, gy = (qy - v.oy) / v.s, gz = (qz - v.oz) / v.s;
    const float fx = floorf(gx), fy = floorf(gy), fz = floorf(gz);
    if (!(fx >= HT_CELL_LO && fx <= HT_CELL_HI && fy >= HT_CELL_LO && fy <= HT_CELL_HI && fz >= HT_CELL_LO && fz <= HT_CELL_HI)) return false;
    tx = gx - fx; ty = gy - fy; tz = gz - fz;
    const int ix = (int)fx, iy = (int)fy, iz = (int)fz;
    const int bx = ix >> 3, by = iy >> 3, bz = iz >> 3, lx = ix & 7, ly = iy & 7, lz = iz & 7;
    if (lx <= 6 && ly <= 6 && lz <= 6) {
        const int blk = ht_lookup(v, bx, by, bz);
        if (blk < 0) return false;
        const size_t at = (size_t)blk * 512 + (size_t)(lz * 64 + ly * 8 + lx);
        const float2* __restrict__ p = v.pool + at;
        const float4* __restrict__ q = cpool + at;
        const float2 a0 = p[0], a1 = p[1], a2 = p[8], a3 = p[9], a4 = p[64], a5 = p[65], a6 = p[72], a7 = p[73];
        const float4 e0 = q[0], e1 = q[1], e2 = q[8], e3 = q[9], e4 = q[64], e5 = q[65], e6 = q[72], e7 = q[73];
        c[0] = a0.x; c[1] = a1.x; c[2] = a2.x; c[3] = a3.x; c[4] = a4.x; c[5] = a5.x; c[6] = a6.x; c[7] = a7.x;
        s[0] = (e0.x + e0.y) + e0.z; s[1] = (e1.x + e1.y) + e1.z; s[2] = (e2.x + e2.y) + e2.z; s[3] = (e3.x + e3.y) + e3.z;
        s[4] = (e4.x + e4.y) + e4.z; s[5] = (e5.x + e5.y) + e5.z; s[6] = (e6.x + e6.y) + e6.z; s[7] = (e7.x + e7.y) + e7.z;
        all8 = e0.w > 0.f && e1.w > 0.f && e2.w > 0.f && e3.w > 0.f && e4.w > 0.f && e5.w > 0.f && e6.w > 0.f && e7.w > 0.f;
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
    bool ok = true, okc = true;
#pragma unroll
    for (int k = 0; k < 8; k++) {
        const int j = k & cross;
        int blk = pb[0];
#pragma unroll
        for (int q = 1; q < 8; q++) blk = j == q ? pb[q] : blk;      // (a chain of selects: no register array is indexed)
        const int off = (((lz + (k >> 2)) & 7) * 64 + ((ly + ((k >> 1) & 1)) & 7) * 8) + ((lx + (k & 1)) & 7);
        const float2 a = v.pool[(size_t)blk * 512 + (size_t)off];
        const float4 e = cpool[(size_t)blk * 512 + (size_t)off];
        c[k] = a.x;
        s[k] = (e.x + e.y) + e.z;
        ok = ok && a.y > 0.f;
        okc = okc && e.w > 0.f;
    }
    all8 = okc;
    return ok;
}

// k_hsdf_accumulate's geometry with k_sdf_accumulate_color's photometric row added into it, that kernel's term order operation for
// operation: the same 29 partials, 3 counts and block_reduce_wide fold, so k_sdf_init_color and k_sdf_solve_color run around it as they are.
// cf.col is the colour POOL here.
__global__ __launch_bounds__(256) void k_hsdf_accumulate_color(const HtVol v, const SdfFrame f, const SdfColorFrame cf, const SdfColorState* __restrict__ st,
                                                               double* __restrict__ partials, int* __restrict__ counts) {
    __shared__ double lds[4 * SDFC_NSUM * 17];
    __shared__ int red[12];
    if (st->stop) return;                              // (uniform) the frame has ended: nothing of this launch is needed
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int su = blockIdx.x * 16 + (wave & 1) * 8 + (lane & 7), sv = blockIdx.y * 16 + (wave >> 1) * 8 + (lane >> 3);
    const float* __restrict__ P = st->pose;
    double acc[SDFC_NSUM];
#pragma unroll
    for (int a = 0; a < SDFC_NSUM; a++) acc[a] = 0.0;
    bool usable = false, valid = false, colored = false;
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
            float c[8], s[8], tx, ty, tz;
            bool all8 = false;
            if (htsdf_cell_both(v, cf.col, q0, q1, q2, c, s, tx, ty, tz, all8)) {
                const float F = sdf_field(c, tx, ty, tz);
                if (fabsf(F) < 1.f) {                  // (a NaN drops out; a sample clamped at the free-space value carries no gradient)
                    valid = true;
                    const uint32_t px = cf.rgbx[(size_t)w * f.width + u];
                    const double p0 = (double)q0, p1 = (double)q1, p2 = (double)q2;
                    {
                        float gx, gy, gz;
                        sdf_gradient(c, tx, ty, tz, gx, gy, gz);
                        const double r = (double)F * (double)v.trunc, sc = (double)v.trunc / (double)v.s;
                        const double g0 = (double)gx * sc, g1 = (double)gy * sc, g2 = (double)gz * sc;
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
                    const float S = sdf_field(s, tx, ty, tz);
                    colored = all8 && isfinite(S);
                    if (colored) {
                        float hx, hy, hz;
                        sdf_gradient(s, tx, ty, tz, hx, hy, hz);
                        const double Ip = (double)(int)((px & 0xFFu) + ((px >> 8) & 0xFFu) + ((px >> 16) & 0xFFu)) / 765.0;
                        const double r = (double)S / 765.0 - Ip, den = 765.0 * (double)v.s;
                        const double g0 = (double)hx / den, g1 = (double)hy / den, g2 = (double)hz / den;
                        const double J[6] = {p1 * g2 - p2 * g1, p2 * g0 - p0 * g2, p0 * g1 - p1 * g0, g0, g1, g2};
                        double wt = (double)cf.weight * (double)cf.weight;
                        if (cf.huber > 0.f) { const double ar = fabs(r), h = (double)cf.huber; wt = wt * (ar <= h ? 1.0 : h / ar); }
                        int k = 0;
#pragma unroll
                        for (int i = 0; i < 6; i++) {
                            const double wj = wt * J[i];
#pragma unroll
                            for (int j = i; j < 6; j++) { acc[k] = acc[k] + wj * J[j]; k++; }
                            acc[21 + i] = acc[21 + i] + -(wj * r);
                        }
                        const double e = (wt * r) * r;
                        acc[27] = acc[27] + e;
                        acc[28] = e;
                    }
                }
            }
        }
    }
    const unsigned long long bu = __ballot(usable), bv = __ballot(valid), bc = __ballot(colored);
    if (lane == 0) { red[3 * wave] = __popcll(bu); red[3 * wave + 1] = __popcll(bv); red[3 * wave + 2] = __popcll(bc); }
    const double tot = block_reduce_wide<SDFC_NSUM, 4>(acc, lds);      // (its barrier also covers red)
    const int nb = gridDim.x * gridDim.y, blk = blockIdx.y * gridDim.x + blockIdx.x;
    if (tid < SDFC_NSUM) partials[(size_t)tid * nb + blk] = tot;
    if (tid >= 64 && tid < 67) { const int q = tid - 64; counts[(size_t)q * nb + blk] = (red[q] + red[3 + q]) + (red[6 + q] + red[9 + q]); }
}
