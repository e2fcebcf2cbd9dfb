// dev_tsdf_hash_raycast.hpp -- the ray-cast of the HASHED TSDF volume: k_tsdf_raycast (dev_tsdf.hpp) read through dev_tsdf_hash.hpp's
// addressing, so the hashed model can be seen from a pose and tracked frame-to-model (icp_tsdf_raycast_hashed, icp_set_target_tsdf_hashed,
// icp_track_depth_model_hashed).  Contract: include/icp_hip.h; tests/htsdf_raycast_restatement.py states the same
// arithmetic in numpy.  Part of icp_device.hpp (included from there, inside namespace icpdev, after dev_tsdf_hash.hpp).
// ------------------------------------------------------------------------------------------------
// The march, the per-sample arithmetic, the end rule, zh and the normal are k_tsdf_raycast's, operation for operation; the cell is
// htsdf_cell's (g, floor, the range test in float, the fractions, corner voxel f + d).  What is new is the cost of finding a sample's
// blocks, and what is saved cannot change a sample's result: EVERY sample of the march is evaluated, in order; none is skipped.
struct HtRay { float min_d, step; };               // the march's two options (HtVol is not extended: every kernel that takes it keeps its instructions)

// The lane's memory of its last lookup: the block coordinate and what ht_lookup returned for it (-1 included).  bx starts at INT_MIN,
// which is no block coordinate (|b| <= 2^20).
struct HtCache { int bx, by, bz, blk; };

// htsdf_cell with the block of the LOWEST corner (f >> 3) found first, through the cache: when that block is missing the sample is invalid
// and nothing is loaded; a cell inside the block (local <= 6 on every axis) costs no further lookup; a cell across a face, an edge or the
// corner looks the other 1, 3 or 7 blocks up only now.  The validity is htsdf_cell's: all eight corners in existing blocks with W > 0.
// The address (g, floor, the range test, the fractions, block and local coordinates) is htsdf_cell's text, written out: taken from a
// helper shared with it, the hashed ray-casts compiled to 75 VGPRs for 92 / 93 and ran 1.1 to 3.1 % slower than the slowest of three
// runs of the parent on all six hashed medians of tools/time_htsdf_raycast.py, in both of two runs.
__device__ __forceinline__ bool htsdf_cell_cached(const HtVol& v, HtCache& h, float qx, float qy, float qz, float (&c)[8], float& tx, float& ty, float& tz) {
    const float gx = (qx - v.ox) / v.s, gy = (qy - v.oy) / v.s, gz = (qz - v.oz) / v.s;
    const float fx = floorf(gx), fy = floorf(gy), fz = floorf(gz);
    if (!(fx >= HT_CELL_LO && fx <= HT_CELL_HI && fy >= HT_CELL_LO && fy <= HT_CELL_HI && fz >= HT_CELL_LO && fz <= HT_CELL_HI)) return false;
    tx = gx - fx; ty = gy - fy; tz = gz - fz;
    const int ix = (int)fx, iy = (int)fy, iz = (int)fz;
    const int bx = ix >> 3, by = iy >> 3, bz = iz >> 3, lx = ix & 7, ly = iy & 7, lz = iz & 7;
    if (!(bx == h.bx && by == h.by && bz == h.bz)) { h.blk = ht_lookup(v, bx, by, bz); h.bx = bx; h.by = by; h.bz = bz; }
    const int b0 = h.blk;
    if (b0 < 0) return false;
    if (lx <= 6 && ly <= 6 && lz <= 6) {
        const float2* __restrict__ p = v.pool + ((size_t)b0 * 512 + (size_t)(lz * 64 + ly * 8 + lx));
        const float2 a0 = p[0], a1 = p[1], a2 = p[8], a3 = p[9], a4 = p[64], a5 = p[65], a6 = p[72], a7 = p[73];
        c[0] = a0.x; c[1] = a1.x; c[2] = a2.x; c[3] = a3.x; c[4] = a4.x; c[5] = a5.x; c[6] = a6.x; c[7] = a7.x;
        return a0.y > 0.f && a1.y > 0.f && a2.y > 0.f && a3.y > 0.f && a4.y > 0.f && a5.y > 0.f && a6.y > 0.f && a7.y > 0.f;
    }
    const bool cx = lx == 7, cy = ly == 7, cz = lz == 7;      // the axes along which the cell leaves its block
    // the seven other blocks, named by the axes they lie across; looked up where the cell reaches them, else the first block stands in
    const int b1 = cx ? ht_lookup(v, bx + 1, by, bz) : b0;
    const int b2 = cy ? ht_lookup(v, bx, by + 1, bz) : b0;
    const int b4 = cz ? ht_lookup(v, bx, by, bz + 1) : b0;
    if ((b1 | b2 | b4) < 0) return false;
    const int b3 = cx && cy ? ht_lookup(v, bx + 1, by + 1, bz) : (cx ? b1 : b2);
    const int b5 = cx && cz ? ht_lookup(v, bx + 1, by, bz + 1) : (cx ? b1 : b4);
    const int b6 = cy && cz ? ht_lookup(v, bx, by + 1, bz + 1) : (cy ? b2 : b4);
    if ((b3 | b5 | b6) < 0) return false;
    const int b7 = cx && cy && cz ? ht_lookup(v, bx + 1, by + 1, bz + 1) : (cx && cy ? b3 : (cx && cz ? b5 : (cy && cz ? b6 : (cx ? b1 : (cy ? b2 : b4)))));
    if (b7 < 0) return false;
    const int x0 = lx, x1 = (lx + 1) & 7, y0 = ly * 8, y1 = ((ly + 1) & 7) * 8, z0 = lz * 64, z1 = ((lz + 1) & 7) * 64;
    const float2 a0 = v.pool[(size_t)b0 * 512 + (size_t)(z0 + y0 + x0)], a1 = v.pool[(size_t)b1 * 512 + (size_t)(z0 + y0 + x1)];
    const float2 a2 = v.pool[(size_t)b2 * 512 + (size_t)(z0 + y1 + x0)], a3 = v.pool[(size_t)b3 * 512 + (size_t)(z0 + y1 + x1)];
    const float2 a4 = v.pool[(size_t)b4 * 512 + (size_t)(z1 + y0 + x0)], a5 = v.pool[(size_t)b5 * 512 + (size_t)(z1 + y0 + x1)];
    const float2 a6 = v.pool[(size_t)b6 * 512 + (size_t)(z1 + y1 + x0)], a7 = v.pool[(size_t)b7 * 512 + (size_t)(z1 + y1 + x1)];
    c[0] = a0.x; c[1] = a1.x; c[2] = a2.x; c[3] = a3.x; c[4] = a4.x; c[5] = a5.x; c[6] = a6.x; c[7] = a7.x;
    return a0.y > 0.f && a1.y > 0.f && a2.y > 0.f && a3.y > 0.f && a4.y > 0.f && a5.y > 0.f && a6.y > 0.f && a7.y > 0.f;
}

// One ray per lane, an 8 x 8 pixel tile per wave (a 16 x 16 tile per block), as k_tsdf_raycast: the 64 rays of a wave pass through the same
// few blocks, so their probes and gathers fall into the same cache lines.  Outputs, holes, the target's padding and the hit count (wave
// ballots, a block sum, one integer atomic per block) are that kernel's.
template <bool SOA>
__global__ __launch_bounds__(256) void k_htsdf_raycast(const HtVol v, const HtRay r, const TsdfCam cam, const TsdfMat pose, const TsdfRayOut o, int* __restrict__ n_hits) {
    __shared__ int red[4];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int u = blockIdx.x * 16 + (wave & 1) * 8 + (lane & 7), w = blockIdx.y * 16 + (wave >> 1) * 8 + (lane >> 3);
    const bool in = u < cam.width && w < cam.height;
    const float* __restrict__ P = pose.m;
    const float a = ((float)u - cam.cx) / cam.fx, b = ((float)w - cam.cy) / cam.fy;
    const float dx = P[0] * a + (P[4] * b + P[8] * 1.f), dy = P[1] * a + (P[5] * b + P[9] * 1.f), dz = P[2] * a + (P[6] * b + P[10] * 1.f);
    float zs = -INFINITY, n0 = -INFINITY, n1 = -INFINITY, n2 = -INFINITY;
    if (in) {
        bool prev_valid = false, ended = false;
        float f_prev = 0.f, z_prev = 0.f, f_end = 0.f;
        float c[8], tx, ty, tz;
        HtCache h; h.bx = h.by = h.bz = (int)0x80000000; h.blk = -1;
        for (int k = 0; ; k++) {
            const float z = r.min_d + (float)k * r.step;
            if (!(z <= v.max_d)) break;
            if (htsdf_cell_cached(v, h, P[12] + z * dx, P[13] + z * dy, P[14] + z * dz, c, tx, ty, tz)) {
                const float e0 = tsdf_lerp(tsdf_lerp(c[0], c[1], tx), tsdf_lerp(c[2], c[3], tx), ty);
                const float e1 = tsdf_lerp(tsdf_lerp(c[4], c[5], tx), tsdf_lerp(c[6], c[7], tx), ty);
                const float f = tsdf_lerp(e0, e1, tz);
                if (f <= 0.f) { ended = true; f_end = f; break; }      // (a NaN never ends a ray)
                prev_valid = true; f_prev = f; z_prev = z;
            } else prev_valid = false;
        }
        if (ended && prev_valid && f_prev > 0.f) {
            const float zh = z_prev + r.step * (f_prev / (f_prev - f_end));
            if (htsdf_cell_cached(v, h, P[12] + zh * dx, P[13] + zh * dy, P[14] + zh * dz, c, tx, ty, tz)) {
                const float gx = tsdf_lerp(tsdf_lerp(c[1] - c[0], c[3] - c[2], ty), tsdf_lerp(c[5] - c[4], c[7] - c[6], ty), tz);
                const float gy = tsdf_lerp(tsdf_lerp(c[2] - c[0], c[3] - c[1], tx), tsdf_lerp(c[6] - c[4], c[7] - c[5], tx), tz);
                const float gz = tsdf_lerp(tsdf_lerp(c[4] - c[0], c[5] - c[1], tx), tsdf_lerp(c[6] - c[2], c[7] - c[3], tx), ty);
                const float x = -(P[0] * gx + (P[1] * gy + P[2] * gz)), y = -(P[4] * gx + (P[5] * gy + P[6] * gz)), zz = -(P[8] * gx + (P[9] * gy + P[10] * gz));
                const float sq = x * x + (y * y + zz * zz);
                const float len = sqrtf(sq);
                const float m0 = x / len, m1 = y / len, m2 = zz / len;
                if (finite3(m0, m1, m2)) { zs = zh; n0 = m0; n1 = m1; n2 = m2; }
            }
        }
    }
    const bool hit = zs != -INFINITY;
    if (in) {
        const size_t p = (size_t)w * cam.width + u;
        const float vx = hit ? a * zs : -INFINITY, vy = hit ? b * zs : -INFINITY;
        if (SOA) {
            o.x[p] = vx; o.y[p] = vy; o.z[p] = zs; o.nx[p] = n0; o.ny[p] = n1; o.nz[p] = n2;
        } else {
            if (o.depth) o.depth[p] = zs;
            if (o.vert) { o.vert[p * 3] = vx; o.vert[p * 3 + 1] = vy; o.vert[p * 3 + 2] = zs; }
            if (o.nrm) { o.nrm[p * 3] = n0; o.nrm[p * 3 + 1] = n1; o.nrm[p * 3 + 2] = n2; }
        }
    }
    if (SOA && blockIdx.x == 0 && blockIdx.y == 0 && tid < 64) {      // the target's padding (upload_cloud's convention)
        const int q = cam.width * cam.height + tid;
        if (q < o.npad) { o.x[q] = INFINITY; o.y[q] = INFINITY; o.z[q] = INFINITY; }
    }
    const unsigned long long bh = __ballot(hit);
    if (lane == 0) red[wave] = __popcll(bh);
    __syncthreads();
    if (tid == 0) {
        const int t = (red[0] + red[1]) + (red[2] + red[3]);
        if (t) atomicAdd(n_hits, t);
    }
}
