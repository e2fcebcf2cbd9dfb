// dev_tsdf_hash_raycast_color.hpp -- the COLOURED ray-cast of the hashed TSDF volume (icp_tsdf_raycast_color_hashed, the target of
// icp_set_target_tsdf_color_hashed and icp_track_depth_model_color_hashed): k_htsdf_raycast (dev_tsdf_hash_raycast.hpp) with the colour
// rule of k_tsdf_raycast_color (dev_tsdf.hpp) read from the colour pool (dev_tsdf_hash_color.hpp).  Contract: include/icp_hip.h, DESIGN.md
// section 6zc; tests/htsdf_color_view_restatement.py states the same arithmetic in numpy.  Part of icp_device.hpp (included from there,
// inside namespace icpdev, after dev_tsdf_hash_raycast.hpp and dev_tsdf_hash_color.hpp).
// ------------------------------------------------------------------------------------------------
// Restated, not shared: k_htsdf_raycast, htsdf_cell_cached and k_tsdf_raycast_color keep their instructions.  The march uses
// htsdf_cell_cached as it is; only the cell of q(z*), the normal's cell, is looked up by the variant below, which hands the eight block
// indices it found to the colour read: the colour corners cost no second table probe and are loaded for that one cell per ray.

// The pool indices of a cell's eight corners (corner k = dx + 2 dy + 4 dz) and the local coordinate of its lowest corner.
struct HtCellBlocks { int b0, b1, b2, b3, b4, b5, b6, b7, lx, ly, lz; };

// htsdf_cell_cached, handing back where it found the corners.  The same loads in the same order, the same verdict.
__device__ __forceinline__ bool htsdf_cell_cached_blocks(const HtVol& v, HtCache& h, float qx, float qy, float qz, float (&c)[8], float& tx, float& ty, float& tz,
                                                         HtCellBlocks& cb) {
    const float gx = (qx - v.ox) / v.s, gy = (qy - v.oy) / v.s, gz = (qz - v.oz) / v.s;
    const float fx = floorf(gx), fy = floorf(gy), fz = floorf(gz);
    if (!(fx >= HT_CELL_LO && fx <= HT_CELL_HI && fy >= HT_CELL_LO && fy <= HT_CELL_HI && fz >= HT_CELL_LO && fz <= HT_CELL_HI)) return false;
    tx = gx - fx; ty = gy - fy; tz = gz - fz;
    const int ix = (int)fx, iy = (int)fy, iz = (int)fz;
    const int bx = ix >> 3, by = iy >> 3, bz = iz >> 3, lx = ix & 7, ly = iy & 7, lz = iz & 7;
    if (!(bx == h.bx && by == h.by && bz == h.bz)) { h.blk = ht_lookup(v, bx, by, bz); h.bx = bx; h.by = by; h.bz = bz; }
    const int b0 = h.blk;
    if (b0 < 0) return false;
    cb.lx = lx; cb.ly = ly; cb.lz = lz;
    if (lx <= 6 && ly <= 6 && lz <= 6) {
        const float2* __restrict__ p = v.pool + ((size_t)b0 * 512 + (size_t)(lz * 64 + ly * 8 + lx));
        const float2 a0 = p[0], a1 = p[1], a2 = p[8], a3 = p[9], a4 = p[64], a5 = p[65], a6 = p[72], a7 = p[73];
        c[0] = a0.x; c[1] = a1.x; c[2] = a2.x; c[3] = a3.x; c[4] = a4.x; c[5] = a5.x; c[6] = a6.x; c[7] = a7.x;
        cb.b0 = b0; cb.b1 = b0; cb.b2 = b0; cb.b3 = b0; cb.b4 = b0; cb.b5 = b0; cb.b6 = b0; cb.b7 = b0;
        return a0.y > 0.f && a1.y > 0.f && a2.y > 0.f && a3.y > 0.f && a4.y > 0.f && a5.y > 0.f && a6.y > 0.f && a7.y > 0.f;
    }
    const bool cx = lx == 7, cy = ly == 7, cz = lz == 7;      // the axes along which the cell leaves its block
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
    cb.b0 = b0; cb.b1 = b1; cb.b2 = b2; cb.b3 = b3; cb.b4 = b4; cb.b5 = b5; cb.b6 = b6; cb.b7 = b7;
    return a0.y > 0.f && a1.y > 0.f && a2.y > 0.f && a3.y > 0.f && a4.y > 0.f && a5.y > 0.f && a6.y > 0.f && a7.y > 0.f;
}

// tsdf_cell_color on the blocks: the packed colour of the cell htsdf_cell_cached_blocks accepted, at its fractions.  Corner (dx, dy, dz) is
// the colour-pool entry of voxel f + d, at the pool index the geometry lookup found for it.
__device__ __forceinline__ uint32_t htsdf_cell_color(const float4* __restrict__ cpool, const HtCellBlocks& cb, float tx, float ty, float tz) {
    const int x0 = cb.lx, x1 = (cb.lx + 1) & 7, y0 = cb.ly * 8, y1 = ((cb.ly + 1) & 7) * 8, z0 = cb.lz * 64, z1 = ((cb.lz + 1) & 7) * 64;
    const float4 a0 = cpool[(size_t)cb.b0 * 512 + (size_t)(z0 + y0 + x0)], a1 = cpool[(size_t)cb.b1 * 512 + (size_t)(z0 + y0 + x1)];
    const float4 a2 = cpool[(size_t)cb.b2 * 512 + (size_t)(z0 + y1 + x0)], a3 = cpool[(size_t)cb.b3 * 512 + (size_t)(z0 + y1 + x1)];
    const float4 a4 = cpool[(size_t)cb.b4 * 512 + (size_t)(z1 + y0 + x0)], a5 = cpool[(size_t)cb.b5 * 512 + (size_t)(z1 + y0 + x1)];
    const float4 a6 = cpool[(size_t)cb.b6 * 512 + (size_t)(z1 + y1 + x0)], a7 = cpool[(size_t)cb.b7 * 512 + (size_t)(z1 + y1 + x1)];
    float r, g, b;
    if (a0.w > 0.f && a1.w > 0.f && a2.w > 0.f && a3.w > 0.f && a4.w > 0.f && a5.w > 0.f && a6.w > 0.f && a7.w > 0.f) {
        r = tsdf_lerp8(a0.x, a1.x, a2.x, a3.x, a4.x, a5.x, a6.x, a7.x, tx, ty, tz);
        g = tsdf_lerp8(a0.y, a1.y, a2.y, a3.y, a4.y, a5.y, a6.y, a7.y, tx, ty, tz);
        b = tsdf_lerp8(a0.z, a1.z, a2.z, a3.z, a4.z, a5.z, a6.z, a7.z, tx, ty, tz);
    } else {
        const bool ux = tx >= 0.5f, uy = ty >= 0.5f, uz = tz >= 0.5f;      // the corner nearest the hit
        const int lo = uy ? (ux ? cb.b3 : cb.b2) : (ux ? cb.b1 : cb.b0), hi = uy ? (ux ? cb.b7 : cb.b6) : (ux ? cb.b5 : cb.b4);      // (selects: no register array is indexed)
        const float4 a = cpool[(size_t)(uz ? hi : lo) * 512 + (size_t)((uz ? z1 : z0) + (uy ? y1 : y0) + (ux ? x1 : x0))];      // (read again)
        if (!(a.w > 0.f)) return 0u;
        r = a.x; g = a.y; b = a.z;
    }
    return tsdf_color_pack(r, g, b);
}

// k_htsdf_raycast with k_tsdf_raycast_color's colour, second ballot and count.  SOA (the coloured target): a hit without colour is written
// as a hole, so every point of the target has a colour.
template <bool SOA>
__global__ __launch_bounds__(256) void k_htsdf_raycast_color(const HtVol v, const HtRay r, const TsdfCam cam, const TsdfMat pose, const TsdfRayOut o, int* __restrict__ n_hits,
                                                             const float4* __restrict__ cpool, const TsdfColorOut co, int* __restrict__ n_colored) {
    __shared__ int red[4], redc[4];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int u = blockIdx.x * 16 + (wave & 1) * 8 + (lane & 7), w = blockIdx.y * 16 + (wave >> 1) * 8 + (lane >> 3);
    const bool in = u < cam.width && w < cam.height;
    const float* __restrict__ P = pose.m;
    const float a = ((float)u - cam.cx) / cam.fx, b = ((float)w - cam.cy) / cam.fy;
    const float dx = P[0] * a + (P[4] * b + P[8] * 1.f), dy = P[1] * a + (P[5] * b + P[9] * 1.f), dz = P[2] * a + (P[6] * b + P[10] * 1.f);
    float zs = -INFINITY, n0 = -INFINITY, n1 = -INFINITY, n2 = -INFINITY;
    uint32_t rgba = 0u;
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
            HtCellBlocks cb;
            if (htsdf_cell_cached_blocks(v, h, P[12] + zh * dx, P[13] + zh * dy, P[14] + zh * dz, c, tx, ty, tz, cb)) {
                const float gx = tsdf_lerp(tsdf_lerp(c[1] - c[0], c[3] - c[2], ty), tsdf_lerp(c[5] - c[4], c[7] - c[6], ty), tz);
                const float gy = tsdf_lerp(tsdf_lerp(c[2] - c[0], c[3] - c[1], tx), tsdf_lerp(c[6] - c[4], c[7] - c[5], tx), tz);
                const float gz = tsdf_lerp(tsdf_lerp(c[4] - c[0], c[5] - c[1], tx), tsdf_lerp(c[6] - c[2], c[7] - c[3], tx), ty);
                const float x = -(P[0] * gx + (P[1] * gy + P[2] * gz)), y = -(P[4] * gx + (P[5] * gy + P[6] * gz)), zz = -(P[8] * gx + (P[9] * gy + P[10] * gz));
                const float sq = x * x + (y * y + zz * zz);
                const float len = sqrtf(sq);
                const float m0 = x / len, m1 = y / len, m2 = zz / len;
                if (finite3(m0, m1, m2)) {
                    rgba = htsdf_cell_color(cpool, cb, tx, ty, tz);
                    if (!SOA || rgba != 0u) { zs = zh; n0 = m0; n1 = m1; n2 = m2; }
                }
            }
        }
    }
    const bool hit = zs != -INFINITY;
    if (in) {
        const size_t p = (size_t)w * cam.width + u;
        const float vx = hit ? a * zs : -INFINITY, vy = hit ? b * zs : -INFINITY;
        if (SOA) {
            o.x[p] = vx; o.y[p] = vy; o.z[p] = zs; o.nx[p] = n0; o.ny[p] = n1; o.nz[p] = n2;
            co.rgba[p] = rgba; color_features(rgba, co.cr[p], co.cg[p], co.cb[p]);
        } else {
            if (o.depth) o.depth[p] = zs;
            if (o.vert) { o.vert[p * 3] = vx; o.vert[p * 3 + 1] = vy; o.vert[p * 3 + 2] = zs; }
            if (o.nrm) { o.nrm[p * 3] = n0; o.nrm[p * 3 + 1] = n1; o.nrm[p * 3 + 2] = n2; }
            if (co.rgba) co.rgba[p] = rgba;
        }
    }
    if (SOA && blockIdx.x == 0 && blockIdx.y == 0 && tid < 64) {      // the target's padding (upload_cloud's convention)
        const int q = cam.width * cam.height + tid;
        if (q < o.npad) {
            o.x[q] = INFINITY; o.y[q] = INFINITY; o.z[q] = INFINITY;
            co.cr[q] = 0.f; co.cg[q] = 0.f; co.cb[q] = 0.f;      // (k_colors' convention)
        }
    }
    const unsigned long long bh = __ballot(hit);
    if (lane == 0) red[wave] = __popcll(bh);
    __syncthreads();
    if (tid == 0) {
        const int t = (red[0] + red[1]) + (red[2] + red[3]);
        if (t) atomicAdd(n_hits, t);
    }
    const unsigned long long bc = __ballot(rgba != 0u);
    if (lane == 0) redc[wave] = __popcll(bc);
    __syncthreads();
    if (tid == 0) {
        const int t = (redc[0] + redc[1]) + (redc[2] + redc[3]);
        if (t) atomicAdd(n_colored, t);
    }
}
