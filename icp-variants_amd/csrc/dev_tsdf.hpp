// dev_tsdf.hpp -- the model of frame-to-model tracking: a dense truncated signed distance volume (Newcombe et al., KinectFusion, ISMAR 2011),
// depth frames fused into it (k_tsdf_integrate) and ray-cast out of it as an organised cloud (k_tsdf_raycast).  Contract: include/icp_hip.h,
// DESIGN.md section 6m.  Part of icp_device.hpp (included from there, inside namespace icpdev); see that file for the build contract.
// ------------------------------------------------------------------------------------------------
// Storage: one float2 (tsdf, weight) per voxel, x fastest -- a ray-cast corner is one 8-byte load, an update one 8-byte load and store.
// Optionally a second array of the same indexing, one float4 (R, G, B, Wc) per voxel: the coloured model of DESIGN.md section 6p
// (k_tsdf_integrate_color, k_tsdf_raycast_color), a colour corner one 16-byte load.
// Every fp32 operation below is written in the contract's order (one rounding each, -ffp-contract=off): tests/tsdf_restatement.py states
// the same arithmetic in numpy and is compared bit for bit.
// The kernels call only __forceinline__ helpers: an existing kernel keeps exactly the code it had.
struct TsdfVol {
    float2* vox;                                  // [nz][ny][nx] (tsdf, weight)
    int nx, ny, nz;
    float ox, oy, oz, s;                          // centre of voxel (0, 0, 0), voxel size
    float trunc, max_w, min_d, max_d, step;
};
struct TsdfCam { int width, height; float fx, fy, cx, cy; };
struct TsdfMat { float m[16]; };                   // integrate: M = pose^-1 as 3x3 row-major + t (12 used); ray-cast: the pose, column-major

constexpr int TSDF_KCHUNK = 16;                    // voxels along z per thread of k_tsdf_integrate

// One thread per (i, j) walks TSDF_KCHUNK voxels along k; a wave holds 64 consecutive i, so every volume access of a wave is one 512-byte
// run.  Whether a voxel is updated is decided from the depth frame alone; the volume is read and written only where it is.
// The world -> camera map is affine in k, but the contract's sum (M_r0 p_x + (M_r1 p_y + M_r2 p_z)) + M_r3 rounds after every operation, so
// a running sum would not keep its bits: what is hoisted out of the walk are the two products that do not depend on k.
// COLOR (k_tsdf_integrate_color): the colour volume `col` -- one float4 (R, G, B, Wc) per voxel, the channels running averages of the byte
// values 0..255 -- is updated from the pixel's own four bytes where the voxel is updated AND !(sdf > truncation): the band, not the free
// space in front of it, whose voxels would take the colour of whatever lies behind them.  Elsewhere its float4 is neither read nor written.
template <bool COLOR>
__device__ __forceinline__ void tsdf_integrate_body(const TsdfVol& v, const TsdfCam& cam, const TsdfMat& mat, const float* __restrict__ depth, int* __restrict__ n_updated,
                                                    int (&red)[4], const uint32_t* __restrict__ rgbx, float4* __restrict__ col, int* __restrict__ n_colored, int (&redc)[4]) {
    const int i = blockIdx.x * 64 + threadIdx.x, j = blockIdx.y * 4 + threadIdx.y;
    const bool in = i < v.nx && j < v.ny;
    const float* __restrict__ M = mat.m;
    const float px = v.ox + (float)i * v.s, py = v.oy + (float)j * v.s;
    const float ax = M[0] * px, ay = M[3] * px, az = M[6] * px;
    const float bx = M[1] * py, by = M[4] * py, bz = M[7] * py;
    const int k0 = blockIdx.z * TSDF_KCHUNK, k1 = min(k0 + TSDF_KCHUNK, v.nz);
    const float wf = (float)cam.width, hf = (float)cam.height;
    const size_t plane = (size_t)v.nx * v.ny;
    size_t idx = (size_t)k0 * plane + (size_t)j * v.nx + i;
    int cnt = 0, ccnt = 0;                         // the wave's updates (coloured voxels) so far (the same in every lane)
    for (int k = k0; k < k1; k++, idx += plane) {
        bool upd = false, paint = false;
        float f = 0.f;
        int pix = 0;
        if (in) {
            const float pz = v.oz + (float)k * v.s;
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
                        if (COLOR) { paint = upd && !(sdf > v.trunc); pix = (int)w * cam.width + (int)u; }
                    }
                }
            }
        }
        if (upd) {
            const float2 o = v.vox[idx];
            float2 r;
            r.x = (o.y * o.x + f) / (o.y + 1.f);
            r.y = fminf(o.y + 1.f, v.max_w);
            v.vox[idx] = r;
        }
        cnt += __popcll(__ballot(upd));
        if (COLOR) {
            if (paint) {
                const uint32_t b = rgbx[pix];
                const float4 o = col[idx];
                float4 r;
                r.x = (o.w * o.x + (float)(int)(b & 0xFFu)) / (o.w + 1.f);
                r.y = (o.w * o.y + (float)(int)((b >> 8) & 0xFFu)) / (o.w + 1.f);
                r.z = (o.w * o.z + (float)(int)((b >> 16) & 0xFFu)) / (o.w + 1.f);
                r.w = fminf(o.w + 1.f, v.max_w);
                col[idx] = r;
            }
            ccnt += __popcll(__ballot(paint));
        }
    }
    // count: wave ballots, a block sum, one integer atomic per block (k_reciprocal's form)
    if (n_updated) {
        if (threadIdx.x == 0) red[threadIdx.y] = cnt;
        __syncthreads();
        if (threadIdx.x == 0 && threadIdx.y == 0) {
            const int t = (red[0] + red[1]) + (red[2] + red[3]);
            if (t) atomicAdd(n_updated, t);
        }
    }
    if (COLOR && n_colored) {
        if (threadIdx.x == 0) redc[threadIdx.y] = ccnt;
        __syncthreads();
        if (threadIdx.x == 0 && threadIdx.y == 0) {
            const int t = (redc[0] + redc[1]) + (redc[2] + redc[3]);
            if (t) atomicAdd(n_colored, t);
        }
    }
}
__global__ __launch_bounds__(256) void k_tsdf_integrate(const TsdfVol v, const TsdfCam cam, const TsdfMat mat, const float* __restrict__ depth,
                                                        int* __restrict__ n_updated) {
    __shared__ int red[4];
    tsdf_integrate_body<false>(v, cam, mat, depth, n_updated, red, nullptr, nullptr, nullptr, red);
}
__global__ __launch_bounds__(256) void k_tsdf_integrate_color(const TsdfVol v, const TsdfCam cam, const TsdfMat mat, const float* __restrict__ depth,
                                                              int* __restrict__ n_updated, const uint32_t* __restrict__ rgbx, float4* __restrict__ col,
                                                              int* __restrict__ n_colored) {
    __shared__ int red[4], redc[4];
    tsdf_integrate_body<true>(v, cam, mat, depth, n_updated, red, rgbx, col, n_colored, redc);
}

// The cell of world point q: its eight corners (c[dx + 2 dy + 4 dz], issued together) and fractions.  false -- and nothing loaded beyond what
// decides it -- when the cell leaves the volume (tested in float: NaN and out-of-range coordinates never reach a cast) or a corner is unobserved.
__device__ __forceinline__ bool tsdf_cell(const TsdfVol& v, float qx, float qy, float qz, float (&c)[8], float& tx, float& ty, float& tz) {
    const float gx = (qx - v.ox) / v.s, gy = (qy - v.oy) / v.s, gz = (qz - v.oz) / v.s;
    const float fx = floorf(gx), fy = floorf(gy), fz = floorf(gz);
    if (!(fx >= 0.f && fx <= (float)(v.nx - 2) && fy >= 0.f && fy <= (float)(v.ny - 2) && fz >= 0.f && fz <= (float)(v.nz - 2))) return false;
    tx = gx - fx; ty = gy - fy; tz = gz - fz;
    const size_t plane = (size_t)v.nx * v.ny;
    const float2* __restrict__ p = v.vox + ((size_t)(int)fz * plane + (size_t)(int)fy * v.nx + (size_t)(int)fx);
    const float2 a0 = p[0], a1 = p[1], a2 = p[v.nx], a3 = p[v.nx + 1];
    const float2 a4 = p[plane], a5 = p[plane + 1], a6 = p[plane + v.nx], a7 = p[plane + v.nx + 1];
    c[0] = a0.x; c[1] = a1.x; c[2] = a2.x; c[3] = a3.x; c[4] = a4.x; c[5] = a5.x; c[6] = a6.x; c[7] = a7.x;
    return a0.y > 0.f && a1.y > 0.f && a2.y > 0.f && a3.y > 0.f && a4.y > 0.f && a5.y > 0.f && a6.y > 0.f && a7.y > 0.f;
}
__device__ __forceinline__ float tsdf_lerp(float a, float b, float t) { return a + t * (b - a); }

// Where the ray-cast writes: the caller's arrays (AoS, any of them null) or the SoA planes of the target, x y z padded with +inf to npad.
struct TsdfRayOut { float *depth, *vert, *nrm; float *x, *y, *z, *nx, *ny, *nz; int npad; };

// One ray per lane, an 8 x 8 pixel tile per wave (a 16 x 16 tile per block): the 64 rays of a wave gather from neighbouring cells.
// Work left out, none of which can change a result: a sample whose cell leaves the volume loads nothing; the interpolant is evaluated only
// for cells whose eight corners are observed; nothing is evaluated behind the sample that ends the ray.
template <bool SOA>
__global__ __launch_bounds__(256) void k_tsdf_raycast(const TsdfVol v, const TsdfCam cam, const TsdfMat pose, const TsdfRayOut o, int* __restrict__ n_hits) {
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
        for (int k = 0; ; k++) {
            const float z = v.min_d + (float)k * v.step;
            if (!(z <= v.max_d)) break;
            if (tsdf_cell(v, P[12] + z * dx, P[13] + z * dy, P[14] + z * dz, c, tx, ty, tz)) {
                const float e0 = tsdf_lerp(tsdf_lerp(c[0], c[1], tx), tsdf_lerp(c[2], c[3], tx), ty);
                const float e1 = tsdf_lerp(tsdf_lerp(c[4], c[5], tx), tsdf_lerp(c[6], c[7], tx), ty);
                const float f = tsdf_lerp(e0, e1, tz);
                if (f <= 0.f) { ended = true; f_end = f; break; }      // (a NaN never ends a ray)
                prev_valid = true; f_prev = f; z_prev = z;
            } else prev_valid = false;
        }
        if (ended && prev_valid && f_prev > 0.f) {
            const float zh = z_prev + v.step * (f_prev / (f_prev - f_end));
            if (tsdf_cell(v, P[12] + zh * dx, P[13] + zh * dy, P[14] + zh * dz, c, tx, ty, tz)) {
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

// k_tsdf_raycast_color: k_tsdf_raycast with the colour of a hit from the cell of q(z*), the cell of the normal -- the nested lerp of its
// eight colour corners when all have Wc > 0, else the corner nearest the hit when that one has, else none; the colour corners are loaded
// for that one cell only.  SOA (the coloured target): a hit without colour is written as a hole, so every point of the target has one.
struct TsdfColorOut { uint32_t* rgba; float *cr, *cg, *cb; };      // packed R | G << 8 | B << 16 | 255 << 24 (0: no colour); SOA: the target's colour planes
__device__ __forceinline__ float tsdf_lerp8(float c0, float c1, float c2, float c3, float c4, float c5, float c6, float c7, float tx, float ty, float tz) {
    return tsdf_lerp(tsdf_lerp(tsdf_lerp(c0, c1, tx), tsdf_lerp(c2, c3, tx), ty), tsdf_lerp(tsdf_lerp(c4, c5, tx), tsdf_lerp(c6, c7, tx), ty), tz);
}
// The packed colour at world point q with fractions (tx, ty, tz) in its cell, which is known to lie inside the volume (tsdf_cell said so).
__device__ __forceinline__ uint32_t tsdf_cell_color(const TsdfVol& v, const float4* __restrict__ col, float qx, float qy, float qz, float tx, float ty, float tz) {
    const float fx = floorf((qx - v.ox) / v.s), fy = floorf((qy - v.oy) / v.s), fz = floorf((qz - v.oz) / v.s);
    const size_t plane = (size_t)v.nx * v.ny;
    const float4* __restrict__ p = col + ((size_t)(int)fz * plane + (size_t)(int)fy * v.nx + (size_t)(int)fx);
    const float4 a0 = p[0], a1 = p[1], a2 = p[v.nx], a3 = p[v.nx + 1];
    const float4 a4 = p[plane], a5 = p[plane + 1], a6 = p[plane + v.nx], a7 = p[plane + v.nx + 1];
    float r, g, b;
    if (a0.w > 0.f && a1.w > 0.f && a2.w > 0.f && a3.w > 0.f && a4.w > 0.f && a5.w > 0.f && a6.w > 0.f && a7.w > 0.f) {
        r = tsdf_lerp8(a0.x, a1.x, a2.x, a3.x, a4.x, a5.x, a6.x, a7.x, tx, ty, tz);
        g = tsdf_lerp8(a0.y, a1.y, a2.y, a3.y, a4.y, a5.y, a6.y, a7.y, tx, ty, tz);
        b = tsdf_lerp8(a0.z, a1.z, a2.z, a3.z, a4.z, a5.z, a6.z, a7.z, tx, ty, tz);
    } else {
        const float4 a = p[(tx >= 0.5f ? 1 : 0) + (ty >= 0.5f ? (size_t)v.nx : 0) + (tz >= 0.5f ? plane : 0)];      // (read again: no register array is indexed)
        if (!(a.w > 0.f)) return 0u;
        r = a.x; g = a.y; b = a.z;
    }
    return tsdf_color_pack(r, g, b);
}

// The march is k_tsdf_raycast's, restated: sharing it through a body template changed that kernel's instructions.
template <bool SOA>
__global__ __launch_bounds__(256) void k_tsdf_raycast_color(const TsdfVol v, const TsdfCam cam, const TsdfMat pose, const TsdfRayOut o, int* __restrict__ n_hits,
                                                            const float4* __restrict__ col, const TsdfColorOut co, int* __restrict__ n_colored) {
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
        for (int k = 0; ; k++) {
            const float z = v.min_d + (float)k * v.step;
            if (!(z <= v.max_d)) break;
            if (tsdf_cell(v, P[12] + z * dx, P[13] + z * dy, P[14] + z * dz, c, tx, ty, tz)) {
                const float e0 = tsdf_lerp(tsdf_lerp(c[0], c[1], tx), tsdf_lerp(c[2], c[3], tx), ty);
                const float e1 = tsdf_lerp(tsdf_lerp(c[4], c[5], tx), tsdf_lerp(c[6], c[7], tx), ty);
                const float f = tsdf_lerp(e0, e1, tz);
                if (f <= 0.f) { ended = true; f_end = f; break; }      // (a NaN never ends a ray)
                prev_valid = true; f_prev = f; z_prev = z;
            } else prev_valid = false;
        }
        if (ended && prev_valid && f_prev > 0.f) {
            const float zh = z_prev + v.step * (f_prev / (f_prev - f_end));
            if (tsdf_cell(v, P[12] + zh * dx, P[13] + zh * dy, P[14] + zh * dz, c, tx, ty, tz)) {
                const float gx = tsdf_lerp(tsdf_lerp(c[1] - c[0], c[3] - c[2], ty), tsdf_lerp(c[5] - c[4], c[7] - c[6], ty), tz);
                const float gy = tsdf_lerp(tsdf_lerp(c[2] - c[0], c[3] - c[1], tx), tsdf_lerp(c[6] - c[4], c[7] - c[5], tx), tz);
                const float gz = tsdf_lerp(tsdf_lerp(c[4] - c[0], c[5] - c[1], tx), tsdf_lerp(c[6] - c[2], c[7] - c[3], tx), ty);
                const float x = -(P[0] * gx + (P[1] * gy + P[2] * gz)), y = -(P[4] * gx + (P[5] * gy + P[6] * gz)), zz = -(P[8] * gx + (P[9] * gy + P[10] * gz));
                const float sq = x * x + (y * y + zz * zz);
                const float len = sqrtf(sq);
                const float m0 = x / len, m1 = y / len, m2 = zz / len;
                if (finite3(m0, m1, m2)) {
                    rgba = tsdf_cell_color(v, col, P[12] + zh * dx, P[13] + zh * dy, P[14] + zh * dz, tx, ty, tz);
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
