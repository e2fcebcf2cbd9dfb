// dev_sdf_color.hpp -- direct SDF tracking with a photometric term from the colour volume (Bylow, Olsson, Kahl 2014): next to the geometric
// row of dev_sdf.hpp a coloured pixel adds a second row, its intensity residual and the gradient of the intensity field, both read from the
// colour array in the cell the distance is read in.  Contract: include/icp_hip.h, DESIGN.md section 6r.  Part of icp_device.hpp (included
// from there, inside namespace icpdev, after dev_sdf.hpp, whose cell, field, gradient and composition it uses).
// ------------------------------------------------------------------------------------------------
// The kernels of dev_sdf.hpp are restated here, not shared through a body template: they keep their instructions (DESIGN.md section 6p did
// the same for the ray-cast march).  tests/sdf_color_restatement.py states the same arithmetic in numpy.
constexpr int SDFC_NSUM = 29;                      // dev_sdf.hpp's 28 with the photometric terms added in, + 1: sum w_c r_c r_c alone
constexpr int SDFC_ROWS = 8;                       // k_sdf_solve_color folds the sums wave, wave + 4, ...: 8 rows of 4, the last three empty
struct SdfColorState {
    float pose[16], pose0[16];                     // as SdfState
    int stop, pad;
    double sums[SDFC_NSUM];
    int counts[3], pad2;                           // n_depth, n_valid, n_color
};
struct SdfColorFrame {
    const float4* col;                             // the colour array, the indexing of TsdfVol::vox
    const uint32_t* rgbx;                          // the colour frame of the depth frame (R | G << 8 | B << 16 | X << 24 per pixel)
    float weight, huber;                           // icp_sdf_color_options
};

// The eight colour corners of the cell of q (known to lie inside the volume: tsdf_cell said so), issued together: s_k = (R_k + G_k) + B_k
// per corner, and whether every corner has Wc > 0.
__device__ __forceinline__ bool sdf_color_cell(const TsdfVol& v, const float4* __restrict__ col, float qx, float qy, float qz, float (&s)[8]) {
    const float fx = floorf((qx - v.ox) / v.s), fy = floorf((qy - v.oy) / v.s), fz = floorf((qz - v.oz) / v.s);
    const size_t plane = (size_t)v.nx * v.ny;
    const float4* __restrict__ p = col + ((size_t)(int)fz * plane + (size_t)(int)fy * v.nx + (size_t)(int)fx);
    const float4 a0 = p[0], a1 = p[1], a2 = p[v.nx], a3 = p[v.nx + 1];
    const float4 a4 = p[plane], a5 = p[plane + 1], a6 = p[plane + v.nx], a7 = p[plane + v.nx + 1];
    s[0] = (a0.x + a0.y) + a0.z; s[1] = (a1.x + a1.y) + a1.z; s[2] = (a2.x + a2.y) + a2.z; s[3] = (a3.x + a3.y) + a3.z;
    s[4] = (a4.x + a4.y) + a4.z; s[5] = (a5.x + a5.y) + a5.z; s[6] = (a6.x + a6.y) + a6.z; s[7] = (a7.x + a7.y) + a7.z;
    return a0.w > 0.f && a1.w > 0.f && a2.w > 0.f && a3.w > 0.f && a4.w > 0.f && a5.w > 0.f && a6.w > 0.f && a7.w > 0.f;
}
// The cell of q by its bounds alone (the geometry's weights play no part) and its fractions: icp_tsdf_sample_color's validity.
__device__ __forceinline__ bool sdf_cell_inside(const TsdfVol& v, float qx, float qy, float qz, float& tx, float& ty, float& tz) {
    const float gx = (qx - v.ox) / v.s, gy = (qy - v.oy) / v.s, gz = (qz - v.oz) / v.s;
    const float fx = floorf(gx), fy = floorf(gy), fz = floorf(gz);
    if (!(fx >= 0.f && fx <= (float)(v.nx - 2) && fy >= 0.f && fy <= (float)(v.ny - 2) && fz >= 0.f && fz <= (float)(v.nz - 2))) return false;
    tx = gx - fx; ty = gy - fy; tz = gz - fz;
    return true;
}

// icp_tsdf_sample_color: the intensity field S and its gradient H per voxel at n world points, one point per thread.
__global__ __launch_bounds__(256) void k_tsdf_sample_color(const TsdfVol v, const float4* __restrict__ col, const float* __restrict__ pts, int n,
                                                           float* __restrict__ s_out, float* __restrict__ h_out, uint8_t* __restrict__ valid_out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float qx = pts[(size_t)i * 3], qy = pts[(size_t)i * 3 + 1], qz = pts[(size_t)i * 3 + 2];
    float s[8], tx, ty, tz, S = 0.f, hx = 0.f, hy = 0.f, hz = 0.f;
    bool ok = sdf_cell_inside(v, qx, qy, qz, tx, ty, tz);
    if (ok) ok = sdf_color_cell(v, col, qx, qy, qz, s);
    if (ok) { S = sdf_field(s, tx, ty, tz); sdf_gradient(s, tx, ty, tz, hx, hy, hz); }
    s_out[i] = sdf_canonical(S);
    h_out[(size_t)i * 3] = sdf_canonical(hx); h_out[(size_t)i * 3 + 1] = sdf_canonical(hy); h_out[(size_t)i * 3 + 2] = sdf_canonical(hz);
    valid_out[i] = ok ? 1 : 0;
}

// k_sdf_init with the colour record.
__global__ void k_sdf_init_color(SdfColorState* st, const TsdfMat pose, icp_sdf_color_frame* rec) {
    const int t = threadIdx.x;
    if (t < 16) { st->pose[t] = pose.m[t]; st->pose0[t] = pose.m[t]; rec->pose[t] = pose.m[t]; }
    if (t == 16) {
        st->stop = 0; st->pad = 0;
        rec->n_depth = 0; rec->n_valid_first = 0; rec->n_valid_last = 0; rec->n_color_first = 0; rec->n_color_last = 0; rec->iterations = 0; rec->status = ICP_OK;
        rec->pad = 0; rec->cost_first = 0.0; rec->cost_last = 0.0; rec->cost_color_first = 0.0; rec->cost_color_last = 0.0;
    }
}

// k_sdf_accumulate's geometry, pose hand-over, stop test and fold, with the photometric row of a coloured lane: its eight 16-byte colour
// corners issued together, the pixel's own four bytes, and the row's terms added INTO the geometric ones the lane already holds (the
// contract's term order), so that a lane never keeps two rows' fresh terms side by side.  partials[29][n_blocks], counts[3][n_blocks].
__global__ __launch_bounds__(256) void k_sdf_accumulate_color(const TsdfVol v, const SdfFrame f, const SdfColorFrame cf, const SdfColorState* __restrict__ st,
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
            float c[8], tx, ty, tz;
            if (tsdf_cell(v, q0, q1, q2, c, tx, ty, tz)) {
                const float F = sdf_field(c, tx, ty, tz);
                if (fabsf(F) < 1.f) {                  // (a NaN drops out; a sample clamped at the free-space value carries no gradient)
                    valid = true;
                    float s[8];
                    const bool all8 = sdf_color_cell(v, cf.col, q0, q1, q2, s);
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

struct SdfColorSolve {
    const double* partials; const int* counts; int n_blocks;
    SdfColorState* st; icp_sdf_color_frame* rec; icp_sdf_color_iter* trace;      // trace: null, or n_iterations records
    int iter, n_iterations, min_valid;
    int step;                                       // 0: fold only (icp_tsdf_sdf_system_color), 1: fold, solve, compose, record
    float stop_rotation, stop_translation;
};
// k_sdf_solve for 29 sums and three counts, with the colour records.  The fold's order is k_sdf_solve's (wave w takes the sums w, w + 4, ...;
// per sum a lane adds the partials of the blocks lane, lane + 64, ... in that order; a shuffle tree joins the lanes); the solve is
// p2plane_lanes_core (an instantiation of its own: its LDS workspaces are per instantiation), its rank guard, solve_normal_svd and sdf_compose, on the entries 0 .. 26.
__global__ __launch_bounds__(256) void k_sdf_solve_color(const SdfColorSolve p) {
    __shared__ double tot[4 * SDFC_ROWS], xs[6];
    __shared__ float np2[16];
    __shared__ int cnt[3], verdict;
    SdfColorState* st = p.st;
    if (st->stop) return;                              // (uniform)
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    {
        const double* __restrict__ base = p.partials + (size_t)wave * p.n_blocks;      // sum wave + 4 j: row 4 j from here
        double x[SDFC_ROWS];
#pragma unroll
        for (int j = 0; j < SDFC_ROWS; j++) x[j] = 0.0;
        for (int b0 = lane; b0 < p.n_blocks; b0 += 4 * WAVE) {
            double v[4][SDFC_ROWS];
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const int b = b0 + u * WAVE;
#pragma unroll
                for (int j = 0; j < SDFC_ROWS; j++) v[u][j] = (b < p.n_blocks && wave + 4 * j < SDFC_NSUM) ? base[(size_t)(4 * j) * p.n_blocks + b] : 0.0;
            }
#pragma unroll
            for (int u = 0; u < 4; u++) {
                if (b0 + u * WAVE < p.n_blocks) {
#pragma unroll
                    for (int j = 0; j < SDFC_ROWS; j++) x[j] += v[u][j];
                }
            }
        }
#pragma unroll
        for (int j = 0; j < SDFC_ROWS; j++) {
            double y = x[j];
            for (int off = 32; off > 0; off >>= 1) y += __shfl_down(y, off, WAVE);
            if (lane == 0) tot[wave + 4 * j] = y;
        }
    }
    if (wave >= 1) {                                   // the three counts
        const int* __restrict__ row = p.counts + (size_t)(wave - 1) * p.n_blocks;
        int x = 0;
        for (int b0 = lane; b0 < p.n_blocks; b0 += 8 * WAVE) {
            int v[8];
#pragma unroll
            for (int u = 0; u < 8; u++) { const int b = b0 + u * WAVE; v[u] = b < p.n_blocks ? row[b] : 0; }
#pragma unroll
            for (int u = 0; u < 8; u++) x += v[u];
        }
        for (int off = 32; off > 0; off >>= 1) x += __shfl_down(x, off, WAVE);
        if (lane == 0) cnt[wave - 1] = x;
    }
    __syncthreads();
    if (tid < SDFC_NSUM) st->sums[tid] = tot[tid];
    if (tid < 3) st->counts[tid] = cnt[tid];
    if (!p.step) return;
    const int n_depth = cnt[0], n_valid = cnt[1], n_color = cnt[2];
    const bool enough = n_valid >= p.min_valid;        // (uniform)
    const float* npose = nullptr;
    if (enough) {
        npose = p2plane_lanes_core<SDF_COLOR_COPY>(tot, st->pose, xs);
        if (!npose) {
            if (tid == 0) {
                double x[6];
                solve_normal_svd<SDF_COLOR_COPY>(tot, x);
                for (int i = 0; i < 6; i++) xs[i] = x[i];
                sdf_compose(x, st->pose, np2);
            }
            __syncthreads();
            npose = np2;
        }
    }
    if (tid == 0) {
        int vd = 2;                                    // 0: go on, 1: the frame ends here with this pose, 2: the step failed
        if (enough) {
            bool fin = true;
            for (int i = 0; i < 6; i++) fin = fin && isfinite(xs[i]);
            for (int i = 0; i < 16; i++) fin = fin && isfinite(npose[i]);
            if (fin) {
                bool small = p.stop_rotation > 0.f && p.stop_translation > 0.f;
                for (int i = 0; i < 3; i++) small = small && fabs(xs[i]) <= (double)p.stop_rotation && fabs(xs[3 + i]) <= (double)p.stop_translation;
                vd = (small || p.iter == p.n_iterations - 1) ? 1 : 0;
            }
        }
        verdict = vd;
    }
    __syncthreads();
    const int vd = verdict;
    const int status = vd == 2 ? (n_depth == 0 ? ICP_ERR_NO_SOURCE : ICP_ERR_NO_CORRESPONDENCES) : ICP_OK;
    if (tid < 16) {
        const float cur = st->pose[tid], carried = vd == 2 ? st->pose0[tid] : npose[tid];      // a failed frame carries the pose it started with
        if (p.trace) p.trace[p.iter].pose[tid] = vd == 2 ? cur : carried;
        p.rec->pose[tid] = carried;
        st->pose[tid] = carried;
    }
    if (tid == 16) {
        if (p.trace) {
            icp_sdf_color_iter& t = p.trace[p.iter];
            t.n_valid = n_valid; t.n_color = n_color; t.status = status; t.pad = 0; t.cost = tot[27]; t.cost_color = tot[28];
        }
        if (p.iter == 0) { p.rec->n_depth = n_depth; p.rec->n_valid_first = n_valid; p.rec->n_color_first = n_color; p.rec->cost_first = tot[27]; p.rec->cost_color_first = tot[28]; }
        p.rec->n_valid_last = n_valid; p.rec->n_color_last = n_color; p.rec->cost_last = tot[27]; p.rec->cost_color_last = tot[28];
        p.rec->iterations = p.iter + 1; p.rec->status = status;
        if (vd) st->stop = 1;
    }
}
