// dev_sdf_cloud_color.hpp -- direct SDF tracking of a COLOURED laser scan with the photometric term (icp_tsdf_cloud_system_color,
// icp_tsdf_align_cloud_color, icp_track_scans_sdf_photometric): dev_sdf_cloud.hpp's point of the resident cloud, with dev_sdf_color.hpp's
// second row -- the intensity field and its gradient read from the colour array in the cell the distance is read in, against the point's
// own colour word.  Contract: include/icp_hip.h; tests/sdf_cloud_color_restatement.py states the same arithmetic in
// numpy.  Part of icp_device.hpp (included from there, inside namespace icpdev, after dev_sdf_cloud.hpp and dev_tsdf_hash_color.hpp: the
// cloud's view and the pass shape are the former's, the both-pools cell the latter's, the dense colour corners dev_sdf_color.hpp's).
// ------------------------------------------------------------------------------------------------
// k_sdf_init_color and k_sdf_solve_color run around these kernels as they are: a block leaves one column of partials[29][n_blocks] and of
// counts[3][n_blocks].  The accumulate is restated, not folded into sc_accumulate_body (DESIGN.md section 6zi measured what sharing costs).
// A point's term k is (geometric + photometric) in the depth contract's order; that sum goes into the lane's running sum in pass order, so
// a lane holds its 29 sums and the two rows' Jacobians, never two rows' 29 fresh terms side by side.
constexpr int SCC_POINTS_PER_LANE = 2;             // a block takes 2 x 256 consecutive points (DESIGN.md section 6zj has the measurement)

__device__ __forceinline__ bool scc_cell(const TsdfVol& v, const float4* __restrict__, float qx, float qy, float qz, float (&c)[8], float (&)[8], float& tx, float& ty,
                                         float& tz, bool&) {
    return tsdf_cell(v, qx, qy, qz, c, tx, ty, tz);
}
__device__ __forceinline__ bool scc_cell(const HtVol& v, const float4* __restrict__ cpool, float qx, float qy, float qz, float (&c)[8], float (&s)[8], float& tx, float& ty,
                                         float& tz, bool& all8) {
    return htsdf_cell_both(v, cpool, qx, qy, qz, c, s, tx, ty, tz, all8);      // (the colours through the block indices the geometry found)
}
// The colour corners of a VALID point: the dense array is read now (k_sdf_accumulate_color's place for it), the hashed pool has been read.
__device__ __forceinline__ void scc_colors(const TsdfVol& v, const float4* __restrict__ col, float qx, float qy, float qz, float (&s)[8], bool& all8) {
    all8 = sdf_color_cell(v, col, qx, qy, qz, s);
}
__device__ __forceinline__ void scc_colors(const HtVol&, const float4* __restrict__, float, float, float, float (&)[8], bool&) {}

// sc_accumulate_body's passes, lanes, geometric row, counts and fold; cf.rgbx is the cloud's packed colour plane (R | G << 8 | B << 16 |
// A << 24 per point, the fourth byte not read), cf.col the volume's colour array or pool.
template <class Vol>
__device__ __forceinline__ void scc_accumulate_body(const Vol& v, const TcCloud& cl, const SdfColorFrame& cf, float huber, const SdfColorState* __restrict__ st,
                                                    double* __restrict__ partials, int* __restrict__ counts) {
    __shared__ double lds[4 * SDFC_NSUM * 17];
    __shared__ int red[12];
    if (st->stop) return;                              // (uniform) the alignment has ended: nothing of this launch is needed
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const float* __restrict__ P = st->pose;
    double acc[SDFC_NSUM];
#pragma unroll
    for (int a = 0; a < SDFC_NSUM; a++) acc[a] = 0.0;
    int n_considered = 0, n_valid = 0, n_colored = 0;
#pragma unroll 1
    for (int pass = 0; pass < SCC_POINTS_PER_LANE; pass++) {
        const int i = (blockIdx.x * SCC_POINTS_PER_LANE + pass) * 256 + tid;
        bool considered = false, valid = false, colored = false;
        if (i < cl.n) {
            const float x = cl.x[i], y = cl.y[i], z = cl.z[i];
            const uint32_t px = cf.rgbx[i];
            considered = finite3(x, y, z);
            if (considered) {
                const float q0 = (P[0] * x + (P[4] * y + P[8] * z)) + P[12];
                const float q1 = (P[1] * x + (P[5] * y + P[9] * z)) + P[13];
                const float q2 = (P[2] * x + (P[6] * y + P[10] * z)) + P[14];
                float c[8], s[8], tx, ty, tz;
                bool all8 = false;
                if (scc_cell(v, cf.col, q0, q1, q2, c, s, tx, ty, tz, all8)) {
                    const float F = sdf_field(c, tx, ty, tz);
                    if (fabsf(F) < 1.f) {              // (a NaN drops out; a sample clamped at the free-space value carries no gradient)
                        valid = true;
                        scc_colors(v, cf.col, q0, q1, q2, s, all8);
                        const double p0 = (double)q0, p1 = (double)q1, p2 = (double)q2;
                        float gx, gy, gz;
                        sdf_gradient(c, tx, ty, tz, gx, gy, gz);
                        const double r = (double)F * (double)v.trunc, sc = (double)v.trunc / (double)v.s;
                        const double g0 = (double)gx * sc, g1 = (double)gy * sc, g2 = (double)gz * sc;
                        const double J[6] = {p1 * g2 - p2 * g1, p2 * g0 - p0 * g2, p0 * g1 - p1 * g0, g0, g1, g2};
                        double wt = 1.0;
                        if (huber > 0.f) { const double ar = fabs(r), h = (double)huber; wt = ar <= h ? 1.0 : h / ar; }
                        const float S = sdf_field(s, tx, ty, tz);
                        colored = all8 && isfinite(S);
                        if (colored) {
                            float hx, hy, hz;
                            sdf_gradient(s, tx, ty, tz, hx, hy, hz);
                            const double Ip = (double)(int)((px & 0xFFu) + ((px >> 8) & 0xFFu) + ((px >> 16) & 0xFFu)) / 765.0;
                            const double rc = (double)S / 765.0 - Ip, den = 765.0 * (double)v.s;
                            const double h0 = (double)hx / den, h1 = (double)hy / den, h2 = (double)hz / den;
                            const double Jc[6] = {p1 * h2 - p2 * h1, p2 * h0 - p0 * h2, p0 * h1 - p1 * h0, h0, h1, h2};
                            double wc = (double)cf.weight * (double)cf.weight;
                            if (cf.huber > 0.f) { const double ar = fabs(rc), h = (double)cf.huber; wc = wc * (ar <= h ? 1.0 : h / ar); }
                            int k = 0;
#pragma unroll
                            for (int a = 0; a < 6; a++) {
                                const double wj = wt * J[a], wjc = wc * Jc[a];
#pragma unroll
                                for (int b = a; b < 6; b++) acc[k++] += wj * J[b] + wjc * Jc[b];
                                acc[21 + a] += -(wj * r) + -(wjc * rc);
                            }
                            const double e = (wc * rc) * rc;
                            acc[27] += (wt * r) * r + e;
                            acc[28] += e;
                        } else {
                            int k = 0;
#pragma unroll
                            for (int a = 0; a < 6; a++) {
                                const double wj = wt * J[a];
#pragma unroll
                                for (int b = a; b < 6; b++) acc[k++] += wj * J[b];
                                acc[21 + a] += -(wj * r);
                            }
                            acc[27] += (wt * r) * r;
                        }
                    }
                }
            }
        }
        const unsigned long long bu = __ballot(considered), bv = __ballot(valid), bc = __ballot(colored);
        n_considered += __popcll(bu); n_valid += __popcll(bv); n_colored += __popcll(bc);
    }
    if (lane == 0) { red[3 * wave] = n_considered; red[3 * wave + 1] = n_valid; red[3 * wave + 2] = n_colored; }
    const double tot = block_reduce_wide<SDFC_NSUM, 4>(acc, lds);      // (its barrier also covers red)
    const int nb = gridDim.x, blk = blockIdx.x;
    if (tid < SDFC_NSUM) partials[(size_t)tid * nb + blk] = tot;
    if (tid >= 64 && tid < 67) { const int q = tid - 64; counts[(size_t)q * nb + blk] = (red[q] + red[3 + q]) + (red[6 + q] + red[9 + q]); }
}
__global__ __launch_bounds__(256) void k_sdf_accumulate_cloud_color(const TsdfVol v, const TcCloud cl, const SdfColorFrame cf, float huber,
                                                                    const SdfColorState* __restrict__ st, double* __restrict__ partials, int* __restrict__ counts) {
    scc_accumulate_body(v, cl, cf, huber, st, partials, counts);
}
__global__ __launch_bounds__(256) void k_hsdf_accumulate_cloud_color(const HtVol v, const TcCloud cl, const SdfColorFrame cf, float huber,
                                                                     const SdfColorState* __restrict__ st, double* __restrict__ partials, int* __restrict__ counts) {
    scc_accumulate_body(v, cl, cf, huber, st, partials, counts);
}
