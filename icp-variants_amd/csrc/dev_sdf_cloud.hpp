// dev_sdf_cloud.hpp -- direct SDF tracking of an unorganised cloud (a laser scan in its sensor frame): the resident cloud aligned to the
// TSDF volume itself, dense or hashed (icp_tsdf_cloud_system, icp_tsdf_align_cloud, icp_track_scans_sdf).  dev_sdf.hpp's step with a
// point of the cloud where that file has a depth pixel behind a pinhole camera: the point moved into the world reads its residual (the
// field) and its normal (the field's gradient) from the eight voxels around it.  Contract: include/icp_hip.h, DESIGN.md section 6zf;
// tests/sdf_cloud_restatement.py states the same arithmetic in numpy.  Part of icp_device.hpp (included from there, inside namespace
// icpdev, after dev_tsdf_hash.hpp and dev_tsdf_cloud.hpp: the cells are dev_tsdf.hpp's and dev_tsdf_hash.hpp's, the field and the gradient
// dev_sdf.hpp's, the cloud's view dev_tsdf_cloud.hpp's).
// ------------------------------------------------------------------------------------------------
// k_sdf_init and k_sdf_solve run around these kernels as they are: the pose is read from SdfState, a launch behind the end of the
// alignment returns on its first instructions, and a block leaves one column of partials[28][n_blocks] and of counts[2][n_blocks].
// Every fp32 operation is written in the contract's order (one rounding each, -ffp-contract=off); the sums are fp64, a lane adds its
// passes in order, and the block's fold is block_reduce_wide's fixed order -- no floating-point atomics, so a run keeps its bits.
constexpr int SC_POINTS_PER_LANE = 2;              // a block takes 2 x 256 consecutive points (DESIGN.md section 6zf has the measurement)

__device__ __forceinline__ bool sc_cell(const TsdfVol& v, float qx, float qy, float qz, float (&c)[8], float& tx, float& ty, float& tz) {
    return tsdf_cell(v, qx, qy, qz, c, tx, ty, tz);
}
__device__ __forceinline__ bool sc_cell(const HtVol& v, float qx, float qy, float qz, float (&c)[8], float& tx, float& ty, float& tz) {
    return htsdf_cell(v, qx, qy, qz, c, tx, ty, tz);
}

// One point per lane and pass over the SoA planes, SC_POINTS_PER_LANE passes of 256 consecutive points per block (k_vgicp_accumulate's
// shape): the planes are read coalesced, and the order of a scan keeps neighbouring lanes in neighbouring cells.  The per-lane terms are
// k_sdf_accumulate's, operation for operation, with the point's z where that kernel has the depth; a lane adds the terms of its passes
// into its 28 sums, block_reduce_wide folds them over the block, the two counts go through ballot and popcount.
template <class Vol>
__device__ __forceinline__ void sc_accumulate_body(const Vol& v, const TcCloud& cl, float huber, const SdfState* __restrict__ st, double* __restrict__ partials,
                                                   int* __restrict__ counts) {
    __shared__ double lds[4 * SDF_NSUM * 17];
    __shared__ int red[8];
    if (st->stop) return;                              // (uniform) the alignment has ended: nothing of this launch is needed
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const float* __restrict__ P = st->pose;
    double acc[SDF_NSUM];
#pragma unroll
    for (int a = 0; a < SDF_NSUM; a++) acc[a] = 0.0;
    int n_considered = 0, n_valid = 0;
#pragma unroll 1
    for (int pass = 0; pass < SC_POINTS_PER_LANE; pass++) {
        const int i = (blockIdx.x * SC_POINTS_PER_LANE + pass) * 256 + tid;
        bool considered = false, valid = false;
        if (i < cl.n) {
            const float x = cl.x[i], y = cl.y[i], z = cl.z[i];
            considered = finite3(x, y, z);
            if (considered) {
                const float q0 = (P[0] * x + (P[4] * y + P[8] * z)) + P[12];
                const float q1 = (P[1] * x + (P[5] * y + P[9] * z)) + P[13];
                const float q2 = (P[2] * x + (P[6] * y + P[10] * z)) + P[14];
                float c[8], tx, ty, tz;
                if (sc_cell(v, q0, q1, q2, c, tx, ty, tz)) {
                    const float F = sdf_field(c, tx, ty, tz);
                    if (fabsf(F) < 1.f) {              // (a NaN drops out; a sample clamped at the free-space value carries no gradient)
                        valid = true;
                        float gx, gy, gz;
                        sdf_gradient(c, tx, ty, tz, gx, gy, gz);
                        const double r = (double)F * (double)v.trunc, sc = (double)v.trunc / (double)v.s;
                        const double g0 = (double)gx * sc, g1 = (double)gy * sc, g2 = (double)gz * sc;
                        const double p0 = (double)q0, p1 = (double)q1, p2 = (double)q2;
                        const double J[6] = {p1 * g2 - p2 * g1, p2 * g0 - p0 * g2, p0 * g1 - p1 * g0, g0, g1, g2};
                        double wt = 1.0;
                        if (huber > 0.f) { const double ar = fabs(r), h = (double)huber; wt = ar <= h ? 1.0 : h / ar; }
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
        const unsigned long long bu = __ballot(considered), bv = __ballot(valid);
        n_considered += __popcll(bu); n_valid += __popcll(bv);
    }
    if (lane == 0) { red[2 * wave] = n_considered; red[2 * wave + 1] = n_valid; }
    const double tot = block_reduce_wide<SDF_NSUM, 4>(acc, lds);      // (its barrier also covers red)
    const int nb = gridDim.x, blk = blockIdx.x;
    if (tid < SDF_NSUM) partials[(size_t)tid * nb + blk] = tot;
    if (tid >= 64 && tid < 66) { const int q = tid - 64; counts[(size_t)q * nb + blk] = (red[q] + red[2 + q]) + (red[4 + q] + red[6 + q]); }
}
__global__ __launch_bounds__(256) void k_sdf_accumulate_cloud(const TsdfVol v, const TcCloud cl, float huber, const SdfState* __restrict__ st,
                                                              double* __restrict__ partials, int* __restrict__ counts) {
    sc_accumulate_body(v, cl, huber, st, partials, counts);
}
__global__ __launch_bounds__(256) void k_hsdf_accumulate_cloud(const HtVol v, const TcCloud cl, float huber, const SdfState* __restrict__ st,
                                                               double* __restrict__ partials, int* __restrict__ counts) {
    sc_accumulate_body(v, cl, huber, st, partials, counts);
}
