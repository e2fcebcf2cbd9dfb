// dev_sdf.hpp -- direct SDF tracking: a depth frame aligned to the TSDF volume itself (Bylow, Sturm, Kerl, Kahl, Cremers, RSS 2013; Canelhas
// et al., IROS 2013).  A depth pixel moved into the world reads its residual (the field) and its normal (the field's gradient) from the eight
// voxels around it: no ray-cast, no target cloud, no index, no search.  Contract: include/icp_hip.h; the cell, the field
// and the gradient are dev_tsdf.hpp's, so this file comes after it.  Part of icp_device.hpp (included from there, inside namespace icpdev).
// ------------------------------------------------------------------------------------------------
// A frame's iterations are enqueued without a host round trip: the pose lives in SdfState, k_sdf_accumulate reads it there, k_sdf_solve
// writes the next one there, and once SdfState::stop is set every launch still queued returns on its first instructions (section 6j's drain).
// Every fp32 operation is written in the contract's order (one rounding each, -ffp-contract=off); tests/sdf_restatement.py states the same
// arithmetic in numpy.  The sums are fp64 and folded in a fixed order at every level -- no floating-point atomics -- so a run keeps its bits.
constexpr int SDF_NSUM = 28;                       // 21 (upper triangle of sum w J J^T) + 6 (-sum w J r) + 1 (sum w r r)
static_assert(SDF_NSUM % 4 == 0, "k_sdf_solve folds SDF_NSUM / 4 sums per wave");
struct SdfState {
    float pose[16], pose0[16];                     // the pose the next iteration samples at; the pose the frame started with (column-major)
    int stop, pad;
    double sums[SDF_NSUM];                         // the folded sums and counts of the last k_sdf_solve that ran
    int counts[2];                                 // n_depth, n_valid
};
struct SdfFrame {
    const float* depth;
    int width, height, stride, ws, hs;             // ws x hs: the grid of sampled pixels, (u, v) = stride (su, sv)
    float fx, fy, cx, cy, huber;
};

// Nested lerps of the cell's eight corners: the field, and the analytic gradient per voxel (k_tsdf_raycast's hit code).
__device__ __forceinline__ float sdf_field(const float (&c)[8], float tx, float ty, float tz) {
    const float e0 = tsdf_lerp(tsdf_lerp(c[0], c[1], tx), tsdf_lerp(c[2], c[3], tx), ty);
    const float e1 = tsdf_lerp(tsdf_lerp(c[4], c[5], tx), tsdf_lerp(c[6], c[7], tx), ty);
    return tsdf_lerp(e0, e1, tz);
}
__device__ __forceinline__ void sdf_gradient(const float (&c)[8], float tx, float ty, float tz, float& gx, float& gy, float& gz) {
    gx = tsdf_lerp(tsdf_lerp(c[1] - c[0], c[3] - c[2], ty), tsdf_lerp(c[5] - c[4], c[7] - c[6], ty), tz);
    gy = tsdf_lerp(tsdf_lerp(c[2] - c[0], c[3] - c[1], tx), tsdf_lerp(c[6] - c[4], c[7] - c[5], tx), tz);
    gz = tsdf_lerp(tsdf_lerp(c[4] - c[0], c[5] - c[1], tx), tsdf_lerp(c[6] - c[2], c[7] - c[3], tx), ty);
}

// icp_tsdf_sample: the field and its gradient at n world points, one point per thread.  A NaN is stored as the canonical quiet NaN (which
// operand's payload an addition of two NaNs keeps is the hardware's choice); an invalid cell reads 0.
__device__ __forceinline__ float sdf_canonical(float x) { return x != x ? __uint_as_float(0x7FC00000u) : x; }
__global__ __launch_bounds__(256) void k_tsdf_sample(const TsdfVol v, const float* __restrict__ pts, int n, float* __restrict__ f_out, float* __restrict__ g_out,
                                                     uint8_t* __restrict__ valid_out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float c[8], tx, ty, tz, F = 0.f, gx = 0.f, gy = 0.f, gz = 0.f;
    const bool ok = tsdf_cell(v, pts[(size_t)i * 3], pts[(size_t)i * 3 + 1], pts[(size_t)i * 3 + 2], c, tx, ty, tz);
    if (ok) { F = sdf_field(c, tx, ty, tz); sdf_gradient(c, tx, ty, tz, gx, gy, gz); }
    f_out[i] = sdf_canonical(F);
    g_out[(size_t)i * 3] = sdf_canonical(gx); g_out[(size_t)i * 3 + 1] = sdf_canonical(gy); g_out[(size_t)i * 3 + 2] = sdf_canonical(gz);
    valid_out[i] = ok ? 1 : 0;
}

// One launch in front of a frame: the incoming pose into the state, the stop word cleared, the frame record zeroed around that pose.
__global__ void k_sdf_init(SdfState* st, const TsdfMat pose, icp_sdf_frame* rec) {
    const int t = threadIdx.x;
    if (t < 16) { st->pose[t] = pose.m[t]; st->pose0[t] = pose.m[t]; rec->pose[t] = pose.m[t]; }
    if (t == 16) {
        st->stop = 0; st->pad = 0;
        rec->n_depth = 0; rec->n_valid_first = 0; rec->n_valid_last = 0; rec->iterations = 0; rec->status = ICP_OK; rec->cost_first = 0.0; rec->cost_last = 0.0;
    }
}

// One sampled pixel per lane, an 8 x 8 tile of sampled pixels per wave (16 x 16 per block, k_tsdf_raycast's shape): the 64 gathers of a wave
// fall in neighbouring cells, and tsdf_cell issues a lane's eight 8-byte corner loads together.  The 28 terms of a lane are folded over the
// block by block_reduce_wide (two cross-lane steps, then the four waves' partials through LDS in a fixed order); the two counts go through
// ballot and popcount.  One column of partials[28][n_blocks] and of counts[2][n_blocks] per block.
__global__ __launch_bounds__(256) void k_sdf_accumulate(const TsdfVol v, const SdfFrame f, const SdfState* __restrict__ st, double* __restrict__ partials,
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
            if (tsdf_cell(v, q0, q1, q2, c, tx, ty, tz)) {
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

// dT * pose for the six-vector x, as solve_generic composes it (the path the rank guard of p2plane_lanes_core sends here): one thread.
__device__ __forceinline__ void sdf_compose(const double* x, const float* pose_in, float* out) {
    const float al = (float)x[0], be = (float)x[1], ga = (float)x[2];
    const float ca = (float)cos((double)al), sa = (float)sin((double)al);
    const float cb = (float)cos((double)be), sb = (float)sin((double)be);
    const float cg = (float)cos((double)ga), sg = (float)sin((double)ga);
    const float Rx[9] = {1, 0, 0, 0, ca, -sa, 0, sa, ca}, Ry[9] = {cb, 0, sb, 0, 1, 0, -sb, 0, cb}, Rz[9] = {cg, -sg, 0, sg, cg, 0, 0, 0, 1};
    float Rxy[9], R[9], dT[16], P[16];
    mat3_mul_f32(Rx, Ry, Rxy); mat3_mul_f32(Rxy, Rz, R);
    const float t[3] = {(float)x[3], (float)x[4], (float)x[5]};
    set_pose_f32(dT, R, t);
    for (int i = 0; i < 16; i++) P[i] = pose_in[i];
    mat4_mul_f32(dT, P, out);
}

struct SdfSolve {
    const double* partials; const int* counts; int n_blocks;
    SdfState* st; icp_sdf_frame* rec; icp_sdf_iter* trace;      // trace: null, or n_iterations records
    int iter, n_iterations, min_valid;
    int step;                                       // 0: fold only (icp_tsdf_sdf_system), 1: fold, solve, compose, record
    float stop_rotation, stop_translation;
};
// One block.  Fold: wave w takes the sums w, w + 4, ...; per sum a lane adds the partials of the blocks lane, lane + 64, ... in that order, a
// shuffle tree joins the lanes -- the same order on every run.  Then the point-to-plane solve of the 27 sums on the block's lanes (p2plane_lanes_core;
// where its rank guard refuses, solve_normal_svd on one thread), pose <- dT pose, the iteration's record, the frame's record, the stop word.
__global__ __launch_bounds__(256) void k_sdf_solve(const SdfSolve p) {
    __shared__ double tot[SDF_NSUM], xs[6];
    __shared__ float np2[16];
    __shared__ int cnt[2], verdict;
    SdfState* st = p.st;
    if (st->stop) return;                              // (uniform)
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    {
        // the seven sums of this wave side by side, four blocks per lane and sum in flight: 28 independent loads per round trip instead of
        // one (a fold that waits for every load takes longer than the rest of the iteration at 1200 blocks); the order of the additions is
        // the one stated above
        const double* __restrict__ base = p.partials + (size_t)wave * p.n_blocks;      // sum wave + 4 j: row 4 j from here
        double x[SDF_NSUM / 4];
#pragma unroll
        for (int j = 0; j < SDF_NSUM / 4; j++) x[j] = 0.0;
        for (int b0 = lane; b0 < p.n_blocks; b0 += 4 * WAVE) {
            double v[4][SDF_NSUM / 4];
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const int b = b0 + u * WAVE;
#pragma unroll
                for (int j = 0; j < SDF_NSUM / 4; j++) v[u][j] = b < p.n_blocks ? base[(size_t)(4 * j) * p.n_blocks + b] : 0.0;
            }
#pragma unroll
            for (int u = 0; u < 4; u++) {
                if (b0 + u * WAVE < p.n_blocks) {
#pragma unroll
                    for (int j = 0; j < SDF_NSUM / 4; j++) x[j] += v[u][j];
                }
            }
        }
#pragma unroll
        for (int j = 0; j < SDF_NSUM / 4; j++) {
            double y = x[j];
            for (int off = 32; off > 0; off >>= 1) y += __shfl_down(y, off, WAVE);
            if (lane == 0) tot[wave + 4 * j] = y;
        }
    }
    if (wave >= 2) {                                   // the two counts, on the waves the pose solve does not start on
        const int* __restrict__ row = p.counts + (size_t)(wave - 2) * p.n_blocks;
        int x = 0;
        for (int b0 = lane; b0 < p.n_blocks; b0 += 8 * WAVE) {
            int v[8];
#pragma unroll
            for (int u = 0; u < 8; u++) { const int b = b0 + u * WAVE; v[u] = b < p.n_blocks ? row[b] : 0; }
#pragma unroll
            for (int u = 0; u < 8; u++) x += v[u];
        }
        for (int off = 32; off > 0; off >>= 1) x += __shfl_down(x, off, WAVE);
        if (lane == 0) cnt[wave - 2] = x;
    }
    __syncthreads();
    if (tid < SDF_NSUM) st->sums[tid] = tot[tid];
    if (tid < 2) st->counts[tid] = cnt[tid];
    if (!p.step) return;
    const int n_depth = cnt[0], n_valid = cnt[1];
    const bool enough = n_valid >= p.min_valid;        // (uniform)
    const float* npose = nullptr;
    if (enough) {
        npose = p2plane_lanes_core<SDF_COPY>(tot, st->pose, xs);
        if (!npose) {
            if (tid == 0) {
                double x[6];
                solve_normal_svd<SDF_COPY>(tot, x);
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
        if (p.trace) { p.trace[p.iter].n_valid = n_valid; p.trace[p.iter].status = status; p.trace[p.iter].cost = tot[27]; }
        if (p.iter == 0) { p.rec->n_depth = n_depth; p.rec->n_valid_first = n_valid; p.rec->cost_first = tot[27]; }
        p.rec->n_valid_last = n_valid; p.rec->cost_last = tot[27]; p.rec->iterations = p.iter + 1; p.rec->status = status;
        if (vd) st->stop = 1;
    }
}
