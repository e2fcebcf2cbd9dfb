// dev_fpfh.hpp -- global registration (icp_register_global): FPFH descriptors, the 33-dimensional matcher, the RANSAC fit and score.
// Part of icp_device.hpp (included from there, inside namespace icpdev); see that file for the build contract.
// ------------------------------------------------------------------------------------------------
// Fast Point Feature Histograms (Rusu, Blodow, Beetz, ICRA 2009) in two passes over a cloud with normals, then an exact 1-NN in
// feature space and RANSAC over three-point hypotheses.  The contract of every step is in include/icp_hip.h (icp_global_options);
// tests/global_restatement.py restates it in numpy.  Every kernel here calls only __forceinline__ helpers or instantiations of its own
// (jacobi_eig_sym<3, GLOBAL_COPY>): an existing kernel keeps exactly the code it had.
constexpr int FPFH_BINS = 11, FPFH_DIM = 3 * FPFH_BINS;
constexpr int GLOBAL_COPY = 3;      // jacobi_eig_sym instantiation of the RANSAC fit (0, 1, 2: see dev_gicp.hpp)

// bin of x over [lo, hi]: floor(11 (x - lo) / (hi - lo)) clamped to 0..10, fp64
__device__ __forceinline__ int fpfh_bin(double x, double lo, double hi) {
    const double t = floor(11.0 * (x - lo) / (hi - lo));
    return t < 0.0 ? 0 : (t > 10.0 ? 10 : (int)t);
}

// The pair features of (p, n_p) and a neighbour (q, n_q), fp64 from the fp32 inputs; false: the pair contributes nothing.
__device__ __forceinline__ bool fpfh_pair(float pxf, float pyf, float pzf, float npx, float npy, float npz, float qxf, float qyf, float qzf, float nqx, float nqy, float nqz,
                                          int& b1, int& b2, int& b3) {
    if (!(finite3(pxf, pyf, pzf) && finite3(npx, npy, npz) && finite3(qxf, qyf, qzf) && finite3(nqx, nqy, nqz))) return false;
    double dx = (double)qxf - (double)pxf, dy = (double)qyf - (double)pyf, dz = (double)qzf - (double)pzf;
    const double f4 = sqrt((dx * dx + dy * dy) + dz * dz);
    double n1x = npx, n1y = npy, n1z = npz, n2x = nqx, n2y = nqy, n2z = nqz;
    const double a1 = ((n1x * dx + n1y * dy) + n1z * dz) / f4, a2 = ((n2x * dx + n2y * dy) + n2z * dz) / f4;
    double f3;
    if (fabs(a1) < fabs(a2)) {        // the pair is taken from q's side
        double t;
        t = n1x; n1x = n2x; n2x = t; t = n1y; n1y = n2y; n2y = t; t = n1z; n1z = n2z; n2z = t;
        dx = -dx; dy = -dy; dz = -dz;
        f3 = -a2;
    } else f3 = a1;
    double vx = dy * n1z - dz * n1y, vy = dz * n1x - dx * n1z, vz = dx * n1y - dy * n1x;      // v = dp x n1
    const double vn = sqrt((vx * vx + vy * vy) + vz * vz);
    if (!(vn > 0.0)) return false;
    vx /= vn; vy /= vn; vz /= vn;
    const double wx = n1y * vz - n1z * vy, wy = n1z * vx - n1x * vz, wz = n1x * vy - n1y * vx;  // w = n1 x v
    const double f1 = (vx * n2x + vy * n2y) + vz * n2z;
    const double f2 = atan2((wx * n2x + wy * n2y) + wz * n2z, (n1x * n2x + n1y * n2y) + n1z * n2z);
    const double pi = 3.141592653589793238462643383279502884;
    b1 = fpfh_bin(f1, -1.0, 1.0); b2 = fpfh_bin(f2, -pi, pi); b3 = fpfh_bin(f3, -1.0, 1.0);
    return true;
}

// Pass 1, one thread per point of the cloud the tree is built over: the K smallest (fp32 d^2, index) pairs over its finite points, the
// point itself included (k_normals_knn's walk and neighbour list, as k_gicp_normals copies them), stored in that order as (index, d^2)
// -- unfilled slots (-1, +inf) -- and the SPFH of the point: 33 integer counts and the number of contributing pairs.  The histogram is
// carried in three 64-bit words, 5 bits per bin (a bin holds at most K - 1 <= 19): no array indexed at run time, no scratch.
template <int K>
__global__ __launch_bounds__(BVH_THREADS) void k_fpfh_spfh(const BvhViewT<3> bv, int n, int tree_depth, const float* __restrict__ nrx, const float* __restrict__ nry,
                                                           const float* __restrict__ nrz, int* __restrict__ nb_idx /* n x K */, float* __restrict__ nb_d2 /* n x K */,
                                                           uint8_t* __restrict__ counts /* n x 33 */, int* __restrict__ pairs /* n */) {
    extern __shared__ unsigned short bvh_lb16[];
    const int tid = threadIdx.x;
    const int i = blockIdx.x * BVH_THREADS + tid;
    if (i >= n) return;
    const float px = bv.tgt.c[0][i], py = bv.tgt.c[1][i], pz = bv.tgt.c[2][i];
    float bd[K]; int bj[K];
#pragma unroll
    for (int q = 0; q < K; q++) { bd[q] = FLT_MAX; bj[q] = 0x7fffffff; }
    if (finite3(px, py, pz) && bv.n_valid >= 1) {
        f2 p2[3] = {{px, px}, {py, py}, {pz, pz}};
        TravState st; st.depth = 0; st.idx = 0; st.pending = 0u; st.alive = true;
        float unused_minlb = FLT_MAX;
        while (st.alive) {
            while (st.alive && st.depth < tree_depth) {
                const f2 l = pair_lb<3>(bv.nodes + ((1 << st.depth) - 1 + st.idx), p2);
                const bool swap = l.y < l.x;
                const float ln = swap ? l.y : l.x, lf = swap ? l.x : l.y;
                const float worst = bd[K - 1];
                const bool take_near = !(ln * 0.99999f > worst), take_far = !(lf * 0.99999f > worst);
                if (take_near) {
                    if (take_far) { bvh_lb16[st.depth * BVH_THREADS + tid] = (unsigned short)(__float_as_uint(lf) >> 16); st.pending |= 1u << st.depth; }
                    st.idx = 2 * st.idx + (swap ? 1 : 0); st.depth++;
                } else st.alive = false;
                trav_pop(st, bvh_lb16, tid, BVH_THREADS, bd[K - 1], unused_minlb);
            }
            if (st.alive) {
                const BvhLeafT<3>* __restrict__ lf = bv.leaves + st.idx;
#pragma unroll
                for (int t = 0; t < BVH_LEAF; t++) {
                    const float dx = px - lf->c[0][t], dy = py - lf->c[1][t], dz = pz - lf->c[2][t];
                    const float d = (dx * dx + dy * dy) + dz * dz;
                    const int j = lf->idx[t];
                    if (j >= 0 && ((d < bd[K - 1]) | ((d == bd[K - 1]) & (j < bj[K - 1])))) knn_insert<K>(bd, bj, d, j);
                }
                st.alive = false;
                trav_pop(st, bvh_lb16, tid, BVH_THREADS, bd[K - 1], unused_minlb);
            }
        }
    }
    const float npx = nrx[i], npy = nry[i], npz = nrz[i];
    unsigned long long h1 = 0ull, h2 = 0ull, h3 = 0ull;
    int np = 0;
#pragma unroll
    for (int q = 0; q < K; q++) {
        const bool have = bd[q] < FLT_MAX;
        nb_idx[(size_t)i * K + q] = have ? bj[q] : -1;
        nb_d2[(size_t)i * K + q] = have ? bd[q] : INFINITY;
    }
    // the pairs, read back from the list this thread has just written (a rolled loop: one copy of the pair code, nothing indexed at run time)
#pragma unroll 1
    for (int q = 0; q < K; q++) {
        const int j = nb_idx[(size_t)i * K + q];
        if (j >= 0 && nb_d2[(size_t)i * K + q] > 0.f) {
            int b1, b2, b3;
            if (fpfh_pair(px, py, pz, npx, npy, npz, bv.tgt.c[0][j], bv.tgt.c[1][j], bv.tgt.c[2][j], nrx[j], nry[j], nrz[j], b1, b2, b3)) {
                h1 += 1ull << (5 * b1); h2 += 1ull << (5 * b2); h3 += 1ull << (5 * b3);
                np++;
            }
        }
    }
    uint8_t* out = counts + (size_t)i * FPFH_DIM;
#pragma unroll
    for (int b = 0; b < FPFH_BINS; b++) {
        out[b] = (uint8_t)((h1 >> (5 * b)) & 31ull);
        out[FPFH_BINS + b] = (uint8_t)((h2 >> (5 * b)) & 31ull);
        out[2 * FPFH_BINS + b] = (uint8_t)((h3 >> (5 * b)) & 31ull);
    }
    pairs[i] = np;
}

// Pass 2, one thread per keypoint r (point r * stride): F = h(p) + sum_i w_i h(q_i), h = SPFH / max(pairs, 1), over the stored
// neighbours with d_i > 0 in their stored order, w_i = (1 / d_i) / sum_j (1 / d_j), d = sqrt of the stored fp32 d^2 in fp64; fp64 sums,
// one rounding to fp32.  33 NaNs for a point with a non-finite position or normal or with no contributing pair.  feat: nk x 33 row-major.
struct FpfhParams {
    const float* x; const float* y; const float* z; const float* nx; const float* ny; const float* nz;
    int stride, nk, K;
    const int* nb_idx; const float* nb_d2; const uint8_t* counts; const int* pairs;
    float* feat;
};
__global__ __launch_bounds__(256) void k_fpfh(const FpfhParams fp) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= fp.nk) return;
    const size_t i = (size_t)r * fp.stride;
    const int np = fp.pairs[i];
    const bool ok = finite3(fp.x[i], fp.y[i], fp.z[i]) && finite3(fp.nx[i], fp.ny[i], fp.nz[i]) && np > 0;
    float* out = fp.feat + (size_t)r * FPFH_DIM;
    if (!ok) {
#pragma unroll
        for (int b = 0; b < FPFH_DIM; b++) out[b] = NAN;
        return;
    }
    double acc[FPFH_DIM];
    {
        const uint8_t* cp = fp.counts + i * FPFH_DIM;
        const double den = (double)np;
#pragma unroll
        for (int b = 0; b < FPFH_DIM; b++) acc[b] = (double)cp[b] / den;
    }
    const int* ni = fp.nb_idx + i * fp.K; const float* nd = fp.nb_d2 + i * fp.K;
    double S = 0.0;
    for (int q = 0; q < fp.K; q++) { const float d2 = nd[q]; if (ni[q] >= 0 && d2 > 0.f) S += 1.0 / sqrt((double)d2); }
    for (int q = 0; q < fp.K; q++) {
        const int j = ni[q]; const float d2 = nd[q];
        if (!(j >= 0 && d2 > 0.f)) continue;
        const double w = (1.0 / sqrt((double)d2)) / S;
        const int nj = fp.pairs[j];
        const double den = (double)(nj > 1 ? nj : 1);
        const uint8_t* cq = fp.counts + (size_t)j * FPFH_DIM;
#pragma unroll
        for (int b = 0; b < FPFH_DIM; b++) acc[b] += w * ((double)cq[b] / den);
    }
#pragma unroll
    for (int b = 0; b < FPFH_DIM; b++) out[b] = (float)acc[b];
}

// ---- the matcher: exact 1-NN in 33 dimensions, the contract of the 3-D brute-force matcher (dev_knn_brute.hpp) ----
// One lane = one query row, held in registers; the target rows go through LDS in tiles of FM_TILE rows (padded to 36 floats: nine
// 16-byte reads per row, every lane of a wave the same address -- a broadcast).  d = sum over the bins in order of (a_b - c_b)^2, fp32,
// no contraction; strict < over ascending target rows keeps the lowest index of a tie; a NaN row (either side) gives a NaN distance,
// which never wins.  blockIdx.y splits the target tiles; the parts merge through a packed (d bits, index) 64-bit atomicMin, the
// lexicographic first minimum (d >= 0: its bit pattern orders as its value).  best64: preset to ~0 (no match).
constexpr int FM_TILE = 256, FM_THREADS = 256, FM_ROW4 = 9;
__global__ __launch_bounds__(FM_THREADS) void k_feature_match(const float* __restrict__ qf, int nq, const float* __restrict__ tf, int nt, int nseg,
                                                              unsigned long long* __restrict__ best64) {
    __shared__ float4 tile[FM_TILE * FM_ROW4];
    const int tid = threadIdx.x;
    const int k = blockIdx.x * FM_THREADS + tid;
    const int kk = k < nq ? k : nq - 1;
    float a[FPFH_DIM];
#pragma unroll
    for (int b = 0; b < FPFH_DIM; b++) a[b] = qf[(size_t)kk * FPFH_DIM + b];
    const int ntiles = (nt + FM_TILE - 1) / FM_TILE;
    const int t0 = (int)(((long long)ntiles * blockIdx.y) / nseg), t1 = (int)(((long long)ntiles * (blockIdx.y + 1)) / nseg);
    float best = INFINITY; int bi = -1;
    for (int t = t0; t < t1; t++) {
        const int row0 = t * FM_TILE;
        const int rows = nt - row0 < FM_TILE ? nt - row0 : FM_TILE;
        __syncthreads();
        float* tl = (float*)tile;
        const float* src = tf + (size_t)row0 * FPFH_DIM;
        for (int e = tid; e < rows * FPFH_DIM; e += FM_THREADS) { const int r = e / FPFH_DIM, col = e - r * FPFH_DIM; tl[r * (4 * FM_ROW4) + col] = src[e]; }
        __syncthreads();
        for (int r = 0; r < rows; r++) {
            float c[4 * FM_ROW4];
#pragma unroll
            for (int v = 0; v < FM_ROW4; v++) { const float4 x = tile[r * FM_ROW4 + v]; c[4 * v] = x.x; c[4 * v + 1] = x.y; c[4 * v + 2] = x.z; c[4 * v + 3] = x.w; }
            float d = 0.f;
#pragma unroll
            for (int b = 0; b < FPFH_DIM; b++) { const float e = a[b] - c[b]; d = d + e * e; }
            if (d < best) { best = d; bi = row0 + r; }
        }
    }
    if (k < nq && bi >= 0) atomicMin(best64 + k, ((unsigned long long)__float_as_uint(best) << 32) | (unsigned int)bi);
}
// fwd[k] = the match of query k (-1: none); keep[k] = it has one, and (back given: mutual) the match's own match is k.
__global__ void k_feature_match_finalize(const unsigned long long* __restrict__ best_fwd, const unsigned long long* __restrict__ best_back, int nq,
                                         int* __restrict__ fwd, uint8_t* __restrict__ keep) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= nq) return;
    const int j = (int)(unsigned int)(best_fwd[k] & 0xFFFFFFFFull);
    bool ok = j >= 0;
    if (ok && best_back) ok = (int)(unsigned int)(best_back[j] & 0xFFFFFFFFull) == k;
    fwd[k] = j; keep[k] = ok ? 1 : 0;
}
// The compacted correspondences: pair m = (kept keypoint list[m], its match), as original point indices and as the two points.
struct CorrPlanes { float* s[3]; float* t[3]; };
__global__ void k_corr_gather(const int* __restrict__ list, const int* __restrict__ fwd, int m_count, int stride, SoA3 src, SoA3 tgt,
                              int* __restrict__ src_idx, int* __restrict__ tgt_idx, CorrPlanes cp) {
    const int m = blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= m_count) return;
    const int r = list[m];
    const int i = r * stride, j = fwd[r] * stride;
    src_idx[m] = i; tgt_idx[m] = j;
    cp.s[0][m] = src.x[i]; cp.s[1][m] = src.y[i]; cp.s[2][m] = src.z[i];
    cp.t[0][m] = tgt.x[j]; cp.t[1][m] = tgt.y[j]; cp.t[2][m] = tgt.z[j];
}

// ---- RANSAC ----
// Fit, one thread per hypothesis h: the draws c_j = select_hash(seed, h, j) mod M; REPEATED when two are equal; EDGES when for one of the
// edges (0,1), (1,2), (2,0) min(l_src, l_tgt) < edge_similarity max(l_src, l_tgt), fp64 lengths; DEGENERATE when on either side
// |e1 x e2|^2 <= 1e-6 |e1|^2 |e2|^2 with e1 = p1 - p0, e2 = p2 - p0 (the three points within 1e-3 rad of a line); else the three-point
// Kabsch in fp64 -- unweighted centroids, A = sum (t_j - tm)(s_j - sm)^T, V from the eigenvectors of A^T A (descending), U_c = A v_c / |A v_c|
// for the two leading columns, the third by the cross product: R = U diag(1, 1, det(U V^T)) V^T as procrustes_rotation writes it (A has
// rank 2 here: three centred points span a plane) -- t = tm - R sm, the pose rounded once to fp32.
__device__ __forceinline__ void ransac_kabsch(const double (&s)[3][3], const double (&t)[3][3], float* pose /* column-major 4 x 4 */) {
    double sm[3], tm[3];
#pragma unroll
    for (int a = 0; a < 3; a++) { sm[a] = ((s[0][a] + s[1][a]) + s[2][a]) / 3.0; tm[a] = ((t[0][a] + t[1][a]) + t[2][a]) / 3.0; }
    double A[9], B[9], V[9], ev[3];
#pragma unroll
    for (int r = 0; r < 3; r++) {
#pragma unroll
        for (int c = 0; c < 3; c++) A[r * 3 + c] = ((t[0][r] - tm[r]) * (s[0][c] - sm[c]) + (t[1][r] - tm[r]) * (s[1][c] - sm[c])) + (t[2][r] - tm[r]) * (s[2][c] - sm[c]);
    }
#pragma unroll
    for (int i = 0; i < 3; i++) {
#pragma unroll
        for (int j = 0; j < 3; j++) B[i * 3 + j] = (A[i] * A[j] + A[3 + i] * A[3 + j]) + A[6 + i] * A[6 + j];
    }
    jacobi_eig_sym<3, GLOBAL_COPY>(B, V, ev);
    // columns of V by descending eigenvalue, without an index array: three compare-and-swaps on (ev, column)
    double v0[3] = {V[0], V[3], V[6]}, v1[3] = {V[1], V[4], V[7]}, v2[3] = {V[2], V[5], V[8]};
    double e0 = ev[0], e1 = ev[1], e2 = ev[2];
#define GLOBAL_CSWAP(ea, va, eb, vb) if (eb > ea) { double t_ = ea; ea = eb; eb = t_; for (int q_ = 0; q_ < 3; q_++) { t_ = va[q_]; va[q_] = vb[q_]; vb[q_] = t_; } }
    GLOBAL_CSWAP(e0, v0, e1, v1) GLOBAL_CSWAP(e0, v0, e2, v2) GLOBAL_CSWAP(e1, v1, e2, v2)
#undef GLOBAL_CSWAP
    double u0[3], u1[3], u2[3];
#pragma unroll
    for (int r = 0; r < 3; r++) u0[r] = (A[r * 3] * v0[0] + A[r * 3 + 1] * v0[1]) + A[r * 3 + 2] * v0[2];
    const double n0 = sqrt((u0[0] * u0[0] + u0[1] * u0[1]) + u0[2] * u0[2]);
#pragma unroll
    for (int r = 0; r < 3; r++) u0[r] /= n0;
#pragma unroll
    for (int r = 0; r < 3; r++) u1[r] = (A[r * 3] * v1[0] + A[r * 3 + 1] * v1[1]) + A[r * 3 + 2] * v1[2];
    const double dp = (u1[0] * u0[0] + u1[1] * u0[1]) + u1[2] * u0[2];
#pragma unroll
    for (int r = 0; r < 3; r++) u1[r] -= dp * u0[r];
    const double n1 = sqrt((u1[0] * u1[0] + u1[1] * u1[1]) + u1[2] * u1[2]);
#pragma unroll
    for (int r = 0; r < 3; r++) u1[r] /= n1;
    u2[0] = u0[1] * u1[2] - u0[2] * u1[1]; u2[1] = u0[2] * u1[0] - u0[0] * u1[2]; u2[2] = u0[0] * u1[1] - u0[1] * u1[0];
    const double detV = (v0[0] * (v1[1] * v2[2] - v1[2] * v2[1]) - v1[0] * (v0[1] * v2[2] - v0[2] * v2[1])) + v2[0] * (v0[1] * v1[2] - v0[2] * v1[1]);
    double R[9];
#pragma unroll
    for (int r = 0; r < 3; r++) {
#pragma unroll
        for (int c = 0; c < 3; c++) R[r * 3 + c] = (u0[r] * v0[c] + u1[r] * v1[c]) + detV * u2[r] * v2[c];
    }
#pragma unroll
    for (int i = 0; i < 16; i++) pose[i] = (i % 5 == 0) ? 1.f : 0.f;
#pragma unroll
    for (int r = 0; r < 3; r++) {
#pragma unroll
        for (int c = 0; c < 3; c++) pose[c * 4 + r] = (float)R[r * 3 + c];
        pose[12 + r] = (float)(tm[r] - ((R[r * 3] * sm[0] + R[r * 3 + 1] * sm[1]) + R[r * 3 + 2] * sm[2]));
    }
}
struct RansacParams {
    const float* s[3]; const float* t[3];      // the correspondences' points, M each
    int M, H;
    uint32_t seed;
    double edge_similarity;
    float inlier_d2;
    icp_global_hypothesis* hyp;                // H records
};
__device__ __forceinline__ bool ransac_collinear(const double (&p)[3][3]) {
    const double ax = p[1][0] - p[0][0], ay = p[1][1] - p[0][1], az = p[1][2] - p[0][2];
    const double bx = p[2][0] - p[0][0], by = p[2][1] - p[0][1], bz = p[2][2] - p[0][2];
    const double cx = ay * bz - az * by, cy = az * bx - ax * bz, cz = ax * by - ay * bx;
    const double cc = (cx * cx + cy * cy) + cz * cz, aa = (ax * ax + ay * ay) + az * az, bb = (bx * bx + by * by) + bz * bz;
    return !(cc > 1e-6 * (aa * bb));
}
__global__ __launch_bounds__(64) void k_ransac_fit(const RansacParams rp) {
    const int h = blockIdx.x * 64 + threadIdx.x;
    if (h >= rp.H) return;
    icp_global_hypothesis* out = rp.hyp + h;
    int c[3];
#pragma unroll
    for (int j = 0; j < 3; j++) c[j] = (int)(select_hash(rp.seed, (uint32_t)h, (uint32_t)j) % (uint32_t)rp.M);
    double s[3][3], t[3][3];
#pragma unroll
    for (int j = 0; j < 3; j++) {
#pragma unroll
        for (int a = 0; a < 3; a++) { s[j][a] = (double)rp.s[a][c[j]]; t[j][a] = (double)rp.t[a][c[j]]; }
    }
    int status = ICP_GLOBAL_VALID;
    if (c[0] == c[1] || c[1] == c[2] || c[0] == c[2]) status = ICP_GLOBAL_REPEATED;
    if (status == ICP_GLOBAL_VALID) {
#pragma unroll
        for (int e = 0; e < 3; e++) {
            const int a = e, b = (e + 1) % 3;
            const double sx = s[b][0] - s[a][0], sy = s[b][1] - s[a][1], sz = s[b][2] - s[a][2];
            const double tx = t[b][0] - t[a][0], ty = t[b][1] - t[a][1], tz = t[b][2] - t[a][2];
            const double ls = sqrt((sx * sx + sy * sy) + sz * sz), lt = sqrt((tx * tx + ty * ty) + tz * tz);
            if (!(fmin(ls, lt) >= rp.edge_similarity * fmax(ls, lt))) status = ICP_GLOBAL_EDGES;
        }
    }
    if (status == ICP_GLOBAL_VALID && (ransac_collinear(s) || ransac_collinear(t))) status = ICP_GLOBAL_DEGENERATE;
    float pose[16];
#pragma unroll
    for (int i = 0; i < 16; i++) pose[i] = (i % 5 == 0) ? 1.f : 0.f;
    if (status == ICP_GLOBAL_VALID) {
        ransac_kabsch(s, t, pose);
        bool fin = true;
#pragma unroll
        for (int i = 0; i < 16; i++) fin = fin && isfinite(pose[i]);
        if (!fin) {
            status = ICP_GLOBAL_DEGENERATE;
#pragma unroll
            for (int i = 0; i < 16; i++) pose[i] = (i % 5 == 0) ? 1.f : 0.f;
        }
    }
#pragma unroll
    for (int i = 0; i < 16; i++) out->pose[i] = pose[i];
    out->n_inliers = 0; out->reserved = 0; out->sum_d2 = 0.0; out->status = status;
    out->draw[0] = c[0]; out->draw[1] = c[1]; out->draw[2] = c[2];
}
// Score, one block per hypothesis over all M correspondences: the source point moved in xform_point's fp32 order, d^2 = (dx^2 + dy^2) + dz^2
// in fp32, an inlier when d^2 <= inlier_d2; an int32 count and an fp64 sum of the inliers' d^2.  Thread t takes m = t, t + 256, ...; the
// lanes fold in a fixed shuffle tree, the waves in order (k_score_multi's scheme): the same sums on every run.
constexpr int RANSAC_THREADS = 256;
__global__ __launch_bounds__(RANSAC_THREADS) void k_ransac_score(const RansacParams rp) {
    __shared__ double wsum[RANSAC_THREADS / WAVE];
    __shared__ int wcnt[RANSAC_THREADS / WAVE];
    icp_global_hypothesis* hyp = rp.hyp + blockIdx.x;
    if (hyp->status != ICP_GLOBAL_VALID) return;      // (uniform over the block; k_ransac_fit left count and sum at 0)
    float P[16];
#pragma unroll
    for (int i = 0; i < 16; i++) P[i] = hyp->pose[i];
    int cnt = 0; double sum = 0.0;
    for (int m = threadIdx.x; m < rp.M; m += RANSAC_THREADS) {
        float x, y, z;
        xform_point(P, rp.s[0][m], rp.s[1][m], rp.s[2][m], x, y, z);
        const float dx = x - rp.t[0][m], dy = y - rp.t[1][m], dz = z - rp.t[2][m];
        const float d2 = (dx * dx + dy * dy) + dz * dz;
        if (d2 <= rp.inlier_d2) { cnt++; sum += (double)d2; }
    }
    for (int off = 32; off > 0; off >>= 1) { cnt += __shfl_down(cnt, off, WAVE); sum += __shfl_down(sum, off, WAVE); }
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) { wsum[w] = sum; wcnt[w] = cnt; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double x = wsum[0]; int n = wcnt[0];
        for (int k = 1; k < RANSAC_THREADS / WAVE; k++) { x += wsum[k]; n += wcnt[k]; }
        hyp->n_inliers = n; hyp->sum_d2 = x;
    }
}
