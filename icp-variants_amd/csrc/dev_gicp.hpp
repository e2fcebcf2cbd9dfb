// dev_gicp.hpp -- Generalized-ICP, plane-to-plane form (Segal, Haehnel, Thrun, RSS 2009): the per-point GICP normals and the post stage.
// Part of icp_device.hpp (included from there, inside namespace icpdev); see that file for the build contract.
// ------------------------------------------------------------------------------------------------
// A plane-to-plane covariance V diag(eps, 1, 1) V^T is I - (1 - eps) n n^T: one unit vector per point is the whole per-point state.
// The step builds the same [J^T J upper triangle (21) | J^T r (6)] block as point-to-plane (SUM_M), so the reduce and the solve are
// k_reduce_solve's point-to-plane path unchanged (the host launches it with metric = point-to-plane); only the post stage is new.
// Every new kernel here calls only __forceinline__ helpers or instantiations of its own (jacobi_eig_sym<3, GICP_COPY>): an existing
// kernel keeps exactly the code it had (tools/dev_isa_compare.py).
constexpr int GICP_COPY = 2;        // jacobi_eig_sym instantiation of the GICP normals (0: the solvers and k_normals_knn, 1: multi-start's solve)

// GICP normal of point i of the cloud the tree is built over: the K smallest (fp32 d^2, index) pairs over its finite points (the
// point itself included), fp64 mean and covariance, fp64 Jacobi, eigenvector of the smallest eigenvalue rounded once to fp32.  The walk
// and the neighbour list are k_normals_knn's (compile-time positions only: knn_insert and the unrolled loops below); no viewpoint flip,
// no curvature.  Output: SoA planes, original point order.
template <int K>
__global__ __launch_bounds__(BVH_THREADS) void k_gicp_normals(const BvhViewT<3> bv, int n, int tree_depth,
                                                              float* __restrict__ nx_out, float* __restrict__ ny_out, float* __restrict__ nz_out) {
    extern __shared__ unsigned short bvh_lb16[];
    const int tid = threadIdx.x;
    const int i = blockIdx.x * BVH_THREADS + tid;
    if (i >= n) return;
    const float px = bv.tgt.c[0][i], py = bv.tgt.c[1][i], pz = bv.tgt.c[2][i];
    float nx = NAN, ny = NAN, nz = NAN;
    if (finite3(px, py, pz) && bv.n_valid >= 3) {
        float bd[K]; int bj[K];
#pragma unroll
        for (int q = 0; q < K; q++) { bd[q] = FLT_MAX; bj[q] = 0x7fffffff; }
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
        int cnt = 0;
        double m[3] = {0, 0, 0}, cxx = 0, cxy = 0, cxz = 0, cyy = 0, cyz = 0, czz = 0;
#pragma unroll
        for (int q = 0; q < K; q++) if (bd[q] < FLT_MAX) { const int j = bj[q]; m[0] += bv.tgt.c[0][j]; m[1] += bv.tgt.c[1][j]; m[2] += bv.tgt.c[2][j]; cnt++; }
        if (cnt >= 3) {
            m[0] /= cnt; m[1] /= cnt; m[2] /= cnt;
#pragma unroll
            for (int q = 0; q < K; q++) if (bd[q] < FLT_MAX) {
                const int j = bj[q];
                const double a = bv.tgt.c[0][j] - m[0], b = bv.tgt.c[1][j] - m[1], c = bv.tgt.c[2][j] - m[2];
                cxx += a * a; cxy += a * b; cxz += a * c; cyy += b * b; cyz += b * c; czz += c * c;
            }
            double A[9] = {cxx / cnt, cxy / cnt, cxz / cnt, cxy / cnt, cyy / cnt, cyz / cnt, cxz / cnt, cyz / cnt, czz / cnt}, V[9], ev[3];
            jacobi_eig_sym<3, GICP_COPY>(A, V, ev);
            int s0 = 0; if (ev[1] < ev[s0]) s0 = 1; if (ev[2] < ev[s0]) s0 = 2;
            double vx = V[0 * 3 + s0], vy = V[1 * 3 + s0], vz = V[2 * 3 + s0];
            const double len = sqrt(vx * vx + vy * vy + vz * vz);
            nx = (float)(vx / len); ny = (float)(vy / len); nz = (float)(vz / len);
        }
    }
    nx_out[i] = nx; ny_out[i] = ny; nz_out[i] = nz;
}

// The GICP normals the post stage reads: the target's by original index (the match), the source's by original index too -- through
// src_orig (sorted position -> original index) when the post stage runs over a Morton-sorted level, else the selection's own index.
struct GicpPost {
    const float* tnx; const float* tny; const float* tnz;
    const float* snx; const float* sny; const float* snz;
    const int* src_orig;
    double one_minus_eps;         // 1 - epsilon, fp64
};

// a, b: fp32 normal -> fp64 unit vector; false when not finite or of zero length
__device__ __forceinline__ bool gicp_unit(float x, float y, float z, double (&u)[3]) {
    if (!finite3(x, y, z)) return false;
    const double a = x, b = y, c = z;
    const double len = sqrt((a * a + b * b) + c * c);
    if (!(len > 0.0)) return false;
    u[0] = a / len; u[1] = b / len; u[2] = c / len;
    return true;
}

// One pair's contributions: Sigma = 2I - (1 - eps)(a a^T + b b^T), M = adj(Sigma) / det(Sigma), J = [A | I] with A = -[p]x, r = q - p.
// H = w^2 J^T M J = w^2 [A^T M A, A^T M; M A, M], g = w^2 [A^T M r; M r], added to slots 0..26 of acc (upper triangle row-major, then g).
__device__ __forceinline__ void gicp_accumulate(const double (&a)[3], const double (&b)[3], double ome, float s0, float s1, float s2,
                                                float d0, float d1, float d2, float w, double* acc /* 27 */) {
    const double S00 = 2.0 - ome * (a[0] * a[0] + b[0] * b[0]), S11 = 2.0 - ome * (a[1] * a[1] + b[1] * b[1]), S22 = 2.0 - ome * (a[2] * a[2] + b[2] * b[2]);
    const double S01 = -ome * (a[0] * a[1] + b[0] * b[1]), S02 = -ome * (a[0] * a[2] + b[0] * b[2]), S12 = -ome * (a[1] * a[2] + b[1] * b[2]);
    const double c00 = S11 * S22 - S12 * S12, c01 = S02 * S12 - S01 * S22, c02 = S01 * S12 - S02 * S11;
    const double c11 = S00 * S22 - S02 * S02, c12 = S01 * S02 - S00 * S12, c22 = S00 * S11 - S01 * S01;
    const double det = (S00 * c00 + S01 * c01) + S02 * c02;
    const double M[3][3] = {{c00 / det, c01 / det, c02 / det}, {c01 / det, c11 / det, c12 / det}, {c02 / det, c12 / det, c22 / det}};
    const double p0 = s0, p1 = s1, p2 = s2;
    const double A[3][3] = {{0.0, p2, -p1}, {-p2, 0.0, p0}, {p1, -p0, 0.0}};      // -[p]x: A w = w x p
    const double r[3] = {(double)d0 - p0, (double)d1 - p1, (double)d2 - p2};
    const double w2 = (double)w * (double)w;
    double MA[3][3], Mr[3];
#pragma unroll
    for (int i = 0; i < 3; i++) {
#pragma unroll
        for (int c = 0; c < 3; c++) MA[i][c] = (M[i][0] * A[0][c] + M[i][1] * A[1][c]) + M[i][2] * A[2][c];
        Mr[i] = (M[i][0] * r[0] + M[i][1] * r[1]) + M[i][2] * r[2];
    }
    int q = 0;
#pragma unroll
    for (int i = 0; i < 6; i++) {
#pragma unroll
        for (int c = i; c < 6; c++) {
            double h;
            if (i < 3 && c < 3) h = (A[0][i] * MA[0][c] + A[1][i] * MA[1][c]) + A[2][i] * MA[2][c];      // A^T M A
            else if (i < 3) h = MA[c - 3][i];                                                              // A^T M = (M A)^T
            else h = M[i - 3][c - 3];
            acc[q] += w2 * h;
            q++;
        }
    }
#pragma unroll
    for (int i = 0; i < 3; i++) acc[21 + i] += w2 * ((A[0][i] * Mr[0] + A[1][i] * Mr[1]) + A[2][i] * Mr[2]);
#pragma unroll
    for (int i = 0; i < 3; i++) acc[24 + i] += w2 * Mr[i];
}

// The post stage of GICP: weight, reject and filter through post_eval (k_post's text), then the GICP rows; block partials in k_post's
// layout ([NSUM][gridDim.x]) for k_reduce_solve.  The records are written back as k_post writes them.
__global__ __launch_bounds__(POST_THREADS) void k_post_gicp(const PostParams pp, const GicpPost gp) {
    __shared__ double lds[4 * 34 * 17];
    double acc[34];
#pragma unroll
    for (int a = 0; a < 34; a++) acc[a] = 0.0;
    for (int k = blockIdx.x * POST_THREADS + threadIdx.x; k < pp.n; k += gridDim.x * POST_THREADS) {
        const icp_match_t m = pp.matches[k];
        if (m.idx < 0) continue;
        const int j = m.idx;
        const float d0 = pp.tx[j], d1 = pp.ty[j], d2 = pp.tz[j];
        float s0, s1, s2, w;
        if (!post_eval(pp, k, m, d0, d1, d2, pp.tnx[j], pp.tny[j], pp.tnz[j], pp.weighting == ICP_WEIGHT_COLORS ? pp.trgba[j] : 0u, s0, s1, s2, w)) continue;
        const int i = pp.sel ? pp.sel[k] : k;
        const int io = gp.src_orig ? gp.src_orig[i] : i;
        double a[3], b[3];
        if (!gicp_unit(gp.tnx[j], gp.tny[j], gp.tnz[j], a)) continue;
        float b0, b1, b2;
        xform_normal(pp.ps->nmat, gp.snx[io], gp.sny[io], gp.snz[io], b0, b1, b2);      // icp_transform_normals
        if (!gicp_unit(b0, b1, b2, b)) continue;
        acc[SUM_N] += 1.0;
        acc[SUM_S] += (double)s0; acc[SUM_S + 1] += (double)s1; acc[SUM_S + 2] += (double)s2;
        acc[SUM_D] += (double)d0; acc[SUM_D + 1] += (double)d1; acc[SUM_D + 2] += (double)d2;
        gicp_accumulate(a, b, gp.one_minus_eps, s0, s1, s2, d0, d1, d2, w, acc + SUM_M);
    }
    const double tot = block_reduce_wide<34, 4>(acc, lds);
    if (threadIdx.x < 34) pp.partials[(size_t)threadIdx.x * gridDim.x + blockIdx.x] = tot;
}
