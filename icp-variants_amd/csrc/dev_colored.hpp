// dev_colored.hpp -- colored ICP (Park, Zhou, Koltun, "Colored Point Cloud Registration Revisited", ICCV 2017): the per-point colour
// gradients of the target and the post stage.
// Part of icp_device.hpp (included from there, inside namespace icpdev); see that file for the build contract.
// ------------------------------------------------------------------------------------------------
// Every pair adds a geometric row (point-to-plane's n^T J) and a photometric row (the gradient of the intensity along the target's tangent
// plane, d^T (I - n n^T) J), weighted lambda and 1 - lambda.  The step builds the same [J^T J upper triangle (21) | J^T r (6)] block as
// point-to-plane (SUM_M), so the reduce and the solve are k_reduce_solve's point-to-plane path unchanged (the host launches it with
// metric = point-to-plane, as for GICP); only the gradients and the post stage are new.  Both kernels call only __forceinline__ helpers:
// an existing kernel keeps exactly the code it had (tools/dev_isa_compare.py).

// R + G + B of an RGBA colour; its intensity is (R + G + B) / 765 in fp64 (exact inputs, one rounding: the same value on host and device).
__device__ __forceinline__ int color_sum(uint32_t c) { return (int)(c & 0xFF) + (int)((c >> 8) & 0xFF) + (int)((c >> 16) & 0xFF); }
__device__ __forceinline__ double color_intensity(uint32_t c) { return (double)color_sum(c) / 765.0; }

// Colour gradient of target point i: the K smallest (fp32 d^2, index) pairs over the finite points (the point itself included; the walk
// and the neighbour list are k_gicp_normals'), then in fp64 one row per neighbour j != i -- a = (q_j projected onto i's tangent plane) - p,
// b = I_j - I_i -- and the constraint row a = (m - 1) n, b = 0 (m: neighbours, i included).  (A^T A) d = A^T b by adjugate and
// determinant, d rounded once to fp32.  A non-finite point or normal, or a zero normal: NaN; fewer than 3 neighbours or a determinant
// <= 1e-12 (tr / 3)^3: (0, 0, 0).  Output: SoA planes, original point order.
template <int K>
__global__ __launch_bounds__(BVH_THREADS) void k_color_gradients(const BvhViewT<3> bv, int n, int tree_depth,
                                                                 const float* __restrict__ tnx, const float* __restrict__ tny, const float* __restrict__ tnz,
                                                                 const uint32_t* __restrict__ trgba,
                                                                 float* __restrict__ gx_out, float* __restrict__ gy_out, float* __restrict__ gz_out) {
    extern __shared__ unsigned short bvh_lb16[];
    const int tid = threadIdx.x;
    const int i = blockIdx.x * BVH_THREADS + tid;
    if (i >= n) return;
    const float px = bv.tgt.c[0][i], py = bv.tgt.c[1][i], pz = bv.tgt.c[2][i];
    float gx = NAN, gy = NAN, gz = NAN;
    double nu[3];
    if (finite3(px, py, pz) && gicp_unit(tnx[i], tny[i], tnz[i], nu)) {
        gx = 0.f; gy = 0.f; gz = 0.f;
        if (bv.n_valid >= 3) {
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
            const double p0 = px, p1 = py, p2d = pz;
            const double Ii = color_intensity(trgba[i]);
            int cnt = 0;
            double a00 = 0, a01 = 0, a02 = 0, a11 = 0, a12 = 0, a22 = 0, b0 = 0, b1 = 0, b2 = 0;
#pragma unroll
            for (int q = 0; q < K; q++) if (bd[q] < FLT_MAX) {
                cnt++;
                const int j = bj[q];
                if (j == i) continue;
                const double v0 = (double)bv.tgt.c[0][j] - p0, v1 = (double)bv.tgt.c[1][j] - p1, v2 = (double)bv.tgt.c[2][j] - p2d;
                const double t = (v0 * nu[0] + v1 * nu[1]) + v2 * nu[2];
                const double e0 = v0 - nu[0] * t, e1 = v1 - nu[1] * t, e2 = v2 - nu[2] * t;      // q'_j - p
                const double db = color_intensity(trgba[j]) - Ii;
                a00 += e0 * e0; a01 += e0 * e1; a02 += e0 * e2; a11 += e1 * e1; a12 += e1 * e2; a22 += e2 * e2;
                b0 += e0 * db; b1 += e1 * db; b2 += e2 * db;
            }
            if (cnt >= 3) {
                const double m1 = (double)(cnt - 1), c2 = m1 * m1;
                a00 += c2 * (nu[0] * nu[0]); a01 += c2 * (nu[0] * nu[1]); a02 += c2 * (nu[0] * nu[2]);
                a11 += c2 * (nu[1] * nu[1]); a12 += c2 * (nu[1] * nu[2]); a22 += c2 * (nu[2] * nu[2]);
                const double c00 = a11 * a22 - a12 * a12, c01 = a02 * a12 - a01 * a22, c02 = a01 * a12 - a02 * a11;
                const double c11 = a00 * a22 - a02 * a02, c12 = a01 * a02 - a00 * a12, c22 = a00 * a11 - a01 * a01;
                const double det = (a00 * c00 + a01 * c01) + a02 * c02;
                const double tr3 = ((a00 + a11) + a22) / 3.0;
                if (det > 1e-12 * (tr3 * tr3 * tr3)) {
                    gx = (float)(((c00 * b0 + c01 * b1) + c02 * b2) / det);
                    gy = (float)(((c01 * b0 + c11 * b1) + c12 * b2) / det);
                    gz = (float)(((c02 * b0 + c12 * b1) + c22 * b2) / det);
                }
            }
        }
    }
    gx_out[i] = gx; gy_out[i] = gy; gz_out[i] = gz;
}

// What k_post_colored reads beside the post parameters: the cached colour gradients of the target (original order) and lambda.
struct ColoredPost {
    const float* gx; const float* gy; const float* gz;
    double lambda;                // lambda_geometric, the fp32 field widened
};

// One pair's contributions: p = s (transformed source point), q = d (target point), n = the target's unit normal, u = (I - n n^T) grad.
// j_G = n^T J = [p x n | n], r_G = n.(q - p); j_C = u^T J = [p x u | u], r_C = I_s - I_q - u.(p - q), J = [-[p]x | I].
// H += w^2 (lambda j_G^T j_G + (1 - lambda) j_C^T j_C), g += w^2 (lambda j_G^T r_G + (1 - lambda) j_C^T r_C): slots 0..26 of acc.
__device__ __forceinline__ void colored_accumulate(const double (&nu)[3], const double (&gr)[3], double lambda, double di,
                                                   float s0, float s1, float s2, float d0, float d1, float d2, float w, double* acc /* 27 */) {
    const double p0 = s0, p1 = s1, p2 = s2;
    const double e0 = (double)d0 - p0, e1 = (double)d1 - p1, e2 = (double)d2 - p2;     // q - p
    const double nd = (nu[0] * gr[0] + nu[1] * gr[1]) + nu[2] * gr[2];
    const double u0 = gr[0] - nu[0] * nd, u1 = gr[1] - nu[1] * nd, u2 = gr[2] - nu[2] * nd;
    const double rg = (nu[0] * e0 + nu[1] * e1) + nu[2] * e2;
    const double rc = di + ((u0 * e0 + u1 * e1) + u2 * e2);
    const double jg[6] = {p1 * nu[2] - p2 * nu[1], p2 * nu[0] - p0 * nu[2], p0 * nu[1] - p1 * nu[0], nu[0], nu[1], nu[2]};
    const double jc[6] = {p1 * u2 - p2 * u1, p2 * u0 - p0 * u2, p0 * u1 - p1 * u0, u0, u1, u2};
    const double w2 = (double)w * (double)w;
    const double lg = w2 * lambda, lc = w2 * (1.0 - lambda);
    int k = 0;
#pragma unroll
    for (int a = 0; a < 6; a++) {
#pragma unroll
        for (int b = a; b < 6; b++) { acc[k] += lg * (jg[a] * jg[b]) + lc * (jc[a] * jc[b]); k++; }
    }
#pragma unroll
    for (int a = 0; a < 6; a++) acc[21 + a] += lg * (jg[a] * rg) + lc * (jc[a] * rc);
}

// The post stage of colored ICP: weight, reject and filter through post_eval (k_post's text), then the two rows; block partials in k_post's
// layout ([NSUM][gridDim.x]) for k_reduce_solve.  The source colour is the query's own (pp.srgba: on a Morton-sorted level that plane is
// already in sorted order).  The records are written back as k_post writes them.  n = n_f32 * (1 / |n_f32|) and
// I_s - I_q = (sum_s - sum_q) / 765, both fp64.  After post_eval the body has no branch: a pair that fails the normal / gradient filter
// adds exact zeros (weight 0, zeroed inputs) -- with a branch per filter the compiler kept two copies of the 34 accumulators (206 VGPRs).
__global__ __launch_bounds__(POST_THREADS) void k_post_colored(const PostParams pp, const ColoredPost cp) {
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
        const float n0 = pp.tnx[j], n1 = pp.tny[j], n2 = pp.tnz[j];
        const float g0 = cp.gx[j], g1 = cp.gy[j], g2 = cp.gz[j];
        const double l = sqrt(((double)n0 * n0 + (double)n1 * n1) + (double)n2 * n2);
        const bool ok = finite3(n0, n1, n2) && finite3(g0, g1, g2) && l > 0.0;
        const double il = ok ? 1.0 / l : 0.0;
        const double nu[3] = {ok ? n0 * il : 0.0, ok ? n1 * il : 0.0, ok ? n2 * il : 0.0};
        const double gr[3] = {ok ? (double)g0 : 0.0, ok ? (double)g1 : 0.0, ok ? (double)g2 : 0.0};
        const int i = pp.sel ? pp.sel[k] : k;
        const double di = ok ? (double)(color_sum(pp.srgba[i]) - color_sum(pp.trgba[j])) / 765.0 : 0.0;
        acc[SUM_N] += ok ? 1.0 : 0.0;
        acc[SUM_S] += ok ? (double)s0 : 0.0; acc[SUM_S + 1] += ok ? (double)s1 : 0.0; acc[SUM_S + 2] += ok ? (double)s2 : 0.0;
        acc[SUM_D] += ok ? (double)d0 : 0.0; acc[SUM_D + 1] += ok ? (double)d1 : 0.0; acc[SUM_D + 2] += ok ? (double)d2 : 0.0;
        colored_accumulate(nu, gr, cp.lambda, di, s0, s1, s2, d0, d1, d2, ok ? w : 0.f, acc + SUM_M);
    }
    const double tot = block_reduce_wide<34, 4>(acc, lds);
    if (threadIdx.x < 34) pp.partials[(size_t)threadIdx.x * gridDim.x + blockIdx.x] = tot;
}
