// dev_lm.hpp -- the non-linear optimiser (CeresICPOptimizer, ICPOptimizer.h:181-483) on the device: k_lm_eval, k_lm_step.
// Part of icp_device.hpp (included from there, inside namespace icpdev); see that file for the build contract.
// ------------------------------------------------------------------------------------------------
// One ceres::Solve per ICP iteration (Levenberg-Marquardt, monotonic, Jacobi scaling; DESIGN.md "The non-linear optimiser" gives the
// contract and the readings of Ceres it rests on).  The residual blocks are the records k_post / the fused matcher leave after
// rejection; the minimiser only ever needs  cost = 1/2 f^T f,  J^T J  and  J^T f,  so one pass over the records at a point x gives
// everything a trust-region iteration consumes:
//   k_lm_eval  every correspondence at x (its residuals and Jacobian in fp64, the autodiff derivative of constraints.h) -> LM_NSUM
//              block partials, one row per sum (the same fixed-order layout as k_post's)
//   k_lm_step  ONE wave: folds the partials in a fixed order, then lane 0 runs the trust-region logic on the state in device memory --
//              decide, check the tolerances, solve the damped 6 x 6 system, write the next candidate -- and, when the minimiser ends,
//              composes the pose and writes the iteration's records.  Later launches of the same solve find `done` and return.

constexpr int LM_N = 0, LM_B = 1, LM_C = 2, LM_H = 3, LM_G = 24;     // valid pairs, residual blocks, f^T f, J^T J (upper, 21), J^T f (6)
constexpr int LM_NSUM = 30;
constexpr int LM_THREADS = 256;
constexpr int LM_BLOCKS = 512;                   // block partials of k_lm_eval at most (grid-stride beyond)

// Minimiser state of the solve in flight (device memory, written by k_lm_step only).
struct LmState {
    double x[6], cand[6], delta[6], scale[6];    // accepted point, candidate, its step, Jacobi scaling (from iteration 0)
    double H[21], g[6];                           // unscaled J^T J (upper triangle) and J^T f at x
    double cost, init_cost, radius, factor, x_norm, mcc, gmax;
    int iter, n_succ, n_unsucc, n_invalid, consec_invalid, done, n_blocks, n_pairs;
    unsigned acc_mask, inv_mask;                  // per LM iteration 1 .. 32: step accepted / invalid (icp_lm_summary)
};

// ---- forward-mode derivatives over the three rotation parameters (ceres::Jet<double, 3>: same rules) ----
struct J3 { double a, v0, v1, v2; };
__device__ __forceinline__ J3 jconst(double a) { return J3{a, 0.0, 0.0, 0.0}; }
__device__ __forceinline__ J3 operator+(J3 f, J3 g) { return J3{f.a + g.a, f.v0 + g.v0, f.v1 + g.v1, f.v2 + g.v2}; }
__device__ __forceinline__ J3 operator-(J3 f, J3 g) { return J3{f.a - g.a, f.v0 - g.v0, f.v1 - g.v1, f.v2 - g.v2}; }
__device__ __forceinline__ J3 operator-(J3 f) { return J3{-f.a, -f.v0, -f.v1, -f.v2}; }
__device__ __forceinline__ J3 operator*(J3 f, J3 g) { return J3{f.a * g.a, f.a * g.v0 + f.v0 * g.a, f.a * g.v1 + f.v1 * g.a, f.a * g.v2 + f.v2 * g.a}; }
__device__ __forceinline__ J3 operator*(J3 f, double s) { return J3{f.a * s, f.v0 * s, f.v1 * s, f.v2 * s}; }
__device__ __forceinline__ J3 jsqrt(J3 f) { const double t = sqrt(f.a), d = 2.0 * t; return J3{t, f.v0 / d, f.v1 / d, f.v2 / d}; }
__device__ __forceinline__ J3 jcos(J3 f) { const double s = -sin(f.a); return J3{cos(f.a), s * f.v0, s * f.v1, s * f.v2}; }
__device__ __forceinline__ J3 jsin(J3 f) { const double c = cos(f.a); return J3{sin(f.a), c * f.v0, c * f.v1, c * f.v2}; }
__device__ __forceinline__ J3 jrecip(J3 g) { const double m = -1.0 / (g.a * g.a); return J3{1.0 / g.a, g.v0 * m, g.v1 * m, g.v2 * m}; }

// ceres::AngleAxisRotatePoint (rotation.h) at the launch's x, its derivative carried as Jets over x[0..2]: the parts that do not depend
// on the point (cos, sin, 1 - cos and the unit axis of theta = |x|, or the axis x itself on the first-order branch), computed once per
// candidate by k_lm_step -- in memory the launch reads them with scalar loads, and the theta^2 > DBL_EPSILON test is one flag for all
// its lanes.  R(-x) p, the symmetric constraint's apply_inv_rotation, uses the same values: negating the axis negates w x p and leaves
// w (w . p)(1 - cos) unchanged, exactly, so only the cross term changes sign.
struct LmRot { J3 c, s, omc, w0, w1, w2; double t[3]; int big; };
__device__ inline LmRot lm_rot(const double* x) {
    LmRot R;
    const J3 a0{x[0], 1.0, 0.0, 0.0}, a1{x[1], 0.0, 1.0, 0.0}, a2{x[2], 0.0, 0.0, 1.0};
    const J3 theta2 = (a0 * a0 + a1 * a1) + a2 * a2;
    R.big = theta2.a > DBL_EPSILON ? 1 : 0;
    if (R.big) {
        const J3 theta = jsqrt(theta2);
        R.c = jcos(theta); R.s = jsin(theta);
        const J3 ti = jrecip(theta);
        R.w0 = a0 * ti; R.w1 = a1 * ti; R.w2 = a2 * ti;
    } else {
        R.c = jconst(1.0); R.s = jconst(0.0); R.w0 = a0; R.w1 = a1; R.w2 = a2;
    }
    R.omc = jconst(1.0) - R.c;
    R.t[0] = x[3]; R.t[1] = x[4]; R.t[2] = x[5];
    return R;
}
// component k of R(sign x) p (sign = +-1): (p_k cos + (w x p)_k sin) + w_k tmp, or p_k + (x x p)_k on the first-order branch
template <int K>
__device__ __forceinline__ J3 lm_rotate(const LmRot& R, double sign, double p0, double p1, double p2, const J3& tmp) {
    const J3 cr = K == 0 ? R.w1 * p2 - R.w2 * p1 : K == 1 ? R.w2 * p0 - R.w0 * p2 : R.w0 * p1 - R.w1 * p0;
    const double pk = K == 0 ? p0 : K == 1 ? p1 : p2;
    const J3& wk = K == 0 ? R.w0 : K == 1 ? R.w1 : R.w2;
    if (R.big) return (R.c * pk + (cr * R.s) * sign) + wk * tmp;
    return jconst(pk) + cr * sign;
}
__device__ __forceinline__ J3 lm_rot_tmp(const LmRot& R, double p0, double p1, double p2) {
    return ((R.w0 * p0 + R.w1 * p1) + R.w2 * p2) * R.omc;
}

// One residual row r with its Jacobian (three rotation columns from the Jet, three translation columns t) into the sums.
__device__ __forceinline__ void lm_add_row(const J3& r, double t0, double t1, double t2, double* acc) {
    const double J[6] = {r.v0, r.v1, r.v2, t0, t1, t2};
    acc[LM_C] += r.a * r.a;
#pragma unroll
    for (int a = 0, q = 0; a < 6; a++) {
#pragma unroll
        for (int b = a; b < 6; b++, q++) acc[LM_H + q] += J[a] * J[b];
        acc[LM_G + a] += J[a] * r.a;
    }
}

struct LmEvalParams {
    PostParams pp;               // records, clouds, pose state (the post stage's own view of this iteration)
    const LmState* st;
    const LmRot* rot;            // the point to evaluate: x = 0 (first) or the state's candidate
    int first;                   // 1: x = 0, the start of a solve (the state is not read)
    double* partials;            // [LM_NSUM][gridDim.x]
};

__global__ __launch_bounds__(LM_THREADS) void k_lm_eval(const LmEvalParams ep) {
    if (!ep.first && ep.st->done) return;                 // uniform: the solve ended in an earlier step
    const LmRot& R = *ep.rot;
    const PostParams& pp = ep.pp;
    const float* __restrict__ P = pp.ps->pose;
    const float* __restrict__ N = pp.ps->nmat;
    const double lam_point = (double)0.1f, lam_one = (double)1.0f;      // constraints.h:46,91,142
    double acc[LM_NSUM];
#pragma unroll
    for (int a = 0; a < LM_NSUM; a++) acc[a] = 0.0;
    for (int k = blockIdx.x * LM_THREADS + threadIdx.x; k < pp.n; k += gridDim.x * LM_THREADS) {
        const icp_match_t m = pp.matches[k];
        if (m.idx < 0) continue;
        const int i = pp.sel ? pp.sel[k] : k, j = m.idx;
        float s0, s1, s2;
        xform_point(P, pp.sx[i], pp.sy[i], pp.sz[i], s0, s1, s2);          // transformPoints, as post_eval
        const float q0 = pp.tx[j], q1 = pp.ty[j], q2 = pp.tz[j];
        if (!(finite3(s0, s1, s2) && finite3(q0, q1, q2))) continue;      // ICPOptimizer.h:375-376
        acc[LM_N] += 1.0;
        acc[LM_B] += 1.0;
        // the second block: point-to-plane with a finite target normal n, symmetric with finite n and moved source normal: m = n_q + n_p
        bool second = false;
        double m0 = 0.0, m1 = 0.0, m2 = 0.0;
        if (pp.metric != ICP_METRIC_POINT_TO_POINT) {
            const float n0 = pp.tnx[j], n1 = pp.tny[j], n2 = pp.tnz[j];
            if (pp.metric == ICP_METRIC_POINT_TO_PLANE) { second = finite3(n0, n1, n2); m0 = n0; m1 = n1; m2 = n2; }      // :414-415
            else {
                float ns0, ns1, ns2;
                xform_normal(N, pp.snx[i], pp.sny[i], pp.snz[i], ns0, ns1, ns2);   // transformNormals: the symmetric block takes the moved normal
                second = finite3(n0, n1, n2) && finite3(ns0, ns1, ns2);            // :458-459
                m0 = (double)n0 + (double)ns0; m1 = (double)n1 + (double)ns1; m2 = (double)n2 + (double)ns2;
            }
        }
        const bool sym = pp.metric == ICP_METRIC_SYMMETRIC;
        const double w = (double)m.weight, lw = lam_point * w, l1 = lam_one * w;
        const double p0 = s0, p1 = s1, p2 = s2, d0 = q0, d1 = q1, d2 = q2;
        const J3 tp = lm_rot_tmp(R, p0, p1, p2);
        const J3 tq = sym ? lm_rot_tmp(R, d0, d1, d2) : jconst(0.0);
        // point-to-point block (constraints.h:29-31): lambda w (R(x) s + t - q), lambda = 0.1f; row k as soon as component k is known,
        // the second block's sum over k alongside: n . (R s + t - q) (:71-75) or (n_q + n_p) . (R(x) s + t - R(-x) q) (:121-125)
        J3 sec = jconst(0.0);
        {
            const J3 st = lm_rotate<0>(R, 1.0, p0, p1, p2, tp) + jconst(R.t[0]);
            const J3 e = st - jconst(d0);
            lm_add_row(e * lw, lw, 0.0, 0.0, acc);
            sec = (sym ? st - lm_rotate<0>(R, -1.0, d0, d1, d2, tq) : e) * m0;
        }
        {
            const J3 st = lm_rotate<1>(R, 1.0, p0, p1, p2, tp) + jconst(R.t[1]);
            const J3 e = st - jconst(d1);
            lm_add_row(e * lw, 0.0, lw, 0.0, acc);
            sec = sec + (sym ? st - lm_rotate<1>(R, -1.0, d0, d1, d2, tq) : e) * m1;
        }
        {
            const J3 st = lm_rotate<2>(R, 1.0, p0, p1, p2, tp) + jconst(R.t[2]);
            const J3 e = st - jconst(d2);
            lm_add_row(e * lw, 0.0, 0.0, lw, acc);
            sec = sec + (sym ? st - lm_rotate<2>(R, -1.0, d0, d1, d2, tq) : e) * m2;
        }
        if (second) {
            acc[LM_B] += 1.0;
            lm_add_row(sec * l1, l1 * m0, l1 * m1, l1 * m2, acc);
        }
    }
    __shared__ double lds[4 * LM_NSUM * 17];
    const double tot = block_reduce_wide<LM_NSUM, 4>(acc, lds);
    if (threadIdx.x < LM_NSUM) ep.partials[(size_t)threadIdx.x * gridDim.x + blockIdx.x] = tot;
}

// slot 0 of the evaluation points: x = 0 (written once per context)
__global__ void k_lm_init(LmRot* rot) {
    const double z[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (threadIdx.x == 0) *rot = lm_rot(z);
}

struct LmStepParams {
    const double* partials; int nblocks;
    LmState* st;
    LmRot* rot;                  // where the candidate's evaluation point goes (k_lm_eval's slot 1)
    icp_lm_options opt;
    PoseState* ps;
    icp_iter_stats* stats;       // record of this ICP iteration (may be null)
    icp_lm_summary* summary;     // LM record of this ICP iteration (may be null)
    int n_src;
    int first;                   // 1: the partials are those of x = 0: set the solve up (iteration 0)
};

// (A + diag) y = b for the symmetric 6 x 6 A (upper triangle, 21): LDL^T, every pivot must be positive and finite.
__device__ __forceinline__ bool lm_solve6(const double* A, double* y) {
    double L[6][6], d[6];
    bool ok = true;
#pragma unroll
    for (int a = 0; a < 6; a++) {
#pragma unroll
        for (int b = 0; b < 6; b++) L[a][b] = 0.0;
    }
#pragma unroll
    for (int a = 0, q = 0; a < 6; a++) {
#pragma unroll
        for (int b = a; b < 6; b++, q++) L[b][a] = A[q];          // lower triangle of the symmetric matrix
    }
#pragma unroll
    for (int k = 0; k < 6; k++) {
        double dk = L[k][k];
#pragma unroll
        for (int p = 0; p < k; p++) dk -= L[k][p] * L[k][p] * d[p];
        d[k] = dk;
        ok = ok && dk > 0.0 && isfinite(dk);
#pragma unroll
        for (int r = k + 1; r < 6; r++) {
            double v = L[r][k];
#pragma unroll
            for (int p = 0; p < k; p++) v -= L[r][p] * L[k][p] * d[p];
            L[r][k] = v / dk;
        }
    }
    if (!ok) return false;
    double z[6];
#pragma unroll
    for (int r = 0; r < 6; r++) {
        double v = y[r];
#pragma unroll
        for (int p = 0; p < r; p++) v -= L[r][p] * z[p];
        z[r] = v;
    }
#pragma unroll
    for (int r = 5; r >= 0; r--) {
        double v = z[r] / d[r];
#pragma unroll
        for (int p = r + 1; p < 6; p++) v -= L[p][r] * y[p];
        y[r] = v;
    }
#pragma unroll
    for (int r = 0; r < 6; r++) ok = ok && isfinite(y[r]);
    return ok;
}

// ceres::AngleAxisToRotationMatrix (fp64, column-major R[3 c + r]) -> fp32 dT, composed from the left: estimatedPose =
// convertToMatrix(poseIncrement) * estimatedPose (ICPOptimizer.h:309, utils.h:79-96).
__device__ inline void lm_compose(const double* x, PoseState* ps) {
    double R[9];
    const double t2 = (x[0] * x[0] + x[1] * x[1]) + x[2] * x[2];
    if (t2 > DBL_EPSILON) {
        const double th = sqrt(t2), wx = x[0] / th, wy = x[1] / th, wz = x[2] / th, c = cos(th), s = sin(th), o = 1.0 - c;
        R[0] = c + wx * wx * o;       R[1] = wz * s + wx * wy * o;  R[2] = -wy * s + wx * wz * o;
        R[3] = wx * wy * o - wz * s;  R[4] = c + wy * wy * o;       R[5] = wx * s + wy * wz * o;
        R[6] = wy * s + wx * wz * o;  R[7] = -wx * s + wy * wz * o; R[8] = c + wz * wz * o;
    } else {
        R[0] = 1.0;   R[1] = x[2];  R[2] = -x[1];
        R[3] = -x[2]; R[4] = 1.0;   R[5] = x[0];
        R[6] = x[1];  R[7] = -x[0]; R[8] = 1.0;
    }
    float dT[16];
#pragma unroll
    for (int i = 0; i < 16; i++) dT[i] = (i % 5 == 0) ? 1.f : 0.f;
#pragma unroll
    for (int cc = 0; cc < 3; cc++) {
#pragma unroll
        for (int r = 0; r < 3; r++) dT[cc * 4 + r] = (float)R[cc * 3 + r];
        dT[12 + cc] = (float)x[3 + cc];
    }
    float np[16];
    mat4_mul_f32(dT, ps->pose, np);                       // the linear path's dT * pose (ICPOptimizer.h:614-620)
#pragma unroll
    for (int i = 0; i < 16; i++) ps->pose[i] = np[i];
    normal_matrix_from_pose(ps->pose, ps->nmat);
}

__global__ __launch_bounds__(WAVE) void k_lm_step(const LmStepParams sp) {
    if (!sp.first && sp.st->done) return;                 // uniform
    __shared__ double tot[LM_NSUM];
    const int lane = threadIdx.x;
    // fixed-order fold: lane l adds the partials l, l + 64, ... of each row, then the shuffle tree.  The rows go side by side, so the
    // loads of one block column are in flight together: nblocks / 64 trips to memory, not one per row and column.
    double v[LM_NSUM];
#pragma unroll
    for (int a = 0; a < LM_NSUM; a++) v[a] = 0.0;
    for (int b = lane; b < sp.nblocks; b += WAVE) {
#pragma unroll
        for (int a = 0; a < LM_NSUM; a++) v[a] += sp.partials[(size_t)a * sp.nblocks + b];
    }
#pragma unroll
    for (int a = 0; a < LM_NSUM; a++) {
        double x = v[a];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) x += __shfl_down(x, off, WAVE);
        if (lane == 0) tot[a] = x;
    }
    if (lane != 0) return;
    const icp_lm_options& o = sp.opt;
    LmState S;
    if (sp.first) {
        // iteration 0 (TrustRegionMinimizer::IterationZero): x = 0, the Jacobian at x and its column scaling
#pragma unroll
        for (int k = 0; k < 6; k++) { S.x[k] = 0.0; S.cand[k] = 0.0; S.delta[k] = 0.0; S.scale[k] = 1.0; }
        S.gmax = 0.0; S.radius = o.initial_trust_region_radius; S.factor = 2.0; S.x_norm = 0.0; S.mcc = 0.0;
        S.iter = 0; S.n_succ = 0; S.n_unsucc = 0; S.n_invalid = 0; S.consec_invalid = 0; S.done = 0; S.acc_mask = 0u; S.inv_mask = 0u;
        S.n_pairs = (int)tot[LM_N]; S.n_blocks = (int)tot[LM_B];
        S.cost = 0.5 * tot[LM_C]; S.init_cost = S.cost;
#pragma unroll
        for (int q = 0; q < 21; q++) S.H[q] = tot[LM_H + q];
#pragma unroll
        for (int k = 0; k < 6; k++) S.g[k] = tot[LM_G + k];
    } else {
        S = *sp.st;
    }
    int reason = -1;                                      // ICP_LM_* once the solve ends
    bool success = false;
    if (sp.first) {
        if (S.n_blocks <= 0) reason = ICP_LM_NO_RESIDUALS;      // ASSERT(numResidualBlock > 0): reported like the linear path's empty iteration
        else {
            bool fin = isfinite(S.cost);
#pragma unroll
            for (int q = 0; q < 21; q++) fin = fin && isfinite(S.H[q]);
#pragma unroll
            for (int k = 0; k < 6; k++) fin = fin && isfinite(S.g[k]);
            if (!fin) reason = ICP_LM_FAILURE;            // the evaluation at the start failed
            else {
                // the scaling: 1 / (1 + column norm) of the Jacobian at the start, kept for the whole solve
                const int dq[6] = {0, 6, 11, 15, 18, 20};
#pragma unroll
                for (int k = 0; k < 6; k++) S.scale[k] = o.jacobi_scaling ? 1.0 / (1.0 + sqrt(S.H[dq[k]])) : 1.0;
                success = true;                           // iteration 0 counts as a successful step
            }
        }
    } else {
        // the candidate of iteration S.iter has been evaluated: its sums are the partials of this launch
        double cc = 0.5 * tot[LM_C];
        if (!isfinite(cc)) cc = DBL_MAX;
        double sn = 0.0;
#pragma unroll
        for (int k = 0; k < 6; k++) sn += S.delta[k] * S.delta[k];
        sn = sqrt(sn);
        if (sn <= o.parameter_tolerance * (S.x_norm + o.parameter_tolerance)) reason = ICP_LM_CONVERGENCE;     // ParameterToleranceReached
        else if (fabs(S.cost - cc) <= o.function_tolerance * S.cost) reason = ICP_LM_CONVERGENCE;             // FunctionToleranceReached
        else {
            const double rho = (S.cost - cc) / S.mcc;
            if (rho > o.min_relative_decrease) {          // HandleSuccessfulStep: x = candidate, J at it, radius grows
                double xn = 0.0;
#pragma unroll
                for (int k = 0; k < 6; k++) { S.x[k] = S.cand[k]; xn += S.x[k] * S.x[k]; }
                S.x_norm = sqrt(xn);
                S.cost = cc;
#pragma unroll
                for (int q = 0; q < 21; q++) S.H[q] = tot[LM_H + q];
#pragma unroll
                for (int k = 0; k < 6; k++) S.g[k] = tot[LM_G + k];
                const double t = 2.0 * rho - 1.0;
                S.radius = fmin(S.radius / fmax(1.0 / 3.0, 1.0 - t * t * t), o.max_trust_region_radius);
                S.factor = 2.0;
                if (S.iter <= 32) S.acc_mask |= 1u << (S.iter - 1);
                success = true;
            } else {                                      // HandleUnsuccessfulStep
                S.radius = S.radius / S.factor; S.factor *= 2.0;
            }
        }
    }
    // FinalizeIterationAndCheckIfMinimizerCanContinue, then the next step; invalid steps loop here without a candidate
#pragma unroll 1
    while (reason < 0) {
        if (success) {
            S.n_succ++;
            double gm = 0.0;
#pragma unroll
            for (int k = 0; k < 6; k++) gm = fmax(gm, fabs(S.g[k]));
            S.gmax = gm;
        } else S.n_unsucc++;
        if (S.iter >= o.max_num_iterations) { reason = ICP_LM_NO_CONVERGENCE; break; }
        if (success && S.gmax <= o.gradient_tolerance) { reason = ICP_LM_CONVERGENCE; break; }
        if (S.radius < o.min_trust_region_radius) { reason = ICP_LM_CONVERGENCE; break; }
        S.iter++;
        // the LM step on the scaled Jacobian Js = J S: (Js^T Js + D^2) y = -Js^T f, D^2 = clamp(diag(Js^T Js)) / radius
        double A[21], Hs[21], gs[6], y[6];
#pragma unroll
        for (int a = 0, q = 0; a < 6; a++) {
#pragma unroll
            for (int b = a; b < 6; b++, q++) { Hs[q] = (S.H[q] * S.scale[a]) * S.scale[b]; A[q] = Hs[q]; }
        }
#pragma unroll
        for (int a = 0, q = 0; a < 6; a++) {
            const double dg = fmin(fmax(Hs[q], o.min_lm_diagonal), o.max_lm_diagonal);
            A[q] += dg / S.radius;
            gs[a] = S.scale[a] * S.g[a]; y[a] = gs[a];
            q += 6 - a;
        }
        bool valid = lm_solve6(A, y);
        double mcc = 0.0;
        if (valid) {
            // model_cost_change = -(step^T Js^T f + 1/2 step^T Js^T Js step), step = -y
            double lin = 0.0, quad = 0.0;
#pragma unroll
            for (int a = 0, q = 0; a < 6; a++) {
                lin += -y[a] * gs[a];
#pragma unroll
                for (int b = a; b < 6; b++, q++) quad += (a == b ? 1.0 : 2.0) * Hs[q] * y[a] * y[b];
            }
            mcc = -(lin + 0.5 * quad);
            valid = mcc > 0.0 && isfinite(mcc);
        }
        if (!valid) {
            S.n_invalid++;
            if (S.iter <= 32) S.inv_mask |= 1u << (S.iter - 1);
            if (++S.consec_invalid >= o.max_num_consecutive_invalid_steps) { reason = ICP_LM_FAILURE; break; }
            S.radius = S.radius / S.factor; S.factor *= 2.0;      // StepIsInvalid = a rejected step
            success = false;
            continue;
        }
        S.consec_invalid = 0;
        S.mcc = mcc;
#pragma unroll
        for (int k = 0; k < 6; k++) { S.delta[k] = -y[k] * S.scale[k]; S.cand[k] = S.x[k] + S.delta[k]; }
        *sp.rot = lm_rot(S.cand);
        break;                                            // k_lm_eval evaluates the candidate next
    }
    if (reason >= 0) {
        S.done = 1;
        int status = ICP_OK;
        double xf[6];
#pragma unroll
        for (int k = 0; k < 6; k++) xf[k] = reason == ICP_LM_FAILURE ? 0.0 : S.x[k];      // FAILURE: the parameters stay at 0
        if (reason == ICP_LM_NO_RESIDUALS) status = ICP_ERR_NO_CORRESPONDENCES;
        else lm_compose(xf, sp.ps);
        if (sp.stats) {
            sp.stats->n_src = sp.n_src; sp.stats->n_valid = S.n_pairs;
#pragma unroll
            for (int i = 0; i < 16; i++) sp.stats->pose[i] = sp.ps->pose[i];
            sp.stats->rmse = -1.f; sp.stats->benchmark_error = -1.f; sp.stats->status = status;
        }
        if (sp.summary) {
            icp_lm_summary& o2 = *sp.summary;
            o2.iterations = S.iter; o2.successful_steps = S.n_succ; o2.unsuccessful_steps = S.n_unsucc; o2.invalid_steps = S.n_invalid;
            o2.termination = reason; o2.n_residual_blocks = S.n_blocks;
            o2.accepted_steps_mask = S.acc_mask; o2.invalid_steps_mask = S.inv_mask;
            o2.initial_cost = reason == ICP_LM_NO_RESIDUALS ? 0.0 : S.init_cost; o2.final_cost = reason == ICP_LM_NO_RESIDUALS ? 0.0 : S.cost;
            o2.trust_region_radius = S.radius;
#pragma unroll
            for (int k = 0; k < 6; k++) o2.x[k] = xf[k];
        }
    }
    *sp.st = S;
}
