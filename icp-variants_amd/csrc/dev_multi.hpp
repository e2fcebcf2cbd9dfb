// dev_multi.hpp -- multi-start ICP (icp_run_multistart): one set of launches per ICP iteration for K initial poses of ONE pair.
// Part of icp_device.hpp (included from there, inside namespace icpdev); see that file for the build contract.
// ------------------------------------------------------------------------------------------------
// Everything a start reads that does not depend on its pose is shared: the target index, the (Morton-sorted) levels of the source, the
// random draws.  What follows from the pose is the start's own, one slice per start: pose state, neighbours and search state, records,
// block partials, hand-over totals and ticket, iteration records.  Start s is blockIdx.y of every launch below, and each kernel moves
// the per-start pointers of its parameters by s before it runs the body of its single-start sibling unchanged.  Those bodies read
// blockIdx.x / gridDim.x only (and the fused matcher's LDS board is per block), so the y-slice s of a launch IS the single-start grid:
// the same queries per block, the same block partials in the same slots, the same fold -- start s follows icp_run bit for bit.
struct MultiStride {
    size_t q;             // elements per start of the per-query buffers (records, distances, neighbours, search state)
    size_t partials;      // doubles per start of the block partials
    size_t totals;        // doubles per start of the hand-over slots (NSUM totals, then the ticket)
    int stats;            // iteration records per start
};

__device__ __forceinline__ void multi_shift_knn(KnnParams& kp, const MultiStride& ms, unsigned s) {
    const size_t q = ms.q * s;
    kp.ps = kp.ps + s;
    if (kp.out) kp.out += q;
    if (kp.d2_out) kp.d2_out += q;
    if (kp.nn_raw) kp.nn_raw += q;
    if (kp.qstate) kp.qstate += q;
    if (kp.qstate2) kp.qstate2 += q;
    if (kp.fault) kp.fault = (int*)((PoseState*)kp.fault + s);      // the start's own PoseState::fault
}
__device__ __forceinline__ void multi_shift_post(PostParams& pp, const MultiStride& ms, unsigned s) {
    pp.ps = pp.ps + s;
    if (pp.matches) pp.matches += ms.q * s;
    pp.partials += ms.partials * s;
}

// The fused matcher (k_knn_bvh_post) for every start.
template <int DIM, bool WIDE>
__global__ __launch_bounds__(BVH_THREADS, DIM == 3 ? ICP_FUSED_WAVES : 4) void k_knn_bvh_post_multi(const KnnParams kp, const BvhViewT<DIM> bv, const int* __restrict__ qorder, const PostParams pp, const MultiStride ms) {
    KnnParams k = kp; PostParams p = pp;
    multi_shift_knn(k, ms, blockIdx.y);
    multi_shift_post(p, ms, blockIdx.y);
    const RingParams none{};
    fused_matcher_body<DIM, WIDE, false>(k, bv, qorder, p, none);
}
// The stand-alone matcher (k_knn_bvh): the symmetric metric's matches, and the score of the final poses.  (The bodies below are the
// single-start kernels' own text, dev_body_*.hpp, run on the shifted parameters.)
template <int DIM>
__global__ __launch_bounds__(BVH_THREADS) void k_knn_bvh_multi(const KnnParams kp_all, const BvhViewT<DIM> bv, const int* __restrict__ qorder, const MultiStride ms) {
    KnnParams kp = kp_all;
    multi_shift_knn(kp, ms, blockIdx.y);
#include "dev_body_knn_bvh.hpp"
}
__global__ __launch_bounds__(POST_THREADS) void k_post_multi(const PostParams pp_all, const MultiStride ms) {
    PostParams pp = pp_all;
    multi_shift_post(pp, ms, blockIdx.y);
#include "dev_body_post.hpp"
}
__global__ __launch_bounds__(POST_THREADS) void k_sym_accumulate_multi(const PostParams pp_all, const MultiStride ms) {
    PostParams pp = pp_all;
    multi_shift_post(pp, ms, blockIdx.y);
#include "dev_body_sym_accumulate.hpp"
}
// k_reduce_solve on a (NSUM_USED, K) grid: start s folds its own partials, hands over through its own totals and ticket, solves into its
// own pose state and writes its own iteration record.
__global__ __launch_bounds__(SOLVE_THREADS) void k_reduce_solve_multi(const SolveParams sp_all, const MultiStride ms) {
    SolveParams sp = sp_all;
    const unsigned s = blockIdx.y;
    sp.partials += ms.partials * s;
    sp.totals += ms.totals * s;
    sp.ticket = (unsigned*)(sp.totals + NSUM);
    sp.ps += s;
    if (sp.stats) sp.stats += (size_t)ms.stats * s;
    sp.sums_out = nullptr;
    // the body calls solve_tail(sp, tot): here that name is the solve's own instantiation (COPY 1, dev_solve.hpp)
    const auto solve_tail = [](const SolveParams& p, const double* t) __attribute__((always_inline)) { icpdev::solve_tail<true, 1>(p, t); };
#include "dev_body_reduce_solve.hpp"
}

// ---- score of the final poses: the full-resolution source, matched in 3-D (k_knn_bvh_multi, unseeded) at each start's final pose ----
// Block b of start s takes positions b * MSCORE_THREADS + t + j * stride (fixed assignment): inliers (idx >= 0), their sum of d^2 in
// fp64, and the finite source points; the lanes fold in a fixed shuffle tree, the waves in order.  k_score_fold then adds the blocks of a
// start in block order -- the same sums on every run.
constexpr int MSCORE_THREADS = 256, MSCORE_BLOCKS = 64;
struct ScoreParams {
    const float* sx; const float* sy; const float* sz;   // the source planes the matcher read (any order: a sum over all of them)
    int n;
    const icp_match_t* matches; const float* d2;         // [K][ms.q]
    size_t q;
    double* partials;                                    // [K][MSCORE_BLOCKS][3]: inliers, sum d^2, finite points
};
__global__ __launch_bounds__(MSCORE_THREADS) void k_score_multi(const ScoreParams sp) {
    __shared__ double wsum[MSCORE_THREADS / WAVE][3];
    const unsigned s = blockIdx.y;
    const icp_match_t* m = sp.matches + sp.q * s; const float* d2 = sp.d2 + sp.q * s;
    double acc[3] = {0.0, 0.0, 0.0};
    for (int k = blockIdx.x * MSCORE_THREADS + threadIdx.x; k < sp.n; k += gridDim.x * MSCORE_THREADS) {
        if (m[k].idx >= 0) { acc[0] += 1.0; acc[1] += (double)d2[k]; }
        if (finite3(sp.sx[k], sp.sy[k], sp.sz[k])) acc[2] += 1.0;
    }
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int a = 0; a < 3; a++) {
        double x = acc[a];
        for (int off = 32; off > 0; off >>= 1) x += __shfl_down(x, off, WAVE);
        if (lane == 0) wsum[w][a] = x;
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        double x = wsum[0][threadIdx.x];
        for (int k = 1; k < MSCORE_THREADS / WAVE; k++) x += wsum[k][threadIdx.x];
        sp.partials[((size_t)s * gridDim.x + blockIdx.x) * 3 + threadIdx.x] = x;
    }
}
// One thread per start: the blocks in order -> n_inliers, fitness, inlier_rmse and the final pose of icp_start_result.
__global__ void k_score_fold(const double* __restrict__ partials, int nblocks, const PoseState* __restrict__ ps, int n_starts, icp_start_result* out) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n_starts) return;
    double a[3] = {0.0, 0.0, 0.0};
    for (int b = 0; b < nblocks; b++)
        for (int j = 0; j < 3; j++) a[j] += partials[((size_t)s * nblocks + b) * 3 + j];
    icp_start_result r;
    for (int i = 0; i < 16; i++) r.pose[i] = ps[s].pose[i];
    r.status = ICP_OK;                                   // (the host fills in the status from the start's records)
    r.n_inliers = (int)a[0];
    r.fitness = a[2] > 0.0 ? (float)(a[0] / a[2]) : 0.f;
    r.inlier_rmse = a[0] > 0.0 ? (float)sqrt(a[1] / a[0]) : -1.f;
    out[s] = r;
}
