// dev_robust.hpp -- trimmed ICP (Chetverikov et al. 2002) and IRLS with an M-estimator (Huber, Cauchy, Tukey): the exact order statistics
// of an iteration's residuals and the reweighting of its records, all on the device (icp_robust_options).
// Part of icp_device.hpp (included from there, inside namespace icpdev); see that file for the build contract.
// ------------------------------------------------------------------------------------------------
// The chain of one iteration, launch-only (the host never waits inside it):
//   k_robust_eval       post_eval with the user's weighting and rejection (the records become what k_post leaves today), then the key of
//                       every entering pair -- the bit pattern of its fp32 r^2, ROBUST_SKIP for a pair that does not enter -- the count m
//                       and the histogram of the first digit (key bits 31..21)
//   k_robust_select<1>  the digit of bits 20..10 of the keys that share the selected first digit, for both targets (ranks K and ceil(K/2))
//   k_robust_select<2>  the digit of bits 9..0 of the keys that share the selected first two digits
//   k_robust_finish     one block: t, med, M and sigma from the three histograms, the iteration's icp_robust_stats, the histograms cleared
//   k_robust_apply      trims (r^2 > t: idx = -1) and reweights the kept records in place
// Every select block re-derives the selected prefix from the global histograms itself (a 2048-bin scan), so no "pick" launch sits between
// the passes.  Histogram counts are integers added with atomics: the result does not depend on the order in which blocks arrive.
// Every kernel here calls only __forceinline__ helpers: an existing kernel keeps exactly the code it had (tools/dev_isa_compare.py).
constexpr int ROBUST_THREADS = 256;
constexpr int ROBUST_BLOCKS = 512;                // grid cap of the per-pair kernels (grid-stride loops past it)
constexpr unsigned int ROBUST_SKIP = 0xFFFFFFFFu; // key of a pair that does not enter: r^2 is never NaN, so no residual has this pattern
constexpr int ROBUST_BINS0 = 2048, ROBUST_BINS1 = 2048, ROBUST_BINS2 = 1024;     // digits of 11 / 11 / 10 bits

// Device state of the chain.  hist*/m are zero between iterations (k_robust_finish clears them; the host clears them once per call).
struct RobustState {
    unsigned int hist0[ROBUST_BINS0];
    unsigned int hist1[2][ROBUST_BINS1];          // [target]: 0 = rank K (t), 1 = rank ceil(K/2) (med)
    unsigned int hist2[2][ROBUST_BINS2];
    unsigned int m;                               // pairs that entered
    unsigned int t_key;                           // results of k_robust_finish for k_robust_apply
    unsigned int active;                          // m > 0
    unsigned int pad;
    double sigma;
};

struct RobustParams {
    RobustState* st;
    unsigned int* keys;                           // [n]
    icp_robust_stats* stats;                      // this iteration's record (never nullptr)
    int kernel;                                   // ICP_ROBUST_*
    int linear_weight;                            // point-to-point: w' = w rho; otherwise w' = w sqrt(rho)
    float tuning;                                 // c, the standard constant already substituted for 0
    float sigma;                                  // > 0: fixed scale; 0: adaptive
    float overlap;                                // xi
    int n;
};

// K = clamp(ceil(xi m), 1, m) in fp64 and the rank of the median, ceil(K / 2)
__device__ __forceinline__ void robust_ranks(float overlap, unsigned int m, unsigned int& K, unsigned int& Kmed) {
    double k = ceil((double)overlap * (double)m);
    if (k < 1.0) k = 1.0;
    if (k > (double)m) k = (double)m;
    K = (unsigned int)k; Kmed = (K + 1u) / 2u;
}

// Block-wide search of the bin holding rank r (1-based) of a histogram, for two ranks at once: on return bin[t] is the bin and before[t]
// the number of keys in the bins below it.  Thread i owns NB / 256 consecutive bins; an inclusive Hillis-Steele scan of the 256 thread
// sums in LDS finds the thread, that thread walks its bins.  scan: 256 + 4 unsigned of LDS.  Every thread of the block calls it.
template <int NB>
__device__ __forceinline__ void robust_find2(const unsigned int* __restrict__ h0, const unsigned int* __restrict__ h1, unsigned int r0, unsigned int r1,
                                             unsigned int* scan0, unsigned int* scan1, unsigned int* res, unsigned int (&bin)[2], unsigned int (&before)[2]) {
    constexpr int PER = NB / ROBUST_THREADS;
    const int tid = threadIdx.x;
    unsigned int a = 0, b = 0;
#pragma unroll
    for (int q = 0; q < PER; q++) { a += h0[tid * PER + q]; b += h1[tid * PER + q]; }
    scan0[tid] = a; scan1[tid] = b;
    if (tid < 4) res[tid] = 0u;                           // (a rank past the total -- never, the counts agree -- still reads bin 0)
    __syncthreads();
    for (int off = 1; off < ROBUST_THREADS; off <<= 1) {
        const unsigned int x = tid >= off ? scan0[tid - off] : 0u, y = tid >= off ? scan1[tid - off] : 0u;
        __syncthreads();
        scan0[tid] += x; scan1[tid] += y;
        __syncthreads();
    }
    const unsigned int inc0 = scan0[tid], inc1 = scan1[tid];
    if (inc0 - a < r0 && r0 <= inc0) {
        unsigned int cum = inc0 - a; int q = 0;
        while (q < PER - 1 && cum + h0[tid * PER + q] < r0) { cum += h0[tid * PER + q]; q++; }
        res[0] = (unsigned int)(tid * PER + q); res[1] = cum;
    }
    if (inc1 - b < r1 && r1 <= inc1) {
        unsigned int cum = inc1 - b; int q = 0;
        while (q < PER - 1 && cum + h1[tid * PER + q] < r1) { cum += h1[tid * PER + q]; q++; }
        res[2] = (unsigned int)(tid * PER + q); res[3] = cum;
    }
    __syncthreads();
    bin[0] = res[0]; before[0] = res[1]; bin[1] = res[2]; before[1] = res[3];
    __syncthreads();
}

// Adds a block's LDS histogram into the global one: one integer atomic per non-zero bin.
template <int NB>
__device__ __forceinline__ void robust_flush(const unsigned int* lh, unsigned int* gh) {
    for (int b = threadIdx.x; b < NB; b += ROBUST_THREADS) { const unsigned int v = lh[b]; if (v) atomicAdd(gh + b, v); }
}

__global__ __launch_bounds__(ROBUST_THREADS) void k_robust_eval(const PostParams pp, const RobustParams rp) {
    __shared__ unsigned int lh[ROBUST_BINS0];
    __shared__ unsigned int lm;
    for (int b = threadIdx.x; b < ROBUST_BINS0; b += ROBUST_THREADS) lh[b] = 0u;
    if (threadIdx.x == 0) lm = 0u;
    __syncthreads();
    unsigned int cnt = 0;
    for (int k = blockIdx.x * ROBUST_THREADS + threadIdx.x; k < pp.n; k += gridDim.x * ROBUST_THREADS) {
        const icp_match_t m = pp.matches[k];
        unsigned int key = ROBUST_SKIP;
        if (m.idx >= 0) {                                     // (post_point's early exit: an unmatched record stays as the matcher wrote it)
            const int j = m.idx;
            const float d0 = pp.tx[j], d1 = pp.ty[j], d2 = pp.tz[j];
            float s0, s1, s2, w;
            if (post_eval(pp, k, m, d0, d1, d2, pp.tnx[j], pp.tny[j], pp.tnz[j], pp.weighting == ICP_WEIGHT_COLORS ? pp.trgba[j] : 0u, s0, s1, s2, w)) {
                const float e0 = s0 - d0, e1 = s1 - d1, e2 = s2 - d2;
                key = __float_as_uint((e0 * e0 + e1 * e1) + e2 * e2);
                atomicAdd(&lh[key >> 21], 1u);
                cnt++;
            }
        }
        rp.keys[k] = key;
    }
    if (cnt) atomicAdd(&lm, cnt);
    __syncthreads();
    robust_flush<ROBUST_BINS0>(lh, rp.st->hist0);
    if (threadIdx.x == 0 && lm) atomicAdd(&rp.st->m, lm);
}

// PASS 1: digit 20..10 of the keys whose digit 31..21 is the selected one; PASS 2: digit 9..0 of those whose bits 31..10 are selected.
template <int PASS>
__global__ __launch_bounds__(ROBUST_THREADS) void k_robust_select(const RobustParams rp) {
    constexpr int NB = PASS == 1 ? ROBUST_BINS1 : ROBUST_BINS2;
    __shared__ unsigned int lh[2][NB];
    __shared__ unsigned int scan0[ROBUST_THREADS], scan1[ROBUST_THREADS], res[4];
    const unsigned int m = rp.st->m;
    if (m == 0u) return;                                  // (uniform over the grid)
    unsigned int K, Kmed;
    robust_ranks(rp.overlap, m, K, Kmed);
    unsigned int bin[2], before[2];
    robust_find2<ROBUST_BINS0>(rp.st->hist0, rp.st->hist0, K, Kmed, scan0, scan1, res, bin, before);
    unsigned int pre[2] = {bin[0], bin[1]};
    if (PASS == 2) {
        const unsigned int r0 = K - before[0], r1 = Kmed - before[1];
        robust_find2<ROBUST_BINS1>(rp.st->hist1[0], rp.st->hist1[1], r0, r1, scan0, scan1, res, bin, before);
        pre[0] = (pre[0] << 11) | bin[0]; pre[1] = (pre[1] << 11) | bin[1];
    }
    constexpr int SHIFT = PASS == 1 ? 21 : 10;
    constexpr unsigned int DMASK = PASS == 1 ? 0x7FFu : 0x3FFu;
    constexpr int DSHIFT = PASS == 1 ? 10 : 0;
    for (int b = threadIdx.x; b < NB; b += ROBUST_THREADS) { lh[0][b] = 0u; lh[1][b] = 0u; }
    __syncthreads();
    for (int k = blockIdx.x * ROBUST_THREADS + threadIdx.x; k < rp.n; k += gridDim.x * ROBUST_THREADS) {
        const unsigned int key = rp.keys[k];
        if (key == ROBUST_SKIP) continue;
        const unsigned int p = key >> SHIFT, d = (key >> DSHIFT) & DMASK;
        if (p == pre[0]) atomicAdd(&lh[0][d], 1u);
        if (p == pre[1]) atomicAdd(&lh[1][d], 1u);
    }
    __syncthreads();
    unsigned int* g0 = PASS == 1 ? rp.st->hist1[0] : rp.st->hist2[0];
    unsigned int* g1 = PASS == 1 ? rp.st->hist1[1] : rp.st->hist2[1];
    robust_flush<NB>(lh[0], g0);
    robust_flush<NB>(lh[1], g1);
}

// One block: the keys of rank K (t) and ceil(K / 2) (med), M = the keys <= t, sigma; the iteration's record; the histograms cleared.
__global__ __launch_bounds__(ROBUST_THREADS) void k_robust_finish(const RobustParams rp) {
    __shared__ unsigned int scan0[ROBUST_THREADS], scan1[ROBUST_THREADS], res[4];
    RobustState* st = rp.st;
    const unsigned int m = st->m;
    if (m > 0u) {
        unsigned int K, Kmed;
        robust_ranks(rp.overlap, m, K, Kmed);
        unsigned int b0[2], f0[2], b1[2], f1[2], b2[2], f2[2];
        robust_find2<ROBUST_BINS0>(st->hist0, st->hist0, K, Kmed, scan0, scan1, res, b0, f0);
        robust_find2<ROBUST_BINS1>(st->hist1[0], st->hist1[1], K - f0[0], Kmed - f0[1], scan0, scan1, res, b1, f1);
        robust_find2<ROBUST_BINS2>(st->hist2[0], st->hist2[1], K - f0[0] - f1[0], Kmed - f0[1] - f1[1], scan0, scan1, res, b2, f2);
        const unsigned int t = (b0[0] << 21) | (b1[0] << 10) | b2[0], med = (b0[1] << 21) | (b1[1] << 10) | b2[1];
        if (threadIdx.x == 0) {
            const unsigned int M = f0[0] + f1[0] + f2[0] + st->hist2[0][b2[0]];      // keys < t, then the ties at t
            double sigma = rp.sigma > 0.f ? (double)rp.sigma : 1.4826 * sqrt((double)__uint_as_float(med));
            st->t_key = t; st->sigma = sigma; st->active = 1u;
            rp.stats->n_entering = (int)m; rp.stats->n_kept = (int)M; rp.stats->trim_d2 = __uint_as_float(t);
            rp.stats->sigma = rp.kernel == ICP_ROBUST_NONE ? -1.f : (float)sigma;
        }
    } else if (threadIdx.x == 0) {
        st->active = 0u;
        rp.stats->n_entering = 0; rp.stats->n_kept = 0; rp.stats->trim_d2 = -1.f; rp.stats->sigma = -1.f;
    }
    __syncthreads();                                      // every read of the histograms above is done
    for (int b = threadIdx.x; b < ROBUST_BINS0; b += ROBUST_THREADS) st->hist0[b] = 0u;
    for (int b = threadIdx.x; b < ROBUST_BINS1; b += ROBUST_THREADS) { st->hist1[0][b] = 0u; st->hist1[1][b] = 0u; }
    for (int b = threadIdx.x; b < ROBUST_BINS2; b += ROBUST_THREADS) { st->hist2[0][b] = 0u; st->hist2[1][b] = 0u; }
    if (threadIdx.x == 0) st->m = 0u;
}

// The robust factor rho of a residual (fp64, the contract's operation order).  sigma == 0 or +inf: 1.
__device__ __forceinline__ double robust_rho(int kernel, double c, double sigma, float r2) {
    if (kernel == ICP_ROBUST_NONE || sigma == 0.0 || isinf(sigma)) return 1.0;
    const double u = sqrt((double)r2) / sigma, q = u / c;
    if (kernel == ICP_ROBUST_HUBER) return u <= c ? 1.0 : c / u;
    if (kernel == ICP_ROBUST_CAUCHY) return 1.0 / (1.0 + q * q);
    return u < c ? (1.0 - q * q) * (1.0 - q * q) : 0.0;
}

__global__ __launch_bounds__(ROBUST_THREADS) void k_robust_apply(const PostParams pp, const RobustParams rp) {
    if (!rp.st->active) return;
    const unsigned int t = rp.st->t_key;
    const double sigma = rp.st->sigma, c = (double)rp.tuning;
    for (int k = blockIdx.x * ROBUST_THREADS + threadIdx.x; k < rp.n; k += gridDim.x * ROBUST_THREADS) {
        const unsigned int key = rp.keys[k];
        if (key == ROBUST_SKIP) continue;
        icp_match_t m = pp.matches[k];
        if (key > t) m.idx = -1;                          // trimmed: marked as rejection marks a pair, weight kept
        else if (rp.kernel != ICP_ROBUST_NONE) {
            const double rho = robust_rho(rp.kernel, c, sigma, __uint_as_float(key));
            m.weight = rp.linear_weight ? (float)((double)m.weight * rho) : (float)((double)m.weight * sqrt(rho));
        } else continue;
        pp.matches[k] = m;
    }
}
