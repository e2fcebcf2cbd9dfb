// dev_nss.hpp -- normal-space sampling (Rusinkiewicz and Levoy 2001), params.selection = ICP_SELECT_NORMAL_SPACE: the contract is in
// include/icp_hip.h, a numpy restatement in tests/nss_restatement.py.
// Part of icp_device.hpp (included from there, inside namespace icpdev); see that file for the build contract.
//
// The chain (host side: nss_* in host_loop.hpp):
//   once per source and grid   k_nss_bucket         one uint16 bucket per source point (NSS_NONE: no bucket)
//   once per level             k_nss_level_hist     per-block bucket counts, bucket-major -> k_select_scan over the table ->
//                              k_nss_level_scatter  the level's candidates sorted by bucket, STABLE: every bucket is one contiguous segment
//                              k_nss_level_segs     of increasing original indices; segment starts; the list of LONG segments and their chunks
//   per run, blockIdx.y = draw k_nss_quota          one block: M, the water-filling cap c, the quotas q_b, the excess choice
//                              k_nss_select_small   one block per (bucket, draw): exact radix select (11 / 11 / 10 bit digits, histogram in
//                                                   LDS, hashes recomputed, never stored) of the q_b-th smallest hash -> threshold t_b
//                              k_nss_long_hist<P> / a segment longer than NSS_LONG (the floor of a room lands in ONE bucket): its chunks of
//                              k_nss_long_pick<P>   NSS_CHUNK points go to a block each, integer atomics on ONE global histogram per (draw,
//                                                   long segment) -- sums of integers: the result does not depend on the order of arrival
//                              k_nss_count / k_nss_scan / k_nss_scatter   keep hash <= t_b, compacted in increasing original index
//
// Why exactly M points come out, with no tie rule: for a fixed (seed, iteration) select_hash is a BIJECTION of the 32-bit index -- the
// inner fmix32 is a constant, index * 0x9E3779B9 is a multiplication by an odd constant (invertible mod 2^32), adding a constant is
// invertible, and fmix32 is a composition of xor-shifts and odd multiplications, each invertible.  Distinct indices therefore have distinct
// keys: the q_b-th smallest key of a bucket is unique, `key <= t_b` keeps exactly q_b points, and the bucket keys 0x80000000 | b of the
// excess rule never tie either.
constexpr int NSS_MAX_BUCKETS = 294;        // 6 * 7 * 7
constexpr int NSS_ROW = 296;                // row stride of the per-draw quota / threshold tables
constexpr unsigned short NSS_NONE = 0xFFFFu;
constexpr int NSS_LEVEL_THREADS = 1024;     // points per block of the per-level counting sort
constexpr int NSS_THREADS = 256;
constexpr int NSS_QUOTA_THREADS = 512;      // >= NSS_MAX_BUCKETS + 1: one bucket per thread
constexpr int NSS_LONG = 16384;             // a segment with more candidates than this is selected by several blocks
constexpr int NSS_CHUNK = 4096;             // candidates per block of a long segment
constexpr int NSS_BINS = 2048;

// The bucket of one normal on a cube map of grid x grid cells per face (icp_hip.h): fp32 only, IEEE division, no transcendental.
__device__ __forceinline__ unsigned short nss_bucket_of(float px, float py, float pz, float x, float y, float z, int grid) {
    if (!finite3(px, py, pz) || !finite3(x, y, z)) return NSS_NONE;
    const float ax = fabsf(x), ay = fabsf(y), az = fabsf(z);
    const float m = fmaxf(ax, fmaxf(ay, az));
    if (m == 0.f) return NSS_NONE;
    int a; float na, u, v;
    if (ax == m) { a = 0; na = x; u = y; v = z; }
    else if (ay == m) { a = 1; na = y; u = x; v = z; }
    else { a = 2; na = z; u = x; v = y; }
    u = u / m; v = v / m;
    const float half = 0.5f * (float)grid;
    int cu = (int)floorf((u + 1.0f) * half), cv = (int)floorf((v + 1.0f) * half);
    cu = cu < grid - 1 ? cu : grid - 1; cv = cv < grid - 1 ? cv : grid - 1;
    const int face = 2 * a + (na < 0.f ? 1 : 0);
    return (unsigned short)(face * grid * grid + cv * grid + cu);
}
__global__ __launch_bounds__(256) void k_nss_bucket(const float* __restrict__ px, const float* __restrict__ py, const float* __restrict__ pz,
                                                    const float* __restrict__ nx, const float* __restrict__ ny, const float* __restrict__ nz, int n, int grid,
                                                    unsigned short* __restrict__ out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = nss_bucket_of(px[i], py[i], pz[i], nx[i], ny[i], nz[i], grid);
}

// ---- once per level: the candidates sorted by bucket ----
// table[bin * nblocks + block] = points of `block` in `bin` (bin nb = no bucket): its exclusive scan is where the block's share of a bin starts
__global__ __launch_bounds__(NSS_LEVEL_THREADS) void k_nss_level_hist(const int* __restrict__ base, int n, const unsigned short* __restrict__ bkt, int nb,
                                                                      int* __restrict__ table, int nblocks) {
    __shared__ int lh[NSS_MAX_BUCKETS + 1];
    for (int b = threadIdx.x; b <= nb; b += NSS_LEVEL_THREADS) lh[b] = 0;
    __syncthreads();
    const int t = blockIdx.x * NSS_LEVEL_THREADS + threadIdx.x;
    if (t < n) { const unsigned short b = bkt[base ? base[t] : t]; atomicAdd(&lh[b == NSS_NONE ? nb : (int)b], 1); }
    __syncthreads();
    for (int b = threadIdx.x; b <= nb; b += NSS_LEVEL_THREADS) table[(size_t)b * nblocks + blockIdx.x] = lh[b];
}
__global__ __launch_bounds__(NSS_LEVEL_THREADS) void k_nss_level_scatter(const int* __restrict__ base, int n, const unsigned short* __restrict__ bkt, int nb,
                                                                         const int* __restrict__ table, int nblocks, int* __restrict__ cand) {
    __shared__ unsigned short lb[NSS_LEVEL_THREADS];
    const int t = blockIdx.x * NSS_LEVEL_THREADS + threadIdx.x;
    int i = 0; unsigned short b = NSS_NONE;
    if (t < n) { i = base ? base[t] : t; b = bkt[i]; }
    lb[threadIdx.x] = b;
    __syncthreads();
    if (b == NSS_NONE) return;
    int rank = 0;                                            // of this point among the block's earlier points of the same bucket: stable
    for (int j = 0; j < (int)threadIdx.x; j++) rank += lb[j] == b ? 1 : 0;
    cand[table[(size_t)b * nblocks + blockIdx.x] + rank] = i;
}
// The long segments of a level: n_long, then per long segment its bucket and the first of its chunks (chunk0[n_long] = all chunks).
struct NssLongs { int n_long; int bucket[NSS_MAX_BUCKETS]; int chunk0[NSS_MAX_BUCKETS + 1]; };
// seg[b] = start of bucket b in cand, seg[nb] = m (the candidates), from the scanned table; one block.
__global__ __launch_bounds__(NSS_QUOTA_THREADS) void k_nss_level_segs(const int* __restrict__ table, int nblocks, int nb, int* __restrict__ seg, NssLongs* __restrict__ longs) {
    __shared__ int s[NSS_MAX_BUCKETS + 1];
    const int t = threadIdx.x;
    if (t <= nb) { s[t] = table[(size_t)t * nblocks]; seg[t] = s[t]; }
    __syncthreads();
    if (t != 0) return;
    int k = 0, chunks = 0;
    for (int b = 0; b < nb; b++) {
        const int cnt = s[b + 1] - s[b];
        if (cnt > NSS_LONG) { longs->bucket[k] = b; longs->chunk0[k] = chunks; chunks += (cnt + NSS_CHUNK - 1) / NSS_CHUNK; k++; }
    }
    longs->chunk0[k] = chunks; longs->n_long = k;
}

// ---- per draw ----
template <int N> __device__ __forceinline__ int nss_block_sum(int v, int* red) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, WAVE);
    __syncthreads();                                         // (red is free again)
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    int s = 0;
#pragma unroll
    for (int w = 0; w < N / WAVE; w++) s += red[w];
    return s;
}
// One block per draw: M = clamp(ceil((double)proba * m), 0, m); c = the smallest cap with sum min(cnt_b, c) >= M; q_b = min(cnt_b, c); the
// excess E = sum q_b - M (< the number of capped buckets, by the minimality of c) is taken one each from the E buckets with cnt_b >= c whose key
// select_hash(seed, iteration, 0x80000000 | b) is smallest.  thr: 0xFFFFFFFF for a bucket taken whole; k_nss_select_* fill in the others.
__global__ __launch_bounds__(NSS_QUOTA_THREADS) void k_nss_quota(const int* __restrict__ seg, int nb, float proba, uint32_t seed, uint32_t word0,
                                                                 unsigned int* __restrict__ quota, unsigned int* __restrict__ thr) {
    __shared__ int red[NSS_QUOTA_THREADS / WAVE];
    __shared__ unsigned int key[NSS_MAX_BUCKETS];
    __shared__ unsigned char elig[NSS_MAX_BUCKETS];
    const int t = threadIdx.x, d = blockIdx.x;
    const uint32_t word = word0 + (uint32_t)d;
    const int cnt = t < nb ? seg[t + 1] - seg[t] : 0, m = seg[nb];
    int M = 0;
    if (m > 0) { const double v = (double)proba * (double)m; M = !(v > 0.0) ? 0 : (v >= (double)m ? m : (int)ceil(v)); }
    int c = 0;
    if (M > 0) {                                             // (uniform over the block)
        int lo = 0, hi = m;                                  // sum min(cnt, lo) < M <= sum min(cnt, hi)
        while (hi - lo > 1) {
            const int mid = lo + (hi - lo) / 2;
            if (nss_block_sum<NSS_QUOTA_THREADS>(cnt < mid ? cnt : mid, red) >= M) hi = mid; else lo = mid;
        }
        c = hi;
    }
    int q = cnt < c ? cnt : c;
    const int E = nss_block_sum<NSS_QUOTA_THREADS>(q, red) - M;
    const bool capped = c > 0 && cnt >= c;
    const unsigned int mykey = select_hash(seed, word, 0x80000000u | (uint32_t)t);
    if (t < nb) { key[t] = mykey; elig[t] = capped ? 1 : 0; }
    __syncthreads();
    if (capped) {
        int rank = 0;
        for (int j = 0; j < nb; j++) rank += (elig[j] && key[j] < mykey) ? 1 : 0;
        if (rank < E) q--;
    }
    if (t < nb) { quota[(size_t)d * NSS_ROW + t] = (unsigned int)q; thr[(size_t)d * NSS_ROW + t] = q == cnt ? 0xFFFFFFFFu : 0u; }
}

// The bin of the rank-th smallest (1-based) entry of a 2048-bin histogram and the entries in front of that bin; one block of NSS_THREADS.
__device__ __forceinline__ void nss_find(const unsigned int* h, unsigned int rank, unsigned int* scan, unsigned int* res, unsigned int& bin, unsigned int& before) {
    constexpr int PER = NSS_BINS / NSS_THREADS;
    const int tid = threadIdx.x;
    unsigned int a = 0;
#pragma unroll
    for (int q = 0; q < PER; q++) a += h[tid * PER + q];
    scan[tid] = a;
    if (tid < 2) res[tid] = 0u;
    __syncthreads();
    for (int off = 1; off < NSS_THREADS; off <<= 1) {
        const unsigned int x = tid >= off ? scan[tid - off] : 0u;
        __syncthreads();
        scan[tid] += x;
        __syncthreads();
    }
    const unsigned int inc = scan[tid];
    if (inc - a < rank && rank <= inc) {
        unsigned int cum = inc - a; int q = 0;
        while (q < PER - 1 && cum + h[tid * PER + q] < rank) { cum += h[tid * PER + q]; q++; }
        res[0] = (unsigned int)(tid * PER + q); res[1] = cum;
    }
    __syncthreads();
    bin = res[0]; before = res[1];
    __syncthreads();
}
// digit PASS (1: bits 31..21, 2: bits 20..10, 3: bits 9..0) of a key whose higher bits equal `prefix`; -1 otherwise
template <int PASS> __device__ __forceinline__ int nss_digit(unsigned int key, unsigned int prefix) {
    if (PASS == 1) return (int)(key >> 21);
    if (PASS == 2) return (key >> 21) == prefix ? (int)((key >> 10) & 0x7FFu) : -1;
    return (key >> 10) == prefix ? (int)(key & 0x3FFu) : -1;
}
template <int PASS> __device__ __forceinline__ void nss_hist_range(const int* __restrict__ cand, int lo, int hi, uint32_t seed, uint32_t word, unsigned int prefix, unsigned int* lh) {
    for (int b = threadIdx.x; b < NSS_BINS; b += NSS_THREADS) lh[b] = 0u;
    __syncthreads();
    for (int k = lo + (int)threadIdx.x; k < hi; k += NSS_THREADS) {
        const int dg = nss_digit<PASS>(select_hash(seed, word, (uint32_t)cand[k]), prefix);
        if (dg >= 0) atomicAdd(&lh[dg], 1u);
    }
    __syncthreads();
}
// grid (nb, draws): the threshold of one bucket of one draw, when its segment is short and neither empty-handed nor taken whole
__global__ __launch_bounds__(NSS_THREADS) void k_nss_select_small(const int* __restrict__ cand, const int* __restrict__ seg, uint32_t seed, uint32_t word0,
                                                                  const unsigned int* __restrict__ quota, unsigned int* __restrict__ thr) {
    __shared__ unsigned int lh[NSS_BINS], scan[NSS_THREADS], res[2];
    const int b = blockIdx.x, d = blockIdx.y;
    const int lo = seg[b], hi = seg[b + 1], cnt = hi - lo;
    const unsigned int q = quota[(size_t)d * NSS_ROW + b];
    if (q == 0u || q == (unsigned int)cnt || cnt > NSS_LONG) return;      // (uniform over the block)
    const uint32_t word = word0 + (uint32_t)d;
    unsigned int rank = q, bin, before, prefix;
    nss_hist_range<1>(cand, lo, hi, seed, word, 0u, lh);
    nss_find(lh, rank, scan, res, bin, before); prefix = bin; rank -= before;
    nss_hist_range<2>(cand, lo, hi, seed, word, prefix, lh);
    nss_find(lh, rank, scan, res, bin, before); prefix = (prefix << 11) | bin; rank -= before;
    nss_hist_range<3>(cand, lo, hi, seed, word, prefix, lh);
    nss_find(lh, rank, scan, res, bin, before);
    if (threadIdx.x == 0) thr[(size_t)d * NSS_ROW + b] = (prefix << 10) | bin;
}
// The select of a long segment, pass by pass: state and histogram of (draw d, long segment k) at index d * max_long + k.
struct NssLongState { unsigned int prefix, rank; };
// grid (chunks, draws): one chunk's digits into the segment's global histogram (left cleared by the pick of the pass before)
template <int PASS>
__global__ __launch_bounds__(NSS_THREADS) void k_nss_long_hist(const int* __restrict__ cand, const int* __restrict__ seg, const NssLongs* __restrict__ longs, int max_long,
                                                               uint32_t seed, uint32_t word0, const unsigned int* __restrict__ quota,
                                                               const NssLongState* __restrict__ state, unsigned int* __restrict__ hist) {
    __shared__ unsigned int lh[NSS_BINS];
    const int x = blockIdx.x, d = blockIdx.y, nl = longs->n_long;
    if (nl > max_long || x >= longs->chunk0[nl]) return;
    int k = 0;
    while (k + 1 < nl && longs->chunk0[k + 1] <= x) k++;
    const int b = longs->bucket[k];
    const int s0 = seg[b], s1 = seg[b + 1];
    const unsigned int q = quota[(size_t)d * NSS_ROW + b];
    if (q == 0u || q == (unsigned int)(s1 - s0)) return;
    const int lo = s0 + (x - longs->chunk0[k]) * NSS_CHUNK, hi = lo + NSS_CHUNK < s1 ? lo + NSS_CHUNK : s1;
    const size_t slot = (size_t)d * max_long + k;
    nss_hist_range<PASS>(cand, lo, hi, seed, word0 + (uint32_t)d, PASS == 1 ? 0u : state[slot].prefix, lh);
    unsigned int* gh = hist + slot * NSS_BINS;
    for (int i = threadIdx.x; i < NSS_BINS; i += NSS_THREADS) { const unsigned int v = lh[i]; if (v) atomicAdd(gh + i, v); }
}
// grid (max_long, draws): the digit of the pass from the segment's histogram, which is cleared for the next pass; PASS 3 writes t_b
template <int PASS>
__global__ __launch_bounds__(NSS_THREADS) void k_nss_long_pick(const int* __restrict__ seg, const NssLongs* __restrict__ longs, int max_long,
                                                               const unsigned int* __restrict__ quota, NssLongState* __restrict__ state,
                                                               unsigned int* __restrict__ hist, unsigned int* __restrict__ thr) {
    __shared__ unsigned int lh[NSS_BINS], scan[NSS_THREADS], res[2];
    const int k = blockIdx.x, d = blockIdx.y, nl = longs->n_long;
    if (nl > max_long || k >= nl) return;
    const int b = longs->bucket[k];
    const unsigned int q = quota[(size_t)d * NSS_ROW + b];
    if (q == 0u || q == (unsigned int)(seg[b + 1] - seg[b])) return;
    const size_t slot = (size_t)d * max_long + k;
    unsigned int* gh = hist + slot * NSS_BINS;
    for (int i = threadIdx.x; i < NSS_BINS; i += NSS_THREADS) { lh[i] = gh[i]; gh[i] = 0u; }
    const NssLongState st = PASS == 1 ? NssLongState{0u, q} : state[slot];
    __syncthreads();
    unsigned int bin, before;
    nss_find(lh, st.rank, scan, res, bin, before);
    if (threadIdx.x == 0) {
        if (PASS == 3) thr[(size_t)d * NSS_ROW + b] = (st.prefix << 10) | bin;
        else state[slot] = NssLongState{PASS == 1 ? bin : (st.prefix << 11) | bin, st.rank - before};
    }
}

// ---- the draw's list: the base set's points with hash <= t_b, in increasing original index (k_select_count / scan / scatter's pattern,
// every draw of a level in one grid: blockIdx.y = draw; block offsets of draw d at block_counts + d * stride) ----
__device__ __forceinline__ bool nss_keep(const int* __restrict__ base, int n, int t, const unsigned short* __restrict__ bkt, uint32_t seed, uint32_t word,
                                         const unsigned int* __restrict__ quota, const unsigned int* __restrict__ thr, int& i) {
    if (t >= n) return false;
    i = base ? base[t] : t;
    const unsigned short b = bkt[i];
    if (b == NSS_NONE || quota[b] == 0u) return false;
    return select_hash(seed, word, (uint32_t)i) <= thr[b];
}
__global__ __launch_bounds__(256) void k_nss_count(const int* __restrict__ base, int n, const unsigned short* __restrict__ bkt, uint32_t seed, uint32_t word0,
                                                   const unsigned int* __restrict__ quota, const unsigned int* __restrict__ thr, int* __restrict__ block_counts, int stride) {
    const int d = blockIdx.y; int i;
    const bool keep = nss_keep(base, n, blockIdx.x * 256 + threadIdx.x, bkt, seed, word0 + (uint32_t)d, quota + (size_t)d * NSS_ROW, thr + (size_t)d * NSS_ROW, i);
    const int c = __syncthreads_count(keep ? 1 : 0);
    if (threadIdx.x == 0) block_counts[(size_t)d * stride + blockIdx.x] = c;
}
__global__ __launch_bounds__(1024) void k_nss_scan(int* __restrict__ block_counts, int nblocks, int stride, int* __restrict__ totals) {
    __shared__ int carry;
    __shared__ int tmp[1024];
    int* bc = block_counts + (size_t)blockIdx.x * stride;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    for (int b0 = 0; b0 < nblocks; b0 += 1024) {
        const int b = b0 + threadIdx.x;
        const int v = b < nblocks ? bc[b] : 0;
        tmp[threadIdx.x] = v;
        __syncthreads();
        for (int off = 1; off < 1024; off <<= 1) {
            const int a = threadIdx.x >= off ? tmp[threadIdx.x - off] : 0;
            __syncthreads();
            tmp[threadIdx.x] += a;
            __syncthreads();
        }
        if (b < nblocks) bc[b] = carry + tmp[threadIdx.x] - v;
        __syncthreads();
        if (threadIdx.x == 1023) carry += tmp[1023];
        __syncthreads();
    }
    if (threadIdx.x == 0) totals[blockIdx.x] = carry;
}
__global__ __launch_bounds__(256) void k_nss_scatter(const int* __restrict__ base, int n, const unsigned short* __restrict__ bkt, uint32_t seed, uint32_t word0,
                                                     const unsigned int* __restrict__ quota, const unsigned int* __restrict__ thr, const int* __restrict__ block_offsets, int stride,
                                                     int* __restrict__ out, size_t out_stride) {
    __shared__ int wave_off[4];
    const int d = blockIdx.y, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int i = 0;
    const bool keep = nss_keep(base, n, blockIdx.x * 256 + threadIdx.x, bkt, seed, word0 + (uint32_t)d, quota + (size_t)d * NSS_ROW, thr + (size_t)d * NSS_ROW, i);
    const unsigned long long m = __ballot(keep);
    const int rank = __builtin_amdgcn_mbcnt_hi((unsigned int)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned int)m, 0u));
    if (lane == 0) wave_off[w] = __popcll(m);
    __syncthreads();
    int off = block_offsets[(size_t)d * stride + blockIdx.x];
    for (int v = 0; v < w; v++) off += wave_off[v];
    if (keep) out[(size_t)d * out_stride + off + rank] = i;
}
