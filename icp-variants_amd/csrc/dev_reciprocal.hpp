// dev_reciprocal.hpp -- reciprocal (mutual nearest-neighbour) correspondence rejection: the "compatibility" test of Rusinkiewicz and Levoy
// (3DIM 2001) as one launch per iteration between the matcher and the post stage (icp_reciprocal_options).
// Part of icp_device.hpp (included from there, inside namespace icpdev); see that file for the build contract.
// ------------------------------------------------------------------------------------------------
// A matched query (original source index i, target t) survives iff i is the (distance, lowest index) argmin over the finite source points
// of the target point taken into the source's frame, q = R^T (t - T).  That is a yes / no question, not a search: the walk over the source's
// BVH starts with best = (d2(i), i) -- the answer a full 1-NN search would have to reach -- never updates it, descends only into boxes whose
// lower bound does not exceed it (pair_lb's operation order and k_normals_knn's slack convention, so a box that holds a rival is never
// skipped) and stops at the first rival.  For a mutual pair the walk visits the boxes that overlap the ball of radius d(i) around q, for a
// many-to-one pair it ends in the first leaf that holds a closer source point.
// The kernel calls only __forceinline__ helpers: an existing kernel keeps exactly the code it had.
struct RecipParams {
    icp_match_t* matches;                         // [n] the matcher's records, by query
    int n;
    const int* order;                             // Morton order of the queries (position -> query; nullptr: identity)
    const int* sel;                               // query -> index in the query cloud (nullptr: identity)
    const int* src_orig;                          // a Morton-sorted level: index in the query cloud -> original source index (nullptr: identity)
    const float* tx; const float* ty; const float* tz;      // target planes by original index
    const PoseState* ps;                          // the pose the matcher searched at
    int tree_depth;                               // binary levels of the source tree
    icp_reciprocal_stats* stats;                  // this iteration's record, zero before the launch
};

// bv: the BVH over the full-resolution resident source; bv.tgt = the source planes by original index.
__global__ __launch_bounds__(BVH_THREADS) void k_reciprocal(const RecipParams rp, const BvhViewT<3> bv) {
    extern __shared__ unsigned short bvh_lb16[];
    __shared__ int red[2][BVH_THREADS / WAVE];
    const int tid = threadIdx.x;
    const int t = xcd_contiguous_block(blockIdx.x, gridDim.x) * BVH_THREADS + tid;
    bool judged = false, rival = false;
    int k = -1;
    if (t < rp.n) {
        k = rp.order ? rp.order[t] : t;
        const int j0 = rp.matches[k].idx;
        if (j0 >= 0) {
            judged = true;
            int i = rp.sel ? rp.sel[k] : k;
            if (rp.src_orig) i = rp.src_orig[i];
            const float* __restrict__ P = rp.ps->pose;
            const float ex = rp.tx[j0] - P[12], ey = rp.ty[j0] - P[13], ez = rp.tz[j0] - P[14];
            const float qx = (P[0] * ex + P[1] * ey) + P[2] * ez;
            const float qy = (P[4] * ex + P[5] * ey) + P[6] * ez;
            const float qz = (P[8] * ex + P[9] * ey) + P[10] * ez;
            float best;
            {
                const float dx = qx - bv.tgt.c[0][i], dy = qy - bv.tgt.c[1][i], dz = qz - bv.tgt.c[2][i];
                best = (dx * dx + dy * dy) + dz * dz;
            }
            if (best == best) {                               // (a NaN distance has no rival: nothing compares below it)
                f2 p2[3] = {{qx, qx}, {qy, qy}, {qz, qz}};
                TravState st; st.depth = 0; st.idx = 0; st.pending = 0u; st.alive = true;
                float unused_minlb = FLT_MAX;
                while (st.alive) {
                    while (st.alive && st.depth < rp.tree_depth) {
                        const f2 l = pair_lb<3>(bv.nodes + ((1 << st.depth) - 1 + st.idx), p2);
                        const bool swap = l.y < l.x;
                        const float ln = swap ? l.y : l.x, lf = swap ? l.x : l.y;
                        const bool take_near = !(ln * 0.99999f > best), take_far = !(lf * 0.99999f > best);
                        if (take_near) {
                            if (take_far) { bvh_lb16[st.depth * BVH_THREADS + tid] = (unsigned short)(__float_as_uint(lf) >> 16); st.pending |= 1u << st.depth; }
                            st.idx = 2 * st.idx + (swap ? 1 : 0); st.depth++;
                        } else st.alive = false;
                        trav_pop(st, bvh_lb16, tid, BVH_THREADS, best, unused_minlb);
                    }
                    if (st.alive && st.idx * BVH_LEAF < bv.n_valid) {      // (best = +inf descends into empty boxes too: no leaf is stored behind the last point)
                        const BvhLeafT<3>* __restrict__ lf = bv.leaves + st.idx;
#pragma unroll 1
                        for (int h = 0; h < BVH_LEAF; h += 4) {          // two rounds of four slots: half the loads in flight, half the registers
#pragma unroll
                            for (int s = 0; s < 4; s++) {
                                const float dx = qx - lf->c[0][h + s], dy = qy - lf->c[1][h + s], dz = qz - lf->c[2][h + s];
                                const float d = (dx * dx + dy * dy) + dz * dz;
                                const int j = lf->idx[h + s];
                                rival |= (j >= 0) & ((d < best) | ((d == best) & (j < i)));
                            }
                        }
                        st.alive = false;
                        if (!rival) trav_pop(st, bvh_lb16, tid, BVH_THREADS, best, unused_minlb);      // the first rival ends the walk
                    } else if (st.alive) { st.alive = false; trav_pop(st, bvh_lb16, tid, BVH_THREADS, best, unused_minlb); }
                }
            }
            if (rival) { icp_match_t m; m.idx = -1; m.weight = 0.f; rp.matches[k] = m; }
        }
    }
    // counts: wave ballots, one pair of integer atomics per block (the result does not depend on the order in which blocks arrive)
    const unsigned long long bj = __ballot(judged), bm = __ballot(judged && !rival);
    if ((tid & (WAVE - 1)) == 0) { red[0][tid / WAVE] = __popcll(bj); red[1][tid / WAVE] = __popcll(bm); }
    __syncthreads();
    if (tid == 0) {
        int nj = 0, nm = 0;
#pragma unroll
        for (int w = 0; w < BVH_THREADS / WAVE; w++) { nj += red[0][w]; nm += red[1][w]; }
        if (nj) atomicAdd(&rp.stats->n_matched, nj);
        if (nm) atomicAdd(&rp.stats->n_mutual, nm);
    }
}

// The naive route, for tools/time_reciprocal.py only (icp_debug_reciprocal_naive): the target points of the matched queries taken into the
// source's frame and written out as a query cloud (unmatched queries: NaN, which the matcher leaves unmatched), a full k_knn_bvh search of
// that cloud against the source tree, and k_reciprocal_compare: mutual iff the search came back with the query's own source point.
__global__ void k_reciprocal_queries(const RecipParams rp, float* __restrict__ qx, float* __restrict__ qy, float* __restrict__ qz) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= rp.n) return;
    const int j0 = rp.matches[k].idx;
    float x = NAN, y = NAN, z = NAN;
    if (j0 >= 0) {
        const float* __restrict__ P = rp.ps->pose;
        const float ex = rp.tx[j0] - P[12], ey = rp.ty[j0] - P[13], ez = rp.tz[j0] - P[14];
        x = (P[0] * ex + P[1] * ey) + P[2] * ez; y = (P[4] * ex + P[5] * ey) + P[6] * ez; z = (P[8] * ex + P[9] * ey) + P[10] * ez;
    }
    qx[k] = x; qy[k] = y; qz[k] = z;
}
__global__ __launch_bounds__(BVH_THREADS) void k_reciprocal_compare(const RecipParams rp, const icp_match_t* __restrict__ nn) {
    __shared__ int red[2][BVH_THREADS / WAVE];
    const int tid = threadIdx.x, k = blockIdx.x * BVH_THREADS + tid;
    bool judged = false, rival = false;
    if (k < rp.n && rp.matches[k].idx >= 0) {
        judged = true;
        int i = rp.sel ? rp.sel[k] : k;
        if (rp.src_orig) i = rp.src_orig[i];
        rival = nn[k].idx != i;
        if (rival) { icp_match_t m; m.idx = -1; m.weight = 0.f; rp.matches[k] = m; }
    }
    const unsigned long long bj = __ballot(judged), bm = __ballot(judged && !rival);
    if ((tid & (WAVE - 1)) == 0) { red[0][tid / WAVE] = __popcll(bj); red[1][tid / WAVE] = __popcll(bm); }
    __syncthreads();
    if (tid == 0) {
        int nj = 0, nm = 0;
#pragma unroll
        for (int w = 0; w < BVH_THREADS / WAVE; w++) { nj += red[0][w]; nm += red[1][w]; }
        if (nj) atomicAdd(&rp.stats->n_matched, nj);
        if (nm) atomicAdd(&rp.stats->n_mutual, nm);
    }
}
