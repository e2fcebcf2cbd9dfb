// dev_body_knn_bvh.hpp -- the body of k_knn_bvh, shared text: included by that kernel and by its multi-start sibling (dev_multi.hpp), so that the
// existing kernel compiles to exactly the code it had (a call of a shared inline function reorders its instructions).
    extern __shared__ uint2 bvh_lbq[];                    // [ICP_SHARE_ROWS][BVH_THREADS]: the shared walk's records
    const int tid = threadIdx.x;
    const int k = knn_bvh_lane_query(kp, qorder, tid);
    float best; int bi, bpos;
    knn_bvh_query<DIM>(kp, bv, k, bvh_lbq, tid, best, bi, bpos);
    if (k < 0) return;
    icp_match_t m;
    if (best <= kp.max_dist) { m.idx = bi; m.weight = 1.f; } else { m.idx = -1; m.weight = 0.f; }
    kp.out[k] = m;
