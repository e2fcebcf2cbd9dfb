// dev_tsdf_hash_evict.hpp -- streaming the HASHED TSDF volume: the blocks beyond a radius leave the pool (icp_tsdf_evict_blocks), blocks from
// the host come in beside the resident ones (icp_tsdf_insert_blocks).  Contract: include/icp_hip.h, DESIGN.md section 6za;
// tests/htsdf_evict_restatement.py states the same rule in numpy.  Part of icp_device.hpp (included from there, inside namespace icpdev,
// after dev_tsdf_hash.hpp, whose table, lookup and key helpers are used as they are).
// ------------------------------------------------------------------------------------------------
//   k_htsdf_evict_mark  one lane per pool block: un-key, the predicate, a flag; kept and evicted blocks counted per wave (a ballot, one
//                       atomic per counter per wave); an evicted block takes the next place in the list of evicted blocks, which is also
//                       its place in the outbox.  The host reads the two counters once: n_keep decides everything that follows.
//   k_htsdf_evict_out   one work-group per evicted block: the block and its key into the outbox (hold != 0 only)
//   k_htsdf_evict_plan  one lane per pool block: an evicted block below n_keep is a HOLE, a kept block at or above n_keep a MOVER; each
//                       takes the next place in its list.  There are as many holes as movers: n_keep = kept below + holes = kept below + movers.
//   k_htsdf_evict_move  one work-group per place j of the two lists: mover j into hole j, block and key.  Sources lie at or above n_keep,
//                       destinations below: disjoint, one launch.  Which mover meets which hole depends on the order the two lists filled
//                       in, a race, as where a block sits in the pool already does; what the volume holds does not.
//   k_htsdf_present     one key per lane looked up in the table: the keys that are resident, counted (in front of an insert)
// The pool's tail is cleared and the table rebuilt (k_htsdf_rehash) by the host.  Integer atomics and plain vector stores only.
constexpr int HE_KEEP = 0, HE_EVICT = 1, HE_HOLES = 2, HE_MOVERS = 3, HE_NCTR = 4;
struct HtSphere { float cx, cy, cz, r2, ox, oy, oz, s; };

// KEPT iff d2 <= r2, with p_a = o_a + ((float)(8 b_a) + 3.5f) s the centre of the block's 512 voxel positions, d_a = p_a - centre_a and
// d2 = (d_x d_x + d_y d_y) + d_z d_z in fp32 (the build does not contract).  An infinite r2 keeps everything: d2 is never NaN for a
// finite centre.
__device__ __forceinline__ bool ht_evict_keeps(const HtSphere& q, int bx, int by, int bz) {
    const float px = q.ox + ((float)(8 * bx) + 3.5f) * q.s, py = q.oy + ((float)(8 * by) + 3.5f) * q.s, pz = q.oz + ((float)(8 * bz) + 3.5f) * q.s;
    const float dx = px - q.cx, dy = py - q.cy, dz = pz - q.cz;
    const float d2 = (dx * dx + dy * dy) + dz * dz;
    return d2 <= q.r2;
}

// The place of a lane among the lanes of its wave that raise `mine`, behind the wave's base in counter `ctr`: one atomic per wave, by the
// first lane that raises it, handed round with a shuffle.  Called by every lane of the wave (uniform).
__device__ __forceinline__ int he_take(bool mine, int lane, int* __restrict__ ctr) {
    const unsigned long long b = __ballot(mine);
    if (!b) return 0;                                  // (uniform)
    const int lead = __ffsll((long long)b) - 1;
    int base = 0;
    if (lane == lead) base = atomicAdd(ctr, __popcll(b));
    base = __shfl(base, lead, WAVE);
    return base + __popcll(b & ((1ull << lane) - 1ull));
}

__global__ __launch_bounds__(256) void k_htsdf_evict_mark(int n_blocks, const unsigned long long* __restrict__ pool_key, const HtSphere q, uint8_t* __restrict__ keep,
                                                          int* __restrict__ evicted, int* __restrict__ ec) {
    const int i = blockIdx.x * 256 + threadIdx.x, lane = threadIdx.x & 63;
    bool kept = false, gone = false;
    if (i < n_blocks) {
        int b[3];
        hm_unkey(pool_key[i], b);
        kept = ht_evict_keeps(q, b[0], b[1], b[2]);
        gone = !kept;
        keep[i] = kept ? 1 : 0;
    }
    const unsigned long long bk = __ballot(kept);
    if (bk && lane == 0) atomicAdd(&ec[HE_KEEP], __popcll(bk));
    const int at = he_take(gone, lane, &ec[HE_EVICT]);
    if (gone) evicted[at] = i;                         // (at < n_blocks: the counter ends at the number of evicted blocks)
}

__global__ __launch_bounds__(512) void k_htsdf_evict_out(const float2* __restrict__ pool, const unsigned long long* __restrict__ pool_key, const int* __restrict__ evicted,
                                                         float2* __restrict__ out_pool, unsigned long long* __restrict__ out_key) {
    const int e = blockIdx.x, src = evicted[e];        // (uniform)
    out_pool[(size_t)e * 512 + threadIdx.x] = pool[(size_t)src * 512 + threadIdx.x];
    if (threadIdx.x == 0) out_key[e] = pool_key[src];
}

__global__ __launch_bounds__(256) void k_htsdf_evict_plan(int n_blocks, int n_keep, const uint8_t* __restrict__ keep, int* __restrict__ holes, int* __restrict__ movers,
                                                          int* __restrict__ ec) {
    const int i = blockIdx.x * 256 + threadIdx.x, lane = threadIdx.x & 63;
    bool hole = false, mover = false;
    if (i < n_blocks) {
        const bool kept = keep[i] != 0;
        hole = i < n_keep && !kept;
        mover = i >= n_keep && kept;
    }
    const int ah = he_take(hole, lane, &ec[HE_HOLES]);
    if (hole) holes[ah] = i;
    const int am = he_take(mover, lane, &ec[HE_MOVERS]);
    if (mover) movers[am] = i;
}

// (launched over a bound of the number of movers, min(n_keep, n_evicted): the groups past the plan's count have nothing to do)
__global__ __launch_bounds__(512) void k_htsdf_evict_move(float2* __restrict__ pool, unsigned long long* __restrict__ pool_key, const int* __restrict__ holes,
                                                          const int* __restrict__ movers, const int* __restrict__ ec) {
    const int j = blockIdx.x;
    if (j >= ec[HE_MOVERS]) return;                    // (uniform)
    const int src = movers[j], dst = holes[j];
    pool[(size_t)dst * 512 + threadIdx.x] = pool[(size_t)src * 512 + threadIdx.x];
    if (threadIdx.x == 0) pool_key[dst] = pool_key[src];
}

__global__ __launch_bounds__(256) void k_htsdf_present(const HtVol v, int n, const int* __restrict__ coords, int* __restrict__ n_present) {
    const int i = blockIdx.x * 256 + threadIdx.x, lane = threadIdx.x & 63;
    bool hit = false;
    if (i < n) hit = ht_lookup(v, coords[3 * (size_t)i], coords[3 * (size_t)i + 1], coords[3 * (size_t)i + 2]) >= 0;
    const unsigned long long bh = __ballot(hit);
    if (bh && lane == 0) atomicAdd(n_present, __popcll(bh));
}
