// dev_vmap_prune.hpp -- forgetting cells of the voxel map beyond a radius (icp_voxel_map_prune, icp_track_scans_vmap_local), for both
// storages, and the compaction of a hashed table that has vacated slots.  Contract: include/icp_hip.h, DESIGN.md section 6v;
// tests/vmap_prune_restatement.py states the same rule in numpy.  Part of icp_device.hpp (included from there, inside namespace icpdev,
// after dev_hmap.hpp).
// ------------------------------------------------------------------------------------------------
// A cell is a count and nine integer sums, so a REMOVED cell is one put back into the cleared state bit for bit: count 0, sums 0, an
// all-zero record, stamp 0 -- what create leaves.  A hashed slot keeps its KEY (linear probing cannot delete one without breaking the
// chains that pass it): it is VACATED, probes pass it, a source point that lands in it reads n = 0, and a later insert of that cell finds
// the key and counts a new cell.  Vacated slots are counted (VM_VACATED) so that the room rule can charge them, and k_hmap_compact drops
// them.  Integer atomics and vector stores only; one lane per cell or slot, no loop but hm_claim's bounded probe in the compaction.
constexpr int VM_VACATED = 7;                       // the map's eighth counter: hashed slots vacated since the last compaction
constexpr int VM_PRUNE_AT = 8, VM_CTR_WORDS = 12;   // the counters of ONE prune sit behind the map's eight, in the same buffer (one copy brings both)
struct VmPruneCtr { int n_removed; int pad; unsigned long long n_points; };      // what ONE prune removed (cleared before it)
struct VmSphere { float cx, cy, cz, r2, vs; };

// KEPT iff d2 <= r2, with d_a = ((float)c_a + 0.5f) * vs - centre_a and d2 = (d_x d_x + d_y d_y) + d_z d_z in fp32 (the build does not
// contract).  An infinite r2 keeps everything: d2 is never NaN for a finite centre.
__device__ __forceinline__ bool vm_prune_keeps(const VmSphere& s, int cx, int cy, int cz) {
    const float dx = ((float)cx + 0.5f) * s.vs - s.cx, dy = ((float)cy + 0.5f) * s.vs - s.cy, dz = ((float)cz + 0.5f) * s.vs - s.cz;
    const float d2 = (dx * dx + dy * dy) + dz * dz;
    return d2 <= s.r2;
}
// the cleared state of cell (or slot) i, with plain stores: 4 + 72 + 40 + 4 bytes
__device__ __forceinline__ void vm_clear_cell(size_t i, int* __restrict__ count, long long* __restrict__ sums, float2* __restrict__ cells, int* __restrict__ stamp) {
    count[i] = 0;
#pragma unroll
    for (int a = 0; a < VG_NSUM; a++) sums[i * VG_NSUM + a] = 0;
#pragma unroll
    for (int a = 0; a < 5; a++) cells[i * 5 + a] = make_float2(0.f, 0.f);
    stamp[i] = 0;
}
// The wave's removed cells (a ballot) and removed points (a 64-bit shuffle sum) into the counters: one atomic per wave per counter, and
// none from a wave that removed nothing.  `vacated`: the map is hashed.
__device__ __forceinline__ void vm_prune_count(int lane, bool removed, int n, bool vacated, int* __restrict__ ctr, VmPruneCtr* __restrict__ pc) {
    const unsigned long long br = __ballot(removed);
    if (!br) return;                                   // (uniform)
    long long pts = removed ? (long long)n : 0ll;
    for (int off = WAVE / 2; off > 0; off >>= 1) pts += __shfl_down(pts, off, WAVE);
    if (lane == 0) {
        const int k = __popcll(br);
        atomicAdd(&pc->n_removed, k);
        atomicAdd(&pc->n_points, (unsigned long long)pts);
        atomicSub(&ctr[VM_OCCUPIED], k);
        if (vacated) atomicAdd(&ctr[VM_VACATED], k);
    }
}

// Dense: one cell per lane.  The count is loaded (4 bytes a cell and nothing else for an empty one); a cell with count > 0 decodes its
// coordinates from its index and is tested; a removed cell is cleared.
__global__ __launch_bounds__(256) void k_vmap_prune(const VgGrid g, const VmSphere s, int n_cells, int* __restrict__ count, long long* __restrict__ sums, float2* __restrict__ cells,
                                                    int* __restrict__ stamp, int* __restrict__ ctr, VmPruneCtr* __restrict__ pc) {
    const int i = blockIdx.x * 256 + threadIdx.x, lane = threadIdx.x & 63;
    bool removed = false;
    int n = 0;
    if (i < n_cells) {
        n = count[i];
        if (n > 0) {
            const int x = i % g.dims[0], yz = i / g.dims[0];
            removed = !vm_prune_keeps(s, g.lo[0] + x, g.lo[1] + yz % g.dims[1], g.lo[2] + yz / g.dims[1]);
            if (removed) vm_clear_cell((size_t)i, count, sums, cells, stamp);
        }
    }
    vm_prune_count(lane, removed, n, false, ctr, pc);
}

// Hashed: one slot per lane.  The key is loaded (8 bytes a slot and nothing else for an empty one); an occupied slot loads its count, and
// one with count > 0 is tested with the coordinates from its key.  A removed slot is cleared and KEEPS its key.
__global__ __launch_bounds__(256) void k_hmap_prune(const unsigned long long* __restrict__ keys, int capacity, const VmSphere s, int* __restrict__ count, long long* __restrict__ sums,
                                                    float2* __restrict__ cells, int* __restrict__ stamp, int* __restrict__ ctr, VmPruneCtr* __restrict__ pc) {
    const int i = blockIdx.x * 256 + threadIdx.x, lane = threadIdx.x & 63;
    bool removed = false;
    int n = 0;
    if (i < capacity) {
        const unsigned long long key = keys[i];
        if (key != HM_EMPTY) {
            n = count[i];
            if (n > 0) {
                int c[3];
                hm_unkey(key, c);
                removed = !vm_prune_keeps(s, c[0], c[1], c[2]);
                if (removed) vm_clear_cell((size_t)i, count, sums, cells, stamp);
            }
        }
    }
    vm_prune_count(lane, removed, n, true, ctr, pc);
}

// Compaction: k_hmap_rehash that skips the slots without points, so the vacated keys are not carried into the new table.
__global__ __launch_bounds__(256) void k_hmap_compact(int old_cap, const unsigned long long* __restrict__ old_keys, const int* __restrict__ old_count, const long long* __restrict__ old_sums,
                                                      const float2* __restrict__ old_cells, unsigned long long* __restrict__ keys, int log2cap, int* __restrict__ count,
                                                      long long* __restrict__ sums, float2* __restrict__ cells, int* __restrict__ ctr) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= old_cap) return;
    const unsigned long long key = old_keys[i];
    if (key == HM_EMPTY) return;
    const int n = old_count[i];
    if (n <= 0) return;
    const int slot = hm_claim(keys, log2cap, key);
    if (slot < 0) { atomicAdd(&ctr[VM_UNPLACED], n); return; }
    count[slot] = n;
#pragma unroll
    for (int a = 0; a < VG_NSUM; a++) sums[(size_t)slot * VG_NSUM + a] = old_sums[(size_t)i * VG_NSUM + a];
#pragma unroll
    for (int a = 0; a < 5; a++) cells[(size_t)slot * 5 + a] = old_cells[(size_t)i * 5 + a];
}
