// dev_vmap.hpp -- the voxel map of scan-to-map laser tracking: dev_vgicp.hpp's grid of cells as PERSISTENT state with a fixed extent, which a
// scan is fused into at a pose (k_vmap_insert, k_vmap_records) and aligned to by k_vgicp_accumulate as it is.  Contract: include/icp_hip.h,
// DESIGN.md section 6t; tests/vmap_restatement.py states the same arithmetic in numpy.  Part of icp_device.hpp (included from there, inside
// namespace icpdev, after dev_vgicp.hpp).
// ------------------------------------------------------------------------------------------------
// The per-cell state is section 6s's: a count and nine INTEGER sums, so fusing another scan is exact in any order and keeps its bits; the
// 40-byte record is vg_record's function of them.  An insert recomputes the records of the cells it touched and of no other: a per-cell
// stamp holds the serial number of the last insert that touched the cell, and the first run head to stamp a cell appends it to a list.
// No floating-point atomics, no host read between the two launches.
struct VmCloud { const float* x; const float* y; const float* z; const float* nx; const float* ny; const float* nz; int n; };
// counters of the map, in icp_voxel_map_insert_info's order: the first five belong to the insert in flight (cleared before it), the
// sixth runs on.  VM_TOUCHED is also the length of the list.
constexpr int VM_CONSIDERED = 0, VM_ENTERED = 1, VM_OUTSIDE = 2, VM_TOUCHED = 3, VM_NEW = 4, VM_OCCUPIED = 5, VM_NCTR = 8;

// The next three functions are k_vg_cells_add's text, operation for operation: the quantisation of one point, the segmented shuffle sum over
// the runs of equal cell, the nine 64-bit atomics of a run's head.  That kernel keeps its own copy: calling these from it changed its
// instruction schedule (the quantisation alone) and added 86 lines of assembly (the segmented sum), and section 6t promises it unchanged.
//
// What one entering point adds to its cell: the cell's index in g (or -1 outside), and then cnt = 1, the three quantised offsets from the
// cell's centre and the six products of the quantised normal components; outside, everything stays 0.
__device__ __forceinline__ int vm_point_terms(const VgGrid& g, float vs, const float (&p)[3], const float (&nr)[3], int& cnt, int (&q)[3], long long (&mm)[6]) {
    int c[3];
#pragma unroll
    for (int a = 0; a < 3; a++) {
        c[a] = vg_cell_coord(p[a], vs);
        const float off = ((p[a] - ((float)c[a] + 0.5f) * vs) / vs) * 65536.0f;
        q[a] = (int)lrintf(fminf(fmaxf(off, -32768.0f), 32768.0f));
    }
    const int cell = vg_cell_index(g.lo, g.dims, c[0], c[1], c[2]);
    if (cell >= 0) {
        cnt = 1;
        long long m[3];
#pragma unroll
        for (int a = 0; a < 3; a++) m[a] = (long long)lrintf(fminf(fmaxf(nr[a], -2.0f), 2.0f) * 16384.0f);
        mm[0] = m[0] * m[0]; mm[1] = m[0] * m[1]; mm[2] = m[0] * m[2]; mm[3] = m[1] * m[1]; mm[4] = m[1] * m[2]; mm[5] = m[2] * m[2];
    } else { q[0] = q[1] = q[2] = 0; }
    return cell;
}
// Runs: a lane heads one when its cell differs from the lane before it; run = how many heads lie at or below the lane.  A segmented
// shuffle sum adds each run's ten values into its head.  Returns whether the lane is a head.
__device__ __forceinline__ bool vm_run_sum(int lane, int cell, int& cnt, int (&q)[3], long long (&mm)[6]) {
    const int prev = __shfl_up(cell, 1, WAVE);
    const bool head = lane == 0 || prev != cell;
    const unsigned long long heads = __ballot(head);
    const int run = __popcll(heads & (~0ull >> (63 - lane)));
    for (int off = 1; off < WAVE; off <<= 1) {
        const bool same = __shfl_down(run, off, WAVE) == run && lane + off < WAVE;
        const int oc = __shfl_down(cnt, off, WAVE);
        int oq[3]; long long om[6];
#pragma unroll
        for (int a = 0; a < 3; a++) oq[a] = __shfl_down(q[a], off, WAVE);
#pragma unroll
        for (int a = 0; a < 6; a++) om[a] = __shfl_down(mm[a], off, WAVE);
        if (same) {
            cnt += oc;
#pragma unroll
            for (int a = 0; a < 3; a++) q[a] += oq[a];       // (at most 64 x 32768)
#pragma unroll
            for (int a = 0; a < 6; a++) mm[a] += om[a];
        }
    }
    return head;
}
// the nine 64-bit integer atomics of one run's head
__device__ __forceinline__ void vm_sums_add(unsigned long long* __restrict__ sums, int cell, const int (&q)[3], const long long (&mm)[6]) {
    unsigned long long* s = sums + (size_t)cell * VG_NSUM;
#pragma unroll
    for (int a = 0; a < 3; a++) atomicAdd(&s[a], (unsigned long long)(long long)q[a]);
#pragma unroll
    for (int a = 0; a < 6; a++) atomicAdd(&s[3 + a], (unsigned long long)mm[a]);
}

// One point per lane.  The pose and the nine entries of its normal matrix go to LDS once per block (k_vgicp_accumulate's entries); the lane
// moves its point and its normal, tests them, and quantises them as k_vg_cells_add does (vm_point_terms); vm_run_sum adds every run of equal
// cell into its head, and the head issues the count's atomicAdd and the nine 64-bit ones.  The count's old value tells the head whether
// the cell is new; the stamp's old value whether this insert has been here before.  First touches are appended to `list` with one atomic
// per wave; the five counters take one atomic instruction per wave (five lanes, one counter each, zeros left out).
__global__ __launch_bounds__(256) void k_vmap_insert(const VmCloud t, const VgGrid g, const TsdfMat pose, int serial, int list_cap, int* __restrict__ count,
                                                     unsigned long long* __restrict__ sums, int* __restrict__ stamp, int* __restrict__ list, int* __restrict__ ctr) {
    __shared__ float P[16];
    __shared__ float nm[9];
    const int tid = threadIdx.x, lane = tid & 63;
    if (tid < 16) P[tid] = pose.m[tid];
    if (tid >= 64 && tid < 73) nm[tid - 64] = vg_normal_matrix_entry(pose.m, tid - 64);
    __syncthreads();
    const int i = blockIdx.x * 256 + tid;
    int cell = -1, cnt = 0, q[3] = {0, 0, 0};
    long long mm[6] = {0, 0, 0, 0, 0, 0};
    bool considered = false, entered = false;
    if (i < t.n) {
        const float sx = t.x[i], sy = t.y[i], sz = t.z[i];
        considered = finite3(sx, sy, sz);
        float p[3], nr[3];
        xform_point(P, sx, sy, sz, p[0], p[1], p[2]);
        xform_normal(nm, t.nx[i], t.ny[i], t.nz[i], nr[0], nr[1], nr[2]);
        entered = considered && finite3(p[0], p[1], p[2]) && finite3(nr[0], nr[1], nr[2]);
        if (entered) cell = vm_point_terms(g, g.vs, p, nr, cnt, q, mm);
    }
    const bool head = vm_run_sum(lane, cell, cnt, q, mm);
    bool fresh = false, first = false;
    if (head && cell >= 0) {
        fresh = atomicAdd(&count[cell], cnt) == 0;
        vm_sums_add(sums, cell, q, mm);
        first = atomicExch(&stamp[cell], serial) != serial;
    }
    const unsigned long long bf = __ballot(first);
    if (bf) {                                          // (uniform) the wave's first touches: one atomic reserves their slots
        const int leader = __ffsll((long long)bf) - 1;
        int base = 0;
        if (lane == leader) base = atomicAdd(&ctr[VM_TOUCHED], __popcll(bf));
        base = __shfl(base, leader, WAVE);
        const int slot = base + __popcll(bf & ((1ull << lane) - 1ull));
        if (first && slot < list_cap) list[slot] = cell;      // (first touches are distinct cells from distinct points: never more than list_cap)
    }
    const int n_considered = __popcll(__ballot(considered)), n_entered = __popcll(__ballot(entered)), n_outside = __popcll(__ballot(entered && cell < 0));
    const int n_new = __popcll(__ballot(fresh));
    if (lane < 6 && lane != VM_TOUCHED) {
        const int v = lane == VM_CONSIDERED ? n_considered : lane == VM_ENTERED ? n_entered : lane == VM_OUTSIDE ? n_outside : n_new;      // (VM_NEW and VM_OCCUPIED both take n_new)
        if (v) atomicAdd(&ctr[lane], v);
    }
}

// The records of the cells the insert touched, one listed cell per lane: the length of the list is read from device memory, lanes past it
// leave.  vg_record is k_vg_finalise's arithmetic.
__global__ __launch_bounds__(256) void k_vmap_records(const VgGrid g, int list_cap, const int* __restrict__ ctr, const int* __restrict__ list, const int* __restrict__ count,
                                                      const long long* __restrict__ sums, float2* __restrict__ cells) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= min(ctr[VM_TOUCHED], list_cap)) return;
    const int cell = list[i];
    vg_record(g, cell, count[cell], sums, cells);
}
