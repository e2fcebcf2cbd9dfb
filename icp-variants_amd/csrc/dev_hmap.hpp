// dev_hmap.hpp -- the HASHED storage of the voxel map: dev_vmap.hpp's per-cell state (a count, nine integer sums, the 40-byte record, a stamp)
// addressed by a hash of the cell's coordinates instead of by its place in a box, so the map has no extent.  Contract: include/icp_hip.h,
// DESIGN.md section 6u; tests/hmap_restatement.py states the same arithmetic in numpy.  Part of icp_device.hpp (included from there, inside
// namespace icpdev, after dev_vmap.hpp).
// ------------------------------------------------------------------------------------------------
// Layout: the 8-byte KEYS are an array of their own (a probe reads nothing else: sixteen keys to a 128-byte line, and a chain of the mean
// length 1.5 stays inside one line); count, sums, record and stamp are dev_vmap.hpp's four arrays, indexed by slot.  Open addressing with
// linear probing; every probe loop is a `for` over at most `capacity` slots.  Where a cell is stored may depend on a race between two
// claims; what it holds is integer sums and does not.  The host keeps capacity >= 2 (occupied + points of the insert), so an insert always
// finds room; a head that finds none is still counted (VM_UNPLACED, which must stay 0).  Integer atomics and vector stores only.
constexpr unsigned long long HM_EMPTY = ~0ull;      // an empty slot: never a key (a key has 63 bits)
constexpr int HM_RANGE = 1 << 20;                   // storable cell coordinates: -2^20 <= c < 2^20 on every axis
constexpr unsigned long long HM_MUL = 0x9E3779B97F4A7C15ull;
constexpr int VM_UNPLACED = 6;                      // the map's seventh counter: points whose cell found no slot, over the map's life
struct HmTable { const unsigned long long* keys; int log2cap; float vs; int min_points; };

__device__ __forceinline__ bool hm_storable(int cx, int cy, int cz) {      // (|c| <= 2^30 by vg_cell_coord: the sums cannot wrap)
    return (unsigned)(cx + HM_RANGE) < 2u * HM_RANGE && (unsigned)(cy + HM_RANGE) < 2u * HM_RANGE && (unsigned)(cz + HM_RANGE) < 2u * HM_RANGE;
}
__device__ __forceinline__ unsigned long long hm_key(int cx, int cy, int cz) {
    return ((unsigned long long)(unsigned)(cz + HM_RANGE) << 42) | ((unsigned long long)(unsigned)(cy + HM_RANGE) << 21) | (unsigned long long)(unsigned)(cx + HM_RANGE);
}
__device__ __forceinline__ void hm_unkey(unsigned long long key, int (&c)[3]) {
    c[0] = (int)(key & 0x1FFFFFull) - HM_RANGE; c[1] = (int)((key >> 21) & 0x1FFFFFull) - HM_RANGE; c[2] = (int)((key >> 42) & 0x1FFFFFull) - HM_RANGE;
}
__device__ __forceinline__ unsigned hm_home(unsigned long long key, int log2cap) { return (unsigned)((key * HM_MUL) >> (64 - log2cap)); }

// The slot that holds `key`, or -1: plain loads (the table was written by earlier launches).  Stops at the first empty slot.
__device__ __forceinline__ int hm_find_from(const unsigned long long* __restrict__ keys, int log2cap, unsigned long long key, unsigned slot, int tried) {
    const unsigned mask = (1u << log2cap) - 1u;
    for (unsigned i = (unsigned)tried; i <= mask; i++) {
        const unsigned long long k = keys[slot];
        if (k == key) return (int)slot;
        if (k == HM_EMPTY) return -1;
        slot = (slot + 1u) & mask;
    }
    return -1;
}
// The slot that holds `key` after this call, or -1 when every slot holds another key.  A relaxed agent-scope load first (keys only ever go
// from empty to a key, so a key read is final and an empty read is settled by the CAS); the claim is a 64-bit atomicCAS(empty -> key),
// and a slot that turns out to hold the key already is accepted.
__device__ __forceinline__ int hm_claim(unsigned long long* __restrict__ keys, int log2cap, unsigned long long key) {
    const unsigned mask = (1u << log2cap) - 1u;
    unsigned slot = hm_home(key, log2cap);
    for (unsigned i = 0; i <= mask; i++) {
        unsigned long long k = __hip_atomic_load(&keys[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (k == HM_EMPTY) {
            k = atomicCAS(&keys[slot], HM_EMPTY, key);
            if (k == HM_EMPTY) return (int)slot;
        }
        if (k == key) return (int)slot;
        slot = (slot + 1u) & mask;
    }
    return -1;
}

// vm_point_terms with the cell's coordinates in place of its index in a box (that function ends in vg_cell_index; the quantisation is its
// text, operation for operation).  Returns the key, or HM_EMPTY for a cell that is not storable: then everything stays 0.
__device__ __forceinline__ unsigned long long hm_point_terms(float vs, const float (&p)[3], const float (&nr)[3], int& cnt, int (&q)[3], long long (&mm)[6]) {
    int c[3];
#pragma unroll
    for (int a = 0; a < 3; a++) {
        c[a] = vg_cell_coord(p[a], vs);
        const float off = ((p[a] - ((float)c[a] + 0.5f) * vs) / vs) * 65536.0f;
        q[a] = (int)lrintf(fminf(fmaxf(off, -32768.0f), 32768.0f));
    }
    if (hm_storable(c[0], c[1], c[2])) {
        cnt = 1;
        long long m[3];
#pragma unroll
        for (int a = 0; a < 3; a++) m[a] = (long long)lrintf(fminf(fmaxf(nr[a], -2.0f), 2.0f) * 16384.0f);
        mm[0] = m[0] * m[0]; mm[1] = m[0] * m[1]; mm[2] = m[0] * m[2]; mm[3] = m[1] * m[1]; mm[4] = m[1] * m[2]; mm[5] = m[2] * m[2];
        return hm_key(c[0], c[1], c[2]);
    }
    q[0] = q[1] = q[2] = 0;
    return HM_EMPTY;
}

// k_vmap_insert with a slot in place of the cell index.  Up to the run sum it is that kernel: the lane moves and tests its point and
// quantises it; runs of equal KEY are numbered (a 64-bit compare with the lane before, a ballot), and vm_run_sum adds each run into its
// head with the run's number as its cell.  Then the head claims or finds its slot -- the divergent probe loop, behind the last shuffle of
// the run sum and with no shuffle or ballot in it -- and goes on as k_vmap_insert does: the count's atomicAdd (old value 0: a new cell),
// the nine 64-bit adds, the stamp's exchange, the wave-aggregated append of first-touched slots, the per-wave counter atomics.
__global__ __launch_bounds__(256) void k_hmap_insert(const VmCloud t, unsigned long long* __restrict__ keys, int log2cap, float vs, const TsdfMat pose, int serial, int list_cap,
                                                     int* __restrict__ count, unsigned long long* __restrict__ sums, int* __restrict__ stamp, int* __restrict__ list, int* __restrict__ ctr) {
    __shared__ float P[16];
    __shared__ float nm[9];
    const int tid = threadIdx.x, lane = tid & 63;
    if (tid < 16) P[tid] = pose.m[tid];
    if (tid >= 64 && tid < 73) nm[tid - 64] = vg_normal_matrix_entry(pose.m, tid - 64);
    __syncthreads();
    const int i = blockIdx.x * 256 + tid;
    unsigned long long key = HM_EMPTY;
    int cnt = 0, q[3] = {0, 0, 0};
    long long mm[6] = {0, 0, 0, 0, 0, 0};
    bool considered = false, entered = false;
    if (i < t.n) {
        const float sx = t.x[i], sy = t.y[i], sz = t.z[i];
        considered = finite3(sx, sy, sz);
        float p[3], nr[3];
        xform_point(P, sx, sy, sz, p[0], p[1], p[2]);
        xform_normal(nm, t.nx[i], t.ny[i], t.nz[i], nr[0], nr[1], nr[2]);
        entered = considered && finite3(p[0], p[1], p[2]) && finite3(nr[0], nr[1], nr[2]);
        if (entered) key = hm_point_terms(vs, p, nr, cnt, q, mm);
    }
    const unsigned long long before = __shfl_up(key, 1, WAVE);
    const unsigned long long starts = __ballot(lane == 0 || before != key);
    const int run = __popcll(starts & (~0ull >> (63 - lane)));
    const bool head = vm_run_sum(lane, run, cnt, q, mm);
    bool fresh = false, first = false;
    int slot = -1;
    if (head && key != HM_EMPTY) {
        slot = hm_claim(keys, log2cap, key);
        if (slot >= 0) {
            fresh = atomicAdd(&count[slot], cnt) == 0;
            vm_sums_add(sums, slot, q, mm);
            first = atomicExch(&stamp[slot], serial) != serial;
        } else atomicAdd(&ctr[VM_UNPLACED], cnt);      // (the room rule excludes it; counted so that it cannot pass unseen)
    }
    const unsigned long long bf = __ballot(first);
    if (bf) {                                          // (uniform) the wave's first touches: one atomic reserves their places in the list
        const int leader = __ffsll((long long)bf) - 1;
        int base = 0;
        if (lane == leader) base = atomicAdd(&ctr[VM_TOUCHED], __popcll(bf));
        base = __shfl(base, leader, WAVE);
        const int at = base + __popcll(bf & ((1ull << lane) - 1ull));
        if (first && at < list_cap) list[at] = slot;
    }
    const int n_considered = __popcll(__ballot(considered)), n_entered = __popcll(__ballot(entered)), n_outside = __popcll(__ballot(entered && key == HM_EMPTY));
    const int n_new = __popcll(__ballot(fresh));
    if (lane < 6 && lane != VM_TOUCHED) {
        const int v = lane == VM_CONSIDERED ? n_considered : lane == VM_ENTERED ? n_entered : lane == VM_OUTSIDE ? n_outside : n_new;      // (VM_NEW and VM_OCCUPIED both take n_new)
        if (v) atomicAdd(&ctr[lane], v);
    }
}

// vg_record with the cell's coordinates given (decoded from the key), its nine sums at `s` and its record at `o`: the same
// fp64 operations on the same integers, each of the nine values rounded once to fp32, five 8-byte stores.
__device__ __forceinline__ void hm_record(float voxel, const int (&c)[3], int n, const long long* __restrict__ s, float2* __restrict__ o) {
    float rec[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (n > 0) {
        const double vs = (double)voxel, dn = (double)n;
#pragma unroll
        for (int a = 0; a < 3; a++) rec[a] = (float)(((double)c[a] + 0.5) * vs + ((double)s[a] / dn) * (vs / 65536.0));
        const long long tr = (s[3] + s[6]) + s[8];
        if (tr > 0) {
            const double dt = (double)tr;
#pragma unroll
            for (int a = 0; a < 6; a++) rec[3 + a] = (float)((double)s[3 + a] / dt);
        }
    }
    o[0] = make_float2(rec[0], rec[1]); o[1] = make_float2(rec[2], rec[3]); o[2] = make_float2(rec[4], rec[5]); o[3] = make_float2(rec[6], rec[7]);
    o[4] = make_float2(rec[8], __int_as_float(n));
}

// The records of the slots the insert touched, one listed slot per lane (k_vmap_records with the coordinates from the key).
__global__ __launch_bounds__(256) void k_hmap_records(const unsigned long long* __restrict__ keys, float vs, int list_cap, const int* __restrict__ ctr, const int* __restrict__ list,
                                                      const int* __restrict__ count, const long long* __restrict__ sums, float2* __restrict__ cells) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= min(ctr[VM_TOUCHED], list_cap)) return;
    const int slot = list[i];
    int c[3];
    hm_unkey(keys[slot], c);
    hm_record(vs, c, count[slot], sums + (size_t)slot * VG_NSUM, cells + (size_t)slot * 5);
}

// k_vgicp_accumulate with the cell found by probing.  The same two points per lane, the same fp64 arithmetic per point operation for
// operation (that kernel's text: sharing it through a function would have to leave its instructions as they are), the same block_reduce_wide
// fold and partials layout, so k_sdf_solve runs behind it as it is.  The lookup: the key of the point's cell, its home slot, and then the
// home slot's KEY AND RECORD loaded together -- six independent loads in flight at once, so a cell that sits in its home slot (more than half
// of them at load 0.5) costs no second round trip.  Only a lane whose home slot holds another key enters the probe loop, and fetches the record
// again from the slot it ends in.  The loop is divergent; no shuffle or ballot in it.
__global__ __launch_bounds__(256) void k_hmap_accumulate(const HmTable g, const float2* __restrict__ cells, const VgSource s, const SdfState* __restrict__ st,
                                                         double* __restrict__ partials, int* __restrict__ counts) {
    __shared__ double lds[4 * SDF_NSUM * 17];
    __shared__ int red[8];
    __shared__ float nm[9];
    if (st->stop) return;                              // (uniform) the alignment has ended: nothing of this launch is needed
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const float* __restrict__ P = st->pose;
    if (tid < 9) nm[tid] = vg_normal_matrix_entry(P, tid);
    __syncthreads();
    double acc[SDF_NSUM];
#pragma unroll
    for (int a = 0; a < SDF_NSUM; a++) acc[a] = 0.0;
    int n_considered = 0, n_valid = 0;
#pragma unroll 1
    for (int j = 0; j < VG_POINTS_PER_LANE; j++) {
        const int i = (blockIdx.x * VG_POINTS_PER_LANE + j) * 256 + tid;
        bool considered = false, valid = false;
        if (i < s.n) {
            const float sx = s.x[i], sy = s.y[i], sz = s.z[i];
            considered = finite3(sx, sy, sz);
            float p0, p1, p2;
            xform_point(P, sx, sy, sz, p0, p1, p2);
            if (considered && finite3(p0, p1, p2)) {
                const int cx = vg_cell_coord(p0, g.vs), cy = vg_cell_coord(p1, g.vs), cz = vg_cell_coord(p2, g.vs);
                if (hm_storable(cx, cy, cz)) {
                    const unsigned long long key = hm_key(cx, cy, cz);
                    const unsigned home = hm_home(key, g.log2cap);
                    const unsigned long long k0 = g.keys[home];
                    const float2* __restrict__ rec = cells + (size_t)home * 5;
                    float2 r0 = rec[0], r1 = rec[1], r2 = rec[2], r3 = rec[3], r4 = rec[4];
                    int slot = k0 == key ? (int)home : -1;
                    if (k0 != key && k0 != HM_EMPTY) {
                        slot = hm_find_from(g.keys, g.log2cap, key, (home + 1u) & ((1u << g.log2cap) - 1u), 1);
                        if (slot >= 0) {
                            rec = cells + (size_t)slot * 5;
                            r0 = rec[0]; r1 = rec[1]; r2 = rec[2]; r3 = rec[3]; r4 = rec[4];
                        }
                    }
                    if (slot >= 0) {
                        const int n = __float_as_int(r4.y);
                        float b0, b1, b2;
                        xform_normal(nm, s.nx[i], s.ny[i], s.nz[i], b0, b1, b2);
                        double b[3];
                        if (n >= g.min_points && gicp_unit(b0, b1, b2, b)) {
                            valid = true;
                            const double ome = s.one_minus_eps, N = (double)n;
                            const double S00 = 2.0 - ome * ((double)r1.y + b[0] * b[0]), S01 = -ome * ((double)r2.x + b[0] * b[1]), S02 = -ome * ((double)r2.y + b[0] * b[2]);
                            const double S11 = 2.0 - ome * ((double)r3.x + b[1] * b[1]), S12 = -ome * ((double)r3.y + b[1] * b[2]), S22 = 2.0 - ome * ((double)r4.x + b[2] * b[2]);
                            const double c00 = S11 * S22 - S12 * S12, c01 = S02 * S12 - S01 * S22, c02 = S01 * S12 - S02 * S11;
                            const double c11 = S00 * S22 - S02 * S02, c12 = S01 * S02 - S00 * S12, c22 = S00 * S11 - S01 * S01;
                            const double det = (S00 * c00 + S01 * c01) + S02 * c02;
                            const double M[3][3] = {{c00 / det, c01 / det, c02 / det}, {c01 / det, c11 / det, c12 / det}, {c02 / det, c12 / det, c22 / det}};
                            const double q0 = p0, q1 = p1, q2 = p2;
                            const double A[3][3] = {{0.0, q2, -q1}, {-q2, 0.0, q0}, {q1, -q0, 0.0}};      // -[p]x
                            const double r[3] = {(double)r0.x - q0, (double)r0.y - q1, (double)r1.x - q2};
                            double MA[3][3], Mr[3];
#pragma unroll
                            for (int a = 0; a < 3; a++) {
#pragma unroll
                                for (int c = 0; c < 3; c++) MA[a][c] = (M[a][0] * A[0][c] + M[a][1] * A[1][c]) + M[a][2] * A[2][c];
                                Mr[a] = (M[a][0] * r[0] + M[a][1] * r[1]) + M[a][2] * r[2];
                            }
                            int k = 0;
#pragma unroll
                            for (int a = 0; a < 6; a++) {
#pragma unroll
                                for (int c = a; c < 6; c++) {
                                    double h;
                                    if (a < 3 && c < 3) h = (A[0][a] * MA[0][c] + A[1][a] * MA[1][c]) + A[2][a] * MA[2][c];      // A^T M A
                                    else if (a < 3) h = MA[c - 3][a];                                                              // A^T M
                                    else h = M[a - 3][c - 3];
                                    acc[k++] += N * h;
                                }
                            }
#pragma unroll
                            for (int a = 0; a < 3; a++) acc[21 + a] += N * ((A[0][a] * Mr[0] + A[1][a] * Mr[1]) + A[2][a] * Mr[2]);
#pragma unroll
                            for (int a = 0; a < 3; a++) acc[24 + a] += N * Mr[a];
                            acc[27] += N * ((r[0] * Mr[0] + r[1] * Mr[1]) + r[2] * Mr[2]);
                        }
                    }
                }
            }
        }
        const unsigned long long bu = __ballot(considered), bv = __ballot(valid);
        n_considered += __popcll(bu); n_valid += __popcll(bv);
    }
    if (lane == 0) { red[2 * wave] = n_considered; red[2 * wave + 1] = n_valid; }
    const double tot = block_reduce_wide<SDF_NSUM, 4>(acc, lds);      // (its barrier also covers red)
    const int nb = gridDim.x, blk = blockIdx.x;
    if (tid < SDF_NSUM) partials[(size_t)tid * nb + blk] = tot;
    if (tid >= 64 && tid < 66) { const int q = tid - 64; counts[(size_t)q * nb + blk] = (red[q] + red[2 + q]) + (red[4 + q] + red[6 + q]); }
}

// Growth: one slot of the old table per lane.  An occupied slot's key is claimed in the new table (CAS: two old slots never hold one key,
// but two lanes may want one new slot), then its count, nine sums and 40-byte record are copied with plain stores; the new table's stamps
// stay 0.  An occupied slot that finds no room is counted (the new table is larger: it cannot happen).
__global__ __launch_bounds__(256) void k_hmap_rehash(int old_cap, const unsigned long long* __restrict__ old_keys, const int* __restrict__ old_count, const long long* __restrict__ old_sums,
                                                     const float2* __restrict__ old_cells, unsigned long long* __restrict__ keys, int log2cap, int* __restrict__ count,
                                                     long long* __restrict__ sums, float2* __restrict__ cells, int* __restrict__ ctr) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= old_cap) return;
    const unsigned long long key = old_keys[i];
    if (key == HM_EMPTY) return;
    const int slot = hm_claim(keys, log2cap, key);
    if (slot < 0) { atomicAdd(&ctr[VM_UNPLACED], old_count[i]); return; }
    count[slot] = old_count[i];
#pragma unroll
    for (int a = 0; a < VG_NSUM; a++) sums[(size_t)slot * VG_NSUM + a] = old_sums[(size_t)i * VG_NSUM + a];
#pragma unroll
    for (int a = 0; a < 5; a++) cells[(size_t)slot * 5 + a] = old_cells[(size_t)i * 5 + a];
}

// Upload: one entry (three coordinates, a count > 0, nine sums; the host has refused duplicates and cells that are not storable) per
// lane: its key is claimed, its state stored, its record computed; the occupied cells are counted per wave.
__global__ __launch_bounds__(256) void k_hmap_place(int n, const int* __restrict__ coords, const int* __restrict__ in_count, const long long* __restrict__ in_sums, float vs,
                                                    unsigned long long* __restrict__ keys, int log2cap, int* __restrict__ count, long long* __restrict__ sums,
                                                    float2* __restrict__ cells, int* __restrict__ ctr) {
    const int i = blockIdx.x * 256 + threadIdx.x, lane = threadIdx.x & 63;
    bool placed = false;
    if (i < n && in_count[i] > 0) {
        const int c[3] = {coords[3 * (size_t)i], coords[3 * (size_t)i + 1], coords[3 * (size_t)i + 2]};
        const int slot = hm_claim(keys, log2cap, hm_key(c[0], c[1], c[2]));
        if (slot < 0) atomicAdd(&ctr[VM_UNPLACED], in_count[i]);
        else {
            placed = true;
            count[slot] = in_count[i];
#pragma unroll
            for (int a = 0; a < VG_NSUM; a++) sums[(size_t)slot * VG_NSUM + a] = in_sums[(size_t)i * VG_NSUM + a];
            hm_record(vs, c, in_count[i], in_sums + (size_t)i * VG_NSUM, cells + (size_t)slot * 5);
        }
    }
    const unsigned long long bp = __ballot(placed);
    if (lane == 0 && bp) atomicAdd(&ctr[VM_OCCUPIED], __popcll(bp));
}
