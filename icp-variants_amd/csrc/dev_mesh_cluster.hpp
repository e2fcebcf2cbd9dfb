// dev_mesh_cluster.hpp -- vertex clustering of an indexed triangle mesh (Rossignac and Borrel 1993): the vertices of one grid cell become one
// vertex, triangles that lose a corner that way are dropped, triangles that become equal are kept once.  Contract: include/icp_hip.h,
// DESIGN.md section 6zk; tests/mesh_cluster_restatement.py states the same arithmetic in numpy.  Part of icp_device.hpp (included from
// there, inside namespace icpdev, after dev_hmap.hpp, whose key and home functions the cell table uses).
// ------------------------------------------------------------------------------------------------
// No sort and no floating-point atomic.  Two open-addressed tables with linear probing, every probe loop a `for` over at most the table's
// slots.  The CELL table (dev_hmap.hpp's idiom): 64-bit keys claimed by atomicCAS, per slot the cluster's first member (atomicMin of the
// vertex index) and a word that is first the "referenced" flag and later rank + 1.  The TRIANGLE table: a slot holds a TRIANGLE INDEX,
// claimed by CAS; a collision compares the occupant's canonical triple, which the launch before wrote, and lowers the index by atomicMin
// when the triples are equal.  Where a cell or a triple is stored depends on races; which vertex is first, which triangle survives and every
// integer sum do not.  Passes (host_mesh_cluster.hpp enqueues them in this order):
//   k_mc_vertices     cell of every vertex, claim, first member, the slot remembered per vertex
//   k_mc_classify     per triangle: invalid / degenerate / the canonical triple of first members
//   k_mc_tri_insert   per triangle with a triple: its slot in the triangle table
//   k_mc_survive      a triangle survives iff its slot names it; survivors flag their clusters; per-block counts -> k_select_scan
//   k_mc_leaders      a vertex leads iff it is its cluster's first member and the cluster is referenced; per-block counts -> k_select_scan
//   k_mc_rank         the rank of every referenced cluster (the scanned offset + the leader's place in its block)
//   (the host reads the counters and both totals back in one copy)
//   k_mc_accumulate   per vertex of a referenced cluster: 64-bit integer adds into arrays indexed by rank
//   k_mc_finalize     per cluster: position, normal, colour
//   k_mc_triangles    per surviving triangle: the remapped indices at its scanned position
constexpr unsigned MC_NONE = 0xFFFFFFFFu;           // an empty slot of the triangle table / no first member yet / a triangle without a triple
constexpr unsigned long long MC_MUL2 = 0xC2B2AE3D27D4EB4Full;
constexpr int MC_INVALID_V = 0, MC_INVALID_T = 1, MC_CELLS = 2, MC_DEGENERATE = 3, MC_DUPLICATE = 4, MC_VERTICES = 5, MC_TRIANGLES = 6, MC_NCTR = 8;
struct McGrid { float cs; float o[3]; };
// the accumulators, indexed by rank: three planes of nv 64-bit words each for the offsets, the normals and the colours, then the two counts
struct McAcc { unsigned long long *S, *M, *C; unsigned *n, *k; int nv; };

// The cell c and the offset q of a point: false for an INVALID vertex (c and q are then 0).
__device__ __forceinline__ bool mc_cell(const McGrid& g, const float (&p)[3], int (&c)[3], int (&q)[3]) {
    bool ok = finite3(p[0], p[1], p[2]);
    float gg[3], f[3];
#pragma unroll
    for (int a = 0; a < 3; a++) {
        gg[a] = (p[a] - g.o[a]) / g.cs;
        f[a] = floorf(gg[a]);
        ok = ok && f[a] >= -1048576.f && f[a] < 1048576.f;
    }
#pragma unroll
    for (int a = 0; a < 3; a++) {
        c[a] = ok ? (int)f[a] : 0;
        q[a] = ok ? (int)((gg[a] - f[a]) * 65536.f) : 0;
    }
    return ok;
}
// hm_claim that also says whether this call made the slot (a new cell).
__device__ __forceinline__ int mc_claim(unsigned long long* __restrict__ keys, int log2cap, unsigned long long key, bool& fresh) {
    const unsigned mask = (1u << log2cap) - 1u;
    unsigned slot = hm_home(key, log2cap);
    fresh = false;
    for (unsigned i = 0; i <= mask; i++) {
        unsigned long long k = __hip_atomic_load(&keys[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (k == HM_EMPTY) {
            k = atomicCAS(&keys[slot], HM_EMPTY, key);
            if (k == HM_EMPTY) { fresh = true; return (int)slot; }
        }
        if (k == key) return (int)slot;
        slot = (slot + 1u) & mask;
    }
    return -1;
}

__global__ __launch_bounds__(256) void k_mc_vertices(int V, const float* __restrict__ vert, const McGrid g, unsigned long long* __restrict__ keys, int log2cap,
                                                     unsigned* __restrict__ first, int* __restrict__ vslot, int* __restrict__ ctr) {
    const int i = blockIdx.x * 256 + threadIdx.x, lane = threadIdx.x & 63;
    bool invalid = false, fresh = false;
    if (i < V) {
        const float p[3] = {vert[3 * (size_t)i], vert[3 * (size_t)i + 1], vert[3 * (size_t)i + 2]};
        int c[3], q[3], slot = -1;
        if (mc_cell(g, p, c, q)) {
            slot = mc_claim(keys, log2cap, hm_key(c[0], c[1], c[2]), fresh);      // (the table has at least 2 V slots: there is room)
            if (slot >= 0) atomicMin(&first[slot], (unsigned)i);
        }
        invalid = slot < 0;
        vslot[i] = slot;
    }
    const unsigned long long bi = __ballot(invalid), bf = __ballot(fresh);
    if (lane == 0 && bi) atomicAdd(&ctr[MC_INVALID_V], __popcll(bi));
    if (lane == 0 && bf) atomicAdd(&ctr[MC_CELLS], __popcll(bf));
}

// The slot of corner index `idx`, or -1: an index beyond the vertices is never used as an address.
__device__ __forceinline__ int mc_corner_slot(const int* __restrict__ vslot, int V, uint32_t idx) { return idx < (uint32_t)V ? vslot[idx] : -1; }

__global__ __launch_bounds__(256) void k_mc_classify(int V, int T, const uint32_t* __restrict__ tris, const int* __restrict__ vslot, const unsigned* __restrict__ first,
                                                     uint4* __restrict__ canon, int* __restrict__ ctr) {
    const int t = blockIdx.x * 256 + threadIdx.x, lane = threadIdx.x & 63;
    bool invalid = false, degenerate = false;
    if (t < T) {
        const int s0 = mc_corner_slot(vslot, V, tris[3 * (size_t)t]), s1 = mc_corner_slot(vslot, V, tris[3 * (size_t)t + 1]), s2 = mc_corner_slot(vslot, V, tris[3 * (size_t)t + 2]);
        uint4 k = make_uint4(MC_NONE, MC_NONE, MC_NONE, 0u);
        invalid = s0 < 0 || s1 < 0 || s2 < 0;
        if (!invalid) {
            const unsigned a = first[s0], b = first[s1], c = first[s2];
            degenerate = a == b || b == c || a == c;
            if (!degenerate) k = (a < b && a < c) ? make_uint4(a, b, c, 0u) : (b < a && b < c) ? make_uint4(b, c, a, 0u) : make_uint4(c, a, b, 0u);
        }
        canon[t] = k;
    }
    const unsigned long long bi = __ballot(invalid), bd = __ballot(degenerate);
    if (lane == 0 && bi) atomicAdd(&ctr[MC_INVALID_T], __popcll(bi));
    if (lane == 0 && bd) atomicAdd(&ctr[MC_DEGENERATE], __popcll(bd));
}

__device__ __forceinline__ unsigned mc_tri_home(const uint4& k, int log2cap) {
    unsigned long long h = (((unsigned long long)k.y << 32) | (unsigned long long)k.x) * HM_MUL;
    h = (h ^ ((unsigned long long)k.z * MC_MUL2)) * HM_MUL;
    return (unsigned)(h >> (64 - log2cap));
}
// canon was written by the launch before, so reading the occupant's triple is safe; the occupant of a slot only ever changes to a lower
// index with the SAME triple, so whichever index the load returns, the comparison has one answer.
__global__ __launch_bounds__(256) void k_mc_tri_insert(int T, const uint4* __restrict__ canon, unsigned* __restrict__ ttab, int log2cap, int* __restrict__ tslot) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= T) return;
    const uint4 k = canon[t];
    if (k.x == MC_NONE) return;
    const unsigned mask = (1u << log2cap) - 1u;
    unsigned slot = mc_tri_home(k, log2cap);
    int found = -1;
    for (unsigned i = 0; i <= mask; i++) {
        unsigned cur = __hip_atomic_load(&ttab[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (cur == MC_NONE) {
            cur = atomicCAS(&ttab[slot], MC_NONE, (unsigned)t);
            if (cur == MC_NONE) { found = (int)slot; break; }
        }
        const uint4 o = canon[cur];                         // (cur < T: only triangle indices are ever stored)
        if (o.x == k.x && o.y == k.y && o.z == k.z) { atomicMin(&ttab[slot], (unsigned)t); found = (int)slot; break; }
        slot = (slot + 1u) & mask;
    }
    tslot[t] = found;                                       // (the table has at least 2 T slots: there is room)
}

__device__ __forceinline__ bool mc_survives(int t, int T, const uint4* __restrict__ canon, const int* __restrict__ tslot, const unsigned* __restrict__ ttab, bool& live) {
    live = t < T && canon[t].x != MC_NONE;
    if (!live) return false;
    const int s = tslot[t];
    return s >= 0 && ttab[s] == (unsigned)t;
}
__global__ __launch_bounds__(256) void k_mc_survive(int V, int T, const uint32_t* __restrict__ tris, const int* __restrict__ vslot, const uint4* __restrict__ canon,
                                                    const int* __restrict__ tslot, const unsigned* __restrict__ ttab, int* __restrict__ ref, int* __restrict__ tblk,
                                                    int* __restrict__ ctr) {
    const int t = blockIdx.x * 256 + threadIdx.x, lane = threadIdx.x & 63;
    bool live;
    const bool keep = mc_survives(t, T, canon, tslot, ttab, live);
    if (keep) {
#pragma unroll
        for (int a = 0; a < 3; a++) ref[mc_corner_slot(vslot, V, tris[3 * (size_t)t + a])] = 1;      // (a triangle with a triple has three valid corners)
    }
    const int n = __syncthreads_count(keep ? 1 : 0);
    if (threadIdx.x == 0) tblk[blockIdx.x] = n;
    const unsigned long long bd = __ballot(live && !keep);
    if (lane == 0 && bd) atomicAdd(&ctr[MC_DUPLICATE], __popcll(bd));
}

__device__ __forceinline__ bool mc_leads(int i, int V, const int* __restrict__ vslot, const unsigned* __restrict__ first, const int* __restrict__ ref, int& slot) {
    slot = i < V ? vslot[i] : -1;
    return slot >= 0 && first[slot] == (unsigned)i && ref[slot] != 0;
}
__global__ __launch_bounds__(256) void k_mc_leaders(int V, const int* __restrict__ vslot, const unsigned* __restrict__ first, const int* __restrict__ ref, int* __restrict__ vblk) {
    int slot;
    const bool lead = mc_leads(blockIdx.x * 256 + threadIdx.x, V, vslot, first, ref, slot);
    const int n = __syncthreads_count(lead ? 1 : 0);
    if (threadIdx.x == 0) vblk[blockIdx.x] = n;
}
// The place of a kept lane among the kept lanes of its block, in lane order (k_select_scatter's ballot and wave offsets).
__device__ __forceinline__ int mc_block_place(bool keep, int* wave_off) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const unsigned long long m = __ballot(keep);
    const int rank = __builtin_amdgcn_mbcnt_hi((unsigned int)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned int)m, 0u));
    if (lane == 0) wave_off[w] = __popcll(m);
    __syncthreads();
    int off = 0;
    for (int v = 0; v < w; v++) off += wave_off[v];
    return off + rank;
}
// voff: the exclusive block offsets k_select_scan left in the leader table.  The leader alone writes its cluster's word (its test read a
// non-zero flag and rank + 1 is non-zero too, so the test of no other lane changes).
__global__ __launch_bounds__(256) void k_mc_rank(int V, const int* __restrict__ vslot, const unsigned* __restrict__ first, int* __restrict__ ref, const int* __restrict__ voff,
                                                 int* __restrict__ cl_slot) {
    __shared__ int wave_off[4];
    int slot;
    const bool lead = mc_leads(blockIdx.x * 256 + threadIdx.x, V, vslot, first, ref, slot);
    const int r = voff[blockIdx.x] + mc_block_place(lead, wave_off);
    if (lead) { ref[slot] = r + 1; cl_slot[r] = slot; }
}

// What one vertex adds to its cluster: n | k << 16 in w, the offsets, the quantised normal (zero when it has a non-finite component), the
// colour bytes (counted in k when alpha != 0).
struct McTerms { int w, q[3], m[3], c[3]; };
__device__ __forceinline__ void mc_add(const McAcc& A, int r, const McTerms& v) {
    const size_t nv = (size_t)A.nv;
    atomicAdd(&A.n[r], (unsigned)(v.w & 0xFFFF));
#pragma unroll
    for (int a = 0; a < 3; a++) atomicAdd(&A.S[a * nv + r], (unsigned long long)v.q[a]);
    if (A.M && (v.m[0] | v.m[1] | v.m[2])) {
#pragma unroll
        for (int a = 0; a < 3; a++) atomicAdd(&A.M[a * nv + r], (unsigned long long)(long long)v.m[a]);      // (two's complement: the sum is signed)
    }
    if (A.C && (v.w >> 16)) {
        atomicAdd(&A.k[r], (unsigned)(v.w >> 16));
#pragma unroll
        for (int a = 0; a < 3; a++) atomicAdd(&A.C[a * nv + r], (unsigned long long)v.c[a]);
    }
}
// COMBINE: the members of a cluster are mostly neighbours in the input order, so neighbouring lanes hit one address.  Runs of equal rank
// are numbered (a compare with the lane before, a ballot), a segmented shuffle-down sum leaves each run's terms in its first lane, and that
// lane alone issues the adds.  A wave's sums fit 32 bits (64 lanes of at most 65536).  Both forms give the same integers.
template <bool COMBINE>
__global__ __launch_bounds__(256) void k_mc_accumulate(int V, const float* __restrict__ vert, const float* __restrict__ nrm, const uint32_t* __restrict__ col, const McGrid g,
                                                       const int* __restrict__ vslot, const int* __restrict__ ref, const McAcc A) {
    const int i = blockIdx.x * 256 + threadIdx.x, lane = threadIdx.x & 63;
    int r = -1;
    McTerms v = {0, {0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
    if (i < V) {
        const int slot = vslot[i];
        if (slot >= 0) r = ref[slot] - 1;
        if (r >= 0) {
            const float p[3] = {vert[3 * (size_t)i], vert[3 * (size_t)i + 1], vert[3 * (size_t)i + 2]};
            int c[3];
            mc_cell(g, p, c, v.q);
            v.w = 1;
            if (nrm) {
                const float n0 = nrm[3 * (size_t)i], n1 = nrm[3 * (size_t)i + 1], n2 = nrm[3 * (size_t)i + 2];
                if (finite3(n0, n1, n2)) {
                    v.m[0] = (int)rintf(fminf(fmaxf(n0, -1.f), 1.f) * 32767.f);
                    v.m[1] = (int)rintf(fminf(fmaxf(n1, -1.f), 1.f) * 32767.f);
                    v.m[2] = (int)rintf(fminf(fmaxf(n2, -1.f), 1.f) * 32767.f);
                }
            }
            if (col) {
                const uint32_t rgba = col[i];
                if (rgba >> 24) { v.w |= 1 << 16; v.c[0] = (int)(rgba & 255u); v.c[1] = (int)((rgba >> 8) & 255u); v.c[2] = (int)((rgba >> 16) & 255u); }
            }
        }
    }
    if (!COMBINE) {
        if (r >= 0) mc_add(A, r, v);
        return;
    }
    const int before = __shfl_up(r, 1, WAVE);
    const unsigned long long starts = __ballot(lane == 0 || before != r);
    const int run = __popcll(starts & (~0ull >> (63 - lane)));
#pragma unroll
    for (int off = 1; off < WAVE; off <<= 1) {
        const int other = __shfl_down(run, off, WAVE);     // (every lane takes part in every shuffle: no shuffle behind a short-circuit)
        const bool take = lane + off < WAVE && other == run;
        const int w = __shfl_down(v.w, off, WAVE);
        if (take) v.w += w;
#pragma unroll
        for (int a = 0; a < 3; a++) {
            const int q = __shfl_down(v.q[a], off, WAVE), m = __shfl_down(v.m[a], off, WAVE), c = __shfl_down(v.c[a], off, WAVE);
            if (take) { v.q[a] += q; v.m[a] += m; v.c[a] += c; }
        }
    }
    if (r >= 0 && ((starts >> lane) & 1ull)) mc_add(A, r, v);
}

__global__ __launch_bounds__(256) void k_mc_finalize(const McGrid g, const unsigned long long* __restrict__ keys, const int* __restrict__ cl_slot, const McAcc A,
                                                     float* __restrict__ vout, float* __restrict__ nout, uint32_t* __restrict__ cout) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= A.nv) return;
    const size_t nv = (size_t)A.nv;
    int c[3];
    hm_unkey(keys[cl_slot[r]], c);
    const long long n = (long long)A.n[r];                  // (>= 1: a referenced cluster has its first member)
#pragma unroll
    for (int a = 0; a < 3; a++) {
        const long long Q = (2 * (long long)A.S[a * nv + r] + n) / (2 * n);
        vout[3 * (size_t)r + a] = g.o[a] + ((float)c[a] + (float)Q * 0x1p-16f) * g.cs;
    }
    if (nout) {
        const float N0 = (float)(long long)A.M[r], N1 = (float)(long long)A.M[nv + r], N2 = (float)(long long)A.M[2 * nv + r];
        const float len = sqrtf(N0 * N0 + (N1 * N1 + N2 * N2));
        float o0 = N0 / len, o1 = N1 / len, o2 = N2 / len;
        if (!finite3(o0, o1, o2)) o0 = o1 = o2 = 0.f;
        nout[3 * (size_t)r] = o0; nout[3 * (size_t)r + 1] = o1; nout[3 * (size_t)r + 2] = o2;
    }
    if (cout) {
        const long long k = (long long)A.k[r];
        uint32_t rgba = 0u;
        if (k > 0) {
            rgba = 255u << 24;
#pragma unroll
            for (int a = 0; a < 3; a++) rgba |= (uint32_t)((2 * (long long)A.C[a * nv + r] + k) / (2 * k)) << (8 * a);
        }
        cout[r] = rgba;
    }
}

// toff: the exclusive block offsets k_select_scan left in the survivor table; ref holds rank + 1 by now.
__global__ __launch_bounds__(256) void k_mc_triangles(int V, int T, const uint32_t* __restrict__ tris, const int* __restrict__ vslot, const uint4* __restrict__ canon,
                                                      const int* __restrict__ tslot, const unsigned* __restrict__ ttab, const int* __restrict__ ref, const int* __restrict__ toff,
                                                      uint32_t* __restrict__ tout) {
    __shared__ int wave_off[4];
    const int t = blockIdx.x * 256 + threadIdx.x;
    bool live;
    const bool keep = mc_survives(t, T, canon, tslot, ttab, live);
    const size_t at = (size_t)(toff[blockIdx.x] + mc_block_place(keep, wave_off));
    if (keep) {
#pragma unroll
        for (int a = 0; a < 3; a++) tout[3 * at + a] = (uint32_t)(ref[mc_corner_slot(vslot, V, tris[3 * (size_t)t + a])] - 1);
    }
}
