// dev_tsdf_mesh.hpp -- the zero level set of the TSDF volume as an indexed triangle mesh with per-vertex normals (icp_tsdf_mesh): every cell
// cut into the six tetrahedra of the Kuhn (Freudenthal) triangulation, marching tetrahedra on each.  Contract: include/icp_hip.h, DESIGN.md
// section 6n.  Part of icp_device.hpp (included from there, inside namespace icpdev, after dev_tsdf.hpp); see that file for the build contract.
// ------------------------------------------------------------------------------------------------
// The volume is read ONCE, by k_tm_classify, into two bitmaps (observed, negative: one 64-bit word per run of 64 consecutive voxels, a
// wave ballot each); every later pass works on bitmaps and bytes and goes back to the volume only where a vertex is written.
//   k_tm_classify   volume -> observed / negative bitmaps
//   k_tm_cells      observed -> valid-cell bitmap (the cell whose lowest corner the voxel is)
//   k_tm_count      negative + valid -> one byte per voxel (the 7-bit mask of the edges it owns that carry a vertex), vertex and triangle
//                   counts per block; k_select_scan turns both tables into offsets
//   k_tm_vertices   mask bytes -> positions and normals in vertex order, and the first vertex index of every run
//   k_tm_triangles  negative + valid + the table -> index triples in triangle order; the index of a vertex owned by another voxel is its
//                   run's base + the set bits of the mask bytes before it in its 64-byte line + the lower codes of its own mask
// Scratch: 3 bits + 1 byte per voxel + 4 bytes per run = 1.4375 bytes per voxel, and two ints per block of TM_BLOCK_VOXELS.
// A block is 4 waves, a wave walks TM_RUNS consecutive runs; ranks come from __ballot / mbcnt, wave counts meet in LDS, no float atomics.
// Every fp32 operation is written in the contract's order: tests/tsdf_mesh_restatement.py states the same arithmetic in numpy.
constexpr int TM_RUNS = 4;                                   // runs of 64 voxels per wave
constexpr int TM_BLOCK_VOXELS = 256 * TM_RUNS;               // voxels per block: one entry of each count table

// ---- the case table, generated at compile time from the contract's rule
struct TmTable {
    uint32_t e[6][16];                            // bits 0..1: triangles (0..2); bits 2 + 3 s ..: the local edge rank of slot s (triangle s / 3, corner s % 3)
    uint16_t q[6];                                // bits 3 a ..: corner q_a of the tetrahedron as dx + 2 dy + 4 dz
};
constexpr int tm_edge_a(int r) { return r < 3 ? 0 : (r < 5 ? 1 : 2); }
constexpr int tm_edge_b(int r) { return r < 3 ? r + 1 : (r < 5 ? r - 1 : 3); }
constexpr int tm_edge_rank(int a, int b) { return (a < b ? a : b) == 0 ? (a < b ? b : a) - 1 : a + b; }
constexpr TmTable tm_make_table() {
    TmTable T{};
    const int perm[6][3] = {{0, 1, 2}, {0, 2, 1}, {1, 0, 2}, {1, 2, 0}, {2, 0, 1}, {2, 1, 0}};      // the axis permutations, lexicographic
    for (int p = 0; p < 6; p++) {
        int q[4][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}, {1, 1, 1}};
        q[1][perm[p][0]] = 1; q[2][perm[p][0]] = 1; q[2][perm[p][1]] = 1;
        for (int a = 0; a < 4; a++) T.q[p] = (uint16_t)(T.q[p] | ((q[a][0] + 2 * q[a][1] + 4 * q[a][2]) << (3 * a)));
        for (int m = 1; m < 15; m++) {
            int neg[4] = {0, 0, 0, 0}, pos[4] = {0, 0, 0, 0}, nn = 0, np = 0;
            for (int a = 0; a < 4; a++) { if ((m >> a) & 1) neg[nn++] = a; else pos[np++] = a; }
            int cyc[4] = {0, 0, 0, 0}, nc = 0;
            if (nn == 1 || np == 1) {              // one corner alone: its three edges in ascending rank
                const int lone = nn == 1 ? neg[0] : pos[0];
                for (int r = 0; r < 6; r++) if (tm_edge_a(r) == lone || tm_edge_b(r) == lone) cyc[nc++] = r;
            } else {                               // two and two: the quad cycle, rotated to start at its smallest rank
                const int raw[4] = {tm_edge_rank(neg[0], pos[0]), tm_edge_rank(neg[0], pos[1]), tm_edge_rank(neg[1], pos[1]), tm_edge_rank(neg[1], pos[0])};
                int s = 0;
                for (int x = 1; x < 4; x++) if (raw[x] < raw[s]) s = x;
                for (int x = 0; x < 4; x++) cyc[x] = raw[(s + x) & 3];
                nc = 4;
            }
            // orientation, crossings at the edge midpoints (all coordinates doubled; free = nn np (mean of positives - mean of negatives))
            int free[3] = {0, 0, 0}, nrm[3] = {0, 0, 0};
            for (int k = 0; k < 3; k++) {
                for (int x = 0; x < np; x++) free[k] += nn * q[pos[x]][k];
                for (int x = 0; x < nn; x++) free[k] -= np * q[neg[x]][k];
            }
            for (int t = 0; t < nc - 2; t++) {
                int u[3] = {0, 0, 0}, w[3] = {0, 0, 0};
                for (int k = 0; k < 3; k++) {
                    const int m0 = q[tm_edge_a(cyc[0])][k] + q[tm_edge_b(cyc[0])][k];
                    u[k] = q[tm_edge_a(cyc[t + 1])][k] + q[tm_edge_b(cyc[t + 1])][k] - m0;
                    w[k] = q[tm_edge_a(cyc[t + 2])][k] + q[tm_edge_b(cyc[t + 2])][k] - m0;
                }
                nrm[0] = u[1] * w[2] - u[2] * w[1]; nrm[1] = u[2] * w[0] - u[0] * w[2]; nrm[2] = u[0] * w[1] - u[1] * w[0];
                if (nrm[0] || nrm[1] || nrm[2]) break;
            }
            if (nrm[0] * free[0] + nrm[1] * free[1] + nrm[2] * free[2] < 0) {      // reversed, keeping the first edge
                const int a = cyc[1]; cyc[1] = cyc[nc - 1]; cyc[nc - 1] = a;
            }
            uint32_t e = (uint32_t)(nc - 2);
            const int slot[6] = {cyc[0], cyc[1], cyc[2], cyc[0], cyc[2], cyc[3]};
            for (int s = 0; s < 3 * (nc - 2); s++) e |= (uint32_t)slot[s] << (2 + 3 * s);
            T.e[p][m] = e;
        }
    }
    return T;
}
__constant__ constexpr TmTable TM_TABLE = tm_make_table();

// ---- exact division of an index below 2^31 by a dimension (Granlund and Montgomery 1994, the round-up form): the host fills it
struct TmDiv { uint32_t m; int s1, s2; };
__host__ __device__ __forceinline__ uint32_t tm_div(uint32_t n, const TmDiv& d) {
#ifdef __HIP_DEVICE_COMPILE__
    const uint32_t t = __umulhi(d.m, n);
#else
    const uint32_t t = (uint32_t)(((uint64_t)d.m * n) >> 32);
#endif
    return (t + ((n - t) >> d.s1)) >> d.s2;
}
struct TmGrid { int nx, ny, nz, n, plane, nruns; TmDiv dx, dp; };      // n voxels, plane = nx ny, nruns = ceil(n / 64); division by nx / by plane

__device__ __forceinline__ int tm_bit(const unsigned long long* __restrict__ bm, int l) { return (int)((bm[l >> 6] >> (l & 63)) & 1ull); }
__device__ __forceinline__ int tm_rank(unsigned long long b) { return (int)__builtin_amdgcn_mbcnt_hi((unsigned int)(b >> 32), __builtin_amdgcn_mbcnt_lo((unsigned int)b, 0u)); }
__device__ __forceinline__ float tm_lerp(float a, float b, float t) { return a + t * (b - a); }
__device__ __forceinline__ void tm_decode(const TmGrid& g, int l, int& i, int& j, int& k) {
    k = (int)tm_div((uint32_t)l, g.dp);
    const int rem = l - k * g.plane;
    j = (int)tm_div((uint32_t)rem, g.dx);
    i = rem - j * g.nx;
}
// the negative bits of the eight corners of cell l (bit dx + 2 dy + 4 dz); the cell must be in range
__device__ __forceinline__ int tm_corner_signs(const TmGrid& g, const unsigned long long* __restrict__ neg, int l) {
    int sg = 0;
#pragma unroll
    for (int c = 0; c < 8; c++) sg |= tm_bit(neg, l + (c & 1) + ((c >> 1) & 1) * g.nx + (c >> 2) * g.plane) << c;
    return sg;
}
// triangles of a valid cell with corner signs sg
__device__ __forceinline__ int tm_cell_triangles(int sg) {
    int n = 0;
#pragma unroll
    for (int p = 0; p < 6; p++) {
        int m = 0;
#pragma unroll
        for (int a = 0; a < 4; a++) m |= ((sg >> ((TM_TABLE.q[p] >> (3 * a)) & 7)) & 1) << a;
        n += (int)(TM_TABLE.e[p][m] & 3u);
    }
    return n;
}
// wave sum / exclusive prefix of a per-lane count below 2^BITS, by one ballot per bit
template <int BITS>
__device__ __forceinline__ void tm_wave_scan(int v, int& before, int& total) {
    before = 0; total = 0;
#pragma unroll
    for (int b = 0; b < BITS; b++) {
        const unsigned long long bal = __ballot((v >> b) & 1);
        before += tm_rank(bal) << b;
        total += __popcll(bal) << b;
    }
}
// per-lane set bits of a mask byte: exclusive prefix over the wave and the wave's total, one ballot per code
__device__ __forceinline__ void tm_mask_scan(int mk, int& before, int& total) {
    before = 0; total = 0;
    if (__ballot(mk != 0) == 0ull) return;
#pragma unroll
    for (int b = 0; b < 7; b++) {
        const unsigned long long bal = __ballot((mk >> b) & 1);
        before += tm_rank(bal);
        total += __popcll(bal);
    }
}

__global__ __launch_bounds__(256) void k_tm_classify(const float2* __restrict__ vox, const TmGrid g, float min_weight,
                                                     unsigned long long* __restrict__ obs, unsigned long long* __restrict__ neg) {
    const int lane = threadIdx.x & 63, run0 = (blockIdx.x * 4 + (threadIdx.x >> 6)) * TM_RUNS;
    float2 a[TM_RUNS];
#pragma unroll
    for (int r = 0; r < TM_RUNS; r++) {
        const int l = (run0 + r) * 64 + lane;
        a[r] = l < g.n ? vox[l] : make_float2(0.f, 0.f);
    }
#pragma unroll
    for (int r = 0; r < TM_RUNS; r++) {
        const unsigned long long bo = __ballot(a[r].y > 0.f && a[r].y >= min_weight && __builtin_isfinite(a[r].x));
        const unsigned long long bn = __ballot(a[r].x < 0.f);
        if (lane == 0 && run0 + r < g.nruns) { obs[run0 + r] = bo; neg[run0 + r] = bn; }
    }
}

__global__ __launch_bounds__(256) void k_tm_cells(const TmGrid g, const unsigned long long* __restrict__ obs, unsigned long long* __restrict__ valid) {
    const int lane = threadIdx.x & 63, run0 = (blockIdx.x * 4 + (threadIdx.x >> 6)) * TM_RUNS;
#pragma unroll 1
    for (int r = 0; r < TM_RUNS; r++) {
        const int run = run0 + r, l = run * 64 + lane;
        if (run >= g.nruns) break;
        bool v = false;
        if (obs[run] != 0ull && l < g.n) {         // (every cell holds its own lowest corner)
            int i, j, k;
            tm_decode(g, l, i, j, k);
            if (i < g.nx - 1 && j < g.ny - 1 && k < g.nz - 1) {
                v = true;
#pragma unroll
                for (int c = 0; c < 8; c++) v = v && tm_bit(obs, l + (c & 1) + ((c >> 1) & 1) * g.nx + (c >> 2) * g.plane);
            }
        }
        const unsigned long long bv = __ballot(v);
        if (lane == 0) valid[run] = bv;
    }
}

// The mask of voxel l: bit code - 1 set iff the edge l -> l + d (code = dx + 2 dy + 4 dz) stays inside the volume, has exactly one negative
// end and lies in a valid cell (the cells l - off, off only on axes where d is 0).
__device__ __forceinline__ int tm_edge_mask(const TmGrid& g, const unsigned long long* __restrict__ neg, const unsigned long long* __restrict__ valid, int l, int i, int j, int k) {
    const int in = (i < g.nx - 1 ? 1 : 0) | (j < g.ny - 1 ? 2 : 0) | (k < g.nz - 1 ? 4 : 0);
    const int own = tm_bit(neg, l);
    int cross = 0;
#pragma unroll
    for (int c = 1; c < 8; c++)
        if ((c & in) == c) cross |= (tm_bit(neg, l + (c & 1) + ((c >> 1) & 1) * g.nx + (c >> 2) * g.plane) ^ own) << (c - 1);
    if (cross == 0) return 0;
    const int lo = (i >= 1 ? 1 : 0) | (j >= 1 ? 2 : 0) | (k >= 1 ? 4 : 0);
    int cells = 0;                                 // bit off: the cell l - off exists and is valid
#pragma unroll
    for (int off = 0; off < 7; off++)
        if ((off & lo) == off) cells |= tm_bit(valid, l - ((off & 1) + ((off >> 1) & 1) * g.nx + (off >> 2) * g.plane)) << off;
    int mk = 0;
#pragma unroll
    for (int c = 1; c < 8; c++) {
        int any = 0;
#pragma unroll
        for (int off = 0; off < 7; off++) if ((off & c) == 0) any |= (cells >> off) & 1;
        mk |= (any & (cross >> (c - 1))) << (c - 1);
    }
    return mk;
}

__global__ __launch_bounds__(256) void k_tm_count(const TmGrid g, const unsigned long long* __restrict__ neg, const unsigned long long* __restrict__ valid,
                                                  uint8_t* __restrict__ mask, int* __restrict__ vblk, int* __restrict__ tblk) {
    __shared__ int red[2][4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, run0 = (blockIdx.x * 4 + wave) * TM_RUNS;
    int nv = 0, nt = 0;                            // the wave's vertices and triangles so far (the same in every lane)
#pragma unroll 1
    for (int r = 0; r < TM_RUNS; r++) {
        const int run = run0 + r, l = run * 64 + lane;
        if (run >= g.nruns) break;
        int mk = 0, tri = 0;
        if (l < g.n) {
            int i, j, k;
            tm_decode(g, l, i, j, k);
            mk = tm_edge_mask(g, neg, valid, l, i, j, k);
            if (mk != 0 && tm_bit(valid, l)) tri = tm_cell_triangles(tm_corner_signs(g, neg, l));      // (all seven edges from a cell's lowest corner are that voxel's own: corners of two signs set a bit of mk)
        }
        mask[l] = (uint8_t)mk;
        int before, total;
        tm_mask_scan(mk, before, total);
        nv += total;
        if (__ballot(tri != 0) != 0ull) { tm_wave_scan<4>(tri, before, total); nt += total; }
    }
    if (lane == 0) { red[0][wave] = nv; red[1][wave] = nt; }
    __syncthreads();
    if (threadIdx.x == 0) {
        vblk[blockIdx.x] = (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]);
        tblk[blockIdx.x] = (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]);
    }
}

// Vertex `code` of voxel l = (i, j, k): the position on the edge and the normal of the first valid cell that holds the edge.
__device__ __forceinline__ void tm_vertex(const TsdfVol& v, const TmGrid& g, const unsigned long long* __restrict__ valid, int l, int i, int j, int k, int code,
                                          float (&p)[3], float (&n)[3]) {
    const int dx = code & 1, dy = (code >> 1) & 1, dz = code >> 2;
    const float fv = v.vox[l].x, fd = v.vox[l + dx + dy * g.nx + dz * g.plane].x;
    const float t = fv / (fv - fd);
    const float ts = t * v.s;
    const float bx = v.ox + (float)i * v.s, by = v.oy + (float)j * v.s, bz = v.oz + (float)k * v.s;
    p[0] = dx ? bx + ts : bx; p[1] = dy ? by + ts : by; p[2] = dz ? bz + ts : bz;
    const int lo = ((i >= 1 ? 1 : 0) | (j >= 1 ? 2 : 0) | (k >= 1 ? 4 : 0)) & ~code;      // the axes a holding cell may be shifted down on
    int off = 0;
#pragma unroll 1
    for (; off < 7; off++)
        if ((off & lo) == off && tm_bit(valid, l - ((off & 1) + ((off >> 1) & 1) * g.nx + (off >> 2) * g.plane))) break;
    n[0] = 0.f; n[1] = 0.f; n[2] = 0.f;
    if (off == 7) return;                          // (cannot happen: the mask bit says that one of these cells is valid)
    const float2* __restrict__ q = v.vox + (l - ((off & 1) + ((off >> 1) & 1) * g.nx + (off >> 2) * g.plane));
    const float c0 = q[0].x, c1 = q[1].x, c2 = q[g.nx].x, c3 = q[g.nx + 1].x;
    const float c4 = q[g.plane].x, c5 = q[g.plane + 1].x, c6 = q[g.plane + g.nx].x, c7 = q[g.plane + g.nx + 1].x;
    const float tx = dx ? t : (float)(off & 1), ty = dy ? t : (float)((off >> 1) & 1), tz = dz ? t : (float)(off >> 2);
    const float gx = tm_lerp(tm_lerp(c1 - c0, c3 - c2, ty), tm_lerp(c5 - c4, c7 - c6, ty), tz);
    const float gy = tm_lerp(tm_lerp(c2 - c0, c3 - c1, tx), tm_lerp(c6 - c4, c7 - c5, tx), tz);
    const float gz = tm_lerp(tm_lerp(c4 - c0, c5 - c1, tx), tm_lerp(c6 - c2, c7 - c3, tx), ty);
    const float len = sqrtf(gx * gx + (gy * gy + gz * gz));
    const float n0 = gx / len, n1 = gy / len, n2 = gz / len;
    const bool ok = __builtin_isfinite(n0) && __builtin_isfinite(n1) && __builtin_isfinite(n2);
    n[0] = ok ? n0 : 0.f; n[1] = ok ? n1 : 0.f; n[2] = ok ? n2 : 0.f;
}

// voff: the exclusive block offsets k_select_scan left in the vertex table.  base[run] receives the first vertex index of every run.
__global__ __launch_bounds__(256) void k_tm_vertices(const TsdfVol v, const TmGrid g, const unsigned long long* __restrict__ valid, const uint8_t* __restrict__ mask,
                                                     const int* __restrict__ voff, int* __restrict__ base, float* __restrict__ vert, float* __restrict__ nrm) {
    __shared__ int red[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, run0 = (blockIdx.x * 4 + wave) * TM_RUNS;
    int mk[TM_RUNS], mine = 0;
#pragma unroll
    for (int r = 0; r < TM_RUNS; r++) {
        mk[r] = run0 + r < g.nruns ? (int)mask[(run0 + r) * 64 + lane] : 0;
        int before, total;
        tm_mask_scan(mk[r], before, total);
        mine += total;
    }
    if (lane == 0) red[wave] = mine;
    __syncthreads();
    int at = voff[blockIdx.x];
    for (int w = 0; w < wave; w++) at += red[w];
#pragma unroll
    for (int r = 0; r < TM_RUNS; r++) {
        const int run = run0 + r, l = run * 64 + lane;
        if (run >= g.nruns) break;
        if (lane == 0) base[run] = at;
        int before, total;
        tm_mask_scan(mk[r], before, total);
        if (mk[r] != 0) {
            int i, j, k, idx = at + before;
            tm_decode(g, l, i, j, k);
#pragma unroll 1
            for (int code = 1; code < 8; code++) {
                if (!((mk[r] >> (code - 1)) & 1)) continue;
                float p[3], n[3];
                tm_vertex(v, g, valid, l, i, j, k, code, p, n);
                vert[(size_t)idx * 3] = p[0]; vert[(size_t)idx * 3 + 1] = p[1]; vert[(size_t)idx * 3 + 2] = p[2];
                if (nrm) { nrm[(size_t)idx * 3] = n[0]; nrm[(size_t)idx * 3 + 1] = n[1]; nrm[(size_t)idx * 3 + 2] = n[2]; }
                idx++;
            }
        }
        at += total;
    }
}

// The index of vertex `code` of voxel u: its run's base, the set bits of the mask bytes before it in its 64-byte line, its own lower codes.
__device__ __forceinline__ uint32_t tm_vertex_index(const uint8_t* __restrict__ mask, const int* __restrict__ base, int u, int code) {
    const int run = u >> 6, p = u & 63, w = p >> 3;
    const unsigned long long* __restrict__ line = (const unsigned long long*)(mask + ((size_t)run << 6));
    int idx = base[run];
#pragma unroll
    for (int x = 0; x < 8; x++) {
        const unsigned long long word = line[x];
        idx += x < w ? __popcll(word) : (x == w ? __popcll(word & ((1ull << ((p & 7) * 8)) - 1ull)) : 0);
    }
    return (uint32_t)(idx + __popc((unsigned int)mask[u] & ((1u << (code - 1)) - 1u)));
}

// toff: the exclusive block offsets k_select_scan left in the triangle table.
__global__ __launch_bounds__(256) void k_tm_triangles(const TmGrid g, const unsigned long long* __restrict__ neg, const unsigned long long* __restrict__ valid,
                                                      const uint8_t* __restrict__ mask, const int* __restrict__ base, const int* __restrict__ toff, uint32_t* __restrict__ tris) {
    __shared__ int red[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, run0 = (blockIdx.x * 4 + wave) * TM_RUNS;
    int sg[TM_RUNS], cnt[TM_RUNS], mine = 0;
#pragma unroll
    for (int r = 0; r < TM_RUNS; r++) {
        const int run = run0 + r, l = run * 64 + lane;
        sg[r] = 0; cnt[r] = 0;
        if (run < g.nruns && mask[l] != 0 && tm_bit(valid, l)) { sg[r] = tm_corner_signs(g, neg, l); cnt[r] = tm_cell_triangles(sg[r]); }
        if (__ballot(cnt[r] != 0) != 0ull) { int before, total; tm_wave_scan<4>(cnt[r], before, total); mine += total; }
    }
    if (lane == 0) red[wave] = mine;
    __syncthreads();
    int at = toff[blockIdx.x];
    for (int w = 0; w < wave; w++) at += red[w];
#pragma unroll
    for (int r = 0; r < TM_RUNS; r++) {
        if (__ballot(cnt[r] != 0) == 0ull) continue;
        const int l = (run0 + r) * 64 + lane;
        int before, total;
        tm_wave_scan<4>(cnt[r], before, total);
        if (cnt[r] != 0) {
            size_t o = (size_t)(at + before) * 3;
#pragma unroll 1
            for (int p = 0; p < 6; p++) {
                const int q = TM_TABLE.q[p];
                int m = 0;
#pragma unroll
                for (int a = 0; a < 4; a++) m |= ((sg[r] >> ((q >> (3 * a)) & 7)) & 1) << a;
                const uint32_t e = TM_TABLE.e[p][m];
                const int ns = 3 * (int)(e & 3u);
#pragma unroll 1
                for (int s = 0; s < ns; s++) {
                    const int rk = (int)((e >> (2 + 3 * s)) & 7u);
                    const int qa = (q >> (3 * tm_edge_a(rk))) & 7, qb = (q >> (3 * tm_edge_b(rk))) & 7;
                    tris[o++] = tm_vertex_index(mask, base, l + (qa & 1) + ((qa >> 1) & 1) * g.nx + (qa >> 2) * g.plane, qa ^ qb);
                }
            }
        }
        at += total;
    }
}
