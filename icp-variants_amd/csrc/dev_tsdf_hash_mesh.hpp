// dev_tsdf_hash_mesh.hpp -- the zero level set of the HASHED TSDF volume as an indexed triangle mesh (icp_tsdf_mesh_hashed): dev_tsdf_mesh.hpp's
// marching tetrahedra read through dev_tsdf_hash.hpp's block pool.  Contract: include/icp_hip.h, DESIGN.md section 6y;
// tests/htsdf_mesh_restatement.py states the same arithmetic in numpy.  Part of icp_device.hpp (included from there, inside namespace icpdev,
// after dev_tsdf_hash.hpp and dev_tsdf_mesh.hpp, whose table, scans, ranks and tm_vertex_index are used as they are).
// ------------------------------------------------------------------------------------------------
// Where a block sits in the pool depends on a race, so everything after the first step is indexed by the block's RANK, its position among
// the keys in ascending order (the host sorts them: order[rank] -> pool index, rank_of[pool index] -> rank).  A voxel's scratch index is
// rank * 512 + local, a run of 64 voxels is one z-layer of one block (run = rank * 8 + lz), every count table has one entry per block.
//   k_htm_neighbours  (rank, one of 27 offsets) -> the neighbour block's rank, or -1: the only kernel that probes the hash table
//   k_htm_classify    pool -> observed / negative words: the only pass over the pool, one 512-byte run per wave
//   k_htm_cells       observed words of the block and its 7 upper neighbours -> valid-cell words
//   k_htm_count       negative (upper neighbours) + valid (lower neighbours) -> one mask byte per voxel, vertex and triangle counts per block
//   k_htm_vertices    mask bytes -> positions and normals in vertex order, the first vertex index of every run; reads the pool at vertices only
//   k_htm_triangles   negative + valid + the table -> index triples; the owner of a vertex may be a voxel of an upper neighbour
// One work-group is one block, one wave one z-layer, a lane one (x, y) of the layer.  What a work-group needs of its neighbours (bitmap
// words, ranks, pool indices) is loaded ONCE, by its first threads, into LDS; a lane then picks by LDS address, so no register array is
// indexed and no lane probes anything.  A missing neighbour's words are 0: its voxels read (0, 0), unobserved and not negative.
// No atomics of any kind: every output position is a function of the bitmaps.
constexpr int HTM_NONE = -1;

// The 36 words a block's lanes need of one bitmap along one direction, into w[cxy * 9 + layer] (threads 0 .. 35; the caller's barrier follows).
// up: cxy = cx + 2 cy with (cx, cy) in {0, 1}^2 the step to the neighbour, layers 0 .. 7 the block's own z-layers and layer 8 layer 0 of the
// block above.  down: (cx, cy) in {0, -1}^2, layer 0 layer 7 of the block below and layers 1 .. 8 the block's own.
template <bool UP>
__device__ __forceinline__ void htm_stage(const unsigned long long* __restrict__ bm, const int* __restrict__ nb, unsigned long long* __restrict__ w, int t) {
    const int cxy = t / 9, layer = t - cxy * 9;
    const int cx = UP ? (cxy & 1) : -(cxy & 1), cy = UP ? (cxy >> 1) : -(cxy >> 1);
    const int cz = UP ? (layer == 8 ? 1 : 0) : (layer == 0 ? -1 : 0), lz = UP ? (layer & 7) : ((layer + 7) & 7);
    const int r = nb[(cz + 1) * 9 + (cy + 1) * 3 + (cx + 1)];
    w[t] = r >= 0 ? bm[(size_t)r * 8 + lz] : 0ull;
}
// bit (x, y, z) of the staged words, coordinates relative to the block: 0 .. 8 for up, -1 .. 7 for down
template <bool UP>
__device__ __forceinline__ int htm_bit(const unsigned long long* __restrict__ w, int x, int y, int z) {
    const int cxy = UP ? ((x >> 3) | ((y >> 3) << 1)) : (((x >> 3) & 1) | (((y >> 3) & 1) << 1));
    return (int)((w[cxy * 9 + (UP ? z : z + 1)] >> (((y & 7) << 3) | (x & 7))) & 1ull);
}
// the negative bits of the eight corners of the cell whose lowest corner is (x, y, z) (bit dx + 2 dy + 4 dz), from the staged `up` words
__device__ __forceinline__ int htm_corner_signs(const unsigned long long* __restrict__ neg_up, int x, int y, int z) {
    int sg = 0;
#pragma unroll
    for (int c = 0; c < 8; c++) sg |= htm_bit<true>(neg_up, x + (c & 1), y + ((c >> 1) & 1), z + (c >> 2)) << c;
    return sg;
}

__global__ __launch_bounds__(256) void k_htm_neighbours(const HtVol v, int n_blocks, const int* __restrict__ order, const int* __restrict__ rank_of, int* __restrict__ nbr) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_blocks * 27) return;
    const int rank = i / 27, o = i - rank * 27;
    int b[3];
    hm_unkey(v.pool_key[order[rank]], b);
    const int bx = b[0] + (o % 3) - 1, by = b[1] + ((o / 3) % 3) - 1, bz = b[2] + (o / 9) - 1;
    int r = HTM_NONE;
    if (bx >= -HM_RANGE && bx < HM_RANGE && by >= -HM_RANGE && by < HM_RANGE && bz >= -HM_RANGE && bz < HM_RANGE) {      // in int, before any key is formed
        const int blk = ht_lookup(v, bx, by, bz);
        if (blk >= 0 && blk < n_blocks) r = rank_of[blk];
    }
    nbr[i] = r;
}

__global__ __launch_bounds__(512) void k_htm_classify(const float2* __restrict__ pool, const int* __restrict__ order, float min_weight,
                                                      unsigned long long* __restrict__ obs, unsigned long long* __restrict__ neg) {
    const int lane = threadIdx.x & 63, run = blockIdx.x * 8 + (threadIdx.x >> 6);
    const float2 a = pool[(size_t)order[blockIdx.x] * 512 + threadIdx.x];
    const unsigned long long bo = __ballot(a.y > 0.f && a.y >= min_weight && __builtin_isfinite(a.x));
    const unsigned long long bn = __ballot(a.x < 0.f);
    if (lane == 0) { obs[run] = bo; neg[run] = bn; }
}

__global__ __launch_bounds__(512) void k_htm_cells(const int* __restrict__ nbr, const unsigned long long* __restrict__ obs, unsigned long long* __restrict__ valid) {
    __shared__ unsigned long long w[36];
    const int tid = threadIdx.x, lane = tid & 63, lz = tid >> 6, lx = lane & 7, ly = lane >> 3;
    if (tid < 36) htm_stage<true>(obs, nbr + (size_t)blockIdx.x * 27, w, tid);
    __syncthreads();
    bool ok = true;
#pragma unroll
    for (int c = 0; c < 8; c++) ok = ok && htm_bit<true>(w, lx + (c & 1), ly + ((c >> 1) & 1), lz + (c >> 2));
    const unsigned long long bv = __ballot(ok);
    if (lane == 0) valid[blockIdx.x * 8 + lz] = bv;
}

// tm_edge_mask without an extent: bit code - 1 set iff the edge (x, y, z) -> + d has exactly one negative end and lies in a valid cell (the
// cells (x, y, z) - off, off only on axes where d is 0).  An edge into a block that does not exist finds no valid cell.  sg: the corner signs.
__device__ __forceinline__ int htm_edge_mask(const unsigned long long* __restrict__ neg_up, const unsigned long long* __restrict__ valid_dn, int x, int y, int z, int& sg) {
    sg = htm_corner_signs(neg_up, x, y, z);
    const int cross = ((sg & 1 ? ~sg : sg) >> 1) & 0x7F;      // bit c - 1: corner c differs from corner 0
    if (cross == 0) return 0;
    int cells = 0;                                 // bit off: the cell (x, y, z) - off is valid
#pragma unroll
    for (int off = 0; off < 7; off++) cells |= htm_bit<false>(valid_dn, x - (off & 1), y - ((off >> 1) & 1), z - (off >> 2)) << off;
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

__global__ __launch_bounds__(512) void k_htm_count(const int* __restrict__ nbr, const unsigned long long* __restrict__ neg, const unsigned long long* __restrict__ valid,
                                                   uint8_t* __restrict__ mask, int* __restrict__ vblk, int* __restrict__ tblk) {
    __shared__ unsigned long long w[72];           // negative, up | valid, down
    __shared__ int red[2][8];
    const int tid = threadIdx.x, lane = tid & 63, lz = tid >> 6, lx = lane & 7, ly = lane >> 3;
    if (tid < 36) htm_stage<true>(neg, nbr + (size_t)blockIdx.x * 27, w, tid);
    else if (tid >= 64 && tid < 100) htm_stage<false>(valid, nbr + (size_t)blockIdx.x * 27, w + 36, tid - 64);
    __syncthreads();
    int sg;
    const int mk = htm_edge_mask(w, w + 36, lx, ly, lz, sg);
    int tri = 0;
    if (mk != 0 && htm_bit<false>(w + 36, lx, ly, lz)) tri = tm_cell_triangles(sg);      // (all seven edges from a cell's lowest corner are that voxel's own)
    mask[(size_t)blockIdx.x * 512 + tid] = (uint8_t)mk;
    int before, nv, nt = 0;
    tm_mask_scan(mk, before, nv);
    if (__ballot(tri != 0) != 0ull) tm_wave_scan<4>(tri, before, nt);
    if (lane == 0) { red[0][lz] = nv; red[1][lz] = nt; }
    __syncthreads();
    if (tid == 0) {
        vblk[blockIdx.x] = ((red[0][0] + red[0][1]) + (red[0][2] + red[0][3])) + ((red[0][4] + red[0][5]) + (red[0][6] + red[0][7]));
        tblk[blockIdx.x] = ((red[1][0] + red[1][1]) + (red[1][2] + red[1][3])) + ((red[1][4] + red[1][5]) + (red[1][6] + red[1][7]));
    }
}

// F of the voxel (x, y, z), coordinates relative to the block in -1 .. 8, through the staged pool indices of the 27 neighbours (a block
// that does not exist reads 0)
__device__ __forceinline__ float htm_f(const float2* __restrict__ pool, const int* __restrict__ pb, int x, int y, int z) {
    const int blk = pb[((z >> 3) + 1) * 9 + ((y >> 3) + 1) * 3 + ((x >> 3) + 1)];
    return blk >= 0 ? pool[(size_t)blk * 512 + (size_t)(((z & 7) << 6) | ((y & 7) << 3) | (x & 7))].x : 0.f;
}

// tm_vertex on the blocks: vertex `code` of the voxel (x, y, z) of the block at b.  That function's text with its voxel reads and bit tests
// replaced (sharing one body through a template would have to leave k_tm_vertices' instructions as they are): the same operations in the
// same order, with the SIGNED GLOBAL voxel coordinate 8 b + local in place of the box index.
__device__ __forceinline__ void htm_vertex(const HtVol& v, const int* __restrict__ pb, const unsigned long long* __restrict__ valid_dn, const int (&b)[3], int x, int y, int z, int code,
                                           float (&p)[3], float (&n)[3]) {
    const int dx = code & 1, dy = (code >> 1) & 1, dz = code >> 2;
    const float fv = htm_f(v.pool, pb, x, y, z), fd = htm_f(v.pool, pb, x + dx, y + dy, z + dz);
    const float t = fv / (fv - fd);
    const float ts = t * v.s;
    const float bx = v.ox + (float)(b[0] * 8 + x) * v.s, by = v.oy + (float)(b[1] * 8 + y) * v.s, bz = v.oz + (float)(b[2] * 8 + z) * v.s;
    p[0] = dx ? bx + ts : bx; p[1] = dy ? by + ts : by; p[2] = dz ? bz + ts : bz;
    int off = 0;
#pragma unroll 1
    for (; off < 7; off++)
        if ((off & code) == 0 && htm_bit<false>(valid_dn, x - (off & 1), y - ((off >> 1) & 1), z - (off >> 2))) break;
    n[0] = 0.f; n[1] = 0.f; n[2] = 0.f;
    if (off == 7) return;                          // (cannot happen: the mask bit says that one of these cells is valid)
    const int qx = x - (off & 1), qy = y - ((off >> 1) & 1), qz = z - (off >> 2);
    const float c0 = htm_f(v.pool, pb, qx, qy, qz), c1 = htm_f(v.pool, pb, qx + 1, qy, qz), c2 = htm_f(v.pool, pb, qx, qy + 1, qz), c3 = htm_f(v.pool, pb, qx + 1, qy + 1, qz);
    const float c4 = htm_f(v.pool, pb, qx, qy, qz + 1), c5 = htm_f(v.pool, pb, qx + 1, qy, qz + 1), c6 = htm_f(v.pool, pb, qx, qy + 1, qz + 1), c7 = htm_f(v.pool, pb, qx + 1, qy + 1, qz + 1);
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
__global__ __launch_bounds__(512) void k_htm_vertices(const HtVol v, const int* __restrict__ order, const int* __restrict__ nbr, const unsigned long long* __restrict__ valid,
                                                      const uint8_t* __restrict__ mask, const int* __restrict__ voff, int* __restrict__ base, float* __restrict__ vert,
                                                      float* __restrict__ nrm) {
    __shared__ unsigned long long w[36];           // valid, down
    __shared__ int pb[27];                         // the pool index of every neighbour, or -1
    __shared__ int red[8];
    const int tid = threadIdx.x, lane = tid & 63, lz = tid >> 6, lx = lane & 7, ly = lane >> 3;
    const int mk = (int)mask[(size_t)blockIdx.x * 512 + tid];
    int before, total;
    tm_mask_scan(mk, before, total);
    if (lane == 0) red[lz] = total;
    if (__syncthreads_or(mk != 0) == 0) {          // (uniform) a block without a vertex: only its run bases
        if (lane == 0) base[blockIdx.x * 8 + lz] = voff[blockIdx.x];
        return;
    }
    if (tid < 36) htm_stage<false>(valid, nbr + (size_t)blockIdx.x * 27, w, tid);
    else if (tid >= 64 && tid < 91) { const int r = nbr[(size_t)blockIdx.x * 27 + (tid - 64)]; pb[tid - 64] = r >= 0 ? order[r] : HTM_NONE; }
    __syncthreads();
    int at = voff[blockIdx.x];
    for (int q = 0; q < lz; q++) at += red[q];
    if (lane == 0) base[blockIdx.x * 8 + lz] = at;
    if (mk == 0) return;
    int b[3];
    hm_unkey(v.pool_key[order[blockIdx.x]], b);
    int idx = at + before;
#pragma unroll 1
    for (int code = 1; code < 8; code++) {
        if (!((mk >> (code - 1)) & 1)) continue;
        float p[3], n[3];
        htm_vertex(v, pb, w, b, lx, ly, lz, code, p, n);
        vert[(size_t)idx * 3] = p[0]; vert[(size_t)idx * 3 + 1] = p[1]; vert[(size_t)idx * 3 + 2] = p[2];
        if (nrm) { nrm[(size_t)idx * 3] = n[0]; nrm[(size_t)idx * 3 + 1] = n[1]; nrm[(size_t)idx * 3 + 2] = n[2]; }
        idx++;
    }
}

// toff: the exclusive block offsets k_select_scan left in the triangle table.
__global__ __launch_bounds__(512) void k_htm_triangles(const int* __restrict__ nbr, const unsigned long long* __restrict__ neg, const unsigned long long* __restrict__ valid,
                                                       const uint8_t* __restrict__ mask, const int* __restrict__ base, const int* __restrict__ toff, uint32_t* __restrict__ tris) {
    __shared__ unsigned long long w[36];           // negative, up
    __shared__ int rk[8];                          // the rank of the block and of its 7 upper neighbours (cx + 2 cy + 4 cz), or -1
    __shared__ int red[8];
    const int tid = threadIdx.x, lane = tid & 63, lz = tid >> 6, lx = lane & 7, ly = lane >> 3;
    const bool cell = mask[(size_t)blockIdx.x * 512 + tid] != 0 && ((valid[blockIdx.x * 8 + lz] >> lane) & 1ull);
    if (__syncthreads_or(cell) == 0) return;       // (uniform) no triangle starts in this block
    if (tid < 36) htm_stage<true>(neg, nbr + (size_t)blockIdx.x * 27, w, tid);
    else if (tid >= 64 && tid < 72) { const int q = tid - 64; rk[q] = nbr[(size_t)blockIdx.x * 27 + ((q >> 2) + 1) * 9 + (((q >> 1) & 1) + 1) * 3 + ((q & 1) + 1)]; }
    __syncthreads();
    int sg = 0, cnt = 0;
    if (cell) { sg = htm_corner_signs(w, lx, ly, lz); cnt = tm_cell_triangles(sg); }
    int before = 0, total = 0;
    if (__ballot(cnt != 0) != 0ull) tm_wave_scan<4>(cnt, before, total);
    if (lane == 0) red[lz] = total;
    __syncthreads();
    if (cnt == 0) return;
    int at = toff[blockIdx.x];
    for (int q = 0; q < lz; q++) at += red[q];
    size_t o = (size_t)(at + before) * 3;
#pragma unroll 1
    for (int p = 0; p < 6; p++) {
        const int q = TM_TABLE.q[p];
        int m = 0;
#pragma unroll
        for (int a = 0; a < 4; a++) m |= ((sg >> ((q >> (3 * a)) & 7)) & 1) << a;
        const uint32_t e = TM_TABLE.e[p][m];
        const int ns = 3 * (int)(e & 3u);
#pragma unroll 1
        for (int s = 0; s < ns; s++) {
            const int r = (int)((e >> (2 + 3 * s)) & 7u);
            const int qa = (q >> (3 * tm_edge_a(r))) & 7, qb = (q >> (3 * tm_edge_b(r))) & 7;
            const int x = lx + (qa & 1), y = ly + ((qa >> 1) & 1), z = lz + (qa >> 2);
            const int owner = rk[(x >> 3) | ((y >> 3) << 1) | ((z >> 3) << 2)];      // (exists: the cell is valid, so its corners are observed)
            tris[o++] = owner >= 0 ? tm_vertex_index(mask, base, owner * 512 + (((z & 7) << 6) | ((y & 7) << 3) | (x & 7)), qa ^ qb) : 0u;
        }
    }
}
