// dev_tsdf_hash_mesh_color.hpp -- per-vertex colours of the hashed model's mesh (icp_tsdf_mesh_color_hashed): k_htm_colors, one packed colour
// per vertex of icp_tsdf_mesh_hashed from the colour pool, placed where k_htm_vertices places that vertex.  k_tm_colors
// (dev_tsdf_mesh_color.hpp) read through dev_tsdf_hash_mesh.hpp's addressing.  Contract: include/icp_hip.h, DESIGN.md section 6zc;
// tests/htsdf_color_view_restatement.py states the same arithmetic in numpy.  Part of icp_device.hpp (included from there, inside namespace
// icpdev, after dev_tsdf_hash_mesh.hpp, dev_tsdf_mesh_color.hpp and dev_tsdf_hash_color.hpp).
// ------------------------------------------------------------------------------------------------
// The colour of the voxel (x, y, z), coordinates relative to the block in -1 .. 8, at the (pool index, local) pair its F is read from
// (a block that does not exist reads (0, 0, 0, 0), uncoloured)
__device__ __forceinline__ float4 htm_c(const float4* __restrict__ cpool, const int* __restrict__ pb, int x, int y, int z) {
    const int blk = pb[((z >> 3) + 1) * 9 + ((y >> 3) + 1) * 3 + ((x >> 3) + 1)];
    return blk >= 0 ? cpool[(size_t)blk * 512 + (size_t)(((z & 7) << 6) | ((y & 7) << 3) | (x & 7))] : make_float4(0.f, 0.f, 0.f, 0.f);
}

// htm_f, restated: F of the voxel (x, y, z) through the staged pool indices.  Calling htm_f itself from a second kernel changed the
// instructions the compiler gives k_htm_vertices (its LDS index arithmetic and register allocation), so this file keeps a copy of its own.
__device__ __forceinline__ float htm_cf(const float2* __restrict__ pool, const int* __restrict__ pb, int x, int y, int z) {
    const int blk = pb[((z >> 3) + 1) * 9 + ((y >> 3) + 1) * 3 + ((x >> 3) + 1)];
    return blk >= 0 ? pool[(size_t)blk * 512 + (size_t)(((z & 7) << 6) | ((y & 7) << 3) | (x & 7))].x : 0.f;
}

// tm_vertex_color on the blocks: vertex `code` of the voxel (x, y, z); the far end (x, y, z) + d may lie in a neighbouring block.
__device__ __forceinline__ uint32_t htm_vertex_color(const float2* __restrict__ pool, const float4* __restrict__ cpool, const int* __restrict__ pb, int x, int y, int z, int code) {
    const int dx = code & 1, dy = (code >> 1) & 1, dz = code >> 2;
    const float4 a = htm_c(cpool, pb, x, y, z), b = htm_c(cpool, pb, x + dx, y + dy, z + dz);
    const bool ha = a.w > 0.f, hb = b.w > 0.f;
    if (!ha && !hb) return 0u;
    float r, gr, bl;
    if (ha && hb) {
        const float fv = htm_cf(pool, pb, x, y, z), fd = htm_cf(pool, pb, x + dx, y + dy, z + dz);
        const float t = fv / (fv - fd);
        r = tm_lerp(a.x, b.x, t); gr = tm_lerp(a.y, b.y, t); bl = tm_lerp(a.z, b.z, t);
    } else { r = ha ? a.x : b.x; gr = ha ? a.y : b.y; bl = ha ? a.z : b.z; }
    return tsdf_color_pack(r, gr, bl);
}

// One work-group per block in rank order, one wave per z-layer, a lane one (x, y): k_htm_vertices' layout, run after it.  A vertex's index
// is base[run] (which that kernel wrote) + its ballot rank, codes ascending.  The 27 neighbours' pool indices are staged in LDS once.
// No atomics.
__global__ __launch_bounds__(512) void k_htm_colors(const float2* __restrict__ pool, const float4* __restrict__ cpool, const int* __restrict__ order, const int* __restrict__ nbr,
                                                    const uint8_t* __restrict__ mask, const int* __restrict__ base, uint32_t* __restrict__ rgba) {
    __shared__ int pb[27];                         // the pool index of every neighbour, or -1
    const int tid = threadIdx.x, lane = tid & 63, lz = tid >> 6, lx = lane & 7, ly = lane >> 3;
    const int mk = (int)mask[(size_t)blockIdx.x * 512 + tid];
    int before, total;
    tm_mask_scan(mk, before, total);
    if (__syncthreads_or(mk != 0) == 0) return;    // (uniform) a block without a vertex
    if (tid < 27) { const int r = nbr[(size_t)blockIdx.x * 27 + tid]; pb[tid] = r >= 0 ? order[r] : HTM_NONE; }
    __syncthreads();
    if (mk == 0) return;
    int idx = base[blockIdx.x * 8 + lz] + before;
#pragma unroll 1
    for (int code = 1; code < 8; code++) {
        if (!((mk >> (code - 1)) & 1)) continue;
        rgba[idx++] = htm_vertex_color(pool, cpool, pb, lx, ly, lz, code);
    }
}
