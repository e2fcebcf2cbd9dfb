// dev_tsdf_mesh_color.hpp -- per-vertex colours of the model mesh (icp_tsdf_mesh_color): k_tm_colors, one packed colour per vertex of
// icp_tsdf_mesh from the volume's colour array, placed as k_tm_vertices places its vertices.  Contract: include/icp_hip.h, DESIGN.md
// section 6p.  Part of icp_device.hpp (included from there, inside namespace icpdev, after dev_tsdf_mesh.hpp).  A file of its own because
// tests/tsdf_mesh_lockstep.cpp compiles dev_tsdf_mesh.hpp on the host with the types that header needed when it was written;
// tests/tsdf_mesh_color_lockstep.cpp does the same for this one.
// ------------------------------------------------------------------------------------------------
// The colour of vertex `code` of voxel l: both ends coloured (Wc > 0): the lerp of the two at the vertex's t; one end: that end's colour;
// neither: 0.  Packed as the ray-cast packs it (tsdf_color_byte).
__device__ __forceinline__ uint32_t tm_vertex_color(const TsdfVol& v, const float4* __restrict__ col, const TmGrid& g, int l, int code) {
    const int m = l + (code & 1) + ((code >> 1) & 1) * g.nx + (code >> 2) * g.plane;
    const float4 a = col[l], b = col[m];
    const bool ha = a.w > 0.f, hb = b.w > 0.f;
    if (!ha && !hb) return 0u;
    float r, gr, bl;
    if (ha && hb) {
        const float fv = v.vox[l].x, fd = v.vox[m].x;
        const float t = fv / (fv - fd);
        r = tm_lerp(a.x, b.x, t); gr = tm_lerp(a.y, b.y, t); bl = tm_lerp(a.z, b.z, t);
    } else { r = ha ? a.x : b.x; gr = ha ? a.y : b.y; bl = ha ? a.z : b.z; }
    return tsdf_color_pack(r, gr, bl);
}

// The vertex order of k_tm_vertices (block offset + the waves before + ballot rank), one packed colour per vertex.  Every ballot sits in
// uniform flow: the scans run for all lanes of a wave, the per-vertex work hangs off them.
__global__ __launch_bounds__(256) void k_tm_colors(const TsdfVol v, const float4* __restrict__ col, const TmGrid g, const uint8_t* __restrict__ mask,
                                                   const int* __restrict__ voff, uint32_t* __restrict__ rgba) {
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
        int before, total;
        tm_mask_scan(mk[r], before, total);
        if (mk[r] != 0) {
            int idx = at + before;
#pragma unroll 1
            for (int code = 1; code < 8; code++) {
                if (!((mk[r] >> (code - 1)) & 1)) continue;
                rgba[idx++] = tm_vertex_color(v, col, g, l, code);
            }
        }
        at += total;
    }
}
