// dev_mesh.hpp -- the triangulated depth mesh of one frame in world coordinates: SimpleMesh(sensor, cameraPose, edgeThreshold)
// (SimpleMesh.h:36-119), what reconstructRoom writes after every frame (saveRoomToFile, utils.h:179-193).
// Part of icp_device.hpp (included from there, inside namespace icpdev); see that file for the build contract.
// ------------------------------------------------------------------------------------------------
// Three passes over one frame (icp_depth_mesh):
//   k_mesh_vertices  one thread per pixel: the vertex (all width*height of them, MINF where the depth is MINF) and its colour,
//                    re-projected from the stored fp32 vertex into the colour frame (:70-80)
//   k_mesh_count     one thread per 2x2 quad: its 0-2 triangles (:86-118), kept triangles per 256-quad block
//   k_mesh_scatter   the same quads again, each kept triangle written at its rank in addFace order (quad-major, row-major, first
//                    triangle before the second); k_select_scan turns the block counts into offsets in between
// The triangle passes read the vertices the vertex pass wrote, so every test sees exactly the stored positions.

// Everything the vertex pass needs about the frame, passed by value.
struct MeshFrame {
    const float* depth; const uint8_t* rgbx;       // device; rgbx null = no colours
    int width, height, color_width, color_height;
    float fx, fy, cx, cy;
    float m[12];                                   // P^-1 E^-1 in depth_point's layout: 3x3 row-major, then t
    float c[12];                                   // Kc Ec P, 3x4 row-major
};

// (unsigned int)x of a float as gcc compiles it for x86-64: cvttss2si to int64 (NaN and out-of-range give INT64_MIN), low 32 bits.
__device__ __forceinline__ uint32_t x86_float_to_u32(float x) {
    const long long t = (x >= -9223372036854775808.f && x < 9223372036854775808.f) ? (long long)x : -9223372036854775807ll - 1;
    return (uint32_t)(unsigned long long)t;
}

// Colour of a vertex (:70-80): project the vertex with Kc Ec P, dehomogenise, floor, cast, clamp to the frame, and read bytes
// 4 idxCol .. 4 idxCol + 3 of the RGBX frame as one little-endian word.
__device__ __forceinline__ uint32_t mesh_color(const MeshFrame& f, float x, float y, float z) {
    const float* C = f.c;
    const float q0 = (C[0] * x + (C[1] * y + C[2] * z)) + C[3];
    const float q1 = (C[4] * x + (C[5] * y + C[6] * z)) + C[7];
    const float q2 = (C[8] * x + (C[9] * y + C[10] * z)) + C[11];
    uint32_t uc = x86_float_to_u32(floorf(q0 / q2)), vc = x86_float_to_u32(floorf(q1 / q2));
    if (uc >= (uint32_t)f.color_width) uc = (uint32_t)f.color_width - 1;
    if (vc >= (uint32_t)f.color_height) vc = (uint32_t)f.color_height - 1;
    return ((const uint32_t*)f.rgbx)[(size_t)vc * f.color_width + uc];
}

// Vertex pass: xyz interleaved (3 floats per pixel); rgba (optional, needs f.rgbx) one packed word per pixel, 0 for a MINF pixel.
__global__ __launch_bounds__(256) void k_mesh_vertices(const MeshFrame f, float* __restrict__ xyz, uint32_t* __restrict__ rgba) {
    const unsigned int t = blockIdx.x * 256u + threadIdx.x;
    if (t >= (unsigned int)(f.width * f.height)) return;
    const int idx = (int)t, v = idx / f.width, u = idx - v * f.width;
    const float d = f.depth[idx];
    float p0, p1, p2;
    depth_point(d, u, v, f.fx, f.fy, f.cx, f.cy, f.m, p0, p1, p2);
    xyz[(size_t)idx * 3] = p0; xyz[(size_t)idx * 3 + 1] = p1; xyz[(size_t)idx * 3 + 2] = p2;
    if (rgba) rgba[idx] = d == -INFINITY ? 0u : mesh_color(f, p0, p1, p2);
}

// (a - b).norm() of two Vector4f with equal w: the SSE2 packet reduction (dx^2 + dz^2) + (dy^2 + 0), then sqrtf.
__device__ __forceinline__ float mesh_edge(const float (&a)[3], const float (&b)[3]) {
    const float dx = a[0] - b[0], dy = a[1] - b[1], dz = a[2] - b[2];
    return sqrtf((dx * dx + dz * dz) + dy * dy);
}

// Quad q (row i = q / (width - 1), column j): first vertex i0 = i * width + j, and whether (i0, i1, i2) and (i1, i3, i2) are kept:
// all three vertices finite and every edge shorter than thr (a NaN edge or threshold keeps nothing).
__device__ __forceinline__ void mesh_quad(const float* __restrict__ xyz, int width, int q, float thr, int& i0, bool& first, bool& second) {
    const int i = q / (width - 1), j = q - i * (width - 1);
    i0 = i * width + j;
    const float* s0 = xyz + (size_t)i0 * 3;
    const float* s1 = s0 + (size_t)width * 3;
    float p0[3], p1[3], p2[3], p3[3];
#pragma unroll
    for (int k = 0; k < 3; k++) { p0[k] = s0[k]; p2[k] = s0[3 + k]; p1[k] = s1[k]; p3[k] = s1[3 + k]; }
    const bool f0 = finite3(p0[0], p0[1], p0[2]), f1 = finite3(p1[0], p1[1], p1[2]);
    const bool f2 = finite3(p2[0], p2[1], p2[2]), f3 = finite3(p3[0], p3[1], p3[2]);
    const bool e12 = thr > mesh_edge(p1, p2);
    first = f0 && f1 && f2 && e12 && thr > mesh_edge(p0, p1) && thr > mesh_edge(p0, p2);
    second = f1 && f2 && f3 && e12 && thr > mesh_edge(p3, p1) && thr > mesh_edge(p3, p2);
}

// Pass 1 of the stable compaction: kept triangles per block of 256 quads.
__global__ __launch_bounds__(256) void k_mesh_count(const float* __restrict__ xyz, int width, int n_quads, float thr, int* __restrict__ block_counts) {
    const int q = blockIdx.x * 256 + threadIdx.x;
    bool first = false, second = false;
    if (q < n_quads) { int i0; mesh_quad(xyz, width, q, thr, i0, first, second); }
    const int a = __syncthreads_count(first ? 1 : 0);
    const int b = __syncthreads_count(second ? 1 : 0);
    if (threadIdx.x == 0) block_counts[blockIdx.x] = a + b;
}

// Pass 2: quad q's first triangle goes to block offset + the kept triangles of the quads before it in its block
// (mbcnt of both ballots, then the waves before it); its second triangle one slot later when the first was kept.
__global__ __launch_bounds__(256) void k_mesh_scatter(const float* __restrict__ xyz, int width, int n_quads, float thr,
                                                      const int* __restrict__ block_offsets, uint32_t* __restrict__ tris) {
    __shared__ int wave_cnt[4];
    const int q = blockIdx.x * 256 + threadIdx.x, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    bool first = false, second = false; int i0 = 0;
    if (q < n_quads) mesh_quad(xyz, width, q, thr, i0, first, second);
    const unsigned long long ma = __ballot(first), mb = __ballot(second);
    const int rank = __builtin_amdgcn_mbcnt_hi((unsigned int)(ma >> 32), __builtin_amdgcn_mbcnt_lo((unsigned int)ma, 0u)) +
                     __builtin_amdgcn_mbcnt_hi((unsigned int)(mb >> 32), __builtin_amdgcn_mbcnt_lo((unsigned int)mb, 0u));
    if (lane == 0) wave_cnt[w] = __popcll(ma) + __popcll(mb);
    __syncthreads();
    int off = block_offsets[blockIdx.x];
    for (int k = 0; k < w; k++) off += wave_cnt[k];
    uint32_t* t = tris + (size_t)(off + rank) * 3;
    const uint32_t v0 = (uint32_t)i0, v1 = v0 + (uint32_t)width, v2 = v0 + 1, v3 = v1 + 1;
    if (first) { t[0] = v0; t[1] = v1; t[2] = v2; t += 3; }
    if (second) { t[0] = v1; t[1] = v3; t[2] = v2; }
}
