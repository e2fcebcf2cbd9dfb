// dev_depth.hpp -- depth frame -> resident cloud in one device pass (RGB-D input, PointCloud.h:78-165).
// Part of icp_device.hpp (included from there, inside namespace icpdev); see that file for the build contract.
// ------------------------------------------------------------------------------------------------
// The per-pixel arithmetic of PointCloud(depthMap, colorFrame, K, extrinsics, width, height, keepOriginalSize, downsampleFactor,
// maxDistance), shared by k_backproject (organised output, icp_backproject_depth) and the two kernels below, which write the
// constructor's filtered, strided cloud straight into the SoA planes of a context cloud (icp_set_target_depth / _source_depth).
// Quirks kept: normals are NOT rotated by the extrinsics (:128-129); borders and pixels next to a hole are MINF (:117-141);
// the colour of pixel i is read from bytes i..i+3 of the RGBX frame instead of 4i..4i+3 (:156-157) unless fix_color_index is set,
// clamped to the frame's last byte at the very end (the reference reads past the frame there).

// Back-projection of pixel idx = v * width + u (:101-110).  inv: 3x3 row-major R^-1, then t^-1 (depthExtrinsics.inverse()).
__device__ __forceinline__ void depth_point(float d, int u, int v, float fx, float fy, float cx, float cy, const float* __restrict__ inv,
                                            float& p0, float& p1, float& p2) {
    p0 = -INFINITY; p1 = -INFINITY; p2 = -INFINITY;
    if (d != -INFINITY) {
        const float a = ((float)u - cx) / fx * d, b = ((float)v - cy) / fy * d, c = d;
        p0 = (inv[0] * a + (inv[1] * b + inv[2] * c)) + inv[9];
        p1 = (inv[3] * a + (inv[4] * b + inv[5] * c)) + inv[10];
        p2 = (inv[6] * a + (inv[7] * b + inv[8] * c)) + inv[11];
    }
}
// Central-difference normal of pixel idx (:113-141): MINF on the border and where a gradient is not finite or exceeds maxDistance / 2.
__device__ __forceinline__ void depth_normal(const float* __restrict__ depth, int idx, int u, int v, int width, int height, float max_distance_halved,
                                             float& n0, float& n1, float& n2) {
    n0 = -INFINITY; n1 = -INFINITY; n2 = -INFINITY;
    if (v >= 1 && v < height - 1 && u >= 1 && u < width - 1) {
        const float du = 0.5f * (depth[idx + 1] - depth[idx - 1]);
        const float dv = 0.5f * (depth[idx + width] - depth[idx - width]);
        if (isfinite(du) && isfinite(dv) && !(fabsf(du) > max_distance_halved) && !(fabsf(dv) > max_distance_halved)) {
            const float x = -du, y = -dv, z = 1.f;
            const float sq = x * x + (y * y + z * z);
            const float len = sqrtf(sq);
            n0 = x / len; n1 = y / len; n2 = z / len;
        }
    }
}
// Colour bytes of pixel idx (:155-157) as one little-endian word (byte k = channel k).
__device__ __forceinline__ uint32_t depth_color(const uint8_t* __restrict__ rgbx, int idx, int n, int fix_color_index) {
    const size_t base = fix_color_index ? (size_t)idx * 4 : (size_t)idx;
    const size_t last = (size_t)n * 4 - 1;
    uint32_t w = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) w |= (uint32_t)rgbx[base + k <= last ? base + k : last] << (8 * k);
    return w;
}

// Everything the two kernels need about the frame, passed by value (no device copy of the inverse).
struct DepthFrame {
    const float* depth; const uint8_t* rgbx;                 // device; rgbx may be null
    int width, height, factor, count;                        // count = ceil(width * height / factor) candidates i = 0, f, 2f, ...
    float fx, fy, cx, cy, max_distance_halved;
    float inv[12];
    int keep_all, fix_color_index;
};

// Candidate j -> pixel i = j * factor; its point, normal and whether the constructor keeps it (:146-152).
__device__ __forceinline__ bool depth_candidate(const DepthFrame& f, int j, float (&p)[3], float (&nm)[3]) {
    const int i = j * f.factor;
    const int v = i / f.width, u = i - v * f.width;
    depth_point(f.depth[i], u, v, f.fx, f.fy, f.cx, f.cy, f.inv, p[0], p[1], p[2]);
    depth_normal(f.depth, i, u, v, f.width, f.height, f.max_distance_halved, nm[0], nm[1], nm[2]);
    return f.keep_all || (finite3(p[0], p[1], p[2]) && finite3(nm[0], nm[1], nm[2]));
}

// Pass 1 of the stable compaction: kept candidates per 256-candidate block.  k_select_scan (one block, carry across its 1024-wide
// chunks) then turns the counts into exclusive block offsets and the total.
__global__ __launch_bounds__(256) void k_depth_count(const DepthFrame f, int* __restrict__ block_counts) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    bool keep = false;
    if (j < f.count) { float p[3], nm[3]; keep = depth_candidate(f, j, p, nm); }
    const int c = __syncthreads_count(keep ? 1 : 0);
    if (threadIdx.x == 0) block_counts[blockIdx.x] = c;
}

// Pass 2: the same candidates again (the arithmetic is cheaper than a round trip of the organised cloud through memory), each kept
// one written at block offset + rank among the kept candidates before it in its block -- the push_back order of :154-163.
// Planes as upload_cloud leaves them: x y z padded with +inf and cr cg cb with 0 up to the next multiple of 64 when pad is set
// (a target), normals n entries, colours (packed + features, k_colors) only with a colour frame.
struct DepthOut { float *x, *y, *z, *nx, *ny, *nz, *cr, *cg, *cb; uint32_t* rgba; };
__global__ __launch_bounds__(256) void k_depth_scatter(const DepthFrame f, const int* __restrict__ block_offsets, const int* __restrict__ total, int pad,
                                                       const DepthOut o) {
    __shared__ int wave_cnt[4];
    const int j = blockIdx.x * 256 + threadIdx.x, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    float p[3], nm[3];
    const bool keep = j < f.count && depth_candidate(f, j, p, nm);
    const unsigned long long m = __ballot(keep);
    const int rank = __builtin_amdgcn_mbcnt_hi((unsigned int)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned int)m, 0u));
    if (lane == 0) wave_cnt[w] = __popcll(m);
    __syncthreads();
    int off = block_offsets[blockIdx.x];
    for (int q = 0; q < w; q++) off += wave_cnt[q];
    if (keep) {
        const int t = off + rank;
        o.x[t] = p[0]; o.y[t] = p[1]; o.z[t] = p[2];
        o.nx[t] = nm[0]; o.ny[t] = nm[1]; o.nz[t] = nm[2];
        if (f.rgbx) {
            const uint32_t v = depth_color(f.rgbx, j * f.factor, f.width * f.height, f.fix_color_index);
            o.rgba[t] = v;
            color_features(v, o.cr[t], o.cg[t], o.cb[t]);
        }
    }
    if (pad) {
        const int n = *total, npad = (n + 63) / 64 * 64;
        if (j >= n && j < npad) {
            o.x[j] = INFINITY; o.y[j] = INFINITY; o.z[j] = INFINITY;
            if (f.rgbx) { o.cr[j] = 0.f; o.cg[j] = 0.f; o.cb[j] = 0.f; }
        }
    }
}

// ConvergenceMeasure(source.getPoints(), transformPoints(source.getPoints(), gt)) (main.cpp:299-305) from the resident source:
// the reference cloud is the source moved by gt (column-major, utils.h:106-118 arithmetic), both built on the device.
struct Pose16 { float m[16]; };
__global__ void k_conv_from_source(const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ z, int n, const Pose16 gt,
                                   float* __restrict__ sx, float* __restrict__ sy, float* __restrict__ sz,
                                   float* __restrict__ rx, float* __restrict__ ry, float* __restrict__ rz) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float a = x[i], b = y[i], c = z[i];
    sx[i] = a; sy[i] = b; sz[i] = c;
    xform_point(gt.m, a, b, c, rx[i], ry[i], rz[i]);
}
