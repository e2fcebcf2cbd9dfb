// dev_depth_filter.hpp -- the bilateral depth filter in front of the trackers (icp_set_depth_filter_options, icp_filter_depth).  Contract:
// include/icp_hip.h, DESIGN.md section 6zd.  Included from icp_device.hpp, inside namespace icpdev.
//
// k_depth_filter<R>: one thread per pixel, blocks of DF_TW x DF_TH = 32 x 8 pixels (four waves, each two rows of 32).  The block stages its
// tile with a halo of R pixels, the (2R + 1)^2 spatial weights and the 256 range weights in LDS; no weight is computed on the device.
//   * Tile pitch: a wave reads, per tap, 32 consecutive floats of one tile row in each of its halves.  ds_read_b32 conflicts only within a
//     32-lane half, and 32 consecutive dwords fall on 32 different banks whatever the pitch is: no padding is needed.
//   * Spatial weight: its index is a compile-time constant of the unrolled tap, one address per wave (a broadcast).
//   * Range weight: a gather by q = (int)t.  Lanes with the same q share an address (broadcast); lanes of one half with different q can
//     fall on one bank only when their q differ by a multiple of 32, i.e. their |n - c| by more than a sigma_range -- across a depth edge.
//   * Pixels outside the image are staged as -inf, which is not usable: the rule's "skip a neighbour outside the image" is then the same
//     test as "skip unless usable", and an image smaller than the tile or than the radius needs no case of its own.
// The accumulation runs in the contract's order in every thread: no cross-lane reduction, no atomics.
constexpr int DF_TW = ICP_DEPTH_FILTER_TILE_W, DF_TH = ICP_DEPTH_FILTER_TILE_H;
static_assert(DF_TW * DF_TH == ICP_DEPTH_FILTER_RANGE_BINS, "one thread stages one range weight");

struct DepthFilterArgs {
    const float* in; float* out;         // width x height, row-major
    const float* spatial; const float* range;   // (2R + 1)^2 and 256 weights (icp_depth_filter_tables)
    int width, height;
    float inv_bin;
};

__device__ __forceinline__ bool df_usable(float d) { return d > 0.f && d <= FLT_MAX; }      // finite and > 0 (a NaN fails the first test)

template <int R>
__global__ __launch_bounds__(DF_TW * DF_TH) void k_depth_filter(DepthFilterArgs a) {
    constexpr int W = 2 * R + 1, PW = DF_TW + 2 * R, PH = DF_TH + 2 * R;
    __shared__ float s_tile[PH * PW];
    __shared__ float s_range[ICP_DEPTH_FILTER_RANGE_BINS];
    __shared__ float s_spatial[W * W];
    const int tid = threadIdx.y * DF_TW + threadIdx.x;
    const int x0 = (int)blockIdx.x * DF_TW - R, y0 = (int)blockIdx.y * DF_TH - R;
    s_range[tid] = a.range[tid];
    if (tid < W * W) s_spatial[tid] = a.spatial[tid];
    for (int i = tid; i < PH * PW; i += DF_TW * DF_TH) {
        const int ly = i / PW, lx = i - ly * PW, gx = x0 + lx, gy = y0 + ly;
        const bool inside = gx >= 0 && gx < a.width && gy >= 0 && gy < a.height;
        s_tile[i] = inside ? a.in[(size_t)gy * a.width + gx] : -INFINITY;
    }
    __syncthreads();
    const int u = x0 + R + (int)threadIdx.x, v = y0 + R + (int)threadIdx.y;
    if (u >= a.width || v >= a.height) return;
    const float* centre = s_tile + (threadIdx.y + R) * PW + threadIdx.x + R;
    const float c = *centre;
    float o = c;
    if (df_usable(c)) {
        float num = 0.f, den = 0.f;
#pragma unroll
        for (int dy = -R; dy <= R; dy++) {
#pragma unroll
            for (int dx = -R; dx <= R; dx++) {
                const float n = centre[dy * PW + dx];
                if (!df_usable(n)) continue;
                const float delta = n - c;
                const float e = delta * delta;
                const float t = e * a.inv_bin;
                if (!(t < 256.0f)) continue;
                const int q = (int)t;                        // 0 .. 255: t >= 0 and t < 256
                const float w = s_spatial[(dy + R) * W + (dx + R)] * s_range[q];
                num = num + w * n;
                den = den + w;
            }
        }
        o = num / den;
    }
    a.out[(size_t)v * a.width + u] = o;
}
