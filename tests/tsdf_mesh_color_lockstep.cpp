// tsdf_mesh_color_lockstep.cpp -- k_tm_colors of icp-variants_amd/csrc/dev_tsdf_mesh_color.hpp, the source as it stands, run on the host behind
// the counting kernels of dev_tsdf_mesh.hpp, as tests/tsdf_mesh_lockstep.cpp runs those: one std::thread per lane, 256 per block, a ballot
// is a barrier among the 64 threads of its wave, so a ballot that the lanes of a wave do not all reach hangs here and not on a device.
// fp32 on the host is IEEE with -ffp-contract=off, so the colours are compared bit for bit with tests/tsdf_color_restatement.py
// (tests/test_tsdf_color_host.py builds and runs this with g++ -std=c++20).  No GPU needed.
// usage: tsdf_mesh_color_lockstep in.bin out.bin
//   in : int32 nx ny nz, float32 ox oy oz s min_weight, then nx ny nz (tsdf, weight) pairs, then nx ny nz (R, G, B, Wc) quadruples, x fastest
//   out: int32 V, V x 4 bytes
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cmath>
#include <vector>
#include <thread>
#include <barrier>
#include <memory>
#include <atomic>
#define __global__
#define __device__
#define __host__
#define __forceinline__ inline
#define __restrict__
#define __constant__
#define __launch_bounds__(x)
#define __shared__ static
struct float2 { float x, y; };
static inline float2 make_float2(float x, float y) { return float2{x, y}; }
struct float4 { float x, y, z, w; };
struct dim3x { int x = 0, y = 0, z = 0; };
static thread_local dim3x threadIdx, blockIdx;
static std::barrier<>* g_block_bar;
static std::barrier<>* g_wave_bar[4];
static std::atomic<unsigned long long> g_bal[4][2];
static std::atomic<int> g_phase[4];
static inline void __syncthreads() { g_block_bar->arrive_and_wait(); }
static thread_local int t_flip = 0;
static inline unsigned long long __ballot(int pred) {
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63, f = t_flip; t_flip ^= 1;
    if (pred) g_bal[w][f].fetch_or(1ull << lane);
    g_wave_bar[w]->arrive_and_wait();
    const unsigned long long r = g_bal[w][f].load();
    g_wave_bar[w]->arrive_and_wait();
    if (lane == 0) g_bal[w][f].store(0);      // the other slot is used by the next ballot; this one is cleared before its reuse two ballots later
    return r;
}
static inline unsigned __builtin_amdgcn_mbcnt_lo(unsigned m, unsigned acc) { const int lane = threadIdx.x & 63; const unsigned k = lane >= 32 ? 0xFFFFFFFFu : ((1u << lane) - 1u); return acc + __builtin_popcount(m & k); }
static inline unsigned __builtin_amdgcn_mbcnt_hi(unsigned m, unsigned acc) { const int lane = threadIdx.x & 63; const unsigned k = lane <= 32 ? 0u : ((1u << (lane - 32)) - 1u); return acc + __builtin_popcount(m & k); }
static inline int __popcll(unsigned long long v) { return __builtin_popcountll(v); }
static inline int __popc(unsigned v) { return __builtin_popcount(v); }
struct TsdfVol { float2* vox; int nx, ny, nz; float ox, oy, oz, s; float trunc, max_w, min_d, max_d, step; };
namespace icpdev {
#include "dev_tsdf_color.hpp"
#include "dev_tsdf_mesh.hpp"
#include "dev_tsdf_mesh_color.hpp"
}
using namespace icpdev;
template <class F> void launch(int nblocks, F f) {
    for (int b = 0; b < nblocks; b++) {
        std::barrier<> bb(256), w0(64), w1(64), w2(64), w3(64);
        g_block_bar = &bb; g_wave_bar[0] = &w0; g_wave_bar[1] = &w1; g_wave_bar[2] = &w2; g_wave_bar[3] = &w3;
        for (auto& a : g_bal) for (auto& x : a) x.store(0);
        std::vector<std::thread> th;
        for (int t = 0; t < 256; t++) th.emplace_back([=] { threadIdx.x = t; blockIdx.x = b; t_flip = 0; f(); });
        for (auto& t : th) t.join();
    }
}
static TmDiv tm_make_div(uint32_t d) { int L = 0; while (((uint64_t)1 << L) < d) L++; TmDiv r; r.m = (uint32_t)((((uint64_t)1 << 32) * (((uint64_t)1 << L) - d)) / d + 1); r.s1 = L < 1 ? L : 1; r.s2 = L > 1 ? L - 1 : 0; return r; }
static void scan(int* t, int n, int* total) { int c = 0; for (int i = 0; i < n; i++) { int v = t[i]; t[i] = c; c += v; } *total = c; }
int main(int argc, char** argv) {
    if (argc != 3) return 1;
    FILE* f = fopen(argv[1], "rb");
    int d[3]; float h[5];
    if (!f || fread(d, 4, 3, f) != 3 || fread(h, 4, 5, f) != 5) return 1;
    TmGrid g; g.nx = d[0]; g.ny = d[1]; g.nz = d[2]; g.plane = g.nx * g.ny; g.n = g.plane * g.nz; g.nruns = (g.n + 63) / 64;
    g.dx = tm_make_div(g.nx); g.dp = tm_make_div(g.plane);
    std::vector<float2> vox(g.n);
    std::vector<float4> col(g.n);
    if (fread(vox.data(), 8, g.n, f) != (size_t)g.n || fread(col.data(), 16, g.n, f) != (size_t)g.n) return 1;
    fclose(f);
    TsdfVol v{}; v.vox = vox.data(); v.nx = g.nx; v.ny = g.ny; v.nz = g.nz; v.ox = h[0]; v.oy = h[1]; v.oz = h[2]; v.s = h[3];
    const int nb = (g.n + TM_BLOCK_VOXELS - 1) / TM_BLOCK_VOXELS;
    std::vector<unsigned long long> obs(g.nruns, ~0ull), neg(g.nruns, ~0ull), valid(g.nruns, ~0ull);
    std::vector<uint8_t> mask((size_t)g.nruns * 64, 0xEE);
    std::vector<int> vblk(nb, -1), tblk(nb, -1);
    launch(nb, [&] { k_tm_classify(vox.data(), g, h[4], obs.data(), neg.data()); });
    launch(nb, [&] { k_tm_cells(g, obs.data(), valid.data()); });
    launch(nb, [&] { k_tm_count(g, neg.data(), valid.data(), mask.data(), vblk.data(), tblk.data()); });
    int nv, nt; scan(vblk.data(), nb, &nv); scan(tblk.data(), nb, &nt);
    std::vector<uint32_t> rgba((size_t)nv + 1, 0xDEADBEEF);
    launch(nb, [&] { k_tm_colors(v, col.data(), g, mask.data(), vblk.data(), rgba.data()); });
    if (rgba[(size_t)nv] != 0xDEADBEEF) { printf("overrun\n"); return 2; }
    for (int i = 0; i < nv; i++) if (rgba[i] == 0xDEADBEEF) { printf("vertex %d not written\n", i); return 3; }
    f = fopen(argv[2], "wb"); fwrite(&nv, 4, 1, f); fwrite(rgba.data(), 4, nv, f); fclose(f);
    printf("V %d\n", nv);
    return 0;
}
