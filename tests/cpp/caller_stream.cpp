// Contexts on the caller's stream (icp_ctx_create_on_stream), driven from C++ with the caller's own work on the stream in front of every
// library call.  tests/test_gpu_context_reuse.py::test_caller_stream builds this with hipcc, runs it on the file it writes and compares
// the printed words with the same calls on a default context.
//
// usage: caller_stream <input file>
// input: arrays of 4-byte words, each behind its int32 word count, in this order: source points, source normals, target points, target
//        normals, a depth frame (width x height floats), the camera (fx, fy, cx, cy, width, height as floats), the volume (nx, ny, nz,
//        ox, oy, oz, voxel size as floats), mesh vertices, mesh triangles, the clustering grid (cell size, ox, oy, oz).
// output: one line per result, "<label> <hex word> ...", and a last line "streams ok".
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "icp_hip.h"

namespace {
typedef std::vector<uint32_t> Words;

#define HIP_OK(expr)                                                                                   \
    do {                                                                                               \
        hipError_t e__ = (expr);                                                                       \
        if (e__ != hipSuccess) {                                                                       \
            fprintf(stderr, "%s failed: %s (line %d)\n", #expr, hipGetErrorString(e__), __LINE__);     \
            exit(3);                                                                                   \
        }                                                                                              \
    } while (0)
#define ICP(ctx, expr)                                                                                 \
    do {                                                                                               \
        int rc__ = (expr);                                                                             \
        if (rc__ != ICP_OK) {                                                                          \
            fprintf(stderr, "%s returned %d: %s (line %d)\n", #expr, rc__, icp_last_error(ctx), __LINE__); \
            exit(4);                                                                                   \
        }                                                                                              \
    } while (0)

Words read_array(FILE* f) {
    int32_t n = 0;
    if (fread(&n, 4, 1, f) != 1 || n < 0) { fprintf(stderr, "short input\n"); exit(2); }
    Words w((size_t)n);
    if (n && fread(w.data(), 4, (size_t)n, f) != (size_t)n) { fprintf(stderr, "short input\n"); exit(2); }
    return w;
}
const float* F(const Words& w) { return (const float*)w.data(); }
void print_words(const std::string& label, const void* p, size_t n_words) {
    const uint32_t* w = (const uint32_t*)p;
    printf("%s", label.c_str());
    for (size_t i = 0; i < n_words; i++) printf(" %08x", w[i]);
    printf("\n");
}

struct Input { Words sp, sn, tp, tn, depth, cam, vol, mv, mt, grid; };

// The caller's own work: a 64 MB memset on the stream, in front of every library call.
struct Caller {
    hipStream_t stream; void* block; unsigned value;
    void work() { HIP_OK(hipMemsetAsync(block, (int)(value++ & 0xFF), (size_t)64 << 20, stream)); }
};

void load_bunny(icp_ctx* c, Caller& k, const Input& in, int metric) {
    icp_params p;
    icp_params_default(&p);
    p.metric = metric; p.n_iterations = 5; p.knn_backend = ICP_KNN_LBVH; p.max_distance = 0.0003f;
    k.work(); ICP(c, icp_set_params(c, &p));
    k.work(); ICP(c, icp_set_target(c, F(in.tp), F(in.tn), nullptr, (int32_t)(in.tp.size() / 3)));
    k.work(); ICP(c, icp_set_source(c, F(in.sp), F(in.sn), nullptr, (int32_t)(in.sp.size() / 3)));
}
void run_bunny(icp_ctx* c, Caller& k, const std::string& label) {
    float pose[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    icp_iter_stats st[8];
    int32_t n = 0;
    k.work(); ICP(c, icp_run(c, pose, st, 8, &n));
    print_words(label + "_pose", pose, 16);
    Words rec;
    for (int i = 0; i < n && i < 8; i++) {
        rec.push_back((uint32_t)st[i].n_src); rec.push_back((uint32_t)st[i].n_valid); rec.push_back((uint32_t)st[i].status);
        const uint32_t* w = (const uint32_t*)st[i].pose;
        rec.insert(rec.end(), w, w + 16);
    }
    print_words(label + "_records", rec.data(), rec.size());
}
void run_volume(icp_ctx* c, Caller& k, const Input& in, const std::string& label) {
    icp_tsdf_options o;
    icp_tsdf_options_default(&o);
    const float* v = F(in.vol);
    for (int a = 0; a < 3; a++) { o.dims[a] = (int32_t)v[a]; o.origin[a] = v[3 + a]; }
    o.voxel_size = v[6];
    k.work(); ICP(c, icp_tsdf_create(c, &o));
    icp_depth_camera cam;
    memset(&cam, 0, sizeof(cam));
    const float* q = F(in.cam);
    cam.fx = q[0]; cam.fy = q[1]; cam.cx = q[2]; cam.cy = q[3]; cam.width = (int32_t)q[4]; cam.height = (int32_t)q[5];
    const float eye[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    memcpy(cam.extrinsics, eye, 64);
    int32_t n_updated = 0;
    k.work(); ICP(c, icp_tsdf_integrate(c, F(in.depth), &cam, eye, &n_updated));
    print_words(label + "_updated", &n_updated, 1);
    int32_t nv = 0, nt = 0;
    k.work(); ICP(c, icp_tsdf_mesh(c, 0.f, 0, 0, nullptr, nullptr, nullptr, &nv, &nt));
    std::vector<float> vert((size_t)nv * 3 + 1), nrm((size_t)nv * 3 + 1);
    Words tris((size_t)nt * 3 + 1);
    if (nv || nt) { k.work(); ICP(c, icp_tsdf_mesh(c, 0.f, nv, nt, vert.data(), nrm.data(), tris.data(), &nv, &nt)); }
    print_words(label + "_vertices", vert.data(), (size_t)nv * 3);
    print_words(label + "_normals", nrm.data(), (size_t)nv * 3);
    print_words(label + "_triangles", tris.data(), (size_t)nt * 3);
    k.work(); ICP(c, icp_tsdf_release(c));
}
void run_cluster(icp_ctx* c, Caller& k, const Input& in, const std::string& label) {
    const int32_t V = (int32_t)(in.mv.size() / 3), T = (int32_t)(in.mt.size() / 3);
    icp_mesh_cluster_options o;
    const float* g = F(in.grid);
    o.cell_size = g[0]; o.origin[0] = g[1]; o.origin[1] = g[2]; o.origin[2] = g[3];
    std::vector<float> vert((size_t)V * 3 + 1);
    Words tris((size_t)T * 3 + 1);
    icp_mesh_cluster_info info;
    k.work(); ICP(c, icp_mesh_cluster(c, V, T, F(in.mv), nullptr, nullptr, in.mt.data(), &o, V, T, vert.data(), nullptr, nullptr, tris.data(), &info));
    print_words(label + "_info", &info, sizeof(info) / 4);
    print_words(label + "_vertices", vert.data(), (size_t)info.n_vertices * 3);
    print_words(label + "_triangles", tris.data(), (size_t)info.n_triangles * 3);
}
}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: caller_stream <input file>\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    Input in;
    in.sp = read_array(f); in.sn = read_array(f); in.tp = read_array(f); in.tn = read_array(f); in.depth = read_array(f); in.cam = read_array(f);
    in.vol = read_array(f); in.mv = read_array(f); in.mt = read_array(f); in.grid = read_array(f);
    fclose(f);
    HIP_OK(hipSetDevice(0));
    hipStream_t streams[2];
    HIP_OK(hipStreamCreate(&streams[0]));                                        // a blocking stream
    HIP_OK(hipStreamCreateWithFlags(&streams[1], hipStreamNonBlocking));
    void* block = nullptr;
    HIP_OK(hipMalloc(&block, (size_t)64 << 20));
    const char* names[2] = {"blocking", "nonblocking"};
    for (int s = 0; s < 2; s++) {
        Caller k = {streams[s], block, 1u};
        icp_ctx* c = nullptr;
        if (icp_ctx_create_on_stream(0, (void*)streams[s], &c) != ICP_OK || !c) { fprintf(stderr, "icp_ctx_create_on_stream failed\n"); return 4; }
        load_bunny(c, k, in, ICP_METRIC_POINT_TO_PLANE);
        run_bunny(c, k, std::string(names[s]) + "_run");
        run_volume(c, k, in, std::string(names[s]) + "_volume");
        run_cluster(c, k, in, std::string(names[s]) + "_cluster");
        ICP(c, icp_ctx_destroy(c));
    }
    {   // two contexts on one stream, their runs in turn
        Caller k = {streams[1], block, 7u};
        icp_ctx *a = nullptr, *b = nullptr;
        if (icp_ctx_create_on_stream(0, (void*)streams[1], &a) != ICP_OK || icp_ctx_create_on_stream(0, (void*)streams[1], &b) != ICP_OK) {
            fprintf(stderr, "icp_ctx_create_on_stream failed\n");
            return 4;
        }
        load_bunny(a, k, in, ICP_METRIC_POINT_TO_PLANE);
        load_bunny(b, k, in, ICP_METRIC_POINT_TO_POINT);
        for (int round = 0; round < 2; round++) {
            run_bunny(a, k, "shared_a" + std::to_string(round));
            run_bunny(b, k, "shared_b" + std::to_string(round));
        }
        ICP(a, icp_ctx_destroy(a));
        ICP(b, icp_ctx_destroy(b));
    }
    // the caller's streams outlive the contexts: idle (every library call waits for its stream before it returns, icp_ctx_destroy too), usable, and theirs to destroy
    for (int s = 0; s < 2; s++) {
        HIP_OK(hipStreamQuery(streams[s]));
        HIP_OK(hipMemsetAsync(block, 0, (size_t)64 << 20, streams[s]));
        HIP_OK(hipStreamSynchronize(streams[s]));
    }
    for (int s = 0; s < 2; s++) HIP_OK(hipStreamDestroy(streams[s]));
    HIP_OK(hipFree(block));
    printf("streams ok\n");
    return 0;
}
