// C++14 driver for setConvergenceCriteria on the adaptor classes (include/icp_hip_adaptor.hpp): the bunny pair, point-to-plane, 20
// iterations, three estimatePose calls -- criteria off, on (bounds from the command line), cleared again.  Reads the clouds from the raw
// dump tests/test_gpu_converge.py writes (the layout of bunny_adaptor.cpp).
//   usage: converge_adaptor <dump.bin> <rotation_eps> <translation_eps>
#include "icp_hip_adaptor.hpp"
#include <cstdio>
#include <cstdlib>
#include <cstring>

static bool read_cloud(FILE* f, PointCloud& pc) {
    int32_t n = 0;
    if (fread(&n, 4, 1, f) != 1) return false;
    pc.getPoints().resize(n); pc.getNormals().resize(n); pc.getColors().resize(n);
    if (fread(pc.getPoints().data(), 12, n, f) != (size_t)n) return false;
    if (fread(pc.getNormals().data(), 12, n, f) != (size_t)n) return false;
    if (fread(pc.getColors().data(), 4, n, f) != (size_t)n) return false;
    return true;
}

int main(int argc, char** argv) {
    if (argc < 4) { std::fprintf(stderr, "usage: %s dump.bin rotation_eps translation_eps\n", argv[0]); return 2; }
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    PointCloud source, target;
    if (!read_cloud(f, source) || !read_cloud(f, target)) return 2;
    std::fclose(f);
    HipLinearICPOptimizer opt;
    opt.setMetric(1); opt.setNbOfIterations(20); opt.setMatchingMethod(0); opt.setMatchingMaxDistance(0.0003f);
    opt.setSelectionMethod(SELECT_ALL); opt.setWeightingMethod(CONSTANT_WEIGHTING);
    size_t n[3]; int same_prefix = 1, ends_on_last_record = 0;
    std::vector<icp_iter_stats> full;
    const int bad = opt.setConvergenceCriteria(0.f, 1.f), bad2 = opt.setConvergenceCriteria(1.f, 1.f, 1, 9);      // refused, nothing changes
    for (int k = 0; k < 3; k++) {
        int rc = ICP_OK;
        if (k == 1) rc = opt.setConvergenceCriteria((float)std::atof(argv[2]), (float)std::atof(argv[3]));
        if (k == 2) rc = opt.clearConvergenceCriteria();
        if (rc != ICP_OK) return 3;
        Matrix4f pose = Matrix4f::Identity();
        opt.estimatePose(source, target, pose);
        if (opt.lastStatus() != ICP_OK) return 4;
        n[k] = opt.iterations().size();
        if (k == 0) full = opt.iterations();
        else for (size_t i = 0; i < n[k] && i < full.size(); i++) same_prefix &= std::memcmp(&full[i], &opt.iterations()[i], sizeof(icp_iter_stats)) == 0;
        if (k == 1) ends_on_last_record = n[k] > 0 && std::memcmp(pose.data(), opt.iterations()[n[k] - 1].pose, 64) == 0;
    }
    HipCeresICPOptimizer ceres;                                     // the non-linear adaptor inherits the setter
    const int ceres_rc = ceres.setConvergenceCriteria(1e-5f, 1e-6f, 2, 2);
    std::printf("off %zu on %zu cleared %zu same_prefix %d ends_on_last_record %d refused %d %d ceres %d\n", n[0], n[1], n[2], same_prefix, ends_on_last_record, bad, bad2, ceres_rc);
    return 0;
}
