// C++14 driver for HipCeresICPOptimizer (include/icp_hip_adaptor.hpp), written like the reference's alignBunnyWithICP with
// USE_LINEAR_ICP 0 (main.cpp:26,51-56 `new CeresICPOptimizer()`): the canonical bunny parameters, estimatePose, the pose and the
// Solver summaries.  Reads the clouds from a raw dump written by tests/test_gpu_lm.py.
//   usage: bunny_ceres_adaptor <dump.bin> <metric>
#include "icp_hip_adaptor.hpp"
#include <cstdio>
#include <cstdlib>

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
    if (argc < 3) { std::fprintf(stderr, "usage: %s dump.bin metric\n", argv[0]); return 2; }
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    PointCloud source, target;
    if (!read_cloud(f, source) || !read_cloud(f, target)) return 2;
    std::fclose(f);

    HipCeresICPOptimizer* ceres = new HipCeresICPOptimizer();      // main.cpp:51-56 `new CeresICPOptimizer()`
    ICPOptimizer* optimizer = ceres;
    optimizer->setMetric((unsigned)std::atoi(argv[2]));             // main.cpp:59-70
    optimizer->setNbOfIterations(20);
    optimizer->setMatchingMethod(0);                                // main.cpp:74-75
    optimizer->setMatchingMaxDistance(0.0003f);
    optimizer->setSelectionMethod(SELECT_ALL);                      // main.cpp:78-81
    optimizer->setWeightingMethod(CONSTANT_WEIGHTING);              // main.cpp:84-95
    optimizer->enableMultiResolution(false);
    Matrix4f estimatedPose = Matrix4f::Identity();
    optimizer->estimatePose(source, target, estimatedPose);         // main.cpp:133

    int converged = 0;
    for (const icp_lm_summary& s : ceres->summaries()) converged += s.termination == ICP_LM_CONVERGENCE || s.termination == ICP_LM_NO_CONVERGENCE;
    std::printf("status %d iterations %zu summaries %zu converged %d\n", ceres->lastStatus(), ceres->iterations().size(), ceres->summaries().size(), converged);
    std::printf("pose");
    for (int r = 0; r < 4; r++) for (int c = 0; c < 4; c++) std::printf(" %.9g", estimatedPose(r, c));
    std::printf("\n");
    delete optimizer;
    return 0;
}
