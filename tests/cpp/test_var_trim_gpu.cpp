// [EXT] VarTrimmedDistOutlierFilter through the C++ drop-in on the device: an ICP object loaded from a VarTrimmed YAML
// (pushParams -> pgicp_set_var_trim inside operator()), its stage-level compute(), and a PoseGraphSlamMT drive whose localizer
// and loop closer run that chain -- the overlap probes (seeded) and the batched loop closer (LoopClosureBatch:
// pgicp_align_residual_batch) included.
#include "common.hpp"
#include <pgslam_amd/slam.hpp>
#include <chrono>
#include <thread>

#define PGSLAM_VT_CHAIN_TAIL \
    "matcher:\n  KDTreeMatcher:\n    knn: 1\n    epsilon: 0\n    maxDist: 2.0\n" \
    "outlierFilters:\n  - VarTrimmedDistOutlierFilter:\n      minRatio: 0.3\n      maxRatio: 0.95\n      lambda: 2.0\n" \
    "errorMinimizer:\n  PointToPlaneWithCovErrorMinimizer:\n    sensorStdDev: 0.01\n" \
    "transformationCheckers:\n  - CounterTransformationChecker:\n      maxIterationCount: 30\n" \
    "  - DifferentialTransformationChecker:\n      minDiffRotErr: 0.001\n      minDiffTransErr: 0.01\n      smoothLength: 3\n" \
    "inspector:\n  NullInspector\nlogger:\n  NullLogger\n"
static const char *kVtYaml = "readingDataPointsFilters:\n  - IdentityDataPointsFilter\n" PGSLAM_VT_CHAIN_TAIL;

template <typename T>
void run_icp(const char *name)
{
    IMPORT_PGSLAM_TYPES(T)
    TransformationPtr rigid = PM::get().REG(Transformation).create("RigidTransformation");
    const DP ref = make_corner<T>(3000, 11, 0.003);
    const Matrix truth = pose<T>(0.05, -0.03, 0.0, 0.02);
    const DP rd = rigid->compute(make_corner<T>(3000, 12, 0.003), truth.inverse());
    typename PM::ICP icp;
    std::istringstream in(kVtYaml);
    icp.loadFromYaml(in);
    auto vt = std::dynamic_pointer_cast<typename PM::VarTrimmedDistOutlierFilter>(icp.outlierFilters.at(0));
    CHECK(vt);
    const Matrix Tres = icp(rd, ref);
    const double r = vt->lastRatio();
    CHECK(r >= 0.3 && r <= 0.95);
    const Matrix d = truth.inverse() * Tres;
    const double dt = std::sqrt((double)(d(0, 3) * d(0, 3) + d(1, 3) * d(1, 3) + d(2, 3) * d(2, 3)));
    CHECK(dt < 0.01);
    // the stage-level filter under the same setting (Localizer.hpp:330)
    typename PM::Matches m(1, 6);
    const T dd[6] = {T(0.01), T(0.02), T(0.03), T(0.04), T(2.0), T(3.0)};
    for (int k = 0; k < 6; k++) { m.dists(0, k) = dd[k]; m.ids(0, k) = k; }
    const typename PM::OutlierWeights w = vt->compute(rd, ref, m);
    CHECK(w(0, 0) == T(1) && w(0, 5) == T(0));
    std::printf("%s: ok  (ratio %.4f, |dt| %.2e m)\n", name, r, dt);
}

template <typename T>
void run_mt(const char *name)
{
    IMPORT_PGSLAM_TYPES(T)
    TransformationPtr rigid = PM::get().REG(Transformation).create("RigidTransformation");
    const int S = 15;
    std::vector<Matrix> truth, odom;
    for (int s = 0; s < S; s++) {
        const double a = 2 * M_PI * s / (S - 1);
        truth.push_back(pose<T>(1.5 + 0.5 * std::cos(a), 1.5 + 0.5 * std::sin(a), 0.0, a * 0.2));
    }
    odom.push_back(truth[0]);
    for (int s = 1; s < S; s++) odom.push_back(odom[s - 1] * (truth[s - 1].inverse() * truth[s]) * pose<T>(0.012, -0.009, 0.0, 0.005));
    pgslam::PoseGraphSlamMT<T> slam;
    slam.SetIcpConfigFromStrings("- IdentityDataPointsFilter\n", kVtYaml, kVtYaml);
    slam.localizer().SetOverlapThreshold(T(0.9999));
    slam.loop_closer().SetTopologicalDistanceThreshold(T(1.0));
    slam.loop_closer().SetGeometricalDistanceThreshold(T(0.6));
    slam.loop_closer().SetOverlapThreshold(T(0.3));
    slam.loop_closer().Pause();
    slam.optimizer().Pause();
    slam.Run();
    for (int s = 0; s < S; s++) {
        auto cloud = std::make_shared<DP>(rigid->compute(make_corner<T>(2000, 70 + s, 0.004), truth[s].inverse()));
        slam.AddData((unsigned long long)s, "world", odom[s], Matrix::Identity(4, 4), cloud);
    }
    slam.WaitIdle();
    slam.loop_closer().Resume();
    while (slam.loop_closer().queued() > 0 || !slam.loop_closer().Idle()) std::this_thread::sleep_for(std::chrono::milliseconds(1));
    slam.RethrowWorkerError();
    const auto edges = slam.loop_closer().edges();
    CHECK(!edges.empty());
    CHECK(slam.loop_closer().batches() >= 1);
    CHECK(slam.loop_closer().device_batches() >= 1);          // the candidates went through the device batch
    int accepted = 0;
    for (const pgicp_edge &e : edges) { CHECK(e.overlap >= 0.0 && e.overlap <= 1.0); accepted += e.accepted; }
    CHECK(accepted >= 1);
    slam.optimizer().Resume();
    slam.WaitIdle();
    std::printf("%s: ok  (%zu candidates, %zu device batches, %d accepted)\n", name, edges.size(), slam.loop_closer().device_batches(), accepted);
}

int main()
{
    run_icp<float>("ICP<float> from a VarTrimmed YAML");
    run_icp<double>("ICP<double> from a VarTrimmed YAML");
    run_mt<float>("PoseGraphSlamMT<float> with a VarTrimmed chain");
    std::puts("var trim gpu tests ok");
    return 0;
}
