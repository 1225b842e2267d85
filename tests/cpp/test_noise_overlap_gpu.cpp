// GPU checks of getOverlap()'s sensor-noise branch through the C++ drop-in layer (include/pgicp_noise.h): the shim arms its
// align call and reads the device's result -- with a Robust chain too; the batch dispatcher's opt-in gives a noisy pair the
// overlap and the pose PairLoopCloser::ProcessCandidate gives it, and still refuses such a pair without the opt-in; the MT loop
// closer keeps noisy candidates in the device batch when told to.
#include <chrono>
#include <thread>
#include "common.hpp"
#include "pgslam_amd/slam.hpp"

static const char *kRobustYaml =
    "matcher:\n  KDTreeMatcher:\n    maxDist: 2.0\noutlierFilters:\n  - RobustOutlierFilter:\n      robustFct: cauchy\n      tuning: 1.5\n"
    "errorMinimizer:\n  PointToPlaneWithCovErrorMinimizer\ntransformationCheckers:\n  - CounterTransformationChecker:\n      maxIterationCount: 30\n"
    "  - DifferentialTransformationChecker:\n      minDiffRotErr: 0.001\n      minDiffTransErr: 0.01\n      smoothLength: 3\n";

template <typename T> struct Raw;
template <> struct Raw<float> {
    static int arm(pgicp_ctx *c, const float *const *r, const int *s, const int *n) { return pgicp_arm_reading_noise_f32(c, 1, r, s, n, PGICP_HOST); }
    static int pair(pgicp_ctx *c, const float *rd, int rs, int n, const float *x, int xs, const float *nr, int ns, int m, const double *Ti, double *To, pgicp_stats *st)
    { return pgicp_icp_pair_f32(c, rd, rs, n, x, xs, nr, ns, m, PGICP_HOST, Ti, To, st); }
};
template <> struct Raw<double> {
    static int arm(pgicp_ctx *c, const double *const *r, const int *s, const int *n) { return pgicp_arm_reading_noise_f64(c, 1, r, s, n, PGICP_HOST); }
    static int pair(pgicp_ctx *c, const double *rd, int rs, int n, const double *x, int xs, const double *nr, int ns, int m, const double *Ti, double *To, pgicp_stats *st)
    { return pgicp_icp_pair_f64(c, rd, rs, n, x, xs, nr, ns, m, PGICP_HOST, Ti, To, st); }
};

// the same pair through the C ABI alone (what the Python binding calls), with the chain the shim pushed to its context
template <typename T>
T raw_overlap(pgicp_ctx *shim_ctx, const typename PointMatcher<T>::DataPoints &noisy, const typename PointMatcher<T>::DataPoints &map,
              const pgslam_amd::Mat<T> &guess, int *n_kept)
{
    pgicp_params prm;
    CHECK(pgicp_get_params(shim_ctx, &prm) == PGICP_OK);
    pgicp_ctx *c = nullptr;
    CHECK(pgicp_ctx_create(0, &c) == PGICP_OK);
    CHECK(pgicp_set_params(c, &prm) == PGICP_OK);
    const T *row = noisy.descriptors.data() + noisy.getDescriptorStartingRow("simpleSensorNoise");
    const int stride = (int)noisy.descriptors.rows(), n = (int)noisy.getNbPoints();
    CHECK(Raw<T>::arm(c, &row, &stride, &n) == PGICP_OK);
    double Ti[16], To[16];
    pgslam_amd::to_row_major16(guess, Ti);
    pgicp_stats st;
    CHECK(Raw<T>::pair(c, noisy.xyzPtr(), noisy.xyzStride(), n, map.xyzPtr(), map.xyzStride(), map.normalsPtr(), map.normalsStride(),
                       (int)map.getNbPoints(), Ti, To, &st) == PGICP_OK);
    double ov = -1.0;
    int nb = 0;
    CHECK(pgicp_last_noise_overlap(c, 0, &ov, &nb) == PGICP_OK);
    CHECK(nb == st.n_kept && nb > 0);
    CHECK(pgicp_last_noise_overlap(c, 1, &ov, &nb) == PGICP_ERR_ARG);
    *n_kept = st.n_kept;
    pgicp_ctx_destroy(c);
    return (T)ov;
}

template <typename T>
void run(const char *name)
{
    IMPORT_PGSLAM_TYPES(T)
    const DP map = make_corner<T>(6000, 11, 0.004);
    const DP scan_world = make_corner<T>(2500, 12, 0.004);
    const Matrix P = pose<T>(0.40, -0.25, 0.10, 0.06, 0.01, -0.015);
    TransformationPtr rigid = PM::get().REG(Transformation).create("RigidTransformation");
    const DP reading = rigid->compute(scan_world, P.inverse());
    const Matrix guess = P * pose<T>(0.08, -0.05, 0.03, 0.02, 0.0, 0.0);
    DP noisy(reading);
    typename PM::SimpleSensorNoiseDataPointsFilter(0, T(1)).inPlaceFilter(noisy);
    CHECK(noisy.descriptorExists("simpleSensorNoise") && noisy.descriptorExists("normals"));

    // --- the shim's getOverlap() with the usual chain and with a Robust one: the C ABI's value for the same pair
    for (const char *yaml : {kIcpYaml, kRobustYaml}) {
        ICP icp;
        { std::istringstream iss(yaml); icp.loadFromYaml(iss); }
        const Matrix T0 = icp(reading, map, guess);
        const T ratio = icp.errorMinimizer->getOverlap();                    // no descriptor: weightedPointUsedRatio
        const Matrix T1 = icp(noisy, map, guess);
        const T ov = icp.errorMinimizer->getOverlap();
        CHECK(pose_diff(T0, T1) == 0.0);                                     // the descriptor changes no pose
        CHECK(icp.errorMinimizer->getWeightedPointUsedRatio() == ratio);
        CHECK(ov != ratio && ov > T(0.3) && ov <= T(1));
        int n_kept = 0;
        CHECK(raw_overlap<T>(icp.ctx, noisy, map, guess, &n_kept) == ov);
        // again, and after a reading without the descriptor: the same value, the ratio in between
        CHECK(pose_diff(icp(reading, map, guess), T0) == 0.0 && icp.errorMinimizer->getOverlap() == ratio);
        CHECK(pose_diff(icp(noisy, map, guess), T0) == 0.0 && icp.errorMinimizer->getOverlap() == ov);
    }

    // --- the batch dispatcher: refused by default, with the opt-in the pair path's overlap and pose
    pgslam::PairLoopCloser<T> pl;
    pl.SetIcpConfigFromString(kIcpYaml);
    const auto rn = pl.ProcessCandidate(noisy, map, guess);
    const auto rc = pl.ProcessCandidate(reading, map, guess);
    CHECK(rn.overlap != rc.overlap);
    auto np = std::make_shared<DP>(noisy), rp = std::make_shared<DP>(reading), mp = std::make_shared<DP>(map);
    pgslam::LoopClosureBatch<T> batch;
    batch.SetIcpConfigFromString(kIcpYaml);
    CHECK(!batch.SensorNoiseOnDevice());
    batch.Add({1, 2, np, mp, guess});
    batch.Add({3, 4, rp, mp, guess});
    batch.Add({5, 6, np, mp, guess});
    bool refused = false;
    try { batch.Run(batch.Shard(1, 0)); } catch (const std::runtime_error &) { refused = true; }
    CHECK(refused);
    batch.SetSensorNoiseOnDevice(true);
    for (int rep = 0; rep < 2; rep++) {
        const auto e = batch.Run(batch.Shard(1, 0), T(0.5));
        CHECK(e.size() == 3);
        for (int k = 0; k < 3; k++) {
            CHECK(e[k].status == 0);
            CHECK(pose_diff(pgslam_amd::from_row_major16<T>(e[k].T_from_to), rn.T_refkf_kf) == 0.0);
        }
        CHECK(e[0].overlap == (double)rn.overlap && e[2].overlap == (double)rn.overlap);      // as a double, the pair path's
        CHECK((T)e[1].overlap == rc.overlap);                                                 // a pair without the row: the ratio (the edge's is the double)
        CHECK(e[0].accepted == (rn.overlap >= T(0.5) && !rn.max_iterations_reached ? 1 : 0));
    }
    batch.SetSensorNoiseOnDevice(false);
    refused = false;
    try { batch.Run(batch.Shard(1, 0)); } catch (const std::runtime_error &) { refused = true; }
    CHECK(refused);
    std::printf("%s ok (overlap %.6f, ratio %.6f)\n", name, (double)rn.overlap, (double)rc.overlap);
}

// the noisy drive of test_slam_gpu.cpp's run_mt_sensor_noise, with the setter: the candidates stay in the device batch
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
    std::vector<pgicp_edge> edges[2];
    for (int on = 0; on < 2; on++) {
        pgslam::PoseGraphSlamMT<T> slam;
        slam.SetIcpConfigFromStrings("- SimpleSensorNoiseDataPointsFilter:\n    sensorType: 0\n    gain: 1\n", kIcpYaml, kIcpYaml);
        slam.localizer().SetOverlapThreshold(T(0.9999));
        slam.loop_closer().SetTopologicalDistanceThreshold(T(1.0));
        slam.loop_closer().SetGeometricalDistanceThreshold(T(0.6));
        slam.loop_closer().SetOverlapThreshold(T(0.3));
        slam.loop_closer().SetSensorNoiseOnDevice(on != 0);
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
        edges[on] = slam.loop_closer().edges();
        CHECK(slam.loop_closer().batches() >= 1);
        CHECK(on ? slam.loop_closer().device_batches() >= 1 : slam.loop_closer().device_batches() == 0);
        slam.optimizer().Resume();
        slam.WaitIdle();
    }
    // the same drive, the same candidates: pair by pair the batch gives the pairwise path's overlap and decision
    CHECK(!edges[0].empty() && edges[0].size() == edges[1].size());
    for (auto &a : edges[0]) {
        bool found = false;
        for (auto &b : edges[1])
            if (a.from_id == b.from_id && a.to_id == b.to_id) {
                found = true;
                CHECK(a.overlap == b.overlap && a.accepted == b.accepted);
            }
        CHECK(found);
    }
    std::printf("%s ok (%zu candidates)\n", name, edges[0].size());
}

int main()
{
    run<float>("sensor-noise getOverlap(), float");
    run<double>("sensor-noise getOverlap(), double");
    run_mt<float>("PoseGraphSlamMT<float>, noisy clouds in the device batch");
    std::puts("noise overlap gpu tests ok");
    return 0;
}
