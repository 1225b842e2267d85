// [EXT] GenericDescriptorOutlierFilter through the C++ drop-in on the device: an ICP object loaded from YAML on clouds carrying
// a `probabilityStatic` descriptor (Matcher::init hands the row to the map: pgicp_map_set_values), PoseGraphSlam drives whose
// filter passes every point equal to the same drive without the filter bit for bit (both through the host-built local maps the
// filter routes to), and a PoseGraphSlamMT drive with labelled dynamic points that runs to the end.
#include "common.hpp"
#include <pgslam_amd/slam.hpp>
#include <algorithm>
#include <chrono>
#include <cstring>
#include <thread>

#define PGSLAM_GD_CHAIN_TAIL(FILTER) \
    "matcher:\n  KDTreeMatcher:\n    knn: 1\n    epsilon: 0\n    maxDist: 2.0\n" \
    "outlierFilters:\n  - TrimmedDistOutlierFilter:\n      ratio: 0.85\n" FILTER \
    "errorMinimizer:\n  PointToPlaneWithCovErrorMinimizer:\n    sensorStdDev: 0.01\n" \
    "transformationCheckers:\n  - CounterTransformationChecker:\n      maxIterationCount: 30\n" \
    "  - DifferentialTransformationChecker:\n      minDiffRotErr: 0.001\n      minDiffTransErr: 0.01\n      smoothLength: 3\n" \
    "inspector:\n  NullInspector\nlogger:\n  NullLogger\n"
#define PGSLAM_GD_HARD "  - GenericDescriptorOutlierFilter:\n      descName: probabilityStatic\n      useLargerThan: 1\n      threshold: 0.5\n"
#define PGSLAM_GD_SOFT "  - GenericDescriptorOutlierFilter:\n      descName: probabilityStatic\n      useSoftThreshold: 1\n"
static const char *kPlain = "readingDataPointsFilters:\n  - IdentityDataPointsFilter\n" PGSLAM_GD_CHAIN_TAIL("");
static const char *kHard = "readingDataPointsFilters:\n  - IdentityDataPointsFilter\n" PGSLAM_GD_CHAIN_TAIL(PGSLAM_GD_HARD);
static const char *kSoft = "readingDataPointsFilters:\n  - IdentityDataPointsFilter\n" PGSLAM_GD_CHAIN_TAIL(PGSLAM_GD_SOFT);

// the cloud with a one-row `probabilityStatic` descriptor: `value` everywhere, 0 on every point where `dynamic` says so
template <typename T, typename DP>
DP labelled(const DP &c, T value, const std::vector<char> &dynamic = {})
{
    DP out(c);
    typename PointMatcher<T>::Matrix d(1, (int)c.getNbPoints());
    for (int i = 0; i < (int)c.getNbPoints(); i++) d(0, i) = (!dynamic.empty() && dynamic[(size_t)i]) ? T(0) : value;
    out.addDescriptor("probabilityStatic", d);
    return out;
}

template <typename T>
void run_icp(const char *name)
{
    IMPORT_PGSLAM_TYPES(T)
    TransformationPtr rigid = PM::get().REG(Transformation).create("RigidTransformation");
    const Matrix truth = pose<T>(0.05, -0.03, 0.0, 0.02);
    const DP ref0 = make_corner<T>(3000, 11, 0.003);
    const DP rd = rigid->compute(make_corner<T>(3000, 12, 0.003), truth.inverse());
    auto icp_of = [](const char *yaml) { auto p = std::make_shared<typename PM::ICP>(); std::istringstream in(yaml); p->loadFromYaml(in); return p; };
    auto plain = icp_of(kPlain), hard = icp_of(kHard), soft = icp_of(kSoft);
    const Matrix Tp = (*plain)(rd, ref0);
    // every point passes: the result is the unfiltered one, bit for bit
    const Matrix Th = (*hard)(rd, labelled<T>(ref0, T(1)));
    const Matrix Ts = (*soft)(rd, labelled<T>(ref0, T(0.625)));
    CHECK(pose_diff(Th, Tp) == 0.0 && pose_diff(Ts, Tp) == 0.0);
    CHECK(hard->errorMinimizer->getOverlap() == plain->errorMinimizer->getOverlap());
    // a block of the reference moved 0.2 m (a parked car that left) and labelled 0: the filter keeps the ICP on the truth
    std::vector<char> dyn(ref0.getNbPoints(), 0);
    for (int i = 0; i < (int)ref0.getNbPoints(); i++) dyn[(size_t)i] = ref0.features(0, i) > T(0.8) && ref0.features(1, i) > T(0.8);
    DP moved = labelled<T>(ref0, T(1), dyn);
    for (int i = 0; i < (int)moved.getNbPoints(); i++) if (dyn[(size_t)i]) moved.features(0, i) += T(0.2);
    const Matrix Tm = (*hard)(rd, moved);
    const Matrix d = truth.inverse() * Tm;
    const double dt = std::sqrt((double)(d(0, 3) * d(0, 3) + d(1, 3) * d(1, 3) + d(2, 3) * d(2, 3)));
    CHECK(dt < 0.01);
    // the reference must carry the row
    bool threw = false;
    try { (*hard)(rd, ref0); } catch (const std::runtime_error &) { threw = true; }
    CHECK(threw);
    std::printf("%s: ok  (pass-all hard and soft equal the unfiltered ICP bit for bit; moved block: |dt| %.2e m)\n", name, dt);
}

template <typename T>
std::vector<typename PointMatcher<T>::TransformationParameters> drive(const char *yaml, bool label, std::vector<typename PointMatcher<T>::TransformationParameters> &loops,
                                                                     std::vector<typename PointMatcher<T>::TransformationParameters> &kf)
{
    IMPORT_PGSLAM_TYPES(T)
    TransformationPtr rigid = PM::get().REG(Transformation).create("RigidTransformation");
    const int S = 15;
    std::vector<Matrix> truth, odom, poses;
    for (int s = 0; s < S; s++) {
        const double a = 2 * M_PI * s / (S - 1);
        truth.push_back(pose<T>(1.5 + 0.5 * std::cos(a), 1.5 + 0.5 * std::sin(a), 0.0, a * 0.2));
    }
    odom.push_back(truth[0]);
    for (int s = 1; s < S; s++) odom.push_back(odom[s - 1] * (truth[s - 1].inverse() * truth[s]) * pose<T>(0.012, -0.009, 0.0, 0.005));
    pgslam::PoseGraphSlam<T> slam;
    slam.SetIcpConfigFromStrings("- IdentityDataPointsFilter\n", yaml, yaml);
    // (every scan a keyframe; the loop closer finds the first keyframes again and closes loops)
    slam.localizer().SetOverlapThreshold(T(0.9999));
    slam.localizer().SetDeviceLocalMap(false);
    slam.loop_closer().SetDeviceCandidates(false);
    slam.loop_closer().SetTopologicalDistanceThreshold(T(1.0));
    slam.loop_closer().SetGeometricalDistanceThreshold(T(0.6));
    slam.loop_closer().SetOverlapThreshold(T(0.3));
    for (int s = 0; s < S; s++) {
        const DP c = rigid->compute(make_corner<T>(2000, 70 + s, 0.004), truth[s].inverse());
        auto cloud = std::make_shared<DP>(label ? labelled<T>(c, T(1)) : c);
        slam.AddData((unsigned long long)s, "world", odom[s], Matrix::Identity(4, 4), cloud);
        poses.push_back(slam.localizer().T_world_robot());
    }
    auto &g = slam.map_manager().GetGraph();
    loops.clear();
    for (size_t e = 0; e < g.NumEdges(); e++) if (g.Edge(e).c.type == Constraint::kLoopConstraint) loops.push_back(g.Edge(e).c.T_from_to);
    kf.clear();
    for (size_t v = 0; v < g.NumVertices(); v++) kf.push_back(g[v].optimized_T_world_kf);
    return poses;
}

template <typename T>
void run_drive(const char *name)
{
    std::vector<typename PointMatcher<T>::TransformationParameters> kf_p, kf_h, kf_s, loops_p, loops_h, loops_s;
    const auto p = drive<T>(kPlain, false, loops_p, kf_p);
    const auto h = drive<T>(kHard, true, loops_h, kf_h);
    const auto s = drive<T>(kSoft, true, loops_s, kf_s);
    CHECK(p.size() == h.size() && p.size() == s.size());
    for (size_t k = 0; k < p.size(); k++) CHECK(pose_diff(p[k], h[k]) == 0.0 && pose_diff(p[k], s[k]) == 0.0);
    CHECK(!loops_p.empty() && loops_h.size() == loops_p.size() && loops_s.size() == loops_p.size());
    for (size_t k = 0; k < loops_p.size(); k++) CHECK(pose_diff(loops_p[k], loops_h[k]) == 0.0 && pose_diff(loops_p[k], loops_s[k]) == 0.0);
    CHECK(kf_p.size() == kf_h.size() && kf_p.size() == kf_s.size());
    for (size_t k = 0; k < kf_p.size(); k++) CHECK(pose_diff(kf_p[k], kf_h[k]) == 0.0 && pose_diff(kf_p[k], kf_s[k]) == 0.0);
    std::printf("%s: ok  (%zu scans, %zu keyframes, %zu loop edges: equal to the unfiltered drive bit for bit)\n", name, p.size(), kf_p.size(), loops_p.size());
}

// a PoseGraphSlamMT drive (loop closer and optimiser held until every scan is in, then released): the loop closer's edges in
// (from, to) order and the keyframe poses after the optimiser ran.  `dynamic`: every seventh point of a scan belongs to a box that
// is somewhere else in every scan, labelled 0 (the others 0.9); else every point is labelled 1 (`label`) or carries no label.
template <typename T>
std::vector<pgicp_edge> mt_drive(const char *yaml, bool label, bool dynamic, std::vector<typename PointMatcher<T>::TransformationParameters> &kf)
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
    slam.SetIcpConfigFromStrings("- IdentityDataPointsFilter\n", yaml, yaml);
    slam.localizer().SetOverlapThreshold(T(0.9999));
    slam.localizer().SetDeviceLocalMap(false);
    slam.loop_closer().SetDeviceCandidates(false);
    slam.loop_closer().SetTopologicalDistanceThreshold(T(1.0));
    slam.loop_closer().SetGeometricalDistanceThreshold(T(0.6));
    slam.loop_closer().SetOverlapThreshold(T(0.3));
    slam.loop_closer().Pause();
    slam.optimizer().Pause();
    slam.Run();
    for (int s = 0; s < S; s++) {
        DP c = make_corner<T>(2000, 70 + s, 0.004);
        std::vector<char> dyn(c.getNbPoints(), 0);
        if (dynamic)
            for (int i = 0; i < (int)c.getNbPoints(); i += 7) {
                dyn[(size_t)i] = 1;
                c.features(0, i) += T(0.3 + 0.05 * s); c.features(1, i) += T(0.1 * (s % 3));
            }
        const DP moved = rigid->compute(c, truth[s].inverse());
        auto cloud = std::make_shared<DP>(dynamic ? labelled<T>(moved, T(0.9), dyn) : label ? labelled<T>(moved, T(1)) : moved);
        slam.AddData((unsigned long long)s, "world", odom[s], Matrix::Identity(4, 4), cloud);
    }
    slam.WaitIdle();
    slam.loop_closer().Resume();
    while (slam.loop_closer().queued() > 0 || !slam.loop_closer().Idle()) std::this_thread::sleep_for(std::chrono::milliseconds(1));
    slam.RethrowWorkerError();
    std::vector<pgicp_edge> edges = slam.loop_closer().edges();
    std::sort(edges.begin(), edges.end(), [](const pgicp_edge &a, const pgicp_edge &b) { return a.from_id != b.from_id ? a.from_id < b.from_id : a.to_id < b.to_id; });
    slam.optimizer().Resume();
    slam.WaitIdle();
    slam.RethrowWorkerError();
    auto lock = slam.map_manager().GetGraphLock();
    auto &g = slam.map_manager().GetGraph();
    kf.clear();
    for (size_t v = 0; v < g.NumVertices(); v++) kf.push_back(g[v].optimized_T_world_kf);
    return edges;
}

template <typename T>
void run_mt_drive(const char *name)
{
    std::vector<typename PointMatcher<T>::TransformationParameters> kf_p, kf_h, kf_s;
    const auto p = mt_drive<T>(kPlain, false, false, kf_p);
    const auto h = mt_drive<T>(kHard, true, false, kf_h);
    const auto s = mt_drive<T>(kSoft, true, false, kf_s);
    int accepted = 0;
    CHECK(!p.empty() && h.size() == p.size() && s.size() == p.size());
    for (size_t k = 0; k < p.size(); k++) {
        for (const pgicp_edge *e : {&h[k], &s[k]}) {
            CHECK(e->from_id == p[k].from_id && e->to_id == p[k].to_id && e->accepted == p[k].accepted && e->iterations == p[k].iterations);
            CHECK(std::memcmp(e->T_from_to, p[k].T_from_to, sizeof e->T_from_to) == 0);
            CHECK(std::memcmp(&e->overlap, &p[k].overlap, sizeof e->overlap) == 0 && std::memcmp(&e->residual, &p[k].residual, sizeof e->residual) == 0);
        }
        accepted += p[k].accepted;
    }
    CHECK(accepted >= 1);
    CHECK(kf_p.size() == kf_h.size() && kf_p.size() == kf_s.size());
    for (size_t k = 0; k < kf_p.size(); k++) CHECK(pose_diff(kf_p[k], kf_h[k]) == 0.0 && pose_diff(kf_p[k], kf_s[k]) == 0.0);
    std::printf("%s: ok  (%zu loop candidates, %d accepted, %zu keyframes: edges and poses equal to the unfiltered drive bit for bit)\n",
                name, p.size(), accepted, kf_p.size());
}

template <typename T>
void run_mt_dynamic(const char *name)
{
    std::vector<typename PointMatcher<T>::TransformationParameters> kf;
    const auto edges = mt_drive<T>(kHard, true, true, kf);
    CHECK(!edges.empty() && !kf.empty());
    int accepted = 0;
    for (const pgicp_edge &e : edges) { CHECK(e.overlap >= 0.0 && e.overlap <= 1.0); accepted += e.accepted; }
    std::printf("%s: ok  (%zu candidates, %d accepted, %zu keyframes)\n", name, edges.size(), accepted, kf.size());
}

int main()
{
    run_icp<float>("ICP<float> from a GenericDescriptor YAML");
    run_icp<double>("ICP<double> from a GenericDescriptor YAML");
    run_drive<float>("PoseGraphSlam<float>, every point passes");
    run_drive<double>("PoseGraphSlam<double>, every point passes");
    run_mt_drive<float>("PoseGraphSlamMT<float>, every point passes");
    run_mt_drive<double>("PoseGraphSlamMT<double>, every point passes");
    run_mt_dynamic<float>("PoseGraphSlamMT<float> with labelled dynamic points");
    run_mt_dynamic<double>("PoseGraphSlamMT<double> with labelled dynamic points");
    std::puts("generic descriptor gpu tests ok");
    return 0;
}
