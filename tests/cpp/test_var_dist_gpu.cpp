// [EXT] KDTreeVarDistMatcher through the C++ drop-in on the device: a missing or three-row field and a device reading throw, naming
// the field; findClosests equals the C call (pgicp_arm_reading_radii + pgicp_match); one ICP::operator() with reading filters
// (RandomSampling + MaxDist) ahead of the matcher equals pgicp_align on the filtered cloud with the filtered row, bit for bit.
#include "common.hpp"
#include <cstring>
#include <sstream>

#define VD_CHAIN_TAIL \
    "outlierFilters:\n  - TrimmedDistOutlierFilter:\n      ratio: 0.85\n" \
    "errorMinimizer:\n  PointToPlaneWithCovErrorMinimizer:\n    sensorStdDev: 0.01\n" \
    "transformationCheckers:\n  - CounterTransformationChecker:\n      maxIterationCount: 30\n" \
    "  - DifferentialTransformationChecker:\n      minDiffRotErr: 0.001\n      minDiffTransErr: 0.01\n      smoothLength: 3\n" \
    "inspector:\n  NullInspector\nlogger:\n  NullLogger\n"
static const char *kVdYaml =
    "readingDataPointsFilters:\n  - RandomSamplingDataPointsFilter:\n      prob: 0.7\n  - MaxDistDataPointsFilter:\n      maxDist: 6.0\n"
    "matcher:\n  KDTreeVarDistMatcher:\n    knn: 1\n" VD_CHAIN_TAIL;
static const char *kVdPlainYaml = "matcher:\n  KDTreeVarDistMatcher:\n    knn: 1\n" VD_CHAIN_TAIL;
static const char *kVdNormalsYaml = "matcher:\n  KDTreeVarDistMatcher:\n    knn: 1\n    maxDistField: normals\n" VD_CHAIN_TAIL;

// radius = base + slope * range, one row named `field`
template <typename T>
void add_radii(typename PointMatcher<T>::DataPoints &dp, const std::string &field, double base = 0.15, double slope = 0.05)
{
    pgslam_amd::Mat<T> r(1, dp.features.cols());
    for (int j = 0; j < dp.features.cols(); j++) {
        const double x = dp.features(0, j), y = dp.features(1, j), z = dp.features(2, j);
        r(0, j) = (T)(base + slope * std::sqrt(x * x + y * y + z * z));
    }
    dp.addDescriptor(field, r);
}

template <typename F>
std::string what_of(F f)
{
    try { f(); } catch (const std::runtime_error &e) { return e.what(); }
    return "";
}

template <typename T>
void run(const char *name)
{
    IMPORT_PGSLAM_TYPES(T)
    using A = pgslam_amd::Abi<T>;
    TransformationPtr rigid = PM::get().REG(Transformation).create("RigidTransformation");
    const DP ref = make_corner<T>(3000, 11, 0.003);
    const Matrix truth = pose<T>(0.15, -0.10, 0.02, 0.04);
    const DP bare = rigid->compute(make_corner<T>(3000, 12, 0.003), truth.inverse());
    DP rd = bare;
    add_radii<T>(rd, "maxSearchDist");
    {   // the refusals name the field
        typename PM::ICP icp;
        std::istringstream in(kVdPlainYaml);
        icp.loadFromYaml(in);
        const std::string missing = what_of([&] { icp(bare, ref); });
        CHECK(missing.find("KDTreeVarDistMatcher") != std::string::npos && missing.find("maxSearchDist") != std::string::npos);
        typename PM::ICP icp3;
        std::istringstream in3(kVdNormalsYaml);
        icp3.loadFromYaml(in3);
        const std::string three = what_of([&] { icp3(rd, ref); });
        CHECK(three.find("normals") != std::string::npos && three.find("one row") != std::string::npos);
        typename PM::ICPSequence seq;
        std::istringstream ins(kVdPlainYaml);
        seq.loadFromYaml(ins);
        seq.setMap(ref);
        const auto dev = seq.uploadReading(rd);
        const std::string device = what_of([&] { seq(dev, Matrix::Identity(4, 4)); });
        CHECK(device.find("device cloud") != std::string::npos && device.find("maxSearchDist") != std::string::npos);
        CHECK(pose_diff<T>(seq(rd, Matrix::Identity(4, 4)), Matrix::Identity(4, 4)) > 0.0);      // the host cloud goes through
    }
    {   // findClosests == arm + match, with radii about as large as the clouds' point spacing: some pairs are cut, some are kept
        DP rd = bare;
        add_radii<T>(rd, "maxSearchDist", 0.02, 0.01);
        typename PM::ICP icp;
        std::istringstream in(kVdPlainYaml);
        icp.loadFromYaml(in);
        icp.matcher->init(ref);
        const typename PM::Matches m = icp.matcher->findClosests(rd);
        const int n = (int)rd.getNbPoints();
        const T *row = rd.descriptors.data() + rd.getDescriptorStartingRow("maxSearchDist");
        const int stride = (int)rd.descriptors.rows();
        std::vector<int32_t> ids(n);
        std::vector<T> d2(n);
        PM::check(icp.ctx, A::arm_radii(icp.ctx, 1, &row, &stride, &n));
        PM::check(icp.ctx, A::match(icp.ctx, icp.matcher->mapId, rd.xyzPtr(), rd.xyzStride(), n, ids.data(), d2.data()));
        int cut = 0, kept = 0;
        for (int j = 0; j < n; j++) {
            CHECK(m.ids(0, j) == ids[j] && std::memcmp(&m.dists(0, j), &d2[j], sizeof(T)) == 0);
            const T r = row[(size_t)j * stride];
            CHECK(ids[j] < 0 ? std::isinf(d2[j]) : d2[j] <= r * r);
            (ids[j] < 0 ? cut : kept)++;
        }
        // unarmed, the same call finds more: the radii did cut
        PM::check(icp.ctx, A::match(icp.ctx, icp.matcher->mapId, rd.xyzPtr(), rd.xyzStride(), n, ids.data(), d2.data()));
        int none = 0;
        for (int j = 0; j < n; j++) none += ids[j] < 0;
        CHECK(kept > 0 && cut > none);
        std::printf("%s: findClosests ok  (%d of %d pairs within their radius, %d without a neighbour under the largest radius)\n", name, kept, n, none);
    }
    {   // ICP::operator() with reading filters ahead of the matcher == pgicp_align on the filtered cloud with the filtered row
        typename PM::ICP icp, twin;
        std::istringstream in(kVdYaml), in2(kVdYaml);
        icp.loadFromYaml(in);
        twin.loadFromYaml(in2);
        const Matrix Tres = icp(rd, ref);
        DP filtered(rd);
        twin.readingDataPointsFilters.init();
        twin.readingDataPointsFilters.apply(filtered);
        const int n = (int)filtered.getNbPoints();
        CHECK(n < (int)rd.getNbPoints() && n > 1000 && n == (int)icp.getPrefilteredReadingPtsCount());
        CHECK(filtered.descriptorExists("maxSearchDist"));
        const T *row = filtered.descriptors.data() + filtered.getDescriptorStartingRow("maxSearchDist");
        const int stride = (int)filtered.descriptors.rows();
        double Ti[16], To[16];
        pgslam_amd::to_row_major16(Matrix(Matrix::Identity(4, 4)), Ti);
        pgicp_stats st;
        // (the object's map of `ref` and its parameters -- max_dist = the largest radius -- are still in its context)
        PM::check(icp.ctx, A::arm_radii(icp.ctx, 1, &row, &stride, &n));
        PM::check(icp.ctx, A::align(icp.ctx, icp.matcher->mapId, filtered.xyzPtr(), filtered.xyzStride(), n, Ti, To, &st));
        const Matrix Tc = pgslam_amd::from_row_major16<T>(To);
        for (int i = 0; i < 4; i++) for (int j = 0; j < 4; j++) CHECK(std::memcmp(&Tres(i, j), &Tc(i, j), sizeof(T)) == 0);
        CHECK(st.n_finite > n / 4 && st.n_finite <= n);
        T largest = 0;
        for (int j = 0; j < n; j++) largest = std::max(largest, row[(size_t)j * stride]);
        CHECK(icp.matcher->maxDist == largest);
        const Matrix d = truth.inverse() * Tres;
        const double dt = std::sqrt((double)(d(0, 3) * d(0, 3) + d(1, 3) * d(1, 3) + d(2, 3) * d(2, 3)));
        CHECK(dt < 0.02);
        std::printf("%s: ok  (%d of %u points after the filters, %d with a neighbour in their radius, |dt| %.2e m)\n", name, n, rd.getNbPoints(), st.n_finite, dt);
    }
}

int main()
{
    run<float>("KDTreeVarDistMatcher <float>");
    run<double>("KDTreeVarDistMatcher <double>");
    std::puts("var dist gpu tests ok");
    return 0;
}
