// [EXT] CovarianceSamplingDataPointsFilter through the C++ drop-in on the device: the device form's picks equal the host form's
// given the device's frame, and a YAML chain SurfaceNormal -> CovarianceSampling on a reading through ICP::operator().
#include "common.hpp"

template <typename T>
void run_forms(const char *name)
{
    typedef PointMatcher<T> PM;
    for (int tn = 0; tn < 3; tn++) {
        const typename PM::DataPoints base = make_corner<T>(3000, 31 + tn, 0.003);
        typename PM::DataPoints dev(base);
        typename PM::CovarianceSamplingDataPointsFilter cs(800, tn);
        unsetenv("PGSLAM_HOST_INPUT_STAGE");
        cs.inPlaceFilter(dev);
        CHECK(cs.ranOnDevice() && dev.getNbPoints() == 800);
        // the host form's picks given the DEVICE's frame, gathered the same way
        std::vector<int32_t> picks;
        cs.hostPicks(base, cs.lastFrame, picks);
        CHECK(picks.size() == 800);
        typename PM::DataPoints hst(base);
        PM::gatherColumns(hst, picks.data(), 800);
        CHECK(std::memcmp(dev.features.data(), hst.features.data(), sizeof(T) * 4 * 800) == 0);
        CHECK(std::memcmp(dev.descriptors.data(), hst.descriptors.data(), sizeof(T) * 3 * 800) == 0);
        // the knob: the host form from end to end; its frame sums in index order, so only the sizes are compared
        setenv("PGSLAM_HOST_INPUT_STAGE", "1", 1);
        typename PM::DataPoints knob(base);
        cs.inPlaceFilter(knob);
        unsetenv("PGSLAM_HOST_INPUT_STAGE");
        CHECK(!cs.ranOnDevice() && knob.getNbPoints() == 800);
    }
    std::printf("%s: ok  (device picks == host picks given the device's frame, torqueNorm 0, 1, 2)\n", name);
}

static const char *kCovIcpYaml =
    "readingDataPointsFilters:\n  - SurfaceNormalDataPointsFilter:\n      knn: 10\n"
    "  - CovarianceSamplingDataPointsFilter:\n      nbSample: 2000\n      torqueNorm: 1\n"
    "referenceDataPointsFilters:\n  - SurfaceNormalDataPointsFilter:\n      knn: 10\n" PGSLAM_TEST_CHAIN_TAIL;

template <typename T>
void run_icp(const char *name)
{
    IMPORT_PGSLAM_TYPES(T)
    TransformationPtr rigid = PM::get().REG(Transformation).create("RigidTransformation");
    const DP ref = make_corner<T>(6000, 21, 0.003);
    const Matrix truth = pose<T>(0.04, -0.03, 0.0, 0.02);
    const DP rd = rigid->compute(make_corner<T>(6000, 22, 0.003), truth.inverse());
    typename PM::ICP icp;
    std::istringstream in(kCovIcpYaml);
    icp.loadFromYaml(in);
    auto cs = std::dynamic_pointer_cast<typename PM::CovarianceSamplingDataPointsFilter>(icp.readingDataPointsFilters.at(1));
    CHECK(cs);
    const Matrix res = icp(rd, ref);
    CHECK(cs->ranOnDevice());
    const Matrix d = truth.inverse() * res;
    const double dt = std::sqrt((double)(d(0, 3) * d(0, 3) + d(1, 3) * d(1, 3) + d(2, 3) * d(2, 3)));
    CHECK(dt < 0.02);
    std::printf("%s: ok  (2000 of %u reading points, |dt| %.2e m)\n", name, rd.getNbPoints(), dt);
}

int main()
{
    run_forms<float>("CovarianceSampling<float>");
    run_forms<double>("CovarianceSampling<double>");
    run_icp<float>("ICP<float>, reading chain [SurfaceNormal, CovarianceSampling]");
    run_icp<double>("ICP<double>, reading chain [SurfaceNormal, CovarianceSampling]");
    std::puts("covariance sampling gpu tests ok");
    return 0;
}
