// [EXT] NormalSpaceDataPointsFilter through the C++ drop-in on the device: the device form leaves the DataPoints the host form
// leaves, bit for bit, on three cases in both precisions, and a YAML reading chain SurfaceNormal -> NormalSpace through
// ICP::operator() runs the filter on the device and converges.
#include "common.hpp"
#include <cstring>

template <typename T>
void run_forms(const char *name)
{
    typedef PointMatcher<T> PM;
    // a room corner: three planes and a table top, so a handful of buckets hold everything and the small ones run out; the
    // jittered copy spreads the normals over many buckets (not unit length: the filter does not ask for it)
    typename PM::DataPoints corner = make_corner<T>(3000, 41, 0.003);
    typename PM::DataPoints spread(corner);
    Lcg g(7);
    for (unsigned i = 0; i < spread.getNbPoints(); i++)
        for (int a = 0; a < 3; a++) spread.descriptors(a, i) += (T)(0.8 * (g.next() - 0.5));
    struct Case { const typename PM::DataPoints *cloud; size_t nb; double eps; unsigned long long seed; };
    const Case cases[3] = {{&corner, 500, 0.09, 1}, {&spread, 2500, 0.09, 77}, {&spread, 9000, 0.0175, 5}};
    for (const Case &k : cases) {
        typename PM::NormalSpaceDataPointsFilter ns(k.nb, k.eps, k.seed);
        typename PM::DataPoints dev(*k.cloud), hst(*k.cloud);
        for (unsigned i = 0; i < dev.getNbPoints(); i++) dev.features(3, i) = hst.features(3, i) = (T)i;   // a further feature row travels with the pick
        unsetenv("PGSLAM_HOST_INPUT_STAGE");
        ns.inPlaceFilter(dev);
        CHECK(ns.ranOnDevice());
        setenv("PGSLAM_HOST_INPUT_STAGE", "1", 1);
        ns.inPlaceFilter(hst);
        unsetenv("PGSLAM_HOST_INPUT_STAGE");
        CHECK(!ns.ranOnDevice());
        CHECK(dev.getNbPoints() == k.nb && hst.getNbPoints() == k.nb && k.nb < k.cloud->getNbPoints());
        CHECK(dev.features.rows() == 4 && dev.descriptors.rows() == 3);
        CHECK(std::memcmp(dev.features.data(), hst.features.data(), sizeof(T) * 4 * k.nb) == 0);
        CHECK(std::memcmp(dev.descriptors.data(), hst.descriptors.data(), sizeof(T) * 3 * k.nb) == 0);
    }
    std::printf("%s: ok  (device form == host form, three cases)\n", name);
}

static const char *kNsIcpYaml =
    "readingDataPointsFilters:\n  - SurfaceNormalDataPointsFilter:\n      knn: 10\n"
    "  - NormalSpaceDataPointsFilter:\n      nbSample: 4000\n      epsilon: 0.2\n"
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
    std::istringstream in(kNsIcpYaml);
    icp.loadFromYaml(in);
    auto ns = std::dynamic_pointer_cast<typename PM::NormalSpaceDataPointsFilter>(icp.readingDataPointsFilters.at(1));
    CHECK(ns);
    const Matrix res = icp(rd, ref);
    CHECK(ns->ranOnDevice());
    const Matrix d = truth.inverse() * res;
    const double dt = std::sqrt((double)(d(0, 3) * d(0, 3) + d(1, 3) * d(1, 3) + d(2, 3) * d(2, 3)));
    CHECK(dt < 0.02);
    std::printf("%s: ok  (|dt| %.2e m)\n", name, dt);
}

int main()
{
    run_forms<float>("NormalSpace<float>");
    run_forms<double>("NormalSpace<double>");
    run_icp<float>("ICP<float>, reading chain [SurfaceNormal, NormalSpace]");
    run_icp<double>("ICP<double>, reading chain [SurfaceNormal, NormalSpace]");
    std::puts("normal space gpu tests ok");
    return 0;
}
