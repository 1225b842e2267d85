// [EXT] OctreeGridDataPointsFilter through the C++ drop-in on the device: the device form leaves the DataPoints the host form
// leaves, bit for bit, and a YAML reading chain OctreeGrid -> SurfaceNormal through ICP::operator() gives the transform the same
// chain gives under PGSLAM_HOST_INPUT_STAGE=1, bit for bit.
#include "common.hpp"
#include <cstring>

template <typename T>
void run_forms(const char *name)
{
    typedef PointMatcher<T> PM;
    typename PM::DataPoints base = make_corner<T>(3000, 41, 0.003);
    for (unsigned i = 0; i < base.getNbPoints(); i++) base.features(3, i) = (T)i;      // a further feature row: it travels with the kept point
    struct Par { size_t mp; T ms; };
    for (int method : {0, 2, 3})
        for (const Par &p : {Par{1, T(0)}, Par{5, T(0)}, Par{400, T(0.8)}, Par{100000, T(0)}}) {
            typename PM::OctreeGridDataPointsFilter oc(p.mp, p.ms, method);
            typename PM::DataPoints dev(base), hst(base);
            unsetenv("PGSLAM_HOST_INPUT_STAGE");
            oc.inPlaceFilter(dev);
            CHECK(oc.ranOnDevice());
            setenv("PGSLAM_HOST_INPUT_STAGE", "1", 1);
            oc.inPlaceFilter(hst);
            unsetenv("PGSLAM_HOST_INPUT_STAGE");
            CHECK(!oc.ranOnDevice());
            CHECK(dev.getNbPoints() == hst.getNbPoints() && dev.getNbPoints() > 0 && dev.getNbPoints() <= base.getNbPoints());
            if (p.mp == 100000) CHECK(dev.getNbPoints() == 1);
            CHECK(dev.features.rows() == 4 && dev.descriptors.rows() == 3);
            CHECK(std::memcmp(dev.features.data(), hst.features.data(), sizeof(T) * 4 * dev.getNbPoints()) == 0);
            CHECK(std::memcmp(dev.descriptors.data(), hst.descriptors.data(), sizeof(T) * 3 * dev.getNbPoints()) == 0);
        }
    std::printf("%s: ok  (device form == host form, methods 0, 2, 3)\n", name);
}

static const char *kOctIcpYaml =
    "readingDataPointsFilters:\n  - OctreeGridDataPointsFilter:\n      maxSizeByNode: 0.08\n      maxPointByNode: 4\n      samplingMethod: 2\n"
    "  - SurfaceNormalDataPointsFilter:\n      knn: 10\n"
    "referenceDataPointsFilters:\n  - SurfaceNormalDataPointsFilter:\n      knn: 10\n" PGSLAM_TEST_CHAIN_TAIL;

template <typename T>
void run_icp(const char *name)
{
    IMPORT_PGSLAM_TYPES(T)
    TransformationPtr rigid = PM::get().REG(Transformation).create("RigidTransformation");
    const DP ref = make_corner<T>(6000, 21, 0.003);
    const Matrix truth = pose<T>(0.04, -0.03, 0.0, 0.02);
    const DP rd = rigid->compute(make_corner<T>(6000, 22, 0.003), truth.inverse());
    Matrix res[2];
    for (int host = 0; host < 2; host++) {
        if (host) setenv("PGSLAM_HOST_INPUT_STAGE", "1", 1); else unsetenv("PGSLAM_HOST_INPUT_STAGE");
        typename PM::ICP icp;
        std::istringstream in(kOctIcpYaml);
        icp.loadFromYaml(in);
        auto oc = std::dynamic_pointer_cast<typename PM::OctreeGridDataPointsFilter>(icp.readingDataPointsFilters.at(0));
        CHECK(oc);
        res[host] = icp(rd, ref);
        CHECK(oc->ranOnDevice() == !host);
    }
    unsetenv("PGSLAM_HOST_INPUT_STAGE");
    CHECK(std::memcmp(res[0].data(), res[1].data(), sizeof(T) * 16) == 0);
    const Matrix d = truth.inverse() * res[0];
    const double dt = std::sqrt((double)(d(0, 3) * d(0, 3) + d(1, 3) * d(1, 3) + d(2, 3) * d(2, 3)));
    CHECK(dt < 0.02);
    std::printf("%s: ok  (|dt| %.2e m, the same bits with the host input stage)\n", name, dt);
}

int main()
{
    run_forms<float>("OctreeGrid<float>");
    run_forms<double>("OctreeGrid<double>");
    run_icp<float>("ICP<float>, reading chain [OctreeGrid, SurfaceNormal]");
    run_icp<double>("ICP<double>, reading chain [OctreeGrid, SurfaceNormal]");
    std::puts("octree grid gpu tests ok");
    return 0;
}
