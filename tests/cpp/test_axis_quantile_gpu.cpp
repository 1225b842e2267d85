// [EXT] MaxQuantileOnAxisDataPointsFilter through the C++ drop-in on the device: a filter list that holds it, run in one device
// pass (filterAndTransformOnDevice, filterOnDeviceDeferred), leaves the DataPoints DataPointsFilters::apply leaves on the host,
// bit for bit, in both precisions; and a YAML reading chain with the filter through ICP::operator() converges.
#include "common.hpp"
#include <cstring>
#include <limits>

template <typename T>
void run_forms(const char *name)
{
    typedef PointMatcher<T> PM;
    const T nan = std::numeric_limits<T>::quiet_NaN(), inf = std::numeric_limits<T>::infinity();
    typename PM::DataPoints base = make_corner<T>(3000, 41, 0.003);
    const int n = (int)base.getNbPoints();
    for (int i = 0; i < n; i++) base.features(3, i) = (T)i;          // a further feature row travels with a kept point
    base.features(2, 5) = nan; base.features(0, 9) = nan; base.features(1, 77) = inf; base.features(2, 78) = -inf;
    base.features(2, 100) = (T)-0.0; base.features(2, 101) = (T)0.0;
    const char *lists[] = {
        "- MaxQuantileOnAxisDataPointsFilter:\n    dim: 2\n    ratio: 0.9\n",
        "- MaxQuantileOnAxisDataPointsFilter:\n    ratio: 0.7\n",
        "- RemoveNaNDataPointsFilter\n- DistanceLimitDataPointsFilter:\n    dist: 6\n    removeInside: 0\n"
        "- MaxQuantileOnAxisDataPointsFilter:\n    dim: 1\n    ratio: 0.95\n- FixStepSamplingDataPointsFilter:\n    startStep: 2\n"
        "- MaxQuantileOnAxisDataPointsFilter:\n    dim: 2\n    ratio: 0.5\n",
        "- MaxQuantileOnAxisDataPointsFilter:\n    dim: 0\n    ratio: 1e-7\n",
    };
    pgslam_amd::LazyContext ctx;
    const typename PM::TransformationParameters I = PM::Matrix::Identity(4, 4);
    int li = 0;
    for (const char *text : lists) {
        std::istringstream a(text), b(text), c(text);
        typename PM::DataPointsFilters on_host(a), on_dev(b), deferred(c);
        typename PM::DataPoints hst(base), dev(base), def(base);
        on_host.apply(hst);
        const T *d = nullptr;
        CHECK(PM::filterAndTransformOnDevice(ctx, on_dev, dev, I, &d));
        CHECK(dev.getNbPoints() == hst.getNbPoints() && dev.features.rows() == 4 && dev.descriptors.rows() == 3);
        const size_t k = hst.getNbPoints();
        CHECK(li == 3 ? k == 0 : (k > 0 && k < (size_t)n));
        CHECK(std::memcmp(dev.features.data(), hst.features.data(), sizeof(T) * 4 * k) == 0);
        CHECK(std::memcmp(dev.descriptors.data(), hst.descriptors.data(), sizeof(T) * 3 * k) == 0);
        // the deferred form: the kept count and the dropped list close the same gaps (when the list holds them)
        int kept = -1;
        std::vector<int32_t> dropped;
        if (PM::filterOnDeviceDeferred(ctx, deferred, def, I, &d, &kept, dropped)) {
            PM::compactByDropped(def, dropped);
            CHECK((size_t)kept == k && def.getNbPoints() == k);
            CHECK(std::memcmp(def.features.data(), hst.features.data(), sizeof(T) * 4 * k) == 0);
        } else
            CHECK((size_t)n - k > 4096);
        li++;
    }
    std::printf("%s: ok  (device list == host filters, four lists)\n", name);
}

static const char *kMqIcpYaml =
    "readingDataPointsFilters:\n  - DistanceLimitDataPointsFilter:\n      dist: 40\n      removeInside: 0\n"
    "  - MaxQuantileOnAxisDataPointsFilter:\n      dim: 2\n      ratio: 0.95\n" PGSLAM_TEST_CHAIN_TAIL;

template <typename T>
void run_icp(const char *name)
{
    IMPORT_PGSLAM_TYPES(T)
    TransformationPtr rigid = PM::get().REG(Transformation).create("RigidTransformation");
    const DP ref = make_corner<T>(6000, 21, 0.003);
    const Matrix truth = pose<T>(0.04, -0.03, 0.0, 0.02);
    const DP rd = rigid->compute(make_corner<T>(6000, 22, 0.003), truth.inverse());
    typename PM::ICP icp;
    std::istringstream in(kMqIcpYaml);
    icp.loadFromYaml(in);
    CHECK(std::dynamic_pointer_cast<typename PM::MaxQuantileOnAxisDataPointsFilter>(icp.readingDataPointsFilters.at(1)));
    const Matrix res = icp(rd, ref);
    const Matrix d = truth.inverse() * res;
    const double dt = std::sqrt((double)(d(0, 3) * d(0, 3) + d(1, 3) * d(1, 3) + d(2, 3) * d(2, 3)));
    CHECK(dt < 0.02);
    std::printf("%s: ok  (|dt| %.2e m)\n", name, dt);
}

int main()
{
    run_forms<float>("MaxQuantileOnAxis<float>");
    run_forms<double>("MaxQuantileOnAxis<double>");
    run_icp<float>("ICP<float>, reading chain [DistanceLimit, MaxQuantileOnAxis]");
    run_icp<double>("ICP<double>, reading chain [DistanceLimit, MaxQuantileOnAxis]");
    std::puts("axis quantile gpu tests ok");
    return 0;
}
