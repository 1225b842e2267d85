// [EXT] The sensor filter chain through the C++ drop-in on the device (tests/test_cpp_sensor_chain.py drives it):
//   test_sensor_chain_gpu <scans> <maxDensity>.  <scans>: int32 n_reading, n_reference, 16 doubles T_init, 16 doubles T_truth
//   (row-major), the reading's and the reference's points as floats (16-ring scans in their sensors' frames).
//   DataPointsFilters::apply with a run as ONE pgicp_sensor_chain_* call against the same list under PGSLAM_HOST_SENSOR_CHAIN=1
//   (filter by filter, as before): the same labels in the same order, the same feature and descriptor bytes, for PointMatcher<float>
//   and PointMatcher<double>; lastFusedRun(); the lists that must not take the call; one ICP whose referenceDataPointsFilters is the
//   six-filter chain, the same pose as under the knob bit for bit.
#include "common.hpp"
#include <cstring>
#include <fstream>
#include <sstream>

template <typename T>
bool same_cloud(const typename PointMatcher<T>::DataPoints &a, const typename PointMatcher<T>::DataPoints &b)
{
    if (a.features.rows() != b.features.rows() || a.features.cols() != b.features.cols() || a.descriptors.rows() != b.descriptors.rows() ||
        a.descriptors.cols() != b.descriptors.cols() || a.descriptorLabels.size() != b.descriptorLabels.size())
        return false;
    for (size_t k = 0; k < a.descriptorLabels.size(); k++)
        if (a.descriptorLabels[k].text != b.descriptorLabels[k].text || a.descriptorLabels[k].span != b.descriptorLabels[k].span) return false;
    const size_t fb = sizeof(T) * (size_t)a.features.rows() * a.features.cols(), db = sizeof(T) * (size_t)a.descriptors.rows() * a.descriptors.cols();
    return (fb == 0 || std::memcmp(a.features.data(), b.features.data(), fb) == 0) &&
           (db == 0 || std::memcmp(a.descriptors.data(), b.descriptors.data(), db) == 0);
}

struct Scans {
    int n[2];
    double Ti[16], Tt[16];
    std::vector<float> rd, rf;
};

static Scans read_scans(const char *path)
{
    Scans s;
    std::ifstream in(path, std::ios::binary);
    in.read((char *)s.n, sizeof s.n); in.read((char *)s.Ti, sizeof s.Ti); in.read((char *)s.Tt, sizeof s.Tt);
    s.rd.resize(3 * (size_t)s.n[0]); s.rf.resize(3 * (size_t)s.n[1]);
    in.read((char *)s.rd.data(), sizeof(float) * s.rd.size());
    in.read((char *)s.rf.data(), sizeof(float) * s.rf.size());
    CHECK(in.good() && s.n[0] > 0 && s.n[1] > 0);
    return s;
}

template <typename T>
typename PointMatcher<T>::DataPoints cloud_of(const std::vector<float> &xyz, int drows)
{
    const int n = (int)xyz.size() / 3;
    std::vector<T> x(xyz.begin(), xyz.end());
    typename PointMatcher<T>::DataPoints c = PointMatcher<T>::DataPoints::fromXYZ(x.data(), n, nullptr);
    Lcg g(41);
    for (int r = 0; r < drows; r++) {
        typename PointMatcher<T>::Matrix d(r + 1, n);                 // spans 1, 2, ...
        for (int j = 0; j < n; j++) for (int k = 0; k <= r; k++) d(k, j) = (T)(g.next() - 0.5);
        c.addDescriptor("d" + std::to_string(r), d);
    }
    return c;
}

template <typename T>
typename PointMatcher<T>::DataPointsFilters from_yaml(const std::string &text)
{
    std::istringstream in(text);
    return typename PointMatcher<T>::DataPointsFilters(in);
}

// the list on a copy of `in`: fused where it can be, and under the knob; the two clouds must be the same object state
template <typename T>
typename PointMatcher<T>::DataPoints both_ways(const std::string &yaml, const typename PointMatcher<T>::DataPoints &in, size_t want_fused, const char *label)
{
    typedef PointMatcher<T> PM;
    unsetenv("PGSLAM_HOST_SENSOR_CHAIN");
    typename PM::DataPointsFilters fd = from_yaml<T>(yaml), fh = from_yaml<T>(yaml);
    typename PM::DataPoints c(in), h(in);
    fd.apply(c);
    if (fd.lastFusedRun() != want_fused) { std::fprintf(stderr, "%s: lastFusedRun() = %zu, expected %zu\n", label, fd.lastFusedRun(), want_fused); std::exit(1); }
    setenv("PGSLAM_HOST_SENSOR_CHAIN", "1", 1);
    fh.apply(h);
    unsetenv("PGSLAM_HOST_SENSOR_CHAIN");
    CHECK(fh.lastFusedRun() == 0);
    if (!same_cloud<T>(c, h)) { std::fprintf(stderr, "%s: the fused cloud differs from the filter-by-filter cloud (%u vs %u points)\n", label, c.getNbPoints(), h.getNbPoints()); std::exit(1); }
    fd.apply(c = in);                                      // and again on the same list object: the same state
    CHECK(same_cloud<T>(c, h) && fd.lastFusedRun() == want_fused);
    return c;
}

template <typename T>
void run_lists(const Scans &s, const std::string &max_density, const char *name)
{
    typedef PointMatcher<T> PM;
    const std::string sn = "- SurfaceNormalDataPointsFilter:\n    knn: 10\n    keepDensities: 1\n";
    const std::string sne = "- SurfaceNormalDataPointsFilter:\n    knn: 10\n    keepDensities: 1\n    keepEigenValues: 1\n";
    const std::string obs = "- ObservationDirectionDataPointsFilter\n", obs2 = "- ObservationDirectionDataPointsFilter:\n    x: 0.5\n    y: -0.25\n    z: 1\n";
    const std::string orient = "- OrientNormalsDataPointsFilter\n", away = "- OrientNormalsDataPointsFilter:\n    towardCenter: 0\n";
    const std::string shadow = "- ShadowDataPointsFilter:\n    eps: 0.2\n";
    const std::string md = "- MaxDensityDataPointsFilter:\n    maxDensity: " + max_density + "\n    seed: 7\n";
    const std::string noise = "- SimpleSensorNoiseDataPointsFilter\n", noise4 = "- SimpleSensorNoiseDataPointsFilter:\n    sensorType: 4\n    gain: 1.5\n";
    const std::string box = "- BoundingBoxDataPointsFilter:\n    xMin: -3\n    xMax: 3\n    yMin: -3\n    yMax: 3\n    zMin: -3\n    zMax: 3\n";
    const typename PM::DataPoints bare = cloud_of<T>(s.rf, 0), carrying = cloud_of<T>(s.rf, 2);
    const unsigned n = bare.getNbPoints();
    int lists = 0;
    {   // the sensor's usual chain: one call for the six filters
        const typename PM::DataPoints c = both_ways<T>(noise + sn + obs + orient + shadow + md, bare, 6, "six");
        CHECK(c.getNbPoints() > n / 10 && c.getNbPoints() < n - n / 10);
        CHECK(c.descriptorLabels.size() == 4 && c.descriptorLabels[0].text == "simpleSensorNoise" && c.descriptorLabels[1].text == "normals" &&
              c.descriptorLabels[2].text == "densities" && c.descriptorLabels[3].text == "observationDirections" && c.descriptors.rows() == 8);
        // every kept normal points toward the sensor at the origin: n . (0 - x) >= 0
        const int rn = c.getDescriptorStartingRow("normals");
        for (unsigned i = 0; i < c.getNbPoints(); i++)
            CHECK(!(c.descriptors(rn, i) * -c.features(0, i) + c.descriptors(rn + 1, i) * -c.features(1, i) + c.descriptors(rn + 2, i) * -c.features(2, i) < 0));
        lists++;
    }
    // descriptors of the cloud's own travel; eigenvalues; the other parameters; MaxDensity ahead of Shadow; stages behind the drops
    both_ways<T>(noise4 + sne + obs2 + away + shadow + md, carrying, 6, "six, carrying"); lists++;
    both_ways<T>(sne + obs + orient + md + shadow, carrying, 5, "MaxDensity ahead of Shadow"); lists++;
    both_ways<T>(sn + shadow + md + obs + away + noise, bare, 6, "stages behind the drops"); lists++;
    // SimpleSensorNoise and ObservationDirection in front of the head
    {
        const typename PM::DataPoints c = both_ways<T>(obs + noise + sn + orient + shadow, bare, 5, "leading stages");
        CHECK(c.descriptorLabels[0].text == "observationDirections" && c.descriptorLabels[1].text == "simpleSensorNoise" && c.descriptorLabels[2].text == "normals");
        lists++;
    }
    // no dropping stage; a single stage
    both_ways<T>(sn + obs + orient, carrying, 3, "no drop"); lists++;
    both_ways<T>(sn + shadow, bare, 2, "shadow alone"); lists++;
    both_ways<T>("- SurfaceNormalDataPointsFilter:\n    knn: 10\n" + noise, bare, 2, "normals and noise"); lists++;
    // a run broken by a BoundingBox in the middle: the head of the list is one call, the rest goes filter by filter
    both_ways<T>(sn + obs + orient + box + shadow + md, bare, 3, "broken by BoundingBox"); lists++;
    // a cloud that already carries a descriptor the run writes: filter by filter, as before
    {
        typename PM::DataPoints pre(bare);
        typename PM::Matrix z(1, (int)n);
        for (unsigned j = 0; j < n; j++) z(0, j) = T(1);
        pre.addDescriptor("simpleSensorNoise", z);
        // (SimpleSensorNoise overwrites its row on the host; what stands behind it is a run of five that writes nothing present)
        both_ways<T>(noise + sn + obs + orient + shadow + md, pre, 5, "noise present"); lists++;
        typename PM::DataPoints pre2(bare);
        typename PM::Matrix up(3, (int)n);
        for (unsigned j = 0; j < n; j++) { up(0, j) = T(0); up(1, j) = T(0); up(2, j) = T(1); }
        pre2.addDescriptor("normals", up);
        both_ways<T>(noise + sn + obs + orient + shadow + md, pre2, 0, "normals present"); lists++;
    }
    // SurfaceNormal + MaxDensity alone: not a run, and still the older fused pass
    {
        unsetenv("PGSLAM_HOST_SENSOR_CHAIN");
        typename PM::DataPointsFilters f = from_yaml<T>(sn + md);
        typename PM::DataPoints c(bare), two(bare);
        f.apply(c);
        auto m = std::dynamic_pointer_cast<typename PM::MaxDensityDataPointsFilter>(f.at(1));
        CHECK(f.lastFusedRun() == 0 && m && m->ranOnDevice() && c.getNbPoints() > 0 && c.getNbPoints() < n);
        f.at(0)->inPlaceFilter(two);
        f.at(1)->inPlaceFilter(two);
        CHECK(same_cloud<T>(c, two));
        lists++;
    }
    // a coordinate that is not finite: the call refuses the cloud, and the list goes filter by filter and says what it always said
    {
        typename PM::DataPoints bad(bare);
        bad.features(1, 37) = std::numeric_limits<T>::quiet_NaN();
        typename PM::DataPointsFilters f = from_yaml<T>(sn + shadow);
        bool threw = false;
        try { f.apply(bad); } catch (const std::exception &) { threw = true; }
        CHECK(threw && f.lastFusedRun() == 0);
        typename PM::DataPoints c(bare);
        f.apply(c);                                       // the list and its context are usable afterwards
        CHECK(f.lastFusedRun() == 2 && c.getNbPoints() > 0);
        lists++;
    }
    std::printf("%s: ok  (%d lists: one chain call == filter by filter, labels, order and bytes)\n", name, lists);
}

static const char *kChainIcpYaml =
    "readingDataPointsFilters:\n  - IdentityDataPointsFilter\n"
    "referenceDataPointsFilters:\n  - SimpleSensorNoiseDataPointsFilter\n  - SurfaceNormalDataPointsFilter:\n      knn: 10\n      keepDensities: 1\n"
    "  - ObservationDirectionDataPointsFilter\n  - OrientNormalsDataPointsFilter\n  - ShadowDataPointsFilter:\n      eps: 0.2\n"
    "  - MaxDensityDataPointsFilter:\n      maxDensity: %s\n      seed: 7\n"
    "matcher:\n  KDTreeMatcher:\n    knn: 1\n    epsilon: 0\n    maxDist: 2.0\n"
    "outlierFilters:\n  - TrimmedDistOutlierFilter:\n      ratio: 0.85\n"
    "errorMinimizer:\n  PointToPlaneErrorMinimizer\n"
    "transformationCheckers:\n  - CounterTransformationChecker:\n      maxIterationCount: 40\n"
    "  - DifferentialTransformationChecker:\n      minDiffRotErr: 0.0001\n      minDiffTransErr: 0.001\n      smoothLength: 3\n"
    "inspector:\n  NullInspector\nlogger:\n  NullLogger\n";

void run_icp(const Scans &s, const char *max_density)
{
    typedef float T;
    IMPORT_PGSLAM_TYPES(T)
    const DP reading = DP::fromXYZ(s.rd.data(), s.n[0], nullptr), reference = DP::fromXYZ(s.rf.data(), s.n[1], nullptr);
    Matrix init(4, 4), truth(4, 4);
    for (int r = 0; r < 4; r++) for (int c = 0; c < 4; c++) { init(r, c) = (T)s.Ti[4 * r + c]; truth(r, c) = (T)s.Tt[4 * r + c]; }
    Matrix poses[2];
    unsigned counts[2] = {0, 0};
    for (int knob = 0; knob < 2; knob++) {
        if (knob) setenv("PGSLAM_HOST_SENSOR_CHAIN", "1", 1); else unsetenv("PGSLAM_HOST_SENSOR_CHAIN");
        PM::ICP icp;
        std::vector<char> text(std::strlen(kChainIcpYaml) + std::strlen(max_density) + 1);
        std::snprintf(text.data(), text.size(), kChainIcpYaml, max_density);
        std::istringstream ys(text.data());
        icp.loadFromYaml(ys);
        CHECK(icp.referenceDataPointsFilters.size() == 6 && icp.referenceDataPointsFilters.sensorChainRunAt(0) == 6);
        poses[knob] = icp(reading, reference, init);
        CHECK(icp.referenceDataPointsFilters.lastFusedRun() == (knob ? 0u : 6u));
        counts[knob] = icp.getPrefilteredReferencePtsCount();
    }
    unsetenv("PGSLAM_HOST_SENSOR_CHAIN");
    CHECK(counts[0] == counts[1] && counts[0] > 0 && (int)counts[0] < s.n[1]);
    CHECK(std::memcmp(poses[0].data(), poses[1].data(), sizeof(T) * 16) == 0);
    const Matrix d = truth.inverse() * poses[0], d0 = truth.inverse() * init;
    const double dt = std::sqrt((double)(d(0, 3) * d(0, 3) + d(1, 3) * d(1, 3) + d(2, 3) * d(2, 3)));
    const double dt0 = std::sqrt((double)(d0(0, 3) * d0(0, 3) + d0(1, 3) * d0(1, 3) + d0(2, 3) * d0(2, 3)));
    std::printf("ICP<float>, reference chain of six as one call: %u of %d reference points, the pose equals the filter-by-filter run's bit for bit; "
                "|dt| %.3e m (from %.3e m)\n", counts[0], s.n[1], dt, dt0);
    CHECK(dt < dt0);
}

int main(int argc, char **argv)
{
    if (argc != 3) { std::fprintf(stderr, "usage: test_sensor_chain_gpu <scans> <maxDensity>\n"); return 2; }
    const Scans s = read_scans(argv[1]);
    run_lists<float>(s, argv[2], "sensor chain<float>");
    run_lists<double>(s, argv[2], "sensor chain<double>");
    run_icp(s, argv[2]);
    std::puts("sensor chain gpu tests ok");
    return 0;
}
