// [EXT] IncidenceAngle, Sphericality and CutAtDescriptorThreshold through the C++ drop-in on the device
// (tests/test_cpp_descriptor_filters.py drives it):
//   test_descriptor_filters_gpu <scans> <incidence threshold> <sphericality threshold> <maxDensity> <unstructureness threshold>
//   <structureness threshold> (medians of the reference scan's rows, chosen by the driver).  <scans>: int32 n_reading, n_reference,
//   16 doubles T_init, 16 doubles T_truth (row-major), the reading's and the reference's points as floats (16-ring scans in their
//   sensors' frames).
//   DataPointsFilters::apply with a run that holds the three filters as ONE pgicp_sensor_chain_ext_* call against the same list under
//   PGSLAM_HOST_SENSOR_CHAIN=1 (filter by filter): the same labels in the same order, the same feature and descriptor bytes, for
//   PointMatcher<float> and PointMatcher<double>; lastFusedRun(); the lists that must not take the call; filterAndTransformOnDevice with
//   a cut entry against host apply followed by the transformation; one ICP whose referenceDataPointsFilters is the list, the same pose
//   as under the knob bit for bit.
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

// the cloud with `drows` descriptors d0, d1, ... of spans 1, 2, ...
template <typename T>
typename PointMatcher<T>::DataPoints cloud_of(const std::vector<float> &xyz, int drows)
{
    const int n = (int)xyz.size() / 3;
    std::vector<T> x(xyz.begin(), xyz.end());
    typename PointMatcher<T>::DataPoints c = PointMatcher<T>::DataPoints::fromXYZ(x.data(), n, nullptr);
    Lcg g(41);
    for (int r = 0; r < drows; r++) {
        typename PointMatcher<T>::Matrix d(r + 1, n);
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

static std::string cut(const std::string &name, int larger, const std::string &thr)
{
    return "- CutAtDescriptorThresholdDataPointsFilter:\n    descName: " + name + "\n    useLargerThan: " + std::to_string(larger) + "\n    threshold: " + thr + "\n";
}

template <typename T>
void run_lists(const Scans &s, const std::string &thr_inc, const std::string &thr_sph, const std::string &max_density, const std::string &thr_uns,
               const std::string &thr_str, const char *name)
{
    typedef PointMatcher<T> PM;
    const std::string sn = "- SurfaceNormalDataPointsFilter:\n    knn: 10\n    keepEigenValues: 1\n    keepDensities: 1\n";
    const std::string obs = "- ObservationDirectionDataPointsFilter\n", orient = "- OrientNormalsDataPointsFilter\n";
    const std::string inc = "- IncidenceAngleDataPointsFilter\n", sph = "- SphericalityDataPointsFilter\n";
    const std::string sphall = "- SphericalityDataPointsFilter:\n    keepUnstructureness: 1\n    keepStructureness: 1\n";
    const std::string shadow = "- ShadowDataPointsFilter:\n    eps: 0.2\n", noise = "- SimpleSensorNoiseDataPointsFilter\n";
    const std::string md = "- MaxDensityDataPointsFilter:\n    maxDensity: " + max_density + "\n    seed: 7\n";
    const std::string box = "- BoundingBoxDataPointsFilter:\n    xMin: -3\n    xMax: 3\n    yMin: -3\n    yMax: 3\n    zMin: -3\n    zMax: 3\n";
    const typename PM::DataPoints bare = cloud_of<T>(s.rf, 0), carrying = cloud_of<T>(s.rf, 2);
    const unsigned n = bare.getNbPoints();
    int lists = 0;
    {   // the issue's list: one call for the eight filters
        const typename PM::DataPoints c = both_ways<T>(sn + obs + orient + inc + cut("incidenceAngles", 1, thr_inc) + sph + cut("sphericality", 1, thr_sph) + md, bare, 8, "the list");
        CHECK(c.getNbPoints() > n / 20 && c.getNbPoints() < n / 2);
        const char *want[] = {"normals", "densities", "eigValues", "observationDirections", "incidenceAngles", "sphericality"};
        CHECK(c.descriptorLabels.size() == 6 && c.descriptors.rows() == 12);
        for (int k = 0; k < 6; k++) CHECK(c.descriptorLabels[k].text == want[k]);
        const int ri = c.getDescriptorStartingRow("incidenceAngles"), rs = c.getDescriptorStartingRow("sphericality");
        const T ti = (T)std::stod(thr_inc), ts = (T)std::stod(thr_sph);
        for (unsigned i = 0; i < c.getNbPoints(); i++) CHECK(c.descriptors(ri, i) <= ti && c.descriptors(rs, i) <= ts);
        lists++;
    }
    // the cloud's own descriptors travel; all three rows of Sphericality, in their order; cuts on them in both directions
    {
        const typename PM::DataPoints c = both_ways<T>(noise + sn + sphall + cut("unstructureness", 0, thr_uns) + obs + inc + cut("structureness", 1, thr_str) + shadow + md, carrying, 9,
                                                       "carrying, three rows");
        CHECK(c.getNbPoints() > 0 && c.getNbPoints() < n && c.descriptorLabels.size() == 11 && c.descriptorLabels[6].text == "sphericality" &&
              c.descriptorLabels[7].text == "unstructureness" && c.descriptorLabels[8].text == "structureness" && c.descriptorLabels[10].text == "incidenceAngles");
        lists++;
    }
    // a cut on a one-row descriptor the cloud carries, ahead of and behind the run's own rows
    {
        const typename PM::DataPoints c = both_ways<T>(sn + cut("d0", 1, "0.1") + obs + inc + cut("d0", 0, "-0.3") + cut("densities", 1, max_density), carrying, 6, "a carried row");
        CHECK(c.getNbPoints() > 0 && c.getNbPoints() < n / 2);
        lists++;
    }
    // each of the three alone behind the head; without OrientNormals the angles lie on both sides of pi / 2
    {
        const typename PM::DataPoints c = both_ways<T>(sn + obs + inc, bare, 3, "incidence alone");
        const int ri = c.getDescriptorStartingRow("incidenceAngles");
        unsigned below = 0, above = 0;
        for (unsigned i = 0; i < n; i++) { below += c.descriptors(ri, i) < T(1.5707963267948966); above += c.descriptors(ri, i) > T(1.5707963267948966); }
        CHECK(c.getNbPoints() == n && below > n / 10 && above > n / 10);
        lists++;
    }
    both_ways<T>(sn + sph, carrying, 2, "sphericality alone"); lists++;
    both_ways<T>(sn + cut("densities", 0, max_density), bare, 2, "a cut alone"); lists++;
    // a cut that drops everything, with stages behind it; a NaN threshold
    CHECK(both_ways<T>(sn + obs + inc + cut("incidenceAngles", 1, "-1") + sph + md, bare, 6, "drops all").getNbPoints() == 0); lists++;
    CHECK(both_ways<T>(sn + cut("densities", 1, "nan"), bare, 2, "NaN threshold").getNbPoints() == 0); lists++;
    // lists that must not fuse, or only in part: the filters run one by one and leave the same cloud
    {
        typename PM::DataPoints w(bare);
        typename PM::Matrix up(3, (int)n);
        for (unsigned j = 0; j < n; j++) { up(0, j) = T(0); up(1, j) = T(0); up(2, j) = T(1); }
        w.addDescriptor("normals", up);
        both_ways<T>(obs + orient + inc + cut("incidenceAngles", 1, thr_inc), w, 0, "no head"); lists++;
    }
    both_ways<T>(sn + obs + inc + box + cut("incidenceAngles", 1, thr_inc), bare, 3, "broken by BoundingBox"); lists++;
    both_ways<T>("- SurfaceNormalDataPointsFilter:\n    knn: 10\n    keepEigenVectors: 1\n    keepEigenValues: 1\n" + sph, bare, 0, "an ext head"); lists++;
    {
        // a cloud that already carries a row the run writes: filter by filter
        typename PM::DataPoints pre(bare);
        typename PM::Matrix z(1, (int)n);
        for (unsigned j = 0; j < n; j++) z(0, j) = T(1);
        pre.addDescriptor("sphericality", z);
        both_ways<T>(sn + sph + cut("sphericality", 1, thr_sph), pre, 0, "sphericality present"); lists++;
        // a cut on a descriptor that is not there ends the run ahead of it, runs on the host, and throws what it always throws
        unsetenv("PGSLAM_HOST_SENSOR_CHAIN");
        typename PM::DataPointsFilters f = from_yaml<T>(sn + obs + inc + cut("nothing", 1, "1"));
        typename PM::DataPoints c(bare);
        bool threw = false;
        try { f.apply(c); } catch (const typename PM::DataPoints::InvalidField &) { threw = true; }
        CHECK(threw && f.lastFusedRun() == 3);
        // ... and one on a descriptor of two rows
        typename PM::DataPointsFilters g = from_yaml<T>(sn + cut("d1", 1, "0"));
        typename PM::DataPoints c2(carrying);
        threw = false;
        try { g.apply(c2); } catch (const typename PM::DataPoints::InvalidField &) { threw = true; }
        CHECK(threw && g.lastFusedRun() == 0);
        lists++;
    }
    // runs without one of the three still take the older call and give what they gave
    both_ways<T>(noise + sn + obs + orient + shadow + md, bare, 6, "six, the older call"); lists++;
    std::printf("%s: ok  (%d lists: one chain call == filter by filter, labels, order and bytes)\n", name, lists);
}

// filterAndTransformOnDevice with a cut entry == host apply followed by the transformation
template <typename T>
void run_input_pass(const Scans &s, const char *name)
{
    IMPORT_PGSLAM_TYPES(T)
    TransformationPtr rigid = PM::get().REG(Transformation).create("RigidTransformation");
    DP base = cloud_of<T>(s.rf, 2);
    const int n = (int)base.getNbPoints();
    {   // normals, so that the pass has a row to rotate beside the rows it cuts on
        Matrix up(3, n);
        for (int j = 0; j < n; j++) { up(0, j) = T(0.6); up(1, j) = T(0); up(2, j) = T(0.8); }
        base.addDescriptor("normals", up);
    }
    const int rd0 = base.getDescriptorStartingRow("d0");
    base.descriptors(rd0, 3) = std::numeric_limits<T>::quiet_NaN();
    base.descriptors(rd0, 4) = std::numeric_limits<T>::infinity();
    const std::string box = "- BoundingBoxDataPointsFilter:\n    xMin: -30\n    xMax: 30\n    yMin: -30\n    yMax: 30\n    zMin: -30\n    zMax: 30\n    removeInside: 0\n";
    const std::string rs = "- RandomSamplingDataPointsFilter:\n    prob: 0.5\n    seed: 9\n";
    const std::string lists[] = {box + cut("d0", 1, "0.2") + rs, cut("d0", 0, "-0.1"), cut("d0", 1, "0.25") + "- FixStepSamplingDataPointsFilter:\n    startStep: 3\n" + cut("d0", 0, "-0.25")};
    pgslam_amd::LazyContext ctx;
    const Matrix I = Matrix::Identity(4, 4), P = pose<T>(0.4, -0.2, 1.1, 0.3, 0.05, -0.02);
    for (const std::string &text : lists) {
        for (const Matrix *Tm : {&I, &P}) {
            typename PM::DataPointsFilters on_host = from_yaml<T>(text), on_dev = from_yaml<T>(text), deferred = from_yaml<T>(text);
            DP hst(base), dev(base);
            on_host.apply(hst);
            hst = rigid->compute(hst, *Tm);
            const T *d = nullptr;
            CHECK(PM::filterAndTransformOnDevice(ctx, on_dev, dev, *Tm, &d) && d != nullptr);
            CHECK(hst.getNbPoints() > 0 && (int)hst.getNbPoints() < n && same_cloud<T>(dev, hst));
            // the deferred form has no descriptors to look at: it declines, and the caller takes the pass above
            int kept = -1;
            std::vector<int32_t> dropped;
            CHECK(!PM::filterOnDeviceDeferred(ctx, deferred, base, I, &d, &kept, dropped));
        }
    }
    // a cut whose descriptor is missing, or has two rows: no device spec, nothing is done, the host path throws
    for (const char *missing : {"nothing", "d1"}) {
        typename PM::DataPointsFilters f = from_yaml<T>(box + cut(missing, 1, "0"));
        DP c(base);
        CHECK(!PM::filterAndTransformOnDevice(ctx, f, c, P) && same_cloud<T>(c, base));
        bool threw = false;
        try { f.apply(c); } catch (const typename DP::InvalidField &) { threw = true; }
        CHECK(threw);
    }
    std::printf("%s: ok  (device input pass with a cut == host filters then the transformation, three lists, two transformations)\n", name);
}

static const char *kChainIcpYaml =
    "readingDataPointsFilters:\n  - IdentityDataPointsFilter\n"
    "referenceDataPointsFilters:\n  - SurfaceNormalDataPointsFilter:\n      knn: 10\n      keepEigenValues: 1\n      keepDensities: 1\n"
    "  - ObservationDirectionDataPointsFilter\n  - OrientNormalsDataPointsFilter\n  - IncidenceAngleDataPointsFilter\n"
    "  - CutAtDescriptorThresholdDataPointsFilter:\n      descName: incidenceAngles\n      useLargerThan: 1\n      threshold: %s\n"
    "  - SphericalityDataPointsFilter\n"
    "  - CutAtDescriptorThresholdDataPointsFilter:\n      descName: sphericality\n      useLargerThan: 1\n      threshold: %s\n"
    "  - MaxDensityDataPointsFilter:\n      maxDensity: %s\n      seed: 7\n"
    "matcher:\n  KDTreeMatcher:\n    knn: 1\n    epsilon: 0\n    maxDist: 2.0\n"
    "outlierFilters:\n  - TrimmedDistOutlierFilter:\n      ratio: 0.85\n"
    "errorMinimizer:\n  PointToPlaneErrorMinimizer\n"
    "transformationCheckers:\n  - CounterTransformationChecker:\n      maxIterationCount: 40\n"
    "  - DifferentialTransformationChecker:\n      minDiffRotErr: 0.0001\n      minDiffTransErr: 0.001\n      smoothLength: 3\n"
    "inspector:\n  NullInspector\nlogger:\n  NullLogger\n";

void run_icp(const Scans &s, const char *thr_inc, const char *thr_sph, const char *max_density)
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
        std::vector<char> text(std::strlen(kChainIcpYaml) + std::strlen(thr_inc) + std::strlen(thr_sph) + std::strlen(max_density) + 1);
        std::snprintf(text.data(), text.size(), kChainIcpYaml, thr_inc, thr_sph, max_density);
        std::istringstream ys(text.data());
        icp.loadFromYaml(ys);
        CHECK(icp.referenceDataPointsFilters.size() == 8 && icp.referenceDataPointsFilters.sensorChainRunAt(0) == 8);
        poses[knob] = icp(reading, reference, init);
        CHECK(icp.referenceDataPointsFilters.lastFusedRun() == (knob ? 0u : 8u));
        counts[knob] = icp.getPrefilteredReferencePtsCount();
    }
    unsetenv("PGSLAM_HOST_SENSOR_CHAIN");
    CHECK(counts[0] == counts[1] && counts[0] > 0 && (int)counts[0] < s.n[1]);
    CHECK(std::memcmp(poses[0].data(), poses[1].data(), sizeof(T) * 16) == 0);
    const Matrix d = truth.inverse() * poses[0], d0 = truth.inverse() * init;
    const double dt = std::sqrt((double)(d(0, 3) * d(0, 3) + d(1, 3) * d(1, 3) + d(2, 3) * d(2, 3)));
    const double dt0 = std::sqrt((double)(d0(0, 3) * d0(0, 3) + d0(1, 3) * d0(1, 3) + d0(2, 3) * d0(2, 3)));
    std::printf("ICP<float>, reference chain of eight as one call: %u of %d reference points, the pose equals the filter-by-filter run's bit for bit; "
                "|dt| %.3e m (from %.3e m)\n", counts[0], s.n[1], dt, dt0);
    CHECK(dt < dt0);
}

int main(int argc, char **argv)
{
    if (argc != 7) {
        std::fprintf(stderr, "usage: test_descriptor_filters_gpu <scans> <incidence threshold> <sphericality threshold> <maxDensity> <unstructureness threshold> "
                             "<structureness threshold>\n");
        return 2;
    }
    const Scans s = read_scans(argv[1]);
    run_lists<float>(s, argv[2], argv[3], argv[4], argv[5], argv[6], "descriptor filters<float>");
    run_lists<double>(s, argv[2], argv[3], argv[4], argv[5], argv[6], "descriptor filters<double>");
    run_input_pass<float>(s, "input pass<float>");
    run_input_pass<double>(s, "input pass<double>");
    // (the issue's own thresholds: the medians above leave a sixth of the reference, too little of it for the ICP to be about anything)
    run_icp(s, "1.3", "0.2", argv[4]);
    std::puts("descriptor filters gpu tests ok");
    return 0;
}
