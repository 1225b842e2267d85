// [EXT] IncidenceAngle, Sphericality and CutAtDescriptorThreshold without a device (tests/test_descriptor_filters_host.py drives it):
//   test_descriptor_filters_cpu host f32|f64 <in> <out>: the host filters that call include/pgslam_amd/descriptor_filters_host.hpp on a
//     cloud that carries the descriptors of <in>: int32 n, keepUnstructureness, keepStructureness, useLargerThan; double threshold; then
//     n normals (3), n observation directions (3), n eigenvalue triples (3) and n values to cut (1), of T.  <out>: n incidence angles, n
//     sphericalities, n unstructurenesses (when kept), n structurenesses (when kept); then int32 kept and the kept points' input
//     indices (int32) as CutAtDescriptorThreshold leaves them.  The same functions are the device kernels'.
//   test_descriptor_filters_cpu acos <in> <out>: int32 n, n doubles -> n doubles, det_acos of each.
//   test_descriptor_filters_cpu yaml: the YAML keys, defaults and refusals, the labels and their order, the errors on a missing or
//     misshapen descriptor, supportedNames(), which lists form a sensor-chain run, and the device spec of a cut.
#include "common.hpp"
#include <cstring>
#include <fstream>
#include <sstream>

template <typename T>
int run_host(const char *fin, const char *fout)
{
    typedef PointMatcher<T> PM;
    typedef typename PM::DataPoints DP;
    typedef typename PM::Matrix Matrix;
    std::ifstream in(fin, std::ios::binary);
    int32_t hdr[4];
    double thr;
    in.read((char *)hdr, sizeof hdr);
    in.read((char *)&thr, sizeof thr);
    const int n = hdr[0];
    std::vector<T> buf(10 * (size_t)n);
    in.read((char *)buf.data(), sizeof(T) * buf.size());
    CHECK(in.good() && n > 0);
    std::vector<T> xyz(3 * (size_t)n);
    for (int i = 0; i < n; i++) xyz[3 * (size_t)i] = (T)i;              // (x carries the input index through the cut)
    DP c = DP::fromXYZ(xyz.data(), n);
    Matrix nrm(3, n), obs(3, n), eig(3, n), val(1, n);
    for (int i = 0; i < n; i++) {
        for (int a = 0; a < 3; a++) { nrm(a, i) = buf[3 * (size_t)i + a]; obs(a, i) = buf[3 * (size_t)(n + i) + a]; eig(a, i) = buf[3 * (size_t)(2 * n + i) + a]; }
        val(0, i) = buf[9 * (size_t)n + i];
    }
    c.addDescriptor("normals", nrm);
    c.addDescriptor("observationDirections", obs);
    c.addDescriptor("eigValues", eig);
    c.addDescriptor("cutMe", val);
    typename PM::DataPointsFilters f;
    f.push_back(std::make_shared<typename PM::IncidenceAngleDataPointsFilter>());
    f.push_back(std::make_shared<typename PM::SphericalityDataPointsFilter>(hdr[1] != 0, hdr[2] != 0));
    CHECK(f.sensorChainRunAt(0, &c) == 0);                    // no SurfaceNormal: not a run
    f.apply(c);
    CHECK(f.lastFusedRun() == 0 && (int)c.getNbPoints() == n);
    std::vector<std::string> want = {"normals", "observationDirections", "eigValues", "cutMe", "incidenceAngles", "sphericality"};
    if (hdr[1]) want.push_back("unstructureness");
    if (hdr[2]) want.push_back("structureness");
    CHECK(c.descriptorLabels.size() == want.size());
    for (size_t k = 0; k < want.size(); k++) CHECK(c.descriptorLabels[k].text == want[k] && c.descriptorLabels[k].span == (k < 3 ? 3u : 1u));
    std::ofstream out(fout, std::ios::binary);
    for (size_t k = 4; k < want.size(); k++) {
        const int r = c.getDescriptorStartingRow(want[k]);
        for (int i = 0; i < n; i++) { const T v = c.descriptors(r, i); out.write((const char *)&v, sizeof v); }
    }
    // a second application reuses the rows (setDescriptor), it does not append
    f.apply(c);
    CHECK(c.descriptorLabels.size() == want.size());
    typename PM::CutAtDescriptorThresholdDataPointsFilter cut("cutMe", hdr[3] != 0, (T)thr);
    const int rows_before = (int)c.descriptors.rows();
    cut.inPlaceFilter(c);
    CHECK((int)c.descriptors.rows() == rows_before && c.descriptorLabels.size() == want.size());
    const int32_t kept = (int32_t)c.getNbPoints();
    out.write((const char *)&kept, sizeof kept);
    const int rv = c.getDescriptorStartingRow("cutMe");
    for (int i = 0; i < kept; i++) {
        const int32_t j = (int32_t)c.features(0, i);
        out.write((const char *)&j, sizeof j);
        // the descriptors travelled with the point
        CHECK(std::memcmp(&c.descriptors(rv, i), &buf[9 * (size_t)n + j], sizeof(T)) == 0 && std::memcmp(&c.descriptors(0, i), &buf[3 * (size_t)j], sizeof(T)) == 0);
    }
    return out.good() ? 0 : 1;
}

int run_acos(const char *fin, const char *fout)
{
    std::ifstream in(fin, std::ios::binary);
    int32_t n = 0;
    in.read((char *)&n, sizeof n);
    std::vector<double> v((size_t)n);
    in.read((char *)v.data(), sizeof(double) * v.size());
    CHECK(in.good());
    for (auto &x : v) x = pgslam_amd::descriptor_filters::det_acos(x);
    std::ofstream out(fout, std::ios::binary);
    out.write((const char *)v.data(), sizeof(double) * v.size());
    return out.good() ? 0 : 1;
}

template <typename T>
typename PointMatcher<T>::DataPointsFilters from_yaml(const std::string &text)
{
    std::istringstream in(text);
    return typename PointMatcher<T>::DataPointsFilters(in);
}
template <typename T>
bool refused(const std::string &text, const char *needle)
{
    try { from_yaml<T>(text); } catch (const std::runtime_error &e) { return std::strstr(e.what(), needle) != nullptr; }
    return false;
}
template <typename E, typename F>
bool throws(F f, const char *needle)
{
    try { f(); } catch (const E &e) { return std::strstr(e.what(), needle) != nullptr; }
    return false;
}

static const char *kSN = "- SurfaceNormalDataPointsFilter:\n    knn: 10\n    keepEigenValues: 1\n    keepDensities: 1\n";
static const char *kSNplain = "- SurfaceNormalDataPointsFilter:\n    knn: 10\n";
static const char *kObs = "- ObservationDirectionDataPointsFilter\n";
static const char *kOrient = "- OrientNormalsDataPointsFilter\n";
static const char *kInc = "- IncidenceAngleDataPointsFilter\n";
static const char *kSph = "- SphericalityDataPointsFilter\n";
static const char *kSphAll = "- SphericalityDataPointsFilter:\n    keepUnstructureness: 1\n    keepStructureness: 1\n";
static const char *kMaxDens = "- MaxDensityDataPointsFilter:\n    maxDensity: 50\n";
static const char *kShadow = "- ShadowDataPointsFilter:\n    eps: 0.2\n";
static const char *kNoise = "- SimpleSensorNoiseDataPointsFilter\n";
static const char *kBox = "- BoundingBoxDataPointsFilter:\n    xMin: -1\n    xMax: 1\n";
static std::string cut(const std::string &name, int larger = 1, const char *thr = "1.3")
{
    return "- CutAtDescriptorThresholdDataPointsFilter:\n    descName: " + name + "\n    useLargerThan: " + std::to_string(larger) + "\n    threshold: " + thr + "\n";
}

template <typename T>
void yaml_and_runs(const char *name)
{
    typedef PointMatcher<T> PM;
    typedef typename PM::DataPoints DP;
    typedef typename PM::Matrix Matrix;
    typedef std::vector<size_t> V;
    const std::string sn(kSN), snp(kSNplain), obs(kObs), orient(kOrient), inc(kInc), sph(kSph), sphall(kSphAll), md(kMaxDens), shadow(kShadow), noise(kNoise), box(kBox);
    // keys and defaults
    {
        auto f = from_yaml<T>(inc + sph + sphall + "- CutAtDescriptorThresholdDataPointsFilter:\n    descName: densities\n    threshold: 0.25\n" + cut("sphericality", 0, "-2"));
        CHECK(f.size() == 5 && dynamic_cast<typename PM::IncidenceAngleDataPointsFilter *>(f[0].get()));
        auto *s0 = dynamic_cast<typename PM::SphericalityDataPointsFilter *>(f[1].get()), *s1 = dynamic_cast<typename PM::SphericalityDataPointsFilter *>(f[2].get());
        CHECK(s0 && !s0->keepUnstructureness && !s0->keepStructureness && s1 && s1->keepUnstructureness && s1->keepStructureness);
        auto *c0 = dynamic_cast<typename PM::CutAtDescriptorThresholdDataPointsFilter *>(f[3].get()), *c1 = dynamic_cast<typename PM::CutAtDescriptorThresholdDataPointsFilter *>(f[4].get());
        CHECK(c0 && c0->descName == "densities" && c0->useLargerThan && c0->threshold == T(0.25));
        CHECK(c1 && c1->descName == "sphericality" && !c1->useLargerThan && c1->threshold == T(-2));
    }
    // refusals: unknown parameters, a cut without its name or its threshold, flags that are not 0 or 1
    CHECK(refused<T>("- IncidenceAngleDataPointsFilter:\n    knn: 3\n", "unknown parameter knn"));
    CHECK(refused<T>("- SphericalityDataPointsFilter:\n    keepSphericality: 1\n", "unknown parameter keepSphericality"));
    CHECK(refused<T>("- SphericalityDataPointsFilter:\n    keepStructureness: 2\n", "must be 0 or 1"));
    CHECK(refused<T>("- CutAtDescriptorThresholdDataPointsFilter:\n    descName: densities\n", "parameter threshold must be given"));
    CHECK(refused<T>("- CutAtDescriptorThresholdDataPointsFilter:\n    threshold: 1\n", "parameter descName must be given"));
    CHECK(refused<T>("- CutAtDescriptorThresholdDataPointsFilter\n", "parameter descName must be given"));
    CHECK(refused<T>(cut("densities") + "    dim: 0\n", "unknown parameter dim"));
    CHECK(refused<T>(cut("densities", 2), "useLargerThan must be 0 or 1"));
    for (const char *n3 : {"IncidenceAngle", "Sphericality", "CutAtDescriptorThreshold"}) CHECK(std::strstr(PM::DataPointsFilters::supportedNames().c_str(), n3));
    CHECK(refused<T>("- RemoveSensorBiasDataPointsFilter\n", "CutAtDescriptorThreshold"));
    // a missing or misshapen descriptor: DataPoints::InvalidField
    {
        typedef typename DP::InvalidField Bad;
        DP c = make_corner<T>(20, 3);                     // carries normals only
        const int n = (int)c.getNbPoints();
        typename PM::IncidenceAngleDataPointsFilter fi;
        typename PM::SphericalityDataPointsFilter fs;
        typename PM::CutAtDescriptorThresholdDataPointsFilter fc("densities", true, T(1));
        CHECK(throws<Bad>([&] { fi.inPlaceFilter(c); }, "cannot find observationDirections in descriptors"));
        CHECK(throws<Bad>([&] { fs.inPlaceFilter(c); }, "cannot find eigValues in descriptors"));
        CHECK(throws<Bad>([&] { fc.inPlaceFilter(c); }, "cannot find densities in descriptors"));
        DP d = DP::fromXYZ(c.features.data(), 0);
        d.features = c.features;
        CHECK(throws<Bad>([&] { fi.inPlaceFilter(d); }, "cannot find normals in descriptors"));
        c.addDescriptor("observationDirections", Matrix(2, n));
        c.addDescriptor("eigValues", Matrix(2, n));
        c.addDescriptor("densities", Matrix(2, n));
        CHECK(throws<Bad>([&] { fi.inPlaceFilter(c); }, "observationDirections must have 3 rows"));
        CHECK(throws<Bad>([&] { fs.inPlaceFilter(c); }, "eigValues must have 3 rows"));
        CHECK(throws<Bad>([&] { fc.inPlaceFilter(c); }, "densities must have 1 row"));
        CHECK(throws<std::runtime_error>([&] { fc.inPlaceFilter(c); }, "densities"));           // (an InvalidField is a runtime_error)
        // the device spec of a cut needs a one-row descriptor of its name in the cloud; its row is the cloud's
        pgicp_filter spec;
        CHECK(!fc.deviceSpec(spec, c) && !fc.deviceSpec(spec));
        typename PM::CutAtDescriptorThresholdDataPointsFilter fn("noise", false, T(0.5));
        CHECK(!fn.deviceSpec(spec, c));
        c.addDescriptor("noise", Matrix(1, n));
        CHECK(fn.deviceSpec(spec, c) && spec.type == PGICP_FILTER_CUT_AT_DESCRIPTOR && spec.p[0] == 9.0 && spec.p[1] == 0.0 && spec.p[2] == 0.5);
        typename PM::DataPointsFilters list = from_yaml<T>(box + cut("noise") + "- RandomSamplingDataPointsFilter:\n    prob: 0.5\n");
        std::vector<pgicp_filter> specs;
        CHECK(!list.deviceSpecs(specs) && list.deviceSpecs(specs, &c) && specs.size() == 3 && specs[1].type == PGICP_FILTER_CUT_AT_DESCRIPTOR && specs[1].p[0] == 9.0);
        CHECK(!list.deviceSpecs(specs, &d));
    }
    // run detection
    auto runs = [](const typename PM::DataPointsFilters &f, const DP *c = nullptr) { V r; for (size_t k = 0; k < f.size(); k++) r.push_back(f.sensorChainRunAt(k, c)); return r; };
    // the issue's list: one run of eight
    CHECK(runs(from_yaml<T>(sn + obs + orient + inc + cut("incidenceAngles") + sph + cut("sphericality", 1, "0.2") + md)) == (V{8, 0, 0, 0, 0, 0, 0, 0}));
    // each of the three alone behind the head makes a run
    CHECK(runs(from_yaml<T>(sn + obs + inc)) == (V{3, 0, 0}));
    CHECK(runs(from_yaml<T>(sn + sph)) == (V{2, 0}));
    CHECK(runs(from_yaml<T>(sn + cut("densities"))) == (V{2, 0}));
    // IncidenceAngle needs the run's ObservationDirection before it and keepNormals; Sphericality keepEigenValues
    CHECK(runs(from_yaml<T>(sn + inc + obs)) == (V{0, 0, 0}));
    CHECK(runs(from_yaml<T>(snp + obs + sph)) == (V{2, 0, 0}));
    CHECK(runs(from_yaml<T>("- SurfaceNormalDataPointsFilter:\n    knn: 10\n    keepNormals: 0\n    keepEigenValues: 1\n" + obs + inc)) == (V{2, 0, 0}));
    // a cut's name: a row the run has made BY THEN, or a one-row descriptor of the cloud; never ahead of the head
    CHECK(runs(from_yaml<T>(sn + cut("sphericality") + sph)) == (V{0, 0, 0}));
    CHECK(runs(from_yaml<T>(sn + sph + cut("unstructureness"))) == (V{2, 0, 0}));
    CHECK(runs(from_yaml<T>(sn + sphall + cut("unstructureness") + cut("structureness", 0))) == (V{4, 0, 0, 0}));
    CHECK(runs(from_yaml<T>(snp + obs + cut("densities"))) == (V{2, 0, 0}));
    CHECK(runs(from_yaml<T>(noise + sn + cut("simpleSensorNoise"))) == (V{3, 0, 0}));
    CHECK(runs(from_yaml<T>(noise + cut("simpleSensorNoise") + sn)) == (V{0, 0, 0}));
    {
        DP c = make_corner<T>(20, 3);
        c.addDescriptor("intensity", Matrix(1, (int)c.getNbPoints()));
        c.addDescriptor("color", Matrix(3, (int)c.getNbPoints()));
        CHECK(runs(from_yaml<T>(sn + cut("intensity")), &c) == (V{2, 0}) && runs(from_yaml<T>(sn + cut("intensity"))) == (V{0, 0}));
        CHECK(runs(from_yaml<T>(sn + cut("color")), &c) == (V{0, 0}) && runs(from_yaml<T>(sn + cut("nothing")), &c) == (V{0, 0}));
    }
    // four cuts at the most; a type twice; a BoundingBox breaks the run
    CHECK(runs(from_yaml<T>(sn + cut("densities") + cut("densities", 0) + cut("densities") + cut("densities", 0) + cut("densities"))) == (V{5, 0, 0, 0, 0, 0}));
    CHECK(runs(from_yaml<T>(sn + obs + inc + inc)) == (V{3, 0, 0, 0}));
    CHECK(runs(from_yaml<T>(sn + sph + sph)) == (V{2, 0, 0}));
    CHECK(runs(from_yaml<T>(sn + obs + inc + box + cut("incidenceAngles"))) == (V{3, 0, 0, 0, 0}));
    // the longest list the device call takes: the head and eleven stages
    CHECK(runs(from_yaml<T>(noise + sn + obs + orient + inc + cut("incidenceAngles") + sphall + cut("sphericality") + cut("unstructureness") + shadow + cut("densities") + md))[0] == 12);
    // runs without one of the three are what they were
    CHECK(runs(from_yaml<T>(noise + sn + obs + orient + shadow + md)) == (V{6, 5, 0, 0, 0, 0}) && runs(from_yaml<T>(sn + md)) == (V{0, 0}));
    // nothing fused without a device: the filters run one by one and leave the labels in their order
    if (pgicp_device_count() == 0) {
        typename PM::DataPointsFilters f = from_yaml<T>(obs + inc + cut("incidenceAngles", 1, "1.5"));
        DP c = make_corner<T>(50, 3);
        const unsigned before = c.getNbPoints();
        f.apply(c);
        CHECK(f.lastFusedRun() == 0 && c.descriptorLabels.size() == 3 && c.descriptorLabels[2].text == "incidenceAngles" && c.getNbPoints() <= before);
        const int r = c.getDescriptorStartingRow("incidenceAngles");
        for (unsigned i = 0; i < c.getNbPoints(); i++) CHECK(c.descriptors(r, (int)i) <= T(1.5));
    }
    // the per-point functions at their guards
    {
        namespace df = pgslam_amd::descriptor_filters;
        const T zero[3] = {0, 0, 0}, ex[3] = {1, 0, 0}, mx[3] = {-2, 0, 0}, ey[3] = {0, 3, 0};
        const T half_pi = (T)1.57079632679489655800, pi = (T)3.1415926535897931160;
        CHECK(df::incidence_angle<T>(zero, ex) == half_pi && df::incidence_angle<T>(ex, zero) == half_pi);      // a zero normal, a point at the sensor
        CHECK(df::incidence_angle<T>(ex, ex) == T(0) && df::incidence_angle<T>(ex, mx) == pi && df::incidence_angle<T>(ex, ey) == half_pi);
        CHECK(df::det_acos(1.0000001) == 0.0 && df::det_acos(-1.5) == 3.1415926535897931160 && df::det_acos(0.0) == 1.57079632679489655800);
        CHECK(std::isnan(df::det_acos(std::nan(""))));
        T s, u, t;
        const T e_sorted[3] = {1, 2, 4}, e_mixed[3] = {4, 1, 2}, e_zero[3] = {0, 0, 1}, e_nan[3] = {1, std::numeric_limits<T>::quiet_NaN(), 2};
        const T e_sub[3] = {1, std::numeric_limits<T>::denorm_min(), 2}, e_eq[3] = {2, 2, 2};
        df::sphericality<T>(e_sorted, s, u, t);
        const T u0 = T(1) / T(4), t0 = (T(2) / T(4)) * ((T(2) - T(1)) / std::sqrt(T(1) * T(1) + T(2) * T(2)));
        CHECK(u == u0 && t == t0 && s == u0 - t0);
        T s2, u2, t2;
        df::sphericality<T>(e_mixed, s2, u2, t2);
        CHECK(s2 == s && u2 == u && t2 == t);
        df::sphericality<T>(e_eq, s, u, t);
        CHECK(u == T(1) && t == T(0) && s == T(1));
        for (const T *e : {e_zero, e_nan}) { df::sphericality<T>(e, s, u, t); CHECK(std::isnan(s) && std::isnan(u) && std::isnan(t)); }
        df::sphericality<T>(e_sub, s, u, t);              // sorted: (denorm, 1, 2): e1 and e2 are normal, e0 / e2 is 0 or tiny
        CHECK(!std::isnan(s) && u >= T(0) && u < std::numeric_limits<T>::min());
        const T nan = std::numeric_limits<T>::quiet_NaN(), inf = std::numeric_limits<T>::infinity();
        CHECK(df::cut_keep<T>(T(1), T(1), true) && df::cut_keep<T>(T(1), T(1), false) && !df::cut_keep<T>(nan, T(1), true) && !df::cut_keep<T>(nan, T(1), false));
        CHECK(!df::cut_keep<T>(inf, T(1), true) && df::cut_keep<T>(-inf, T(1), true) && df::cut_keep<T>(inf, T(1), false) && !df::cut_keep<T>(-inf, T(1), false));
        CHECK(!df::cut_keep<T>(T(1), nan, true) && !df::cut_keep<T>(T(1), nan, false));
    }
    std::printf("%s: ok\n", name);
}

int main(int argc, char **argv)
{
    if (argc == 5 && std::strcmp(argv[1], "host") == 0)
        return std::strcmp(argv[2], "f32") == 0 ? run_host<float>(argv[3], argv[4]) : run_host<double>(argv[3], argv[4]);
    if (argc == 4 && std::strcmp(argv[1], "acos") == 0) return run_acos(argv[2], argv[3]);
    if (argc == 2 && std::strcmp(argv[1], "yaml") == 0) {
        yaml_and_runs<float>("descriptor filters<float>");
        yaml_and_runs<double>("descriptor filters<double>");
        std::puts("descriptor filters cpu tests ok");
        return 0;
    }
    std::fprintf(stderr, "usage: test_descriptor_filters_cpu host f32|f64 <in> <out> | acos <in> <out> | yaml\n");
    return 2;
}
