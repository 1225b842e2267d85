// [EXT] The sensor filter chain without a device (tests/test_sensor_chain_host.py drives it):
//   test_sensor_chain_cpu host f32|f64 <in> <out>: the host filters that call include/pgslam_amd/sensor_chain_host.hpp -- SimpleSensorNoise,
//     ObservationDirection, OrientNormals, Shadow, in that order -- on a cloud that carries the normals of <in>: int32 n, toward,
//     sensorType; doubles centre[3], eps, gain; n points and n normals of T.  <out>: int32 kept, the kept points (3 a point), their
//     descriptors (7 a point: normals, simpleSensorNoise, observationDirections).  The same functions are the device kernel's.
//   test_sensor_chain_cpu runs: which filter lists form a run of DataPointsFilters (sensorChainRunAt), which do not, and
//     lastFusedRun() == 0 where nothing was fused; the per-point functions on a zero normal and on the origin.
#include "common.hpp"
#include <cstring>
#include <fstream>
#include <sstream>

template <typename T>
int run_host(const char *fin, const char *fout)
{
    typedef PointMatcher<T> PM;
    typedef typename PM::DataPoints DP;
    std::ifstream in(fin, std::ios::binary);
    int32_t hdr[3];
    double prm[5];
    in.read((char *)hdr, sizeof hdr);
    in.read((char *)prm, sizeof prm);
    const int n = hdr[0];
    std::vector<T> xyz(3 * (size_t)n), nrm(3 * (size_t)n);
    in.read((char *)xyz.data(), sizeof(T) * xyz.size());
    in.read((char *)nrm.data(), sizeof(T) * nrm.size());
    CHECK(in.good() && n > 0);
    DP c = DP::fromXYZ(xyz.data(), n, nrm.data());
    typename PM::DataPointsFilters f;
    f.push_back(std::make_shared<typename PM::SimpleSensorNoiseDataPointsFilter>(hdr[2], (T)prm[4]));
    f.push_back(std::make_shared<typename PM::ObservationDirectionDataPointsFilter>((T)prm[0], (T)prm[1], (T)prm[2]));
    f.push_back(std::make_shared<typename PM::OrientNormalsDataPointsFilter>(hdr[1] != 0));
    f.push_back(std::make_shared<typename PM::ShadowDataPointsFilter>((T)prm[3]));
    CHECK(f.sensorChainRunAt(0) == 0);                    // no SurfaceNormal: not a run
    f.apply(c);
    CHECK(f.lastFusedRun() == 0);
    CHECK(c.descriptorLabels.size() == 3 && c.descriptorLabels[0].text == "normals" && c.descriptorLabels[1].text == "simpleSensorNoise" &&
          c.descriptorLabels[2].text == "observationDirections" && c.descriptors.rows() == 7);
    const int32_t kept = (int32_t)c.getNbPoints();
    std::ofstream out(fout, std::ios::binary);
    out.write((const char *)&kept, sizeof kept);
    for (int i = 0; i < kept; i++) for (int a = 0; a < 3; a++) { const T v = c.features(a, i); out.write((const char *)&v, sizeof v); }
    for (int i = 0; i < kept; i++) for (int r = 0; r < 7; r++) { const T v = c.descriptors(r, i); out.write((const char *)&v, sizeof v); }
    return out.good() ? 0 : 1;
}

template <typename T>
typename PointMatcher<T>::DataPointsFilters from_yaml(const std::string &text)
{
    std::istringstream in(text);
    return typename PointMatcher<T>::DataPointsFilters(in);
}

static const char *kSN = "- SurfaceNormalDataPointsFilter:\n    knn: 10\n    keepDensities: 1\n";
static const char *kObs = "- ObservationDirectionDataPointsFilter\n";
static const char *kOrient = "- OrientNormalsDataPointsFilter\n";
static const char *kShadow = "- ShadowDataPointsFilter:\n    eps: 0.2\n";
static const char *kMaxDens = "- MaxDensityDataPointsFilter:\n    maxDensity: 100\n";
static const char *kNoise = "- SimpleSensorNoiseDataPointsFilter\n";
static const char *kBox = "- BoundingBoxDataPointsFilter:\n    xMin: -1\n    xMax: 1\n";

template <typename T>
void run_detection(const char *name)
{
    typedef PointMatcher<T> PM;
    typedef typename PM::SurfaceNormalDataPointsFilter SN;
    const T inf = std::numeric_limits<T>::infinity();
    auto runs = [](const typename PM::DataPointsFilters &f) { std::vector<size_t> r; for (size_t k = 0; k < f.size(); k++) r.push_back(f.sensorChainRunAt(k)); return r; };
    typedef std::vector<size_t> V;
    const std::string sn(kSN), obs(kObs), orient(kOrient), shadow(kShadow), md(kMaxDens), noise(kNoise), box(kBox);
    // the sensor's usual chain: one run of six
    CHECK(runs(from_yaml<T>(noise + sn + obs + orient + shadow + md)) == (V{6, 5, 0, 0, 0, 0}));
    // SurfaceNormal + MaxDensity alone: none of the four host filters, the older pair fusion's
    CHECK(runs(from_yaml<T>(sn + md)) == (V{0, 0}));
    CHECK(runs(from_yaml<T>(sn)) == (V{0}));
    // ObservationDirection and SimpleSensorNoise may lead; nothing else may
    CHECK(runs(from_yaml<T>(obs + noise + sn + shadow)) == (V{4, 3, 2, 0}));
    CHECK(runs(from_yaml<T>(shadow + sn)) == (V{0, 0}));
    CHECK(runs(from_yaml<T>(obs + box + sn + orient)) == (V{0, 0, 0, 0}));
    // a BoundingBox in the middle breaks the run; what stands behind it has no SurfaceNormal
    CHECK(runs(from_yaml<T>(sn + obs + orient + box + shadow + md)) == (V{3, 0, 0, 0, 0, 0}));
    // OrientNormals without the run's ObservationDirection before it ends the run
    CHECK(runs(from_yaml<T>(sn + orient + obs)) == (V{0, 0, 0}));
    CHECK(runs(from_yaml<T>(sn + noise + orient)) == (V{2, 0, 0}));
    // a type twice, a second SurfaceNormal
    CHECK(runs(from_yaml<T>(sn + obs + obs)) == (V{2, 0, 0}));
    CHECK(runs(from_yaml<T>(sn + obs + sn + shadow)) == (V{2, 3, 2, 0}));
    CHECK(runs(from_yaml<T>(sn + shadow + md + shadow)) == (V{3, 0, 0, 0}));
    // rows the head does not keep; an ext output; knn beyond the device's
    CHECK(runs(from_yaml<T>("- SurfaceNormalDataPointsFilter:\n    knn: 10\n    keepNormals: 0\n    keepDensities: 1\n" + obs + shadow)) == (V{2, 0, 0}));
    CHECK(runs(from_yaml<T>("- SurfaceNormalDataPointsFilter:\n    knn: 10\n" + obs + md)) == (V{2, 0, 0}));
    CHECK(runs(from_yaml<T>("- SurfaceNormalDataPointsFilter:\n    knn: 10\n    keepEigenVectors: 1\n" + obs)) == (V{0, 0}));
    {
        typename PM::DataPointsFilters f;
        f.push_back(std::make_shared<SN>(40, inf, true, false, true));
        f.push_back(std::make_shared<typename PM::ObservationDirectionDataPointsFilter>(T(0), T(0), T(0)));
        CHECK(runs(f) == (V{0, 0}));
        typename PM::DataPointsFilters g;
        g.push_back(std::make_shared<SN>(10, inf, true, false, true));
        g.push_back(std::make_shared<typename PM::ShadowDataPointsFilter>(T(0.2)));
        g.push_back(std::make_shared<typename PM::MaxDensityDataPointsFilter>(T(-1), 1));        // parameters the device refuses
        CHECK(runs(g) == (V{2, 0, 0}));
    }
    // nothing fused where there is no device, no run, or no point
    {
        typename PM::DataPointsFilters f = from_yaml<T>(noise + sn + obs);
        CHECK(f.lastFusedRun() == 0 && f.sensorChainRunAt(0) == 3);
        typename PM::DataPoints e;
        e.features = typename PM::Matrix(4, 0);
        f.apply(e);
        CHECK(f.lastFusedRun() == 0 && e.getNbPoints() == 0);
        if (pgicp_device_count() == 0) {
            typename PM::DataPointsFilters h = from_yaml<T>(obs + noise);
            typename PM::DataPoints c = make_corner<T>(50, 3);
            h.apply(c);
            CHECK(h.lastFusedRun() == 0 && c.descriptorExists("observationDirections") && c.descriptorExists("simpleSensorNoise"));
        }
    }
    // the per-point functions at their guards: a zero normal is not normalised (the cosine is 0: dropped for any eps, also 0),
    // nor is the origin; a unit normal along the ray has |cosine| 1 and stays below pi / 2
    {
        namespace sc = pgslam_amd::sensor_chain;
        const T zero[3] = {0, 0, 0}, ex[3] = {1, 0, 0}, p[3] = {3, 0, 0}, q[3] = {0, 4, 0};
        CHECK(!sc::shadow_keep<T>(zero, p, sc::shadow_threshold<T>(T(0))) && !sc::shadow_keep<T>(ex, zero, sc::shadow_threshold<T>(T(0))));
        CHECK(sc::shadow_keep<T>(ex, p, sc::shadow_threshold<T>(T(1.5))) && !sc::shadow_keep<T>(ex, q, sc::shadow_threshold<T>(T(0))));
        CHECK(!sc::orient_flips<T>(zero, p, true) && !sc::orient_flips<T>(zero, p, false));
        CHECK(sc::orient_flips<T>(ex, p, false) && !sc::orient_flips<T>(ex, p, true));
        CHECK(sc::shadow_eps_ok(0.0) && sc::shadow_eps_ok(3.14159265358979323846) && !sc::shadow_eps_ok(-1e-9) && !sc::shadow_eps_ok(3.1416) && !sc::shadow_eps_ok(std::nan("")));
        sc::NoiseModel<T> m;
        CHECK(!sc::noise_model<T>(5, T(1), m) && !sc::noise_model<T>(-1, T(1), m) && sc::noise_model<T>(0, T(2), m));
        CHECK(sc::noise_value<T>(m, zero) == T(2) * T(0.012));
    }
    std::printf("%s: ok\n", name);
}

int main(int argc, char **argv)
{
    if (argc == 5 && std::strcmp(argv[1], "host") == 0)
        return std::strcmp(argv[2], "f32") == 0 ? run_host<float>(argv[3], argv[4]) : run_host<double>(argv[3], argv[4]);
    if (argc == 2 && std::strcmp(argv[1], "runs") == 0) {
        run_detection<float>("sensor chain runs<float>");
        run_detection<double>("sensor chain runs<double>");
        std::puts("sensor chain cpu tests ok");
        return 0;
    }
    std::fprintf(stderr, "usage: test_sensor_chain_cpu host f32|f64 <in> <out> | runs\n");
    return 2;
}
