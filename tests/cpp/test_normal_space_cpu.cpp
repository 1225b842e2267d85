// [EXT] NormalSpaceDataPointsFilter through the C++ drop-in without a device (tests/test_cpp_normal_space.py drives it):
//   golden <file>                 the filter's host form, loaded from YAML, on every record of tests/golden/normal_space_small.bin
//                                 (written by tests/normal_space_ref.py) against the recorded picks and buckets;
//   apply <f32|f64> <in> <out>    the host form on the cloud of <in> (n, nbSample, drows as int32; epsilon, seed as double; xyz;
//                                 normals; descriptors, drows a point): per pick the kept index (feature row 3 carries the input
//                                 index), the coordinates, the normal and the descriptor rows, then every pick's bucket from
//                                 normalspace_host.hpp's host_select;
//   time <f32|f64> <in>           the host form's wall time on the cloud of <in>, in milliseconds (tools/bench_normal_space.py);
//   yaml                          YAML acceptance and each refusal, the filter in an ICP object's chain, the clouds it refuses,
//                                 and the library's exports of what include/pgicp_normalspace.h declares.
// With PGSLAM_HOST_INPUT_STAGE=1 the host form is forced; without a device it is taken anyway.
#include "common.hpp"
#include <chrono>
#include <cstring>
#include <fstream>
#include <limits>

template <typename T>
typename PointMatcher<T>::DataPoints make_cloud(const std::vector<T> &xyz, const std::vector<T> &nrm, const std::vector<T> &desc, int n, int drows)
{
    typedef PointMatcher<T> PM;
    typename PM::DataPoints c = PM::DataPoints::fromXYZ(xyz.data(), n, nrm.data());
    for (int i = 0; i < n; i++) c.features(3, i) = (T)i;         // a further feature row: it travels with the pick
    if (drows > 0) {
        typename PM::Matrix d(drows, n);
        for (int i = 0; i < n; i++) for (int r = 0; r < drows; r++) d(r, i) = desc[(size_t)i * drows + r];
        c.addDescriptor("rows", d);
    }
    return c;
}

template <typename T>
std::shared_ptr<typename PointMatcher<T>::NormalSpaceDataPointsFilter> load_filter(typename PointMatcher<T>::DataPointsFilters &filters, int nb, double eps,
                                                                                     double seed)
{
    char yaml[512];
    std::snprintf(yaml, sizeof yaml, "- NormalSpaceDataPointsFilter:\n    nbSample: %d\n    epsilon: %.17g\n    seed: %.0f\n", nb, eps, seed);
    std::istringstream ys(yaml);
    filters = typename PointMatcher<T>::DataPointsFilters(ys);
    auto ns = std::dynamic_pointer_cast<typename PointMatcher<T>::NormalSpaceDataPointsFilter>(filters.at(0));
    CHECK(ns && ns->nbSample == (size_t)nb && ns->epsilon == eps && ns->seed == (unsigned long long)seed);
    return ns;
}

template <typename T>
int apply(const char *fin, const char *fout, bool time_only = false)
{
    typedef PointMatcher<T> PM;
    std::ifstream in(fin, std::ios::binary);
    int n = 0, nb = 0, drows = 0;
    double eps = 0, seed = 0;
    in.read((char *)&n, sizeof n); in.read((char *)&nb, sizeof nb); in.read((char *)&drows, sizeof drows);
    in.read((char *)&eps, sizeof eps); in.read((char *)&seed, sizeof seed);
    std::vector<T> xyz(3 * (size_t)n), nrm(3 * (size_t)n), desc((size_t)drows * n);
    in.read((char *)xyz.data(), sizeof(T) * xyz.size());
    in.read((char *)nrm.data(), sizeof(T) * nrm.size());
    in.read((char *)desc.data(), sizeof(T) * desc.size());
    CHECK(in.good());
    typename PM::DataPoints c = make_cloud<T>(xyz, nrm, desc, n, drows);
    typename PM::DataPointsFilters filters;
    auto ns = load_filter<T>(filters, nb, eps, seed);
    const auto t0 = std::chrono::steady_clock::now();
    filters.apply(c);
    const double ms_taken = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    CHECK(!ns->ranOnDevice());
    const int m = (int)c.features.cols();
    if (time_only) { std::printf("host_form_ms %.3f picks %d\n", ms_taken, m); return 0; }
    CHECK(c.features.rows() == 4 && (int)c.descriptors.rows() == 3 + drows && m == std::min(n, nb));
    std::ofstream out(fout, std::ios::binary);
    out.write((const char *)&m, sizeof m);
    for (int o = 0; o < m; o++) {
        const int32_t i = (int32_t)c.features(3, o);
        out.write((const char *)&i, sizeof i);
        for (int r = 0; r < 3; r++) out.write((const char *)&c.features(r, o), sizeof(T));
        for (int r = 0; r < 3 + drows; r++) out.write((const char *)&c.descriptors(r, o), sizeof(T));
    }
    std::vector<int32_t> kept, bucket;
    CHECK(pgslam_amd::normalspace::host_select<T>(n, [&](int i, int a) { return nrm[3 * (size_t)i + a]; }, nb, eps, (unsigned long long)seed, kept, bucket));
    CHECK((int)bucket.size() == m);
    out.write((const char *)bucket.data(), sizeof(int32_t) * (size_t)m);
    return 0;
}

template <typename T>
void golden_record(std::ifstream &in, int n, int nb, int m, double eps, double seed)
{
    typedef PointMatcher<T> PM;
    std::vector<T> nrm(3 * (size_t)n), xyz(3 * (size_t)n), none;
    std::vector<int32_t> want_kept((size_t)m), want_bucket((size_t)m);
    in.read((char *)nrm.data(), sizeof(T) * nrm.size());
    in.read((char *)want_kept.data(), sizeof(int32_t) * (size_t)m);
    in.read((char *)want_bucket.data(), sizeof(int32_t) * (size_t)m);
    CHECK(in.good());
    for (int i = 0; i < n; i++) for (int a = 0; a < 3; a++) xyz[3 * (size_t)i + a] = (T)(i + 0.25 * a);
    typename PM::DataPoints c = make_cloud<T>(xyz, nrm, none, n, 0);
    typename PM::DataPointsFilters filters;
    auto ns = load_filter<T>(filters, nb, eps, seed);
    filters.apply(c);
    CHECK(!ns->ranOnDevice() && (int)c.features.cols() == m && c.descriptors.rows() == 3);
    std::vector<int32_t> kept, bucket;
    CHECK(pgslam_amd::normalspace::host_select<T>(n, [&](int i, int a) { return nrm[3 * (size_t)i + a]; }, nb, eps, (unsigned long long)seed, kept, bucket));
    CHECK(kept == want_kept && bucket == want_bucket);
    for (int o = 0; o < m; o++) {
        const int i = want_kept[(size_t)o];
        CHECK((int)c.features(3, o) == i);
        for (int a = 0; a < 3; a++) CHECK(c.features(a, o) == xyz[3 * (size_t)i + a] && std::memcmp(&c.descriptors(a, o), &nrm[3 * (size_t)i + a], sizeof(T)) == 0);
    }
}

int golden(const char *path)
{
    std::ifstream in(path, std::ios::binary);
    int records = 0;
    in.read((char *)&records, sizeof records);
    CHECK(in.good() && records > 0);
    for (int r = 0; r < records; r++) {
        int n = 0, nb = 0, f32 = 0, m = 0;
        double eps = 0, seed = 0;
        in.read((char *)&n, sizeof n); in.read((char *)&nb, sizeof nb); in.read((char *)&f32, sizeof f32); in.read((char *)&m, sizeof m);
        in.read((char *)&eps, sizeof eps); in.read((char *)&seed, sizeof seed);
        CHECK(in.good() && m == std::min(n, nb));
        if (f32) golden_record<float>(in, n, nb, m, eps, seed); else golden_record<double>(in, n, nb, m, eps, seed);
    }
    CHECK(in.peek() == std::ifstream::traits_type::eof());
    std::printf("normal space golden ok (%d records)\n", records);
    return 0;
}

template <typename T>
void yaml()
{
    typedef PointMatcher<T> PM;
    typedef typename PM::NormalSpaceDataPointsFilter NS;
    auto load = [](const std::string &text) { std::istringstream ys(text); return typename PM::DataPointsFilters(ys); };
    auto message = [&](const std::string &text) {
        try { load(text); } catch (const std::runtime_error &e) { return std::string(e.what()); }
        return std::string();
    };
    auto refused = [&](const std::string &text, const char *what) { return message(text).find(what) != std::string::npos; };
    const std::string head = "- NormalSpaceDataPointsFilter:\n";
    {   // the defaults of what is not given
        auto f = load(head + "    nbSample: 700\n");
        auto ns = std::dynamic_pointer_cast<NS>(f.at(0));
        CHECK(ns && ns->nbSample == 700 && ns->epsilon == 0.09 && ns->seed == 1);
        NS direct;                                    // constructed directly: upstream's defaults
        CHECK(direct.nbSample == 5000 && direct.epsilon == 0.09 && direct.seed == 1);
        NS one(1);                                    // the constructor takes any nbSample >= 1
        CHECK(one.nbSample == 1);
        pgicp_filter spec;
        CHECK(!ns->deviceSpec(spec));
        std::vector<pgicp_filter> specs;
        CHECK(!f.deviceSpecs(specs));                 // the one-pass device input stage says no to a chain that holds it
    }
    {   // every documented parameter
        auto f = load(head + "    nbSample: 12\n    epsilon: 0.25\n    seed: 77\n");
        auto ns = std::dynamic_pointer_cast<NS>(f.at(0));
        CHECK(ns && ns->nbSample == 12 && ns->epsilon == 0.25 && ns->seed == 77);
        auto g = load(head + "    nbSample: 1\n    epsilon: 3.141592653589793\n    seed: 9007199254740991\n");
        auto ng = std::dynamic_pointer_cast<NS>(g.at(0));
        CHECK(ng && ng->nbSample == 1 && ng->epsilon == 3.141592653589793 && ng->seed == 9007199254740991ULL);
    }
    CHECK(refused(head + "    nbSample: 10\n    nbSamples: 3\n", "unknown parameter"));
    CHECK(refused(head + "    nbSample: 10\n    torqueNorm: 1\n", "unknown parameter"));
    CHECK(refused(head + "    nbSample: 2.5\n", "nbSample"));
    CHECK(refused(head + "    nbSample: 0\n", "nbSample"));
    CHECK(refused(head + "    nbSample: -3\n", "nbSample"));
    CHECK(refused(head + "    nbSample: 10\n    epsilon: 0\n", "epsilon"));
    CHECK(refused(head + "    nbSample: 10\n    epsilon: -0.1\n", "epsilon"));
    CHECK(refused(head + "    nbSample: 10\n    epsilon: 4.0\n", "epsilon"));
    CHECK(refused(head + "    nbSample: 10\n    epsilon: 0.001\n", "epsilon"));
    CHECK(refused(head + "    nbSample: 10\n    epsilon: inf\n", "epsilon"));
    CHECK(refused(head + "    nbSample: 10\n    seed: -1\n", "seed"));
    CHECK(refused(head + "    nbSample: 10\n    seed: 9007199254740992\n", "seed"));
    {   // without nbSample the entry stays refused, and the message says what to give and what is supported
        for (const std::string &text : {std::string("- NormalSpaceDataPointsFilter\n"), head + "    epsilon: 0.09\n"}) {
            const std::string msg = message(text);
            CHECK(msg.rfind("DataPointsFilters: unsupported filter 'NormalSpaceDataPointsFilter' without nbSample", 0) == 0);
            CHECK(msg.find("give nbSample") != std::string::npos && msg.find("OctreeGrid") != std::string::npos && msg.find("NormalSpace,") != std::string::npos);
            const std::string names = PM::DataPointsFilters::supportedNames();
            CHECK(msg.size() >= names.size() && msg.compare(msg.size() - names.size(), names.size(), names) == 0);
        }
        CHECK(message("- NoSuchDataPointsFilter\n").find("NormalSpace") != std::string::npos);
    }
    for (const char *bad : {"0", "4.0", "0.001"}) {   // the constructor refuses what the loader refuses
        bool threw = false;
        try { NS f(10, std::atof(bad)); } catch (const std::runtime_error &) { threw = true; }
        CHECK(threw);
    }
    {   // in an ICP object's reading chain, behind the filter that makes the normals
        typename PM::ICP icp;
        std::istringstream in(std::string("readingDataPointsFilters:\n  - SurfaceNormalDataPointsFilter:\n      knn: 10\n"
                                          "  - NormalSpaceDataPointsFilter:\n      nbSample: 500\n      epsilon: 0.2\n"
                                          "referenceDataPointsFilters:\n  - SurfaceNormalDataPointsFilter:\n      knn: 10\n") + kIcpYamlTail);
        icp.loadFromYaml(in);
        CHECK(icp.readingDataPointsFilters.size() == 2 && icp.referenceDataPointsFilters.size() == 1);
        CHECK(std::dynamic_pointer_cast<NS>(icp.readingDataPointsFilters.at(1)));
    }
    {   // a 2-D cloud and a cloud without normals throw; the no-op leaves the cloud alone; a NaN normal is refused
        NS ns(2);
        typename PM::DataPoints flat(typename PM::Matrix(3, 5), typename PM::DataPoints::Labels(), typename PM::Matrix(3, 5), typename PM::DataPoints::Labels());
        flat.descriptorLabels.push_back(typename PM::DataPoints::Label("normals", 3));
        bool threw = false;
        try { ns.inPlaceFilter(flat); } catch (const std::runtime_error &e) { threw = std::string(e.what()).find("3-D") != std::string::npos; }
        CHECK(threw);
        const T pts[9] = {T(0), T(0), T(0), T(1), T(0), T(2), T(3), T(1), T(2)};
        typename PM::DataPoints bare = PM::DataPoints::fromXYZ(pts, 3);
        threw = false;
        try { ns.inPlaceFilter(bare); } catch (const std::runtime_error &e) { threw = std::string(e.what()).find("normals") != std::string::npos; }
        CHECK(threw && bare.getNbPoints() == 3);
        const T nan = std::numeric_limits<T>::quiet_NaN();
        const T nrm[9] = {T(0), T(0), T(1), T(1), nan, T(0), T(0), T(1), T(0)};
        setenv("PGSLAM_HOST_INPUT_STAGE", "1", 1);
        typename PM::DataPoints bad = PM::DataPoints::fromXYZ(pts, 3, nrm);
        threw = false;
        try { ns.inPlaceFilter(bad); } catch (const std::runtime_error &e) { threw = std::string(e.what()).find("NaN") != std::string::npos; }
        CHECK(threw && bad.getNbPoints() == 3);
        NS all(3);                                    // nbSample >= n: the normals are not read, the cloud stays as it is
        all.inPlaceFilter(bad);
        CHECK(bad.getNbPoints() == 3 && bad.features(0, 1) == T(1) && !all.ranOnDevice());
    }
}

int main(int argc, char **argv)
{
    const bool f32 = argc > 2 && std::strcmp(argv[2], "f32") == 0;
    if (argc == 3 && std::strcmp(argv[1], "golden") == 0) { setenv("PGSLAM_HOST_INPUT_STAGE", "1", 1); return golden(argv[2]); }
    if (argc == 5 && std::strcmp(argv[1], "apply") == 0) return f32 ? apply<float>(argv[3], argv[4]) : apply<double>(argv[3], argv[4]);
    if (argc == 4 && std::strcmp(argv[1], "time") == 0) return f32 ? apply<float>(argv[3], nullptr, true) : apply<double>(argv[3], nullptr, true);
    if (argc == 2 && std::strcmp(argv[1], "yaml") == 0) {
        yaml<float>();
        yaml<double>();
        // the library exports what the header declares: the two addresses resolve at link time, and a call without a context is
        // refused as a bad argument
        int n_out = -1;
        CHECK(pgicp_normal_space_sampling_f32(nullptr, nullptr, 3, nullptr, 3, 0, PGICP_HOST, 1, 0.09, 1, nullptr, 0, nullptr, nullptr, 3, nullptr, nullptr,
                                              nullptr, &n_out) == PGICP_ERR_ARG);
        CHECK(pgicp_normal_space_sampling_f64(nullptr, nullptr, 3, nullptr, 3, 0, PGICP_HOST, 1, 0.09, 1, nullptr, 0, nullptr, nullptr, 3, nullptr, nullptr,
                                              nullptr, &n_out) == PGICP_ERR_ARG);
        std::puts("normal space cpu tests ok");
        return 0;
    }
    std::fprintf(stderr, "usage: test_normal_space_cpu golden <file> | apply <f32|f64> <in> <out> | time <f32|f64> <in> | yaml\n");
    return 2;
}
