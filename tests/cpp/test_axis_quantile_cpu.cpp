// [EXT] MaxQuantileOnAxisDataPointsFilter and DistanceLimitDataPointsFilter through the C++ drop-in without a device
// (tests/test_axis_quantile_host.py drives it):
//   apply <f32|f64> <in> <out>    the filter, loaded from YAML, applied on the host (inPlaceFilter: axis_quantile_host.hpp) to every
//                                 group of <in> (tests/axis_quantile_ref.py: write_groups) at every ratio: per scene the limit (T),
//                                 k, below, the kept count and the kept indices -- read off a descriptor row that travelled;
//   time <f32|f64> <n>            the host statement's wall time on an n-point cloud, in milliseconds;
//   yaml                          YAML acceptance, defaults and each refusal of both filters, DistanceLimit against Min / MaxDist
//                                 index for index at the limit, both filters in an ICP object's reading chain, the device list
//                                 entry, and the library's exports of what include/pgicp_quantile.h declares.
#include "common.hpp"
#include <chrono>
#include <cstring>
#include <fstream>
#include <limits>

template <typename T>
typename PointMatcher<T>::DataPointsFilters load(const std::string &text)
{
    std::istringstream ys(text);
    return typename PointMatcher<T>::DataPointsFilters(ys);
}

template <typename T>
int apply(const char *fin, const char *fout)
{
    typedef PointMatcher<T> PM;
    namespace aq = pgslam_amd::axis_quantile;
    std::ifstream in(fin, std::ios::binary);
    std::ofstream out(fout, std::ios::binary);
    int32_t groups = 0;
    in.read((char *)&groups, sizeof groups);
    CHECK(in.good() && groups > 0);
    for (int g = 0; g < groups; g++) {
        int32_t n = 0, dim = 0, nr = 0;
        in.read((char *)&n, sizeof n); in.read((char *)&dim, sizeof dim); in.read((char *)&nr, sizeof nr);
        std::vector<double> ratios((size_t)nr);
        in.read((char *)ratios.data(), sizeof(double) * ratios.size());
        std::vector<T> f(4 * (size_t)n);
        in.read((char *)f.data(), sizeof(T) * f.size());
        CHECK(in.good() && n > 0);
        for (double ratio : ratios) {
            typename PM::DataPoints c(typename PM::Matrix(4, n), typename PM::DataPoints::Labels(), typename PM::Matrix(2, n), typename PM::DataPoints::Labels());
            c.descriptorLabels.push_back(typename PM::DataPoints::Label("id", 1));
            c.descriptorLabels.push_back(typename PM::DataPoints::Label("tag", 1));
            for (int i = 0; i < n; i++) {
                for (int r = 0; r < 4; r++) c.features(r, i) = f[4 * (size_t)i + r];
                c.descriptors(0, i) = (T)i;
                c.descriptors(1, i) = (T)(n - i) * (T)0.5;
            }
            char yaml[256];
            std::snprintf(yaml, sizeof yaml, "- MaxQuantileOnAxisDataPointsFilter:\n    dim: %d\n    ratio: %.17g\n", (int)dim, ratio);
            auto filters = load<T>(yaml);
            auto mq = std::dynamic_pointer_cast<typename PM::MaxQuantileOnAxisDataPointsFilter>(filters.at(0));
            CHECK(mq && mq->dim == dim && mq->ratio == (T)ratio);
            filters.apply(c);
            const aq::Result<T> r = aq::select<T>(f.data() + dim, 4, n, (T)ratio);
            const int32_t k = r.k, below = r.below, kept = (int32_t)c.features.cols();
            CHECK(kept == below && kept <= k && c.features.rows() == 4 && (kept == 0 || (int)c.descriptors.cols() == kept));
            out.write((const char *)&r.limit, sizeof(T));
            out.write((const char *)&k, sizeof k); out.write((const char *)&below, sizeof below); out.write((const char *)&kept, sizeof kept);
            int32_t last = -1;
            for (int o = 0; o < kept; o++) {
                const int32_t i = (int32_t)c.descriptors(0, o);
                CHECK(i > last && i < n);                                                          // order is preserved
                last = i;
                CHECK(std::memcmp(&c.features(0, o), &f[4 * (size_t)i], 4 * sizeof(T)) == 0);        // the features travel, bit for bit
                CHECK(c.descriptors(1, o) == (T)(n - i) * (T)0.5);                                 // and every descriptor row
                out.write((const char *)&i, sizeof i);
            }
        }
    }
    CHECK(out.good());
    return 0;
}

template <typename T>
int time_host(int n)
{
    namespace aq = pgslam_amd::axis_quantile;
    Lcg g(11);
    std::vector<T> f(4 * (size_t)n);
    for (auto &v : f) v = (T)(60.0 * (g.next() - 0.5));
    double best = 1e30;
    int below = 0;
    for (int rep = 0; rep < 20; rep++) {
        const auto t0 = std::chrono::steady_clock::now();
        below = aq::select<T>(f.data(), 4, n, (T)0.95).below;
        best = std::min(best, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    }
    std::printf("host_statement_ms %.3f (best of 20, n %d, below %d)\n", best, n, below);
    return 0;
}

template <typename T>
void yaml()
{
    typedef PointMatcher<T> PM;
    typedef typename PM::MaxQuantileOnAxisDataPointsFilter MQ;
    typedef typename PM::DistLimitDataPointsFilter DL;
    auto message = [&](const std::string &text) {
        try { load<T>(text); } catch (const std::runtime_error &e) { return std::string(e.what()); }
        return std::string();
    };
    auto refused = [&](const std::string &text, const char *what) { return message(text).find(what) != std::string::npos; };
    const std::string head = "- MaxQuantileOnAxisDataPointsFilter:\n";
    {   // dim defaults to 0; the device list entry
        auto f = load<T>(head + "    ratio: 0.7\n");
        auto mq = std::dynamic_pointer_cast<MQ>(f.at(0));
        CHECK(mq && mq->dim == 0 && mq->ratio == (T)0.7);
        auto g = load<T>(head + "    dim: 2\n    ratio: 0.9999999\n");
        auto mg = std::dynamic_pointer_cast<MQ>(g.at(0));
        CHECK(mg && mg->dim == 2 && mg->ratio == (T)0.9999999);
        CHECK(std::dynamic_pointer_cast<MQ>(load<T>(head + "    dim: 1\n    ratio: 1e-7\n").at(0))->dim == 1);
        pgicp_filter spec;
        CHECK(mg->deviceSpec(spec) && spec.type == PGICP_FILTER_MAX_QUANTILE_ON_AXIS && spec.type == 8 && spec.p[0] == 2.0 && spec.p[1] == (double)(T)0.9999999);
        std::vector<pgicp_filter> specs;
        CHECK(g.deviceSpecs(specs) && specs.size() == 1 && specs[0].type == 8);
        MQ direct;                                    // constructed directly: upstream's defaults
        CHECK(direct.dim == 0 && direct.ratio == (T)0.5);
    }
    CHECK(refused(head + "    ratio: 0.5\n    dims: 1\n", "unknown parameter"));
    CHECK(refused(head + "    ratio: 0.5\n    maxDist: 1\n", "unknown parameter"));
    CHECK(refused(head + "    ratio: 0.5\n    dim: 3\n", "dim"));
    CHECK(refused(head + "    ratio: 0.5\n    dim: -1\n", "dim"));
    CHECK(refused(head + "    ratio: 0.5\n    dim: 0.5\n", "dim"));
    CHECK(refused(head + "    ratio: 0\n", "ratio"));
    CHECK(refused(head + "    ratio: 1\n", "ratio"));
    CHECK(refused(head + "    ratio: 1e-8\n", "ratio"));
    CHECK(refused(head + "    ratio: 0.99999999\n", "ratio"));
    CHECK(refused(head + "    ratio: -0.5\n", "ratio"));
    CHECK(refused(head + "    ratio: nan\n", "ratio"));
    CHECK(refused(head + "    ratio: inf\n", "ratio"));
    {   // without ratio the entry is refused, and the message names the parameter and what is supported
        for (const std::string &text : {std::string("- MaxQuantileOnAxisDataPointsFilter\n"), head + "    dim: 1\n"}) {
            const std::string msg = message(text);
            CHECK(msg.rfind("DataPointsFilters: unsupported filter 'MaxQuantileOnAxisDataPointsFilter' without ratio", 0) == 0);
            CHECK(msg.find("give ratio") != std::string::npos && msg.find("MaxQuantileOnAxis,") != std::string::npos && msg.find("DistanceLimit,") != std::string::npos);
            const std::string names = PM::DataPointsFilters::supportedNames();
            CHECK(msg.size() >= names.size() && msg.compare(msg.size() - names.size(), names.size(), names) == 0);
        }
        CHECK(message("- NoSuchDataPointsFilter\n").find("MaxQuantileOnAxis") != std::string::npos);
    }
    for (double bad : {0.0, 1.0, 1e-8, -1.0}) {       // the constructor refuses what the loader refuses
        bool threw = false;
        try { MQ f(0, (T)bad); } catch (const std::runtime_error &) { threw = true; }
        CHECK(threw);
    }
    { bool threw = false; try { MQ f(3, (T)0.5); } catch (const std::runtime_error &) { threw = true; } CHECK(threw); }
    {   // an empty cloud: nothing happens
        MQ mq(1, (T)0.5);
        typename PM::DataPoints none(typename PM::Matrix(4, 0), typename PM::DataPoints::Labels());
        mq.inPlaceFilter(none);
        CHECK(none.getNbPoints() == 0);
    }

    // ---- DistanceLimit: the newer spelling of Min / MaxDist
    const std::string dhead = "- DistanceLimitDataPointsFilter:\n";
    {
        auto f = load<T>("- DistanceLimitDataPointsFilter\n");          // the defaults: dim -1, dist 1, removeInside 1 = MinDist{1}
        auto dl = std::dynamic_pointer_cast<DL>(f.at(0));
        CHECK(dl && dl->dim == -1 && dl->limit == (T)1 && !dl->keepInside);
        auto g = load<T>(dhead + "    dim: 2\n    dist: 3.5\n    removeInside: 0\n");
        auto dg = std::dynamic_pointer_cast<DL>(g.at(0));
        CHECK(dg && dg->dim == 2 && dg->limit == (T)3.5 && dg->keepInside);
        pgicp_filter spec;
        CHECK(dg->deviceSpec(spec) && spec.type == PGICP_FILTER_MAX_DIST && spec.p[0] == 3.5 && spec.p[1] == 3.0);
        CHECK(dl->deviceSpec(spec) && spec.type == PGICP_FILTER_MIN_DIST && spec.p[0] == 1.0 && spec.p[1] == 0.0);
    }
    CHECK(refused(dhead + "    dist: 1\n    maxDist: 2\n", "unknown parameter"));
    CHECK(refused(dhead + "    dim: 3\n", "dim"));
    CHECK(refused(dhead + "    dim: -2\n", "dim"));
    CHECK(refused(dhead + "    removeInside: 2\n", "removeInside"));
    {   // index for index what MinDist / MaxDist keep, on a cloud with points exactly on, one ulp below and one ulp above the limit
        const T L = (T)7.25, inf = std::numeric_limits<T>::infinity();
        const T lo = std::nextafter(L, (T)0), hi = std::nextafter(L, inf);
        std::vector<T> xyz;
        for (int a = 0; a < 3; a++)
            for (T v : {L, lo, hi, -L, -lo, -hi, (T)0, std::numeric_limits<T>::quiet_NaN()})
                for (int b = 0; b < 3; b++) xyz.push_back(b == a ? v : (T)0);
        Lcg g(3);
        for (int i = 0; i < 600; i++) {                                   // directions times the limit: norms within a few ulps of it
            double d[3] = {g.next() - 0.5, g.next() - 0.5, g.next() - 0.5};
            const double s = std::sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
            for (int b = 0; b < 3; b++) xyz.push_back((T)(d[b] / s * (double)L));
        }
        const int n = (int)xyz.size() / 3;
        for (int dim = -1; dim <= 2; dim++)
            for (int inside = 0; inside <= 1; inside++)
                for (double dist : {(double)L, -(double)L}) {
                    char ya[256], yb[256];
                    std::snprintf(ya, sizeof ya, "- DistanceLimitDataPointsFilter:\n    dim: %d\n    dist: %.17g\n    removeInside: %d\n", dim, dist, inside ? 0 : 1);
                    std::snprintf(yb, sizeof yb, "- %s:\n    dim: %d\n    %s: %.17g\n", inside ? "MaxDistDataPointsFilter" : "MinDistDataPointsFilter", dim,
                                  inside ? "maxDist" : "minDist", dist);
                    typename PM::DataPoints a = PM::DataPoints::fromXYZ(xyz.data(), n), b = PM::DataPoints::fromXYZ(xyz.data(), n);
                    for (int i = 0; i < n; i++) { a.features(3, i) = (T)i; b.features(3, i) = (T)i; }
                    load<T>(ya).apply(a);
                    load<T>(yb).apply(b);
                    CHECK(a.getNbPoints() == b.getNbPoints() && a.getNbPoints() > 0 && (int)a.getNbPoints() < n);
                    for (int o = 0; o < (int)a.getNbPoints(); o++) CHECK(a.features(3, o) == b.features(3, o));
                    if (dist > 0 && dim <= 0) {
                        // points 0, 1, 2 = (L, 0, 0), (lo, 0, 0), (hi, 0, 0), by x or by radius: on the limit dropped either way,
                        // one ulp off it kept on the right side only
                        bool has[3] = {false, false, false};
                        for (int o = 0; o < (int)a.getNbPoints(); o++) if (a.features(3, o) < (T)3) has[(int)a.features(3, o)] = true;
                        CHECK(!has[0] && has[1] == (inside == 1) && has[2] == (inside == 0));
                    }
                }
    }
    {   // both filters in an ICP object's reading chain
        typename PM::ICP icp;
        std::istringstream in(std::string("readingDataPointsFilters:\n  - DistanceLimitDataPointsFilter:\n      dist: 40\n      removeInside: 0\n"
                                          "  - MaxQuantileOnAxisDataPointsFilter:\n      dim: 2\n      ratio: 0.95\n") + kIcpYamlTail);
        icp.loadFromYaml(in);
        CHECK(icp.readingDataPointsFilters.size() == 2);
        CHECK(std::dynamic_pointer_cast<DL>(icp.readingDataPointsFilters.at(0)) && std::dynamic_pointer_cast<MQ>(icp.readingDataPointsFilters.at(1)));
        std::vector<pgicp_filter> specs;
        CHECK(icp.readingDataPointsFilters.deviceSpecs(specs) && specs.size() == 2 && specs[0].type == PGICP_FILTER_MAX_DIST && specs[1].type == 8);
    }
}

int main(int argc, char **argv)
{
    const bool f32 = argc > 2 && std::strcmp(argv[2], "f32") == 0;
    if (argc == 5 && std::strcmp(argv[1], "apply") == 0) return f32 ? apply<float>(argv[3], argv[4]) : apply<double>(argv[3], argv[4]);
    if (argc == 4 && std::strcmp(argv[1], "time") == 0) return f32 ? time_host<float>(std::atoi(argv[3])) : time_host<double>(std::atoi(argv[3]));
    if (argc == 2 && std::strcmp(argv[1], "yaml") == 0) {
        yaml<float>();
        yaml<double>();
        // the library exports what the header declares: the two addresses resolve at link time, and a call without a context is
        // refused as a bad argument
        float lf = 0; double ld = 0; int k = -1, below = -1;
        CHECK(pgicp_axis_quantile_f32(nullptr, nullptr, 3, 0, PGICP_HOST, 0, 0.5, &lf, &k, &below) == PGICP_ERR_ARG);
        CHECK(pgicp_axis_quantile_f64(nullptr, nullptr, 3, 0, PGICP_HOST, 0, 0.5, &ld, &k, &below) == PGICP_ERR_ARG);
        std::puts("axis quantile cpu tests ok");
        return 0;
    }
    std::fprintf(stderr, "usage: test_axis_quantile_cpu apply <f32|f64> <in> <out> | time <f32|f64> <n> | yaml\n");
    return 2;
}
