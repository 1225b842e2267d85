// [EXT] ElipsoidsDataPointsFilter without a device (tests/test_elipsoids_host.py drives it; a stand-alone program, so it can be built
// with -fsanitize=address,undefined to check include/pgslam_amd/elipsoids_host.hpp and the filter's host form):
//   host <f32|f64> <in> <out>     the filter's host form (PGSLAM_HOST_ELIPSOIDS=1 is set here) with every row on every case of <in>:
//                                 int32 cases, then per case int32 n, drows, knn, method, average, double ratio, maxBoxDim, seed,
//                                 minPlanarity, the points (3 a point) and the descriptors (drows a point, labelled d0, d1, ...).
//                                 <out>, per case: int32 kept, int32 descriptor rows, the kept points (3 a point), the descriptors
//                                 (all rows of a point together).  Checked here: the labels and their order, each row alone against
//                                 the filter with all rows, overwrite-when-present, and -- with minPlanarity 0 and only keepNormals --
//                                 SamplingSurfaceNormalDataPointsFilter's host form byte for byte;
//   yaml                          YAML loading of every key, the refusals, the constructors, and the library's exports of what
//                                 include/pgicp_elipsoids.h declares.
#include "common.hpp"
#include <cstring>
#include <fstream>
#include <sstream>

static const char *kNames[8] = {"normals", "densities", "eigValues", "eigVectors", "covariance", "weights", "means", "shapes"};
static const int kSpans[8] = {3, 1, 3, 9, 9, 1, 3, 3};

template <typename T>
bool same_bytes(const typename PointMatcher<T>::DataPoints &a, const typename PointMatcher<T>::DataPoints &b)
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

template <typename T>
int host(const char *fin, const char *fout)
{
    typedef PointMatcher<T> PM;
    typedef typename PM::ElipsoidsDataPointsFilter EL;
    typedef typename PM::SamplingSurfaceNormalDataPointsFilter SSN;
    setenv("PGSLAM_HOST_ELIPSOIDS", "1", 1);
    setenv("PGSLAM_HOST_SAMPLING_NORMALS", "1", 1);
    std::ifstream in(fin, std::ios::binary);
    std::ofstream out(fout, std::ios::binary);
    int cases = 0;
    in.read((char *)&cases, sizeof cases);
    for (int cs = 0; cs < cases; cs++) {
        int h[5];
        double p[4];
        in.read((char *)h, sizeof h); in.read((char *)p, sizeof p);
        const int n = h[0], drows = h[1], knn = h[2], method = h[3], average = h[4];
        const T ratio = (T)p[0], box = (T)p[1], minp = (T)p[3];
        const unsigned long long seed = (unsigned long long)p[2];
        std::vector<T> xyz(3 * (size_t)n), desc((size_t)drows * n);
        in.read((char *)xyz.data(), sizeof(T) * xyz.size());
        in.read((char *)desc.data(), sizeof(T) * desc.size());
        CHECK(in.good());
        auto make = [&]() {
            auto cloud = PM::DataPoints::fromXYZ(xyz.data(), n, nullptr);
            for (int r = 0; r < drows; r++) {
                typename PM::Matrix d(1, n);
                for (int j = 0; j < n; j++) d(0, j) = desc[(size_t)j * drows + r];
                cloud.addDescriptor("d" + std::to_string(r), d);
            }
            return cloud;
        };
        EL all(ratio, knn, method, box, minp, average != 0, true, true, true, true, true, true, true, true, seed);
        auto c = make();
        all.inPlaceFilter(c);
        CHECK(!all.ranOnDevice());
        // the statement's order after the cloud's own rows
        CHECK((int)c.descriptorLabels.size() == drows + 8 && (int)c.descriptors.rows() == drows + 32);
        for (int k = 0, row = drows; k < 8; row += kSpans[k], k++) {
            CHECK(c.descriptorLabels[drows + k].text == kNames[k] && (int)c.descriptorLabels[drows + k].span == kSpans[k]);
            CHECK(c.getDescriptorStartingRow(kNames[k]) == row);
        }
        // only keepNormals: the same points and the same first rows, one new label ...
        EL plain(ratio, knn, method, box, minp, average != 0, true, false, false, false, false, false, false, false, seed);
        auto cp = make();
        plain.inPlaceFilter(cp);
        CHECK(cp.features.cols() == c.features.cols() && (int)cp.descriptors.rows() == drows + 3 && (int)cp.descriptorLabels.size() == drows + 1);
        for (int j = 0; j < (int)c.features.cols(); j++) {
            for (int r = 0; r < (int)c.features.rows(); r++) CHECK(std::memcmp(&cp.features(r, j), &c.features(r, j), sizeof(T)) == 0);
            for (int r = 0; r < drows + 3; r++) CHECK(std::memcmp(&cp.descriptors(r, j), &c.descriptors(r, j), sizeof(T)) == 0);
        }
        // ... and with minPlanarity 0 it is SamplingSurfaceNormalDataPointsFilter's host form byte for byte
        if (p[3] == 0.0) {
            SSN ssn(ratio, knn, method, box, average != 0, true, seed);
            auto cs7 = make();
            ssn.inPlaceFilter(cs7);
            CHECK(!ssn.ranOnDevice());
            CHECK(same_bytes<T>(cs7, cp));
        }
        // without keepNormals and with nothing else: no label at all, the same points
        {
            EL none(ratio, knn, method, box, minp, average != 0, false, false, false, false, false, false, false, false, seed);
            auto cn = make();
            none.inPlaceFilter(cn);
            CHECK(cn.features.cols() == c.features.cols() && (int)cn.descriptorLabels.size() == drows);
        }
        // each row alone equals its rows of the filter with all rows; rows that exist already are overwritten in place
        for (int one = 0; one < 8; one++) {
            EL f(ratio, knn, method, box, minp, average != 0, one == 0, one == 1, one == 2, one == 3, one == 4, one == 5, one == 6, one == 7, seed);
            auto c1 = make();
            f.inPlaceFilter(c1);
            const char *name = kNames[one];
            CHECK((int)c1.descriptorLabels.size() == drows + 1 && c1.descriptorLabels[drows].text == name && (int)c1.descriptorLabels[drows].span == kSpans[one]);
            CHECK(c1.features.cols() == c.features.cols());
            const int r1 = c1.getDescriptorStartingRow(name), ra = c.getDescriptorStartingRow(name);
            for (int j = 0; j < (int)c.features.cols(); j++)
                for (int r = 0; r < kSpans[one]; r++) CHECK(std::memcmp(&c1.descriptors(r1 + r, j), &c.descriptors(ra + r, j), sizeof(T)) == 0);
            if (drows == 0 || !(method == 1 && average)) {
                // (with averaging the second pass would average the first pass's rows too: the other descriptors would differ)
                const int rows_before = (int)c1.descriptors.rows(), kept_before = (int)c1.features.cols();
                EL again(T(0.999), knn, 1, std::numeric_limits<T>::infinity(), T(0), false, one == 0, one == 1, one == 2, one == 3, one == 4, one == 5,
                         one == 6, one == 7, 1);
                again.inPlaceFilter(c1);
                CHECK((int)c1.descriptors.rows() == rows_before && (int)c1.descriptorLabels.size() == drows + 1);
                CHECK((int)c1.features.cols() <= kept_before);
            }
        }
        const int kept = (int)c.features.cols(), dr = (int)c.descriptors.rows();
        out.write((const char *)&kept, sizeof kept); out.write((const char *)&dr, sizeof dr);
        for (int j = 0; j < kept; j++) for (int r = 0; r < 3; r++) out.write((const char *)&c.features(r, j), sizeof(T));
        for (int j = 0; j < kept; j++) for (int r = 0; r < dr; r++) out.write((const char *)&c.descriptors(r, j), sizeof(T));
    }
    return out.good() ? 0 : 1;
}

template <typename T>
void yaml()
{
    typedef PointMatcher<T> PM;
    typedef typename PM::ElipsoidsDataPointsFilter EL;
    const T inf = std::numeric_limits<T>::infinity();
    auto load = [](const std::string &text) { std::istringstream ys(text); return typename PM::DataPointsFilters(ys); };
    auto message = [&](const std::string &text) {
        try { load(text); } catch (const std::runtime_error &e) { return std::string(e.what()); }
        return std::string();
    };
    const std::string name = "ElipsoidsDataPointsFilter";
    const std::string head = "- ElipsoidsDataPointsFilter:\n    keepNormals: 1\n";
    {   // the defaults
        auto s = std::dynamic_pointer_cast<EL>(load(head).at(0));
        CHECK(s && s->ratio == T(0.5) && s->knn == 7 && s->samplingMethod == 0 && s->maxBoxDim == inf && s->minPlanarity == T(0) &&
              s->averageExistingDescriptors && s->keepNormals && !s->keepDensities && !s->keepEigenValues && !s->keepEigenVectors &&
              !s->keepCovariances && !s->keepWeights && !s->keepMeans && !s->keepShapes && s->seed == 1 && s->maxTimeWindow == inf);
    }
    {   // every key loads
        auto s = std::dynamic_pointer_cast<EL>(load("- ElipsoidsDataPointsFilter:\n    ratio: 0.25\n    knn: 9\n    samplingMethod: 1\n    maxBoxDim: 2.5\n"
                                                    "    minPlanarity: 0.125\n    maxTimeWindow: inf\n    averageExistingDescriptors: 0\n    keepNormals: 0\n"
                                                    "    keepDensities: 1\n    keepEigenValues: 1\n    keepEigenVectors: 1\n    keepCovariances: 1\n"
                                                    "    keepWeights: 1\n    keepMeans: 1\n    keepShapes: 1\n    seed: 23\n").at(0));
        CHECK(s && s->ratio == T(0.25) && s->knn == 9 && s->samplingMethod == 1 && s->maxBoxDim == T(2.5) && s->minPlanarity == T(0.125) &&
              !s->averageExistingDescriptors && !s->keepNormals && s->keepDensities && s->keepEigenValues && s->keepEigenVectors &&
              s->keepCovariances && s->keepWeights && s->keepMeans && s->keepShapes && s->seed == 23 && s->maxTimeWindow == inf);
    }
    {   // each keep flag alone
        const char *keys[7] = {"keepDensities", "keepEigenValues", "keepEigenVectors", "keepCovariances", "keepWeights", "keepMeans", "keepShapes"};
        for (int k = 0; k < 7; k++) {
            auto s = std::dynamic_pointer_cast<EL>(load(head + "    " + keys[k] + ": 1\n").at(0));
            const bool got[7] = {s->keepDensities, s->keepEigenValues, s->keepEigenVectors, s->keepCovariances, s->keepWeights, s->keepMeans, s->keepShapes};
            for (int j = 0; j < 7; j++) CHECK(got[j] == (j == k));
        }
        CHECK(std::dynamic_pointer_cast<EL>(load(head + "    minPlanarity: 0\n").at(0))->minPlanarity == T(0));
        CHECK(std::dynamic_pointer_cast<EL>(load(head + "    minPlanarity: 1\n").at(0))->minPlanarity == T(1));
    }
    // the refusals, each by the filter's name
    auto refused = [&](const std::string &text, const char *word) {
        const std::string msg = message(text);
        if (!(msg.find(name) == 0 && msg.find(word) != std::string::npos)) std::fprintf(stderr, "not refused as expected: '%s' -> '%s'\n", text.c_str(), msg.c_str());
        CHECK(msg.find(name) == 0 && msg.find(word) != std::string::npos);
    };
    refused("- ElipsoidsDataPointsFilter\n", "keepNormals");                                             // missing keepNormals
    refused("- ElipsoidsDataPointsFilter:\n    knn: 9\n", "keepNormals");
    refused(head + "    maxTimeWindow: 0.5\n", "maxTimeWindow");
    refused(head + "    maxTimeWindow: 0\n", "maxTimeWindow");
    refused(head + "    minPlanarity: -0.1\n", "minPlanarity");
    refused(head + "    minPlanarity: 1.5\n", "minPlanarity");
    refused(head + "    minPlanarity: nan\n", "minPlanarity");
    refused(head + "    keepIndices: 1\n", "unknown parameter keepIndices");
    refused(head + "    keepIndices: 0\n", "unknown parameter keepIndices");
    refused(head + "    knn: 2\n", "knn");
    refused(head + "    ratio: 1.5\n", "ratio");
    refused(head + "    ratio: 0\n", "ratio");
    refused(head + "    samplingMethod: 2\n", "samplingMethod");
    refused(head + "    noSuchParameter: 1\n", "unknown parameter noSuchParameter");
    {   // the list of supported names carries it; an unknown filter's message shows the list
        CHECK(PM::DataPointsFilters::supportedNames().find("Elipsoids") != std::string::npos);
        CHECK(message("- NoSuchDataPointsFilter\n").find("Elipsoids") != std::string::npos);
    }
    {   // constructors
        EL none;
        CHECK(none.knn == 7 && none.ratio == T(0.5) && none.samplingMethod == 0 && none.minPlanarity == T(0) && none.keepNormals && !none.keepShapes &&
              none.seed == 1);
        EL some(T(0.3), 5, 1, T(3), T(0.25), false, false, true, false, true, false, true, false, true, 5);
        CHECK(some.knn == 5 && some.samplingMethod == 1 && some.maxBoxDim == T(3) && some.minPlanarity == T(0.25) && !some.averageExistingDescriptors &&
              !some.keepNormals && some.keepDensities && !some.keepEigenValues && some.keepEigenVectors && !some.keepCovariances && some.keepWeights &&
              !some.keepMeans && some.keepShapes && some.seed == 5);
        auto throws = [](T minp, T window) {
            try { EL f(T(0.5), 7, 0, std::numeric_limits<T>::infinity(), minp, true, true, false, false, false, false, false, false, false, 1, window); }
            catch (const std::runtime_error &) { return true; }
            return false;
        };
        CHECK(!throws(T(0), inf) && !throws(T(1), inf));
        CHECK(throws(T(-0.1), inf) && throws(T(1.5), inf) && throws(std::numeric_limits<T>::quiet_NaN(), inf) && throws(T(0), T(0.1)));
        pgicp_filter spec;
        CHECK(!none.deviceSpec(spec));                               // a chain that holds it takes the per-filter path
    }
    {   // an empty cloud passes through untouched
        EL s(T(0.5), 7, 0, inf, T(0), true, true, true, true, true, true, true, true, true, 1);
        const T origin[3] = {T(0), T(0), T(0)};
        typename PM::DataPoints c = PM::DataPoints::fromXYZ(origin, 0);
        s.inPlaceFilter(c);
        CHECK(c.descriptors.rows() == 0 && c.descriptorLabels.empty());
    }
    {   // elipsoids_host.hpp on a box whose answer is exact: eigenvalues 0, 1, 3 (sum 4)
        namespace eh = pgslam_amd::elipsoids;
        const double ev[3] = {1.0, 0.0, 3.0};
        const eh::Shape<T> sh = eh::shape_of<T>(ev, 1, 0, 2);
        CHECK(sh.planarity == T(0.5) && sh.cylindricality == T(0.5) && sh.sphericality == T(0));
        CHECK(!eh::dropped_by_planarity<T>(sh, T(0)) && !eh::dropped_by_planarity<T>(sh, T(0.5)) && eh::dropped_by_planarity<T>(sh, T(0.75)));
        CHECK(eh::min_planarity_ok(0.0) && eh::min_planarity_ok(1.0) && !eh::min_planarity_ok(-0.1) && !eh::min_planarity_ok(1.5) &&
              !eh::min_planarity_ok(std::nan("")) && !eh::min_planarity_ok(1.0 / 0.0));
    }
}

int main(int argc, char **argv)
{
    const bool f32 = argc > 2 && std::strcmp(argv[2], "f32") == 0;
    if (argc == 5 && std::strcmp(argv[1], "host") == 0) return f32 ? host<float>(argv[3], argv[4]) : host<double>(argv[3], argv[4]);
    if (argc == 2 && std::strcmp(argv[1], "yaml") == 0) {
        yaml<float>();
        yaml<double>();
        // the library exports what the header declares: the addresses resolve at link time, and a call without a context is refused
        // as a bad argument
        int n_out = 0;
        CHECK(pgicp_elipsoids_f32(nullptr, nullptr, 3, 0, PGICP_HOST, 7, 0.5, 0, 1.0, 1, nullptr, 0, 0, nullptr, 3, nullptr, 3, nullptr, nullptr, &n_out, nullptr,
                                  nullptr, nullptr, nullptr, 0.0, nullptr, nullptr, nullptr, nullptr) == PGICP_ERR_ARG);
        CHECK(pgicp_elipsoids_f64(nullptr, nullptr, 3, 0, PGICP_HOST, 7, 0.5, 0, 1.0, 1, nullptr, 0, 0, nullptr, 3, nullptr, 3, nullptr, nullptr, &n_out, nullptr,
                                  nullptr, nullptr, nullptr, 0.0, nullptr, nullptr, nullptr, nullptr) == PGICP_ERR_ARG);
        std::puts("elipsoids cpu tests ok");
        return 0;
    }
    std::fprintf(stderr, "usage: test_elipsoids_cpu host <f32|f64> <in> <out> | yaml\n");
    return 2;
}
