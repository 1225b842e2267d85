// [EXT] SurfaceNormalDataPointsFilter's further outputs without a device (tests/test_cpp_surface_normals_ext.py drives it):
//   host <f32|f64> <in> <out>     the host statement (include/pgslam_amd/surface_normals_host.hpp) on the cloud and the neighbour
//                                 table of <in> (n, knn as int32; xyz, 3 a point; ids, knn a point as int32): normals, eigValues,
//                                 eigVectors, meanDists, matchedIds and the smoothed normals, one array after the other;
//   yaml                          YAML loading of keepEigenVectors, keepMatchedIds, keepMeanDist and smoothNormals -- each alone and
//                                 all together --, the fields they set, the one new refusal, the constructors, and the library's
//                                 exports of what include/pgicp_normals_ext.h declares.
#include "common.hpp"
#include "pgslam_amd/surface_normals_host.hpp"
#include <cstring>
#include <fstream>

template <typename T>
int host(const char *fin, const char *fout)
{
    std::ifstream in(fin, std::ios::binary);
    int n = 0, knn = 0;
    in.read((char *)&n, sizeof n); in.read((char *)&knn, sizeof knn);
    std::vector<T> xyz(3 * (size_t)n);
    std::vector<int32_t> ids((size_t)n * knn);
    in.read((char *)xyz.data(), sizeof(T) * xyz.size());
    in.read((char *)ids.data(), sizeof(int32_t) * ids.size());
    CHECK(in.good());
    const auto r = pgslam_amd::surface_normals::rows<T>(xyz.data(), 3, n, ids.data(), knn);
    const auto s = pgslam_amd::surface_normals::smooth<T>(r.normals.data(), 3, n, ids.data(), knn);
    // the strides are honoured: the same cloud and normals in rows of 5
    std::vector<T> wide(5 * (size_t)n, T(7)), nwide(5 * (size_t)n, T(7));
    for (int i = 0; i < n; i++) for (int a = 0; a < 3; a++) { wide[5 * (size_t)i + a] = xyz[3 * (size_t)i + a]; nwide[5 * (size_t)i + a] = r.normals[3 * (size_t)i + a]; }
    const auto r5 = pgslam_amd::surface_normals::rows<T>(wide.data(), 5, n, ids.data(), knn);
    CHECK(r5.eigVectors == r.eigVectors && r5.meanDists == r.meanDists && r5.normals == r.normals);
    CHECK(pgslam_amd::surface_normals::smooth<T>(nwide.data(), 5, n, ids.data(), knn) == s);
    std::ofstream out(fout, std::ios::binary);
    for (const std::vector<T> *v : {&r.normals, &r.eigValues, &r.eigVectors, &r.meanDists, &r.matchedIds, &s})
        out.write((const char *)v->data(), sizeof(T) * v->size());
    return out.good() ? 0 : 1;
}

template <typename T>
void yaml()
{
    typedef PointMatcher<T> PM;
    typedef typename PM::SurfaceNormalDataPointsFilter SN;
    auto load = [](const std::string &text) { std::istringstream ys(text); return typename PM::DataPointsFilters(ys); };
    auto message = [&](const std::string &text) {
        try { load(text); } catch (const std::runtime_error &e) { return std::string(e.what()); }
        return std::string();
    };
    const std::string head = "- SurfaceNormalDataPointsFilter:\n    knn: 9\n";
    struct Flags { bool ev, mi, md, sm; };
    auto flags = [&](const std::string &text) {
        auto f = load(text);
        auto sn = std::dynamic_pointer_cast<SN>(f.at(0));
        CHECK(sn && sn->knn == 9 && sn->keepNormals && !sn->keepEigenValues && !sn->keepDensities);
        return Flags{sn->keepEigenVectors, sn->keepMatchedIds, sn->keepMeanDist, sn->smoothNormals};
    };
    auto is = [](const Flags &f, bool ev, bool mi, bool md, bool sm) { return f.ev == ev && f.mi == mi && f.md == md && f.sm == sm; };
    CHECK(is(flags(head), false, false, false, false));
    CHECK(is(flags(head + "    keepEigenVectors: 1\n"), true, false, false, false));
    CHECK(is(flags(head + "    keepMatchedIds: 1\n"), false, true, false, false));
    CHECK(is(flags(head + "    keepMeanDist: 1\n"), false, false, true, false));
    CHECK(is(flags(head + "    smoothNormals: 1\n"), false, false, false, true));
    CHECK(is(flags(head + "    keepEigenVectors: 0\n    keepMatchedIds: 0\n    keepMeanDist: 0\n    smoothNormals: 0\n"), false, false, false, false));
    {   // all together, with the older ones
        auto f = load(head + "    maxDist: 0.5\n    keepNormals: 1\n    keepDensities: 1\n    keepEigenValues: 1\n    keepEigenVectors: 1\n    keepMatchedIds: 1\n"
                             "    keepMeanDist: 1\n    smoothNormals: 1\n");
        auto sn = std::dynamic_pointer_cast<SN>(f.at(0));
        CHECK(sn && sn->knn == 9 && sn->maxDist == T(0.5) && sn->keepNormals && sn->keepDensities && sn->keepEigenValues && sn->keepEigenVectors &&
              sn->keepMatchedIds && sn->keepMeanDist && sn->smoothNormals && sn->wantsExt());
    }
    {   // without the normals the other rows still load; smoothing does not: there is nothing to smooth into
        auto f = load(head + "    keepNormals: 0\n    keepEigenVectors: 1\n");
        auto sn = std::dynamic_pointer_cast<SN>(f.at(0));
        CHECK(sn && !sn->keepNormals && sn->keepEigenVectors);
        const std::string msg = message(head + "    keepNormals: 0\n    smoothNormals: 1\n");
        CHECK(msg.find("SurfaceNormalDataPointsFilter") == 0 && msg.find("smoothNormals needs keepNormals") != std::string::npos);
        bool threw = false;
        try { SN bad(5, T(1), false, false, false, false, false, false, true); } catch (const std::runtime_error &) { threw = true; }
        CHECK(threw);
    }
    // what the entry's parsing refused before, it refuses still
    CHECK(message(head + "    epsilon: -1\n").find("epsilon") != std::string::npos);
    CHECK(message("- SurfaceNormalDataPointsFilter:\n    knn: 2\n").find("knn") != std::string::npos);
    CHECK(message("- SurfaceNormalDataPointsFilter:\n    knn: 33\n    keepEigenVectors: 1\n").find("knn") != std::string::npos);
    {   // the five-argument constructor, and the new arguments in upstream's order
        SN five(7, T(2), true, true, true);
        CHECK(five.knn == 7 && five.keepNormals && five.keepEigenValues && five.keepDensities && !five.wantsExt());
        SN four(7, T(2), true, false);
        CHECK(!four.keepDensities && !four.wantsExt());
        SN nine(7, T(2), true, false, false, true, false, true, false);
        CHECK(nine.keepEigenVectors && !nine.keepMatchedIds && nine.keepMeanDist && !nine.smoothNormals && nine.wantsExt());
    }
    {   // an empty cloud passes through; nothing asked for: the cloud stays as it is, and no context is made
        SN sn(5, T(1), false, false);
        const T pts[9] = {T(0), T(0), T(0), T(1), T(0), T(2), T(3), T(1), T(2)};
        typename PM::DataPoints c = PM::DataPoints::fromXYZ(pts, 3);
        sn.inPlaceFilter(c);
        CHECK(c.descriptors.rows() == 0 && c.descriptorLabels.empty());
    }
    {   // MaxDensity does not fuse with a SurfaceNormal filter that asks for a new row (decided before any device is looked for)
        typename PM::MaxDensityDataPointsFilter md(T(10), 1);
        SN sn(5, T(1), true, false, true, true);
        const T pts[9] = {T(0), T(0), T(0), T(1), T(0), T(2), T(3), T(1), T(2)};
        typename PM::DataPoints c = PM::DataPoints::fromXYZ(pts, 3);
        CHECK(!md.fusedWith(sn, c) && c.descriptors.rows() == 0);
    }
}

int main(int argc, char **argv)
{
    const bool f32 = argc > 2 && std::strcmp(argv[2], "f32") == 0;
    if (argc == 5 && std::strcmp(argv[1], "host") == 0) return f32 ? host<float>(argv[3], argv[4]) : host<double>(argv[3], argv[4]);
    if (argc == 2 && std::strcmp(argv[1], "yaml") == 0) {
        yaml<float>();
        yaml<double>();
        // the library exports what the header declares: the four addresses resolve at link time, and a call without a context is
        // refused as a bad argument
        CHECK(pgicp_surface_normals_ext_f32(nullptr, nullptr, 3, 0, PGICP_HOST, 5, 1.0, 0, nullptr, 3, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == PGICP_ERR_ARG);
        CHECK(pgicp_surface_normals_ext_f64(nullptr, nullptr, 3, 0, PGICP_HOST, 5, 1.0, 0, nullptr, 3, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == PGICP_ERR_ARG);
        CHECK(pgicp_smooth_normals_f32(nullptr, nullptr, 3, nullptr, 5, 0, PGICP_HOST, nullptr, 3) == PGICP_ERR_ARG);
        CHECK(pgicp_smooth_normals_f64(nullptr, nullptr, 3, nullptr, 5, 0, PGICP_HOST, nullptr, 3) == PGICP_ERR_ARG);
        CHECK(PGICP_NORMALS_EXT_MAX_IDS_F32 == (1 << 24));
        std::puts("surface normals ext cpu tests ok");
        return 0;
    }
    std::fprintf(stderr, "usage: test_surface_normals_ext_cpu host <f32|f64> <in> <out> | yaml\n");
    return 2;
}
