// [EXT] SamplingSurfaceNormalDataPointsFilter's further outputs without a device (tests/test_sampling_normals_ext_host.py drives it):
//   host <f32|f64> <in> <out>     the filter's host form (PGSLAM_HOST_SAMPLING_NORMALS=1 is set here) with keepDensities,
//                                 keepEigenValues and keepEigenVectors on every case of <in>: int32 cases, then per case int32 n, drows,
//                                 knn, method, average, double ratio, maxBoxDim, seed, the points (3 a point) and the descriptors
//                                 (drows a point, labelled d0, d1, ...).  <out>, per case: int32 kept, int32 descriptor rows, the kept
//                                 points (3 a point), the descriptors (all rows of a point together); the labels are checked here;
//   yaml                          YAML loading of keepEigenValues and keepEigenVectors -- each alone and together --, keepDensities
//                                 still refused, unknown keys treated as before, the constructors, and the library's exports of what
//                                 include/pgicp_ssn_ext.h declares.
#include "common.hpp"
#include <cstring>
#include <fstream>
#include <sstream>

template <typename T>
int host(const char *fin, const char *fout)
{
    typedef PointMatcher<T> PM;
    typedef typename PM::SamplingSurfaceNormalDataPointsFilter SSN;
    setenv("PGSLAM_HOST_SAMPLING_NORMALS", "1", 1);
    std::ifstream in(fin, std::ios::binary);
    std::ofstream out(fout, std::ios::binary);
    int cases = 0;
    in.read((char *)&cases, sizeof cases);
    for (int cs = 0; cs < cases; cs++) {
        int h[5];
        double p[3];
        in.read((char *)h, sizeof h); in.read((char *)p, sizeof p);
        const int n = h[0], drows = h[1], knn = h[2], method = h[3], average = h[4];
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
        SSN all((T)p[0], knn, method, (T)p[1], average != 0, true, (unsigned long long)p[2], true, true, true);
        auto c = make();
        all.inPlaceFilter(c);
        CHECK(!all.ranOnDevice());
        // upstream's order after the cloud's own rows: normals, densities, eigValues, eigVectors
        const char *names[4] = {"normals", "densities", "eigValues", "eigVectors"};
        const int spans[4] = {3, 1, 3, 9};
        CHECK((int)c.descriptorLabels.size() == drows + 4 && (int)c.descriptors.rows() == drows + 16);
        for (int k = 0, row = drows; k < 4; row += spans[k], k++) {
            CHECK(c.descriptorLabels[drows + k].text == names[k] && (int)c.descriptorLabels[drows + k].span == spans[k]);
            CHECK(c.getDescriptorStartingRow(names[k]) == row);
        }
        // the seven-argument form leaves what it left before: the same points, the same first rows, no new label
        SSN seven((T)p[0], knn, method, (T)p[1], average != 0, true, (unsigned long long)p[2]);
        CHECK(!seven.wantsExt());
        auto c7 = make();
        seven.inPlaceFilter(c7);
        CHECK(c7.features.cols() == c.features.cols() && (int)c7.descriptors.rows() == drows + 3 && (int)c7.descriptorLabels.size() == drows + 1);
        for (int j = 0; j < (int)c.features.cols(); j++) {
            for (int r = 0; r < (int)c.features.rows(); r++) CHECK(std::memcmp(&c7.features(r, j), &c.features(r, j), sizeof(T)) == 0);
            for (int r = 0; r < drows + 3; r++) CHECK(std::memcmp(&c7.descriptors(r, j), &c.descriptors(r, j), sizeof(T)) == 0);
        }
        // each row alone equals its rows of the filter with all three; rows that exist already are overwritten in place
        for (int one = 0; one < 3; one++) {
            SSN f((T)p[0], knn, method, (T)p[1], average != 0, true, (unsigned long long)p[2], one == 0, one == 1, one == 2);
            auto c1 = make();
            f.inPlaceFilter(c1);
            const char *name = names[1 + one];
            CHECK((int)c1.descriptorLabels.size() == drows + 2 && c1.descriptorLabels[drows + 1].text == name);
            const int r1 = c1.getDescriptorStartingRow(name), ra = c.getDescriptorStartingRow(name);
            for (int j = 0; j < (int)c.features.cols(); j++)
                for (int r = 0; r < spans[1 + one]; r++) CHECK(std::memcmp(&c1.descriptors(r1 + r, j), &c.descriptors(ra + r, j), sizeof(T)) == 0);
            if (drows == 0 || !(method == 1 && average)) {
                // (with averaging the second pass would average the first pass's rows too: the other descriptors would differ)
                const int rows_before = (int)c1.descriptors.rows(), kept_before = (int)c1.features.cols();
                SSN again((T)1, knn, 1, std::numeric_limits<T>::infinity(), false, true, 1, one == 0, one == 1, one == 2);
                again.inPlaceFilter(c1);
                CHECK((int)c1.descriptors.rows() == rows_before && (int)c1.descriptorLabels.size() == drows + 2);
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
    typedef typename PM::SamplingSurfaceNormalDataPointsFilter SSN;
    auto load = [](const std::string &text) { std::istringstream ys(text); return typename PM::DataPointsFilters(ys); };
    auto message = [&](const std::string &text) {
        try { load(text); } catch (const std::runtime_error &e) { return std::string(e.what()); }
        return std::string();
    };
    const std::string head = "- SamplingSurfaceNormalDataPointsFilter:\n    knn: 9\n    ratio: 0.25\n";
    struct Flags { bool kd, ke, kev; };
    auto flags = [&](const std::string &text) {
        auto f = load(text);
        auto s = std::dynamic_pointer_cast<SSN>(f.at(0));
        CHECK(s && s->knn == 9 && s->ratio == T(0.25) && s->keepNormals && s->samplingMethod == 0 && s->averageExistingDescriptors && s->seed == 1);
        return Flags{s->keepDensities, s->keepEigenValues, s->keepEigenVectors};
    };
    auto is = [](const Flags &f, bool kd, bool ke, bool kev) { return f.kd == kd && f.ke == ke && f.kev == kev; };
    CHECK(is(flags(head), false, false, false));
    CHECK(is(flags(head + "    keepEigenValues: 1\n"), false, true, false));
    CHECK(is(flags(head + "    keepEigenVectors: 1\n"), false, false, true));
    CHECK(is(flags(head + "    keepEigenValues: 1\n    keepEigenVectors: 1\n"), false, true, true));
    CHECK(is(flags(head + "    keepDensities: 0\n    keepEigenValues: 0\n    keepEigenVectors: 0\n"), false, false, false));
    {   // together with the older parameters
        auto f = load(head + "    samplingMethod: 1\n    maxBoxDim: 2.5\n    averageExistingDescriptors: 0\n    keepNormals: 0\n    seed: 23\n"
                             "    keepEigenValues: 1\n    keepEigenVectors: 1\n");
        auto s = std::dynamic_pointer_cast<SSN>(f.at(0));
        CHECK(s && s->samplingMethod == 1 && s->maxBoxDim == T(2.5) && !s->averageExistingDescriptors && !s->keepNormals && s->seed == 23 &&
              !s->keepDensities && s->keepEigenValues && s->keepEigenVectors && s->wantsExt());
    }
    // keepDensities stays refused from YAML, alone and beside the keys that load
    {
        const std::string msg = message(head + "    keepDensities: 1\n");
        CHECK(msg.find("SamplingSurfaceNormalDataPointsFilter") == 0 && msg.find("keepDensities is not supported") != std::string::npos);
        CHECK(message(head + "    keepEigenValues: 1\n    keepDensities: 1\n").find("keepDensities") != std::string::npos);
    }
    // what the entry's parsing refused before, it refuses still; a key it never looked at is passed over as before
    CHECK(message("- SamplingSurfaceNormalDataPointsFilter:\n    ratio: 1.5\n").find("ratio") != std::string::npos);
    CHECK(message("- SamplingSurfaceNormalDataPointsFilter:\n    knn: 2\n    keepEigenValues: 1\n").find("knn") != std::string::npos);
    CHECK(message("- SamplingSurfaceNormalDataPointsFilter:\n    samplingMethod: 2\n").find("samplingMethod") != std::string::npos);
    CHECK(is(flags(head + "    noSuchParameter: 1\n"), false, false, false));
    {   // the seven-argument constructor and the shorter ones compile and leave the new fields off; the new arguments trail
        SSN seven(T(0.5), 7, 0, std::numeric_limits<T>::infinity(), true, true, 1);
        CHECK(!seven.keepDensities && !seven.keepEigenValues && !seven.keepEigenVectors && !seven.wantsExt());
        SSN none;
        CHECK(none.knn == 7 && none.ratio == T(0.5) && !none.wantsExt());
        SSN ten(T(0.5), 7, 1, T(3), false, true, 5, true, false, true);
        CHECK(ten.keepDensities && !ten.keepEigenValues && ten.keepEigenVectors && ten.wantsExt() && ten.seed == 5);
    }
    {   // an empty cloud passes through untouched
        SSN s(T(0.5), 7, 0, std::numeric_limits<T>::infinity(), true, true, 1, true, true, true);
        const T origin[3] = {T(0), T(0), T(0)};
        typename PM::DataPoints c = PM::DataPoints::fromXYZ(origin, 0);
        s.inPlaceFilter(c);
        CHECK(c.descriptors.rows() == 0 && c.descriptorLabels.empty());
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
        CHECK(pgicp_sampling_surface_normal_ext_f32(nullptr, nullptr, 3, 0, PGICP_HOST, 7, 0.5, 0, 1.0, 1, nullptr, 0, 0, nullptr, 3, nullptr, 3, nullptr,
                                                    nullptr, &n_out, nullptr, nullptr, nullptr, nullptr) == PGICP_ERR_ARG);
        CHECK(pgicp_sampling_surface_normal_ext_f64(nullptr, nullptr, 3, 0, PGICP_HOST, 7, 0.5, 0, 1.0, 1, nullptr, 0, 0, nullptr, 3, nullptr, 3, nullptr,
                                                    nullptr, &n_out, nullptr, nullptr, nullptr, nullptr) == PGICP_ERR_ARG);
        std::puts("sampling normals ext cpu tests ok");
        return 0;
    }
    std::fprintf(stderr, "usage: test_sampling_normals_ext_cpu host <f32|f64> <in> <out> | yaml\n");
    return 2;
}
