// [EXT] VoxelGridDataPointsFilter in the C++ drop-in.
//   test_voxel_grid_cpu yaml
//     loadFromYaml: the defaults, the members upstream spells, the refusals (the sizes given together or not at all), the unsupported-filter message, and the input
//     stage's one-pass paths declining a chain that holds it.  No device needed.
//   test_voxel_grid_cpu apply f32|f64 IN.bin OUT.bin [REPS]
//     applies the filter to a cloud read from IN.bin and writes what it leaves.  The host form runs where there is no device or
//     PGSLAM_HOST_VOXEL_GRID=1; tests/test_voxel_grid_host.py compares it with tests/voxel_grid_ref.py, and
//     tests/test_gpu_voxel_grid.py compares the device path with the host one.  With REPS, the filter's mean wall time over
//     REPS calls after a warm-up is printed (tools/bench_voxel_grid.py).
//     IN.bin: int32 n, int32 drows, double v[3], int32 use_centroid, int32 average, n x 4 features (T, a point's 4 rows
//     contiguous), n x drows descriptors (T).  OUT.bin: int32 n_out, int32 on_device, int32 refused, n_out x 4 features,
//     n_out x drows descriptors, then the descriptor labels as int32 count and (int32 span, int32 length, bytes) each.
#include "common.hpp"
#include <chrono>
#include <cstring>
#include <sstream>
#include <string>

template <typename T>
void yaml()
{
    using PM = PointMatcher<T>;
    auto load = [](const std::string &y) {
        std::istringstream in(y);
        return typename PM::DataPointsFilters(in);
    };
    auto refused = [&](const std::string &y, const char *needle = nullptr) {
        try { load(y); } catch (const std::runtime_error &e) { return !needle || std::string(e.what()).find(needle) != std::string::npos; }
        return false;
    };
    {   // upstream's defaults: 1 m, centroid, averaged descriptors
        auto f = load("- VoxelGridDataPointsFilter\n");
        CHECK(f.size() == 1);
        auto v = std::dynamic_pointer_cast<typename PM::VoxelGridDataPointsFilter>(f[0]);
        CHECK(v && v->vSizeX == T(1) && v->vSizeY == T(1) && v->vSizeZ == T(1) && v->useCentroid && v->averageExistingDescriptors);
        CHECK(!v->ranOnDevice());
    }
    {
        auto f = load("- VoxelGridDataPointsFilter:\n    vSizeX: 0.2\n    vSizeY: 0.3\n    vSizeZ: 0.05\n    useCentroid: 0\n"
                      "    averageExistingDescriptors: 0\n");
        auto v = std::dynamic_pointer_cast<typename PM::VoxelGridDataPointsFilter>(f.at(0));
        CHECK(v && v->vSizeX == T(0.2) && v->vSizeY == T(0.3) && v->vSizeZ == T(0.05) && !v->useCentroid && !v->averageExistingDescriptors);
    }
    auto sizes = [](const char *x, const char *y, const char *z) {
        return std::string("- VoxelGridDataPointsFilter:\n    vSizeX: ") + x + "\n    vSizeY: " + y + "\n    vSizeZ: " + z + "\n";
    };
    for (const char *bad : {"0", "-1", "nan", "inf", "-inf", "1e-60"})
        for (int axis = 0; axis < 3; axis++) {
            const std::string y = sizes(axis == 0 ? bad : "0.1", axis == 1 ? bad : "0.1", axis == 2 ? bad : "0.1");
            // (1e-60 is > 0 in double and 0 in float: refused in float only)
            if (std::strcmp(bad, "1e-60") == 0 && sizeof(T) == 8) { load(y); continue; }
            CHECK(refused(y, "finite and > 0"));
        }
    // the sizes together or not at all: one or two alone would leave the others at 1 m
    for (const char *part : {"    vSizeX: 0.1\n", "    vSizeY: 0.1\n", "    vSizeZ: 0.1\n", "    vSizeX: 0.1\n    vSizeY: 0.1\n",
                             "    vSizeY: 0.1\n    vSizeZ: 0.1\n", "    vSizeX: 0.1\n    vSizeZ: 0.1\n    useCentroid: 0\n"})
        CHECK(refused(std::string("- VoxelGridDataPointsFilter:\n") + part, "together"));
    {
        auto f = load("- VoxelGridDataPointsFilter:\n    useCentroid: 0\n");        // no size: 1 m each
        auto v = std::dynamic_pointer_cast<typename PM::VoxelGridDataPointsFilter>(f.at(0));
        CHECK(v && v->vSizeX == T(1) && v->vSizeY == T(1) && v->vSizeZ == T(1) && !v->useCentroid && v->averageExistingDescriptors);
    }
    CHECK(refused(sizes("0.1", "0.1", "0.1") + "    vSize: 0.1\n", "unknown parameter"));
    {   // the unsupported-filter message names it among the supported ones
        std::string msg;
        try { load("- OctreeGridDataPointsFilter\n"); } catch (const std::runtime_error &e) { msg = e.what(); }
        CHECK(msg.find("unsupported filter 'OctreeGridDataPointsFilter'") != std::string::npos);
        CHECK(msg.find("VoxelGrid") != std::string::npos);
    }
    {   // in an ICP object's reading and reference chains
        typename PM::ICP icp;
        std::istringstream in(std::string("readingDataPointsFilters:\n  - VoxelGridDataPointsFilter:\n      vSizeX: 0.1\n      vSizeY: 0.1\n      vSizeZ: 0.1\n"
                                          "referenceDataPointsFilters:\n  - VoxelGridDataPointsFilter:\n      vSizeX: 0.05\n      vSizeY: 0.05\n      vSizeZ: 0.05\n"
                                          "  - SurfaceNormalDataPointsFilter:\n      knn: 10\n") + kIcpYamlTail);
        icp.loadFromYaml(in);
        CHECK(icp.readingDataPointsFilters.size() == 1 && icp.referenceDataPointsFilters.size() == 2);
    }
    {   // the input stage's one-pass forms decline the chain (no deviceSpec: the filter changes values): per-filter path
        auto f = load("- MinDistDataPointsFilter:\n    minDist: 0.5\n" + sizes("0.1", "0.1", "0.1"));
        std::vector<pgicp_filter> specs;
        CHECK(!f.deviceSpecs(specs));
        std::vector<T> xyz = {T(1), T(2), T(3), T(4), T(5), T(6)};
        auto cloud = PM::DataPoints::fromXYZ(xyz.data(), 2);
        const typename PM::TransformationParameters I = PM::Matrix::Identity(4, 4);
        const T *dev = nullptr;
        int kept = -1;
        std::vector<int32_t> dropped;
        CHECK(!PM::filterOnDeviceDeferred(nullptr, f, cloud, I, &dev, &kept, dropped));
        CHECK(!PM::filterAndTransformOnDevice(nullptr, f, cloud, I, &dev));
        CHECK(cloud.getNbPoints() == 2 && kept == -1);
    }
    {   // the host form's refusals point at RemoveNaN
        auto f = load(sizes("0.1", "0.1", "0.1"));
        for (T bad : {std::numeric_limits<T>::quiet_NaN(), std::numeric_limits<T>::infinity()}) {
            std::vector<T> xyz = {T(1), T(2), T(3), bad, T(5), T(6)};
            auto cloud = PM::DataPoints::fromXYZ(xyz.data(), 2);
            std::string msg;
            setenv("PGSLAM_HOST_VOXEL_GRID", "1", 1);
            try { f.apply(cloud); } catch (const std::runtime_error &e) { msg = e.what(); }
            CHECK(msg.find("RemoveNaNDataPointsFilter") != std::string::npos);
        }
        {   // a numDiv >= 2^31
            auto g = load(sizes("1e-6", "1", "1"));
            std::vector<T> xyz = {T(0), T(0), T(0), T(1e4), T(0), T(0)};
            auto cloud = PM::DataPoints::fromXYZ(xyz.data(), 2);
            std::string msg;
            try { g.apply(cloud); } catch (const std::runtime_error &e) { msg = e.what(); }
            CHECK(msg.find("too fine") != std::string::npos && msg.find("RemoveNaNDataPointsFilter") != std::string::npos);
        }
        {   // a product of divisions >= 2^62 (each < 2^31)
            auto g = load("- VoxelGridDataPointsFilter:\n    vSizeX: 1e-3\n    vSizeY: 1e-3\n    vSizeZ: 1e-3\n");
            std::vector<T> xyz = {T(0), T(0), T(0), T(1e6), T(1e6), T(1e6)};
            auto cloud = PM::DataPoints::fromXYZ(xyz.data(), 2);
            std::string msg;
            try { g.apply(cloud); } catch (const std::runtime_error &e) { msg = e.what(); }
            CHECK(msg.find("2^62") != std::string::npos);
        }
        unsetenv("PGSLAM_HOST_VOXEL_GRID");
        // an empty cloud stays empty, a 2-D cloud is refused
        typename PM::DataPoints empty = PM::DataPoints::fromXYZ(nullptr, 0);
        f.apply(empty);
        CHECK(empty.getNbPoints() == 0);
        typename PM::DataPoints flat;
        flat.features = typename PM::Matrix(3, 2);
        bool threw = false;
        try { f.apply(flat); } catch (const std::runtime_error &) { threw = true; }
        CHECK(threw);
    }
}

template <typename T>
int apply(const char *in, const char *out, int reps)
{
    using PM = PointMatcher<T>;
    FILE *fi = std::fopen(in, "rb");
    if (!fi) return 2;
    int n = 0, drows = 0, cen = 0, avg = 0;
    double v[3];
    if (std::fread(&n, 4, 1, fi) != 1 || std::fread(&drows, 4, 1, fi) != 1 || std::fread(v, 8, 3, fi) != 3 || std::fread(&cen, 4, 1, fi) != 1 ||
        std::fread(&avg, 4, 1, fi) != 1)
        return 2;
    typename PM::DataPoints c;
    c.features = typename PM::Matrix(4, n);
    c.featureLabels.push_back(typename PM::DataPoints::Label("x", 1)); c.featureLabels.push_back(typename PM::DataPoints::Label("y", 1));
    c.featureLabels.push_back(typename PM::DataPoints::Label("z", 1)); c.featureLabels.push_back(typename PM::DataPoints::Label("pad", 1));
    if (std::fread(c.features.data(), sizeof(T), (size_t)4 * n, fi) != (size_t)4 * n) return 2;
    if (drows > 0) {
        typename PM::Matrix d(drows, n);
        if (std::fread(d.data(), sizeof(T), (size_t)drows * n, fi) != (size_t)drows * n) return 2;
        c.addDescriptor("d0", d.block(0, 0, 1, n));
        if (drows > 1) c.addDescriptor("rest", d.block(1, 0, drows - 1, n));
    }
    std::fclose(fi);
    typename PM::VoxelGridDataPointsFilter f((T)v[0], (T)v[1], (T)v[2], cen != 0, avg != 0);
    int refused = 0;
    if (reps > 0) {   // timing: one warm-up call (the context made, scratch allocated), then the mean of `reps` calls
        typename PM::DataPoints w(c);
        f.inPlaceFilter(w);
        double ms = 0;
        for (int r = 0; r < reps; r++) {
            typename PM::DataPoints t(c);
            const auto t0 = std::chrono::steady_clock::now();
            f.inPlaceFilter(t);
            ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        }
        std::printf("ms=%.4f on_device=%d\n", ms / reps, f.ranOnDevice() ? 1 : 0);
    }
    try { f.inPlaceFilter(c); } catch (const std::runtime_error &) { refused = 1; }
    FILE *fo = std::fopen(out, "wb");
    const int m = refused ? 0 : (int)c.getNbPoints(), dev = f.ranOnDevice() ? 1 : 0;
    std::fwrite(&m, 4, 1, fo); std::fwrite(&dev, 4, 1, fo); std::fwrite(&refused, 4, 1, fo);
    if (m) std::fwrite(c.features.data(), sizeof(T), (size_t)4 * m, fo);
    if (m && drows) std::fwrite(c.descriptors.data(), sizeof(T), (size_t)drows * m, fo);
    const int nl = (int)c.descriptorLabels.size();
    std::fwrite(&nl, 4, 1, fo);
    for (auto &l : c.descriptorLabels) {
        const int span = (int)l.span, len = (int)l.text.size();
        std::fwrite(&span, 4, 1, fo); std::fwrite(&len, 4, 1, fo); std::fwrite(l.text.data(), 1, len, fo);
    }
    std::fclose(fo);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc == 2 && !std::strcmp(argv[1], "yaml")) {
        yaml<float>();
        yaml<double>();
        std::puts("voxel grid cpu tests ok");
        return 0;
    }
    if ((argc == 5 || argc == 6) && !std::strcmp(argv[1], "apply")) {
        const int reps = argc == 6 ? std::atoi(argv[5]) : 0;
        return !std::strcmp(argv[2], "f64") ? apply<double>(argv[3], argv[4], reps) : apply<float>(argv[3], argv[4], reps);
    }
    std::fprintf(stderr, "usage: test_voxel_grid_cpu yaml | apply f32|f64 IN.bin OUT.bin [REPS]\n");
    return 1;
}
