// Applies a DataPointsFilters YAML list (SamplingSurfaceNormalDataPointsFilter) of the drop-in's PointMatcher shim to a cloud twice
// -- with PGSLAM_HOST_SAMPLING_NORMALS unset (the device path) and set to 1 (the host recursion) -- and compares the two DataPoints:
//   ssn_device_apply f32|f64 FILTERS.yaml IN.bin OUT.bin
// IN.bin: int32 n, int32 drows, n x 3 points (T), n x drows descriptor values (T; labelled "d0", "d1", ... one row each).
// Prints "ran_on_device off=<0|1> on=<0|1> identical=<0|1> n_out=<k>" and "wall_ms off=<ms> on=<ms>" (the chain's second apply); OUT.bin (the first run): int32 n_out, int32 frows,
// int32 drows, frows x n_out features, drows x n_out descriptors (column-major), int32 first row of "normals" (-1: none).
// (tests/test_gpu_sampling_normals.py)
#include <pointmatcher/PointMatcher.h>

#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

template <typename T>
static bool same(const typename PointMatcher<T>::Matrix &a, const typename PointMatcher<T>::Matrix &b)
{
    if (a.rows() != b.rows() || a.cols() != b.cols()) return false;
    const size_t k = (size_t)a.rows() * (size_t)a.cols();
    return k == 0 || std::memcmp(a.data(), b.data(), sizeof(T) * k) == 0;
}

template <typename T>
static int run(const char *yaml, const char *in, const char *out)
{
    using PM = PointMatcher<T>;
    FILE *fi = std::fopen(in, "rb");
    if (!fi) return 2;
    int n = 0, drows = 0;
    if (std::fread(&n, 4, 1, fi) != 1 || std::fread(&drows, 4, 1, fi) != 1) return 2;
    std::vector<T> xyz((size_t)3 * n), desc((size_t)drows * n);
    if (std::fread(xyz.data(), sizeof(T), xyz.size(), fi) != xyz.size()) return 2;
    if (std::fread(desc.data(), sizeof(T), desc.size(), fi) != desc.size()) return 2;
    std::fclose(fi);
    auto make = [&]() {
        auto cloud = PM::DataPoints::fromXYZ(xyz.data(), n, nullptr);
        for (int r = 0; r < drows; r++) {
            typename PM::Matrix d(1, n);
            for (int j = 0; j < n; j++) d(0, j) = desc[(size_t)j * drows + r];
            cloud.addDescriptor("d" + std::to_string(r), d);
        }
        return cloud;
    };
    auto apply = [&](bool host, bool &on_device, double &ms) {
        if (host) setenv("PGSLAM_HOST_SAMPLING_NORMALS", "1", 1); else unsetenv("PGSLAM_HOST_SAMPLING_NORMALS");
        std::ifstream fy(yaml);
        typename PM::DataPointsFilters filters(fy);
        filters.init();
        { auto warm = make(); filters.apply(warm); }            // (the filter's device context is made at its first use)
        auto cloud = make();
        const auto t0 = std::chrono::steady_clock::now();
        filters.apply(cloud);
        ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        on_device = false;
        for (auto &f : filters)
            if (auto *s = dynamic_cast<typename PM::SamplingSurfaceNormalDataPointsFilter *>(f.get())) on_device = on_device || s->ranOnDevice();
        return cloud;
    };
    bool dev_off = false, dev_on = false;
    double ms_off = 0, ms_on = 0;
    const auto a = apply(false, dev_off, ms_off);
    const auto b = apply(true, dev_on, ms_on);
    bool identical = same<T>(a.features, b.features) && same<T>(a.descriptors, b.descriptors) &&
                     a.descriptorLabels.size() == b.descriptorLabels.size() && a.featureLabels.size() == b.featureLabels.size();
    for (size_t k = 0; identical && k < a.descriptorLabels.size(); k++)
        identical = a.descriptorLabels[k].text == b.descriptorLabels[k].text && a.descriptorLabels[k].span == b.descriptorLabels[k].span;
    const int m = (int)a.features.cols(), fr = (int)a.features.rows(), dr = (int)a.descriptors.rows();
    std::printf("ran_on_device off=%d on=%d identical=%d n_out=%d\n", dev_off ? 1 : 0, dev_on ? 1 : 0, identical ? 1 : 0, m);
    std::printf("wall_ms off=%.3f on=%.3f\n", ms_off, ms_on);
    FILE *fo = std::fopen(out, "wb");
    if (!fo) return 2;
    std::fwrite(&m, 4, 1, fo); std::fwrite(&fr, 4, 1, fo); std::fwrite(&dr, 4, 1, fo);
    std::fwrite(a.features.data(), sizeof(T), (size_t)fr * m, fo);
    if (dr) std::fwrite(a.descriptors.data(), sizeof(T), (size_t)dr * m, fo);
    const int nr = a.descriptorExists("normals") ? a.getDescriptorStartingRow("normals") : -1;
    std::fwrite(&nr, 4, 1, fo);
    std::fclose(fo);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc != 5) { std::fprintf(stderr, "usage: ssn_device_apply f32|f64 FILTERS.yaml IN.bin OUT.bin\n"); return 1; }
    try {
        return !std::strcmp(argv[1], "f64") ? run<double>(argv[2], argv[3], argv[4]) : run<float>(argv[2], argv[3], argv[4]);
    } catch (const std::exception &e) { std::fprintf(stderr, "ssn_device_apply: %s\n", e.what()); return 3; }
}
