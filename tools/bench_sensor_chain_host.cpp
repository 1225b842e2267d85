// DataPointsFilters::apply on the sensor's six-filter chain, timed both ways: tools/bench_sensor_chain.py builds and runs it.
//   bench_sensor_chain_host <cloud.bin> <maxDensity> <reps> [descriptor]      <cloud.bin>: int32 n, then n points (3 floats a point).
//   The list: SimpleSensorNoise, SurfaceNormal{knn 10, keepDensities}, ObservationDirection, OrientNormals, Shadow{eps 0.2},
//   MaxDensity{maxDensity}; with `descriptor` the list of include/pgicp_descriptor_filters.h -- SurfaceNormal{knn 10, keepEigenValues,
//   keepDensities}, ObservationDirection, OrientNormals, IncidenceAngle, CutAtDescriptorThreshold{incidenceAngles, 1.3}, Sphericality,
//   CutAtDescriptorThreshold{sphericality, 0.2}, MaxDensity{maxDensity} -- as one pgicp_sensor_chain_ext_* call.  Alternating, after two warm-up runs of each: the run as one pgicp_sensor_chain_* call, and the same list
//   under PGSLAM_HOST_SENSOR_CHAIN=1 -- filter by filter, which is what apply did before the chain call existed.  Wall time around
//   apply (it returns with the cloud on the host).  Prints the medians in ms, their ratio and the points kept.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <vector>
#include "pgslam_amd/pgslam.hpp"

int main(int argc, char **argv)
{
    if (argc != 4 && argc != 5) { std::fprintf(stderr, "usage: bench_sensor_chain_host <cloud.bin> <maxDensity> <reps> [descriptor]\n"); return 2; }
    const bool descriptor = argc == 5;
    const unsigned run = descriptor ? 8u : 6u;
    typedef PointMatcher<float> PM;
    std::ifstream in(argv[1], std::ios::binary);
    int n = 0;
    in.read((char *)&n, sizeof n);
    std::vector<float> xyz(3 * (size_t)n);
    in.read((char *)xyz.data(), sizeof(float) * xyz.size());
    if (!in.good() || n <= 0) { std::fprintf(stderr, "bench_sensor_chain_host: cannot read %s\n", argv[1]); return 1; }
    const PM::DataPoints cloud = PM::DataPoints::fromXYZ(xyz.data(), n, nullptr);
    const std::string yaml = descriptor ?
        std::string("- SurfaceNormalDataPointsFilter:\n    knn: 10\n    keepEigenValues: 1\n    keepDensities: 1\n- ObservationDirectionDataPointsFilter\n"
                    "- OrientNormalsDataPointsFilter\n- IncidenceAngleDataPointsFilter\n"
                    "- CutAtDescriptorThresholdDataPointsFilter:\n    descName: incidenceAngles\n    useLargerThan: 1\n    threshold: 1.3\n"
                    "- SphericalityDataPointsFilter\n- CutAtDescriptorThresholdDataPointsFilter:\n    descName: sphericality\n    useLargerThan: 1\n    threshold: 0.2\n"
                    "- MaxDensityDataPointsFilter:\n    maxDensity: ") + argv[2] + "\n" :
                             std::string("- SimpleSensorNoiseDataPointsFilter\n- SurfaceNormalDataPointsFilter:\n    knn: 10\n    keepDensities: 1\n"
                                         "- ObservationDirectionDataPointsFilter\n- OrientNormalsDataPointsFilter\n- ShadowDataPointsFilter:\n    eps: 0.2\n"
                                         "- MaxDensityDataPointsFilter:\n    maxDensity: ") + argv[2] + "\n";
    std::istringstream ys(yaml);
    PM::DataPointsFilters filters(ys);
    const int reps = std::atoi(argv[3]);
    std::vector<double> ms[2];
    unsigned kept[2] = {0, 0};
    for (int r = -2; r < reps; r++)
        for (int knob = 0; knob < 2; knob++) {
            if (knob) setenv("PGSLAM_HOST_SENSOR_CHAIN", "1", 1); else unsetenv("PGSLAM_HOST_SENSOR_CHAIN");
            PM::DataPoints c(cloud);
            const auto t0 = std::chrono::steady_clock::now();
            filters.apply(c);
            const double t = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
            if (filters.lastFusedRun() != (knob ? 0u : run)) { std::fprintf(stderr, "bench_sensor_chain_host: lastFusedRun() = %zu\n", filters.lastFusedRun()); return 1; }
            kept[knob] = c.getNbPoints();
            if (r >= 0) ms[knob].push_back(t);
        }
    if (kept[0] != kept[1]) { std::fprintf(stderr, "bench_sensor_chain_host: the two ways keep %u and %u points\n", kept[0], kept[1]); return 1; }
    for (auto &v : ms) std::sort(v.begin(), v.end());
    const double fused = ms[0][ms[0].size() / 2], one_by_one = ms[1][ms[1].size() / 2];
    std::printf("{\"points\": %d, \"kept\": %u, \"apply_fused_median_ms\": %.3f, \"apply_filter_by_filter_median_ms\": %.3f, \"ratio\": %.2f}\n", n, kept[0],
                fused, one_by_one, one_by_one / fused);
    return 0;
}
