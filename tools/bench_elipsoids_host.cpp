// The host form of ElipsoidsDataPointsFilter (PGSLAM_HOST_ELIPSOIDS=1), timed: tools/bench_elipsoids.py builds and runs it.
//   bench_elipsoids_host <cloud.bin> <reps>      <cloud.bin>: int32 n, then n points (3 floats a point); knn 7, samplingMethod 1, every
//                                                row asked for.  Prints the median wall time of <reps> runs in ms and the points kept.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <vector>
#include "pgslam_amd/pgslam.hpp"

int main(int argc, char **argv)
{
    if (argc != 3) { std::fprintf(stderr, "usage: bench_elipsoids_host <cloud.bin> <reps>\n"); return 2; }
    typedef PointMatcher<float> PM;
    setenv("PGSLAM_HOST_ELIPSOIDS", "1", 1);
    std::ifstream in(argv[1], std::ios::binary);
    int n = 0;
    in.read((char *)&n, sizeof n);
    std::vector<float> xyz(3 * (size_t)n);
    in.read((char *)xyz.data(), sizeof(float) * xyz.size());
    if (!in.good() || n <= 0) { std::fprintf(stderr, "bench_elipsoids_host: cannot read %s\n", argv[1]); return 1; }
    const PM::DataPoints cloud = PM::DataPoints::fromXYZ(xyz.data(), n, nullptr);
    PM::ElipsoidsDataPointsFilter f(0.5f, 7, 1, std::numeric_limits<float>::infinity(), 0.0f, true, true, true, true, true, true, true, true, true, 1);
    std::vector<double> ms;
    unsigned kept = 0;
    for (int r = 0; r < std::atoi(argv[2]); r++) {
        PM::DataPoints c(cloud);
        const auto t0 = std::chrono::steady_clock::now();
        f.inPlaceFilter(c);
        ms.push_back(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
        kept = c.getNbPoints();
        if (f.ranOnDevice()) { std::fprintf(stderr, "bench_elipsoids_host: the filter ran on the device\n"); return 1; }
    }
    std::sort(ms.begin(), ms.end());
    std::printf("{\"points\": %d, \"kept\": %u, \"host_median_ms\": %.3f}\n", n, kept, ms[ms.size() / 2]);
    return 0;
}
