// MaxQuantileOnAxis' host statement (include/pgslam_amd/axis_quantile_host.hpp) alone, with no library behind it: the program a
// sanitizer build runs (g++ -fsanitize=address,undefined) and tests/test_axis_quantile_host.py compares with the numpy reference.
//   axis_quantile_host_main <f32|f64> <in> <out>
// <in>: the groups of tests/axis_quantile_ref.py (write_groups); <out>: per group and ratio the limit (T), k, below, the kept count
// (int32) and the kept indices.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <vector>
#include "pgslam_amd/axis_quantile_host.hpp"

template <typename T>
int run(const char *fin, const char *fout)
{
    namespace aq = pgslam_amd::axis_quantile;
    std::ifstream in(fin, std::ios::binary);
    std::ofstream out(fout, std::ios::binary);
    int32_t groups = 0;
    in.read((char *)&groups, sizeof groups);
    if (!in.good() || groups < 0) return 1;
    long scenes = 0;
    for (int g = 0; g < groups; g++) {
        int32_t n = 0, dim = 0, nr = 0;
        in.read((char *)&n, sizeof n); in.read((char *)&dim, sizeof dim); in.read((char *)&nr, sizeof nr);
        if (!in.good() || n < 0 || dim < 0 || dim > 2 || nr < 0) return 1;
        std::vector<double> ratios((size_t)nr);
        in.read((char *)ratios.data(), sizeof(double) * ratios.size());
        std::vector<T> f(4 * (size_t)n);
        in.read((char *)f.data(), sizeof(T) * f.size());
        if (!in.good()) return 1;
        for (double ratio : ratios) {
            if (!aq::dim_ok(dim) || !aq::ratio_ok(ratio)) return 1;
            const aq::Result<T> r = aq::select<T>(f.data() + dim, 4, n, (T)ratio);
            const std::vector<int> keep = aq::kept_indices<T>(f.data() + dim, 4, n, (T)ratio);
            if ((int)keep.size() != r.below) return 1;
            const int32_t k = r.k, below = r.below, kept = (int32_t)keep.size();
            out.write((const char *)&r.limit, sizeof(T));
            out.write((const char *)&k, sizeof k); out.write((const char *)&below, sizeof below); out.write((const char *)&kept, sizeof kept);
            out.write((const char *)keep.data(), sizeof(int32_t) * keep.size());
            scenes++;
        }
    }
    // the empty cloud: nothing happens
    const aq::Result<T> e = aq::select<T>(nullptr, 4, 0, (T)0.5);
    if (e.limit == e.limit || e.k != 0 || e.below != 0 || !aq::kept_indices<T>(nullptr, 4, 0, (T)0.5).empty()) return 1;
    std::printf("axis quantile host statement ok (%ld scenes)\n", scenes);
    return out.good() ? 0 : 1;
}

int main(int argc, char **argv)
{
    if (argc != 4) { std::fprintf(stderr, "usage: axis_quantile_host_main <f32|f64> <in> <out>\n"); return 2; }
    return std::strcmp(argv[1], "f32") == 0 ? run<float>(argv[2], argv[3]) : run<double>(argv[2], argv[3]);
}
