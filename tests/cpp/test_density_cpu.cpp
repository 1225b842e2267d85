// [EXT] MaxDensityDataPointsFilter through the C++ drop-in without a device (tests/test_density_host.py drives it):
//   apply <f32|f64> <in> <out>   the filter on a cloud that carries the given `densities` row: the kept points' first feature row
//                                (the test stores the point's index there), the onDevice flag, whether the filter refused;
//   refuse                       the refusal without a `densities` descriptor, and YAML loading.
// With PGSLAM_HOST_MAX_DENSITY=1 the host loop is forced; without a device it is taken anyway.
#include "common.hpp"
#include <cstring>
#include <fstream>

template <typename T>
int apply(const char *fin, const char *fout)
{
    typedef PointMatcher<T> PM;
    std::ifstream in(fin, std::ios::binary);
    int n = 0;
    double max_density = 0, seed = 0;
    in.read((char *)&n, sizeof n);
    in.read((char *)&max_density, sizeof max_density);
    in.read((char *)&seed, sizeof seed);
    std::vector<T> dens((size_t)n);
    in.read((char *)dens.data(), sizeof(T) * (size_t)n);
    CHECK(in.good() || n == 0);
    typename PM::DataPoints c;
    c.features = typename PM::Matrix(4, n);
    for (int i = 0; i < n; i++) { c.features(0, i) = (T)i; c.features(1, i) = 0; c.features(2, i) = 0; c.features(3, i) = 1; }
    typename PM::Matrix own(2, n), d(1, n);
    for (int i = 0; i < n; i++) { own(0, i) = (T)(2 * i); own(1, i) = (T)(-i); d(0, i) = dens[(size_t)i]; }
    c.addDescriptor("own", own);
    c.addDescriptor("densities", d);
    char yaml[256];
    std::snprintf(yaml, sizeof yaml, "- MaxDensityDataPointsFilter:\n    maxDensity: %.17g\n    seed: %.17g\n", max_density, seed);
    std::istringstream ys(yaml);
    typename PM::DataPointsFilters filters(ys);
    auto md = std::dynamic_pointer_cast<typename PM::MaxDensityDataPointsFilter>(filters.at(0));
    CHECK(md);
    int refused = 0;
    try { filters.apply(c); } catch (const std::exception &) { refused = 1; }
    const int m = (int)c.features.cols(), dev = md->onDevice ? 1 : 0;
    // the descriptors travel with their points
    for (int o = 0; o < m && !refused; o++) {
        const int i = (int)c.features(0, o);
        CHECK(c.descriptors(0, o) == (T)(2 * i) && c.descriptors(1, o) == (T)(-i));
        CHECK(std::memcmp(&c.descriptors(2, o), &dens[(size_t)i], sizeof(T)) == 0);
    }
    std::ofstream out(fout, std::ios::binary);
    out.write((const char *)&m, sizeof m);
    out.write((const char *)&dev, sizeof dev);
    out.write((const char *)&refused, sizeof refused);
    for (int o = 0; o < m; o++) { const int i = (int)c.features(0, o); out.write((const char *)&i, sizeof i); }
    return 0;
}

template <typename T>
void refuse()
{
    typedef PointMatcher<T> PM;
    const typename PM::DataPoints base = make_corner<T>(50, 3);
    typename PM::DataPoints c(base.features, base.featureLabels);
    typename PM::MaxDensityDataPointsFilter md((T)100, 1);
    bool threw = false;
    try { md.inPlaceFilter(c); } catch (const std::runtime_error &e) { threw = std::string(e.what()).find("no densities found") != std::string::npos; }
    CHECK(threw && !md.onDevice && !md.ranOnDevice());
    CHECK(c.getNbPoints() == base.getNbPoints());
    // through a list: MaxDensity first in the list is not the fused pattern either
    std::istringstream ys("- MaxDensityDataPointsFilter:\n    maxDensity: 100\n");
    typename PM::DataPointsFilters filters(ys);
    threw = false;
    try { filters.apply(c); } catch (const std::runtime_error &) { threw = true; }
    CHECK(threw);
    for (const char *bad : {"- MaxDensityDataPointsFilter:\n    maxDensity: 0\n", "- MaxDensityDataPointsFilter:\n    seed: 9007199254740992\n"}) {
        std::istringstream bs(bad);
        threw = false;
        try { typename PM::DataPointsFilters f(bs); } catch (const std::runtime_error &) { threw = true; }
        CHECK(threw);
    }
    // an empty cloud with the descriptor: nothing to do
    typename PM::DataPoints e;
    e.features = typename PM::Matrix(4, 0);
    e.descriptors = typename PM::Matrix(1, 0);
    e.descriptorLabels.push_back(typename PM::DataPoints::Label("densities", 1));
    md.inPlaceFilter(e);
    CHECK(e.getNbPoints() == 0 && !md.onDevice);
}

int main(int argc, char **argv)
{
    if (argc == 5 && std::strcmp(argv[1], "apply") == 0)
        return std::strcmp(argv[2], "f32") == 0 ? apply<float>(argv[3], argv[4]) : apply<double>(argv[3], argv[4]);
    if (argc == 2 && std::strcmp(argv[1], "refuse") == 0) {
        refuse<float>();
        refuse<double>();
        std::puts("density cpu tests ok");
        return 0;
    }
    std::fprintf(stderr, "usage: test_density_cpu apply <f32|f64> <in> <out> | refuse\n");
    return 2;
}
