// [EXT] CovarianceSamplingDataPointsFilter through the C++ drop-in without a device (tests/test_covariance_sampling_host.py
// drives it):
//   apply <f32|f64> <in> <out>    the filter's host form on the cloud of <in> (n, nbSample, torqueNorm, xyz, normals): the frame it
//                                 computed and its picks;
//   framed <f32|f64> <in>         the host form's picks given the frame of <in> against the picks of <in> (the reference's);
//   yaml                          YAML acceptance, each refusal, the no-normals throw, the nbSample >= n no-op.
// With PGSLAM_HOST_INPUT_STAGE=1 the host form is forced; without a device it is taken anyway.
#include "common.hpp"
#include <cstring>
#include <fstream>

template <typename T>
typename PointMatcher<T>::DataPoints read_cloud(std::ifstream &in, int &nb, int &tn)
{
    typedef PointMatcher<T> PM;
    int n = 0;
    in.read((char *)&n, sizeof n);
    in.read((char *)&nb, sizeof nb);
    in.read((char *)&tn, sizeof tn);
    std::vector<T> xyz(3 * (size_t)n), nrm(3 * (size_t)n);
    in.read((char *)xyz.data(), sizeof(T) * xyz.size());
    in.read((char *)nrm.data(), sizeof(T) * nrm.size());
    CHECK(in.good());
    typename PM::DataPoints c = PM::DataPoints::fromXYZ(xyz.data(), n, nrm.data());
    typename PM::Matrix own(1, n);
    for (int i = 0; i < n; i++) own(0, i) = (T)i;
    c.addDescriptor("own", own);
    return c;
}

template <typename T>
int apply(const char *fin, const char *fout)
{
    typedef PointMatcher<T> PM;
    std::ifstream in(fin, std::ios::binary);
    int nb = 0, tn = 0;
    typename PM::DataPoints c = read_cloud<T>(in, nb, tn);
    const typename PM::DataPoints before(c);
    char yaml[256];
    std::snprintf(yaml, sizeof yaml, "- CovarianceSamplingDataPointsFilter:\n    nbSample: %d\n    torqueNorm: %d\n", nb, tn);
    std::istringstream ys(yaml);
    typename PM::DataPointsFilters filters(ys);
    auto cs = std::dynamic_pointer_cast<typename PM::CovarianceSamplingDataPointsFilter>(filters.at(0));
    CHECK(cs && cs->nbSample == (size_t)nb && (int)cs->normalizationMethod == tn);
    filters.apply(c);
    CHECK(!cs->ranOnDevice());
    const int m = (int)c.features.cols(), ro = c.getDescriptorStartingRow("own"), rn = c.getDescriptorStartingRow("normals");
    std::ofstream out(fout, std::ios::binary);
    out.write((const char *)&m, sizeof m);
    out.write((const char *)&cs->lastFrame, sizeof cs->lastFrame);
    for (int o = 0; o < m; o++) {
        const int i = (int)c.descriptors(ro, o);
        // every row travels with its point
        for (int r = 0; r < 4; r++) CHECK(std::memcmp(&c.features(r, o), &before.features(r, i), sizeof(T)) == 0);
        for (int r = 0; r < 3; r++) CHECK(std::memcmp(&c.descriptors(rn + r, o), &before.descriptors(rn + r, i), sizeof(T)) == 0);
        out.write((const char *)&i, sizeof i);
    }
    return 0;
}

template <typename T>
int framed(const char *fin)
{
    typedef PointMatcher<T> PM;
    std::ifstream in(fin, std::ios::binary);
    int nb = 0, tn = 0;
    const typename PM::DataPoints c = read_cloud<T>(in, nb, tn);
    pgicp_cov_frame frame;
    in.read((char *)&frame, sizeof frame);
    std::vector<int32_t> want((size_t)nb), got;
    in.read((char *)want.data(), sizeof(int32_t) * want.size());
    CHECK(in.good());
    typename PM::CovarianceSamplingDataPointsFilter cs((size_t)nb, tn);
    cs.hostPicks(c, frame, got);
    CHECK(got.size() == want.size());
    for (size_t j = 0; j < want.size(); j++)
        if (got[j] != want[j]) { std::fprintf(stderr, "pick %zu: %d, the reference has %d\n", j, got[j], want[j]); return 1; }
    return 0;
}

template <typename T>
void yaml()
{
    typedef PointMatcher<T> PM;
    {
        std::istringstream ys("- CovarianceSamplingDataPointsFilter\n");
        typename PM::DataPointsFilters f(ys);
        auto cs = std::dynamic_pointer_cast<typename PM::CovarianceSamplingDataPointsFilter>(f.at(0));
        CHECK(cs && cs->nbSample == 5000 && cs->normalizationMethod == PM::CovarianceSamplingDataPointsFilter::Lavg);
        pgicp_filter spec;
        CHECK(!cs->deviceSpec(spec));
        std::vector<pgicp_filter> specs;
        CHECK(!f.deviceSpecs(specs));                 // the one-pass device input stage says no to a chain that holds it
    }
    for (const char *bad : {"- CovarianceSamplingDataPointsFilter:\n    nbSample: 0\n", "- CovarianceSamplingDataPointsFilter:\n    nbSample: -3\n",
                            "- CovarianceSamplingDataPointsFilter:\n    torqueNorm: 3\n", "- CovarianceSamplingDataPointsFilter:\n    torqueNorm: -1\n",
                            "- CovarianceSamplingDataPointsFilter:\n    nbSample: 10.5\n", "- CovarianceSamplingDataPointsFilter:\n    nbSamples: 10\n"}) {
        std::istringstream bs(bad);
        bool threw = false;
        try { typename PM::DataPointsFilters f(bs); } catch (const std::runtime_error &) { threw = true; }
        CHECK(threw);
    }
    {   // the name is among the supported ones of the refusal message
        std::istringstream bs("- OctreeGridDataPointsFilter\n");
        bool named = false;
        try { typename PM::DataPointsFilters f(bs); } catch (const std::runtime_error &e) { named = std::string(e.what()).find("CovarianceSampling") != std::string::npos; }
        CHECK(named);
    }
    const typename PM::DataPoints base = make_corner<T>(50, 3);
    {   // no normals: upstream's InvalidField
        typename PM::DataPoints c(base.features, base.featureLabels);
        typename PM::CovarianceSamplingDataPointsFilter cs(10, 1);
        bool threw = false;
        try { cs.inPlaceFilter(c); } catch (const std::runtime_error &e) { threw = std::string(e.what()).find("cannot find normals") != std::string::npos; }
        CHECK(threw && !cs.ranOnDevice() && c.getNbPoints() == base.getNbPoints());
    }
    for (size_t nb : {(size_t)base.getNbPoints(), (size_t)base.getNbPoints() + 7}) {   // nbSample >= n: the cloud as it is
        typename PM::DataPoints c(base);
        typename PM::CovarianceSamplingDataPointsFilter cs(nb, 2);
        cs.inPlaceFilter(c);
        CHECK(!cs.ranOnDevice() && c.getNbPoints() == base.getNbPoints());
        CHECK(std::memcmp(c.features.data(), base.features.data(), sizeof(T) * 4 * base.getNbPoints()) == 0);
        CHECK(std::memcmp(c.descriptors.data(), base.descriptors.data(), sizeof(T) * 3 * base.getNbPoints()) == 0);
    }
}

int main(int argc, char **argv)
{
    const bool f32 = argc > 2 && std::strcmp(argv[2], "f32") == 0;
    if (argc == 5 && std::strcmp(argv[1], "apply") == 0) return f32 ? apply<float>(argv[3], argv[4]) : apply<double>(argv[3], argv[4]);
    if (argc == 4 && std::strcmp(argv[1], "framed") == 0) return f32 ? framed<float>(argv[3]) : framed<double>(argv[3]);
    if (argc == 2 && std::strcmp(argv[1], "yaml") == 0) {
        yaml<float>();
        yaml<double>();
        std::puts("covariance sampling cpu tests ok");
        return 0;
    }
    std::fprintf(stderr, "usage: test_covariance_sampling_cpu apply <f32|f64> <in> <out> | framed <f32|f64> <in> | yaml\n");
    return 2;
}
