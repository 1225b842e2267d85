// [EXT] SamplingSurfaceNormalDataPointsFilter's further outputs through the C++ drop-in on the device:
//   the descriptors the filter appends -- labels, spans, row order, bytes -- against the direct call
//   (pgicp_sampling_surface_normal_ext_*), and the filter without the new rows against the older call;
//   the host form (PGSLAM_HOST_SAMPLING_NORMALS=1) against the device form, bit for bit;
//   a constructed SamplingSurfaceNormal{keepDensities} -> MaxDensity through DataPointsFilters::apply against the two steps by hand;
//   an ICPSequence whose referenceDataPointsFilters holds SamplingSurfaceNormal{keepEigenValues: 1} against the same chain without the
//   key: the same T bit for bit, and the map carries the row.
#include "common.hpp"
#include <cstring>
#include <sstream>

// the corner's coordinates, with `drows` descriptor rows d0, d1, ... of its own
template <typename T>
typename PointMatcher<T>::DataPoints bare_corner(int per_plane, unsigned long long seed, int drows = 0)
{
    typedef PointMatcher<T> PM;
    const typename PM::DataPoints c = make_corner<T>(per_plane, seed, 0.003);
    const int n = (int)c.getNbPoints();
    std::vector<T> xyz(3 * (size_t)n);
    for (int i = 0; i < n; i++) for (int a = 0; a < 3; a++) xyz[3 * (size_t)i + a] = c.features(a, i);
    typename PM::DataPoints out = PM::DataPoints::fromXYZ(xyz.data(), n, nullptr);
    Lcg g(seed + 7);
    for (int r = 0; r < drows; r++) {
        typename PM::Matrix d(1, n);
        for (int j = 0; j < n; j++) d(0, j) = (T)(g.next() - 0.5);
        out.addDescriptor("d" + std::to_string(r), d);
    }
    return out;
}

template <typename T>
bool same_cloud(const typename PointMatcher<T>::DataPoints &a, const typename PointMatcher<T>::DataPoints &b)
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
void run_descriptors(const char *name)
{
    typedef PointMatcher<T> PM;
    typedef typename PM::SamplingSurfaceNormalDataPointsFilter SSN;
    const int knn = 9;
    const T ratio = T(0.4), box = T(1.5);
    unsetenv("PGSLAM_HOST_SAMPLING_NORMALS");
    for (int method = 0; method < 2; method++)
        for (int drows = 0; drows <= 3; drows += 3) {
            const typename PM::DataPoints in = bare_corner<T>(700, 31, drows);
            const int n = (int)in.getNbPoints();
            typename PM::DataPoints c(in);
            SSN f(ratio, knn, method, box, true, true, 23, true, true, true);
            f.inPlaceFilter(c);
            CHECK(f.ranOnDevice());
            const int kept = (int)c.getNbPoints();
            CHECK(kept > 0 && kept < n);
            const char *names[4] = {"normals", "densities", "eigValues", "eigVectors"};
            const size_t spans[4] = {3, 1, 3, 9};
            CHECK((int)c.descriptorLabels.size() == drows + 4 && (int)c.descriptors.rows() == drows + 16);
            for (int k = 0; k < 4; k++) CHECK(c.descriptorLabels[drows + k].text == names[k] && c.descriptorLabels[drows + k].span == spans[k]);
            // the direct call, every output packed
            const size_t N = (size_t)n;
            std::vector<T> ox(3 * N), nrm(3 * N), od((size_t)(drows ? drows : 1) * N), eig(3 * N), vec(9 * N), dens(N);
            std::vector<int32_t> idx(N);
            int k2 = 0;
            pgslam_amd::LazyContext ctx;
            CHECK(pgslam_amd::Abi<T>::sampling_normals_ext(ctx, in.features.data(), (int)in.features.rows(), n, knn, (double)ratio, method, (double)box, 23,
                                                           drows ? in.descriptors.data() : nullptr, drows, 1, ox.data(), nrm.data(), drows ? od.data() : nullptr,
                                                           idx.data(), &k2, eig.data(), vec.data(), dens.data()) == PGICP_OK);
            CHECK(k2 == kept);
            const T *rows[4] = {nrm.data(), dens.data(), eig.data(), vec.data()};
            for (int k = 0; k < 4; k++) {
                const int r0 = c.getDescriptorStartingRow(names[k]);
                for (int i = 0; i < kept; i++)
                    for (size_t r = 0; r < spans[k]; r++) CHECK(std::memcmp(&c.descriptors(r0 + (int)r, i), &rows[k][(size_t)i * spans[k] + r], sizeof(T)) == 0);
            }
            for (int i = 0; i < kept; i++) {
                for (int r = 0; r < 3; r++) CHECK(std::memcmp(&c.features(r, i), &ox[3 * (size_t)i + r], sizeof(T)) == 0);
                for (int r = 0; r < drows; r++) CHECK(std::memcmp(&c.descriptors(r, i), &od[(size_t)i * drows + r], sizeof(T)) == 0);
                for (int r = 0; r < 3; r++) CHECK(vec[9 * (size_t)i + r] == nrm[3 * (size_t)i + r]);
                CHECK(eig[3 * (size_t)i] <= eig[3 * (size_t)i + 1] && eig[3 * (size_t)i + 1] <= eig[3 * (size_t)i + 2]);
                CHECK(std::isfinite((double)dens[i]) && dens[i] > T(0));
            }
            // the filter without the new rows leaves what the older call leaves, and those are the first rows of the above
            typename PM::DataPoints c7(in);
            SSN seven(ratio, knn, method, box, true, true, 23);
            seven.inPlaceFilter(c7);
            CHECK(seven.ranOnDevice() && (int)c7.getNbPoints() == kept && (int)c7.descriptors.rows() == drows + 3);
            for (int i = 0; i < kept; i++) {
                for (int r = 0; r < (int)c.features.rows(); r++) CHECK(std::memcmp(&c7.features(r, i), &c.features(r, i), sizeof(T)) == 0);
                for (int r = 0; r < drows + 3; r++) CHECK(std::memcmp(&c7.descriptors(r, i), &c.descriptors(r, i), sizeof(T)) == 0);
            }
            // the host form: the same DataPoints bit for bit
            setenv("PGSLAM_HOST_SAMPLING_NORMALS", "1", 1);
            typename PM::DataPoints h(in);
            SSN fh(ratio, knn, method, box, true, true, 23, true, true, true);
            fh.inPlaceFilter(h);
            unsetenv("PGSLAM_HOST_SAMPLING_NORMALS");
            CHECK(!fh.ranOnDevice());
            CHECK(same_cloud<T>(h, c));
        }
    std::printf("%s: ok  (labels, spans, order and bytes of four descriptors; host form == device form)\n", name);
}

template <typename T>
void run_max_density(const char *name)
{
    typedef PointMatcher<T> PM;
    typedef typename PM::SamplingSurfaceNormalDataPointsFilter SSN;
    typename PM::DataPoints chain = bare_corner<T>(1500, 33), hand = bare_corner<T>(1500, 33);
    // a density the boxes straddle: the median of the boxes' densities
    T max_density;
    {
        typename PM::DataPoints probe = bare_corner<T>(1500, 33);
        SSN s(T(0.9), 10, 0, std::numeric_limits<T>::infinity(), true, true, 3, true);
        s.inPlaceFilter(probe);
        const int r0 = probe.getDescriptorStartingRow("densities");
        std::vector<T> d;
        for (unsigned i = 0; i < probe.getNbPoints(); i++) d.push_back(probe.descriptors(r0, i));
        std::sort(d.begin(), d.end());
        max_density = d[d.size() / 2];
    }
    const unsigned n0 = chain.getNbPoints();
    typename PM::DataPointsFilters filters;
    filters.push_back(std::make_shared<SSN>(T(0.9), 10, 0, std::numeric_limits<T>::infinity(), true, true, 3, true));
    auto md = std::make_shared<typename PM::MaxDensityDataPointsFilter>(max_density, 5);
    filters.push_back(md);
    filters.apply(chain);
    SSN s(T(0.9), 10, 0, std::numeric_limits<T>::infinity(), true, true, 3, true);
    typename PM::MaxDensityDataPointsFilter md2(max_density, 5);
    s.inPlaceFilter(hand);
    const unsigned n1 = hand.getNbPoints();
    CHECK(s.ranOnDevice() && hand.descriptorExists("densities") && hand.getDescriptorDimension("densities") == 1);
    md2.inPlaceFilter(hand);
    CHECK(md->ranOnDevice() && md2.ranOnDevice());
    CHECK(chain.getNbPoints() > 0 && chain.getNbPoints() < n1 && n1 < n0);          // both filters dropped points and kept points
    CHECK(same_cloud<T>(chain, hand));
    CHECK(chain.descriptorLabels.size() == 2 && chain.descriptorLabels[0].text == "normals" && chain.descriptorLabels[1].text == "densities");
    std::printf("%s: ok  (%u of %u of %u points kept; chain == by hand)\n", name, chain.getNbPoints(), n1, n0);
}

#define SSN_ICP_YAML(EXTRA) \
    "readingDataPointsFilters:\n  - IdentityDataPointsFilter\n" \
    "referenceDataPointsFilters:\n  - SamplingSurfaceNormalDataPointsFilter:\n      knn: 10\n      ratio: 0.6\n      seed: 11\n" EXTRA PGSLAM_TEST_CHAIN_TAIL

template <typename T>
void run_icp(const char *name)
{
    IMPORT_PGSLAM_TYPES(T)
    typedef typename PM::SamplingSurfaceNormalDataPointsFilter SSN;
    TransformationPtr rigid = PM::get().REG(Transformation).create("RigidTransformation");
    const DP ref = bare_corner<T>(4000, 21);
    const Matrix truth = pose<T>(0.04, -0.03, 0.0, 0.02);
    const DP rd = rigid->compute(bare_corner<T>(4000, 22), truth.inverse());
    typename PM::ICPSequence with_key, without;
    { std::istringstream in(SSN_ICP_YAML("      keepEigenValues: 1\n")); with_key.loadFromYaml(in); }
    { std::istringstream in(SSN_ICP_YAML("")); without.loadFromYaml(in); }
    auto a = std::dynamic_pointer_cast<SSN>(with_key.referenceDataPointsFilters.at(0)), b = std::dynamic_pointer_cast<SSN>(without.referenceDataPointsFilters.at(0));
    CHECK(a && a->keepEigenValues && !a->keepEigenVectors && !a->keepDensities && a->knn == 10 && b && !b->wantsExt());
    with_key.setMap(ref);
    without.setMap(ref);
    CHECK(a->ranOnDevice() && b->ranOnDevice());
    const Matrix Ta = with_key(rd), Tb = without(rd);
    CHECK(Ta.rows() == 4 && Ta.cols() == 4 && std::memcmp(Ta.data(), Tb.data(), sizeof(T) * 16) == 0);
    {   // the plain ICP object (LoopCloser's call): reference filters inside operator()
        typename PM::ICP one, two;
        { std::istringstream in(SSN_ICP_YAML("      keepEigenValues: 1\n      keepEigenVectors: 1\n")); one.loadFromYaml(in); }
        { std::istringstream in(SSN_ICP_YAML("")); two.loadFromYaml(in); }
        const Matrix T1 = one(rd, ref), T2 = two(rd, ref);
        CHECK(std::memcmp(T1.data(), T2.data(), sizeof(T) * 16) == 0 && std::memcmp(T1.data(), Ta.data(), sizeof(T) * 16) == 0);
        CHECK(one.getPrefilteredReferencePtsCount() == two.getPrefilteredReferencePtsCount());
    }
    const DP &ma = with_key.getPrefilteredMap(), &mb = without.getPrefilteredMap();
    CHECK(ma.getNbPoints() == mb.getNbPoints() && ma.getNbPoints() > 0 && ma.getNbPoints() < ref.getNbPoints());
    CHECK(ma.descriptorLabels.size() == 2 && ma.descriptorLabels[1].text == "eigValues" && ma.descriptorLabels[1].span == 3 && ma.descriptors.rows() == 6);
    CHECK(mb.descriptorLabels.size() == 1 && mb.descriptors.rows() == 3);
    for (unsigned i = 0; i < ma.getNbPoints(); i++) {
        for (int r = 0; r < 3; r++) CHECK(std::memcmp(&ma.descriptors(r, i), &mb.descriptors(r, i), sizeof(T)) == 0);
        for (int r = 0; r < (int)ma.features.rows(); r++) CHECK(std::memcmp(&ma.features(r, i), &mb.features(r, i), sizeof(T)) == 0);
        CHECK(ma.descriptors(3, i) <= ma.descriptors(4, i) && ma.descriptors(4, i) <= ma.descriptors(5, i) && ma.descriptors(5, i) > T(0));
    }
    const Matrix d = truth.inverse() * Ta;
    const double dt = std::sqrt((double)(d(0, 3) * d(0, 3) + d(1, 3) * d(1, 3) + d(2, 3) * d(2, 3)));
    CHECK(dt < 0.02);
    std::printf("%s: ok  (the same T bit for bit, the map carries eigValues, |dt| %.2e m)\n", name, dt);
}

int main()
{
    run_descriptors<float>("SamplingSurfaceNormal<float>, four descriptors");
    run_descriptors<double>("SamplingSurfaceNormal<double>, four descriptors");
    run_max_density<float>("SamplingSurfaceNormal{keepDensities} -> MaxDensity <float>");
    run_max_density<double>("SamplingSurfaceNormal{keepDensities} -> MaxDensity <double>");
    run_icp<float>("ICPSequence<float>, reference chain [SamplingSurfaceNormal{keepEigenValues}]");
    run_icp<double>("ICPSequence<double>, reference chain [SamplingSurfaceNormal{keepEigenValues}]");
    std::puts("sampling normals ext gpu tests ok");
    return 0;
}
