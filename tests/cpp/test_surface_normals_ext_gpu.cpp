// [EXT] SurfaceNormalDataPointsFilter's further outputs through the C++ drop-in on the device:
//   the descriptors the filter appends -- labels, spans, row order, bytes -- against the direct call (pgicp_surface_normals_ext_*);
//   SurfaceNormal{keepDensities, keepEigenVectors} -> MaxDensity through DataPointsFilters::apply against the same two filters applied
//   by hand, bit for bit, and its old rows against the fused pair's;
//   an ICP object whose referenceDataPointsFilters holds SurfaceNormal{smoothNormals: 1} against the same chain fed a reference that
//   already carries the direct call's normals: the same T, bit for bit.
#include "common.hpp"
#include <cstring>

// the corner's coordinates alone: a cloud that carries no descriptor yet
template <typename T>
typename PointMatcher<T>::DataPoints bare_corner(int per_plane, unsigned long long seed, const T *normals = nullptr)
{
    const typename PointMatcher<T>::DataPoints c = make_corner<T>(per_plane, seed, 0.003);
    const int n = (int)c.getNbPoints();
    std::vector<T> xyz(3 * (size_t)n);
    for (int i = 0; i < n; i++) for (int a = 0; a < 3; a++) xyz[3 * (size_t)i + a] = c.features(a, i);
    return PointMatcher<T>::DataPoints::fromXYZ(xyz.data(), n, normals);
}

template <typename T>
bool same_cloud(const typename PointMatcher<T>::DataPoints &a, const typename PointMatcher<T>::DataPoints &b)
{
    if (a.features.rows() != b.features.rows() || a.features.cols() != b.features.cols() || a.descriptors.rows() != b.descriptors.rows() ||
        a.descriptors.cols() != b.descriptors.cols() || a.descriptorLabels.size() != b.descriptorLabels.size())
        return false;
    for (size_t k = 0; k < a.descriptorLabels.size(); k++)
        if (a.descriptorLabels[k].text != b.descriptorLabels[k].text || a.descriptorLabels[k].span != b.descriptorLabels[k].span) return false;
    return std::memcmp(a.features.data(), b.features.data(), sizeof(T) * (size_t)a.features.rows() * a.features.cols()) == 0 &&
           std::memcmp(a.descriptors.data(), b.descriptors.data(), sizeof(T) * (size_t)a.descriptors.rows() * a.descriptors.cols()) == 0;
}

template <typename T>
void run_descriptors(const char *name)
{
    typedef PointMatcher<T> PM;
    const int knn = 9;
    const double md = 0.25;
    for (int smooth = 0; smooth < 2; smooth++) {
        typename PM::DataPoints c = bare_corner<T>(700, 31);
        const int n = (int)c.getNbPoints();
        typename PM::SurfaceNormalDataPointsFilter sn(knn, (T)md, true, true, true, true, true, true, smooth != 0);
        sn.inPlaceFilter(c);
        const char *names[6] = {"normals", "densities", "eigValues", "eigVectors", "matchedIds", "meanDists"};
        const size_t spans[6] = {3, 1, 3, 9, (size_t)knn, 1};
        CHECK(c.descriptorLabels.size() == 6 && c.descriptors.rows() == 17 + knn && (int)c.descriptors.cols() == n);
        for (int k = 0; k < 6; k++) CHECK(c.descriptorLabels[k].text == names[k] && c.descriptorLabels[k].span == spans[k]);
        // the direct call, every output packed
        const size_t N = (size_t)n;
        std::vector<T> nrm(3 * N), eig(3 * N), vec(9 * N), dist(N), mids(N * knn), d2(N * knn), dens(N);
        std::vector<int32_t> ids(N * knn);
        pgslam_amd::LazyContext ctx;
        CHECK(pgslam_amd::pick<T>(pgicp_surface_normals_ext_f32, pgicp_surface_normals_ext_f64)(
                  ctx, c.features.data(), (int)c.features.rows(), n, PGICP_HOST, knn, md, smooth, nrm.data(), 3, eig.data(), vec.data(), dist.data(),
                  mids.data(), ids.data(), d2.data(), dens.data()) == PGICP_OK);
        const T *rows[6] = {nrm.data(), dens.data(), eig.data(), vec.data(), mids.data(), dist.data()};
        int short_lists = 0;
        for (int k = 0; k < 6; k++) {
            const int r0 = c.getDescriptorStartingRow(names[k]);
            for (int i = 0; i < n; i++)
                for (size_t r = 0; r < spans[k]; r++) CHECK(std::memcmp(&c.descriptors(r0 + (int)r, i), &rows[k][(size_t)i * spans[k] + r], sizeof(T)) == 0);
        }
        for (size_t k = 0; k < N * knn; k++) { CHECK(mids[k] == (T)ids[k]); short_lists += ids[k] < 0; }
        CHECK(short_lists > 0);                        // maxDist bites: some lists are padded
        // the old rows are the old calls' rows (smoothing apart)
        std::vector<T> nrm0(3 * N), eig0(3 * N), dens0(N);
        CHECK(pgslam_amd::Abi<T>::densities(ctx, c.features.data(), (int)c.features.rows(), n, knn, md, nrm0.data(), 3, eig0.data(), dens0.data()) == PGICP_OK);
        CHECK(eig0 == eig && std::memcmp(dens0.data(), dens.data(), sizeof(T) * N) == 0);
        CHECK((nrm0 == nrm) == (smooth == 0));
        for (int i = 0; i < n; i++) for (int a = 0; a < 3; a++) CHECK(vec[9 * (size_t)i + a] == nrm0[3 * (size_t)i + a]);     // eigVectors stay raw
    }
    std::printf("%s: ok  (labels, spans, order and bytes of six descriptors, raw and smoothed)\n", name);
}

template <typename T>
void run_max_density(const char *name)
{
    typedef PointMatcher<T> PM;
    const T max_density = T(150);
    typename PM::DataPoints chain = bare_corner<T>(1500, 33), hand = bare_corner<T>(1500, 33), fused = bare_corner<T>(1500, 33);
    const unsigned n0 = chain.getNbPoints();
    typename PM::DataPointsFilters filters;
    filters.push_back(std::make_shared<typename PM::SurfaceNormalDataPointsFilter>(10, std::numeric_limits<T>::infinity(), true, false, true, true));
    auto md = std::make_shared<typename PM::MaxDensityDataPointsFilter>(max_density, 5);
    filters.push_back(md);
    filters.apply(chain);
    typename PM::SurfaceNormalDataPointsFilter sn(10, std::numeric_limits<T>::infinity(), true, false, true, true);
    typename PM::MaxDensityDataPointsFilter md2(max_density, 5);
    sn.inPlaceFilter(hand);
    md2.inPlaceFilter(hand);
    CHECK(md->ranOnDevice() && md2.ranOnDevice());
    CHECK(chain.getNbPoints() > 0 && chain.getNbPoints() < n0);          // the filter dropped points and kept points
    CHECK(same_cloud<T>(chain, hand));
    CHECK(chain.descriptorLabels.size() == 3 && chain.descriptorLabels[2].text == "eigVectors" && chain.descriptorLabels[2].span == 9);
    // the pair without the new row fuses; its rows are the unfused pair's old rows, bit for bit
    typename PM::DataPointsFilters old;
    old.push_back(std::make_shared<typename PM::SurfaceNormalDataPointsFilter>(10, std::numeric_limits<T>::infinity(), true, false, true));
    old.push_back(std::make_shared<typename PM::MaxDensityDataPointsFilter>(max_density, 5));
    old.apply(fused);
    CHECK(fused.getNbPoints() == chain.getNbPoints() && fused.descriptors.rows() == 4 && chain.descriptors.rows() == 13);
    for (unsigned i = 0; i < fused.getNbPoints(); i++) {
        for (int r = 0; r < 4; r++) CHECK(std::memcmp(&fused.features(r, i), &chain.features(r, i), sizeof(T)) == 0);
        for (int r = 0; r < 4; r++) CHECK(std::memcmp(&fused.descriptors(r, i), &chain.descriptors(r, i), sizeof(T)) == 0);
    }
    std::printf("%s: ok  (%u of %u points kept; chain == by hand; old rows == the fused pair's)\n", name, chain.getNbPoints(), n0);
}

static const char *kSmoothIcpYaml =
    "readingDataPointsFilters:\n  - IdentityDataPointsFilter\n"
    "referenceDataPointsFilters:\n  - SurfaceNormalDataPointsFilter:\n      knn: 10\n      smoothNormals: 1\n" PGSLAM_TEST_CHAIN_TAIL;

template <typename T>
void run_icp(const char *name)
{
    IMPORT_PGSLAM_TYPES(T)
    TransformationPtr rigid = PM::get().REG(Transformation).create("RigidTransformation");
    const DP ref = bare_corner<T>(4000, 21);
    const int n = (int)ref.getNbPoints();
    const Matrix truth = pose<T>(0.04, -0.03, 0.0, 0.02);
    const DP rd = rigid->compute(bare_corner<T>(4000, 22), truth.inverse());
    typename PM::ICP with_filter, fed;
    { std::istringstream in(kSmoothIcpYaml); with_filter.loadFromYaml(in); }
    { std::istringstream in(kIcpYaml); fed.loadFromYaml(in); }
    auto sn = std::dynamic_pointer_cast<typename PM::SurfaceNormalDataPointsFilter>(with_filter.referenceDataPointsFilters.at(0));
    CHECK(sn && sn->smoothNormals && sn->knn == 10 && fed.referenceDataPointsFilters.empty());
    const Matrix a = with_filter(rd, ref);
    // the direct call's smoothed normals, carried by the reference
    std::vector<T> nrm(3 * (size_t)n), raw(3 * (size_t)n);
    pgslam_amd::LazyContext ctx;
    CHECK(pgslam_amd::Abi<T>::normals_ext(ctx, ref.features.data(), (int)ref.features.rows(), n, 10, 1e300, 1, nrm.data(), 3, nullptr, nullptr, nullptr, nullptr, nullptr) == PGICP_OK);
    CHECK(pgslam_amd::Abi<T>::normals(ctx, ref.features.data(), (int)ref.features.rows(), n, 10, 1e300, raw.data(), 3, nullptr) == PGICP_OK);
    CHECK(nrm != raw);                                 // smoothing changed something
    DP ref_n(ref);
    Matrix nm(3, n);
    for (int i = 0; i < n; i++) for (int r = 0; r < 3; r++) nm(r, i) = nrm[3 * (size_t)i + r];
    ref_n.addDescriptor("normals", nm);
    const Matrix b = fed(rd, ref_n);
    CHECK(a.rows() == 4 && a.cols() == 4 && std::memcmp(a.data(), b.data(), sizeof(T) * 16) == 0);
    const Matrix d = truth.inverse() * a;
    const double dt = std::sqrt((double)(d(0, 3) * d(0, 3) + d(1, 3) * d(1, 3) + d(2, 3) * d(2, 3)));
    CHECK(dt < 0.02);
    std::printf("%s: ok  (the same T bit for bit, |dt| %.2e m)\n", name, dt);
}

int main()
{
    run_descriptors<float>("SurfaceNormal<float>, six descriptors");
    run_descriptors<double>("SurfaceNormal<double>, six descriptors");
    run_max_density<float>("SurfaceNormal{keepDensities, keepEigenVectors} -> MaxDensity <float>");
    run_max_density<double>("SurfaceNormal{keepDensities, keepEigenVectors} -> MaxDensity <double>");
    run_icp<float>("ICP<float>, reference chain [SurfaceNormal{smoothNormals}]");
    run_icp<double>("ICP<double>, reference chain [SurfaceNormal{smoothNormals}]");
    std::puts("surface normals ext gpu tests ok");
    return 0;
}
