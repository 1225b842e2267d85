// [EXT] ElipsoidsDataPointsFilter through the C++ drop-in on the device (tests/test_cpp_elipsoids.py drives it):
//   the device form (ranOnDevice() true) against the host form (PGSLAM_HOST_ELIPSOIDS=1, ranOnDevice() false), bit for bit, from the
//   constructor and from YAML -- every row and a sparse subset, both sampling methods, with and without descriptors of the cloud's
//   own, with and without a planarity threshold that some boxes pass and some do not;
//   test_elipsoids_gpu <scans> <minPlanarity>: besides, one ICP whose referenceDataPointsFilters is this filter (keepNormals: 1,
//   samplingMethod 1, the given minPlanarity) with the point-to-plane minimiser on the two scans of <scans>: int32 n_reading,
//   n_reference, 16 doubles T_init, 16 doubles T_truth (row-major), the reading's and the reference's points as floats; the pose must
//   end within 0.02 m of the truth (the bound of the SamplingSurfaceNormal end-to-end test, tests/cpp/test_sampling_normals_ext_gpu.cpp).
#include "common.hpp"
#include <cstring>
#include <fstream>
#include <sstream>

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

// a planarity the boxes of `in` straddle: the median of the kept points' planarities (samplingMethod 1: one point a box)
template <typename T>
T median_planarity(const typename PointMatcher<T>::DataPoints &in, int knn)
{
    typedef PointMatcher<T> PM;
    typename PM::DataPoints probe(in);
    typename PM::ElipsoidsDataPointsFilter f(T(0.5), knn, 1, std::numeric_limits<T>::infinity(), T(0), true, false, false, false, false, false, false, false, true, 1);
    f.inPlaceFilter(probe);
    const int r0 = probe.getDescriptorStartingRow("shapes");
    std::vector<T> p;
    for (unsigned i = 0; i < probe.getNbPoints(); i++) p.push_back(probe.descriptors(r0, i));
    std::sort(p.begin(), p.end());
    CHECK(p.size() > 4 && p.front() < p.back());
    return p[p.size() / 2];
}

template <typename T>
void run_forms(const char *name)
{
    typedef PointMatcher<T> PM;
    typedef typename PM::ElipsoidsDataPointsFilter EL;
    const int knn = 9;
    const T ratio = T(0.4), box = T(1.5), inf = std::numeric_limits<T>::infinity();
    unsetenv("PGSLAM_HOST_ELIPSOIDS");
    int runs = 0;
    for (int method = 0; method < 2; method++)
        for (int drows = 0; drows <= 3; drows += 3) {
            const typename PM::DataPoints in = bare_corner<T>(700, 31, drows);
            const int n = (int)in.getNbPoints();
            const T thr = median_planarity<T>(in, knn);
            for (int form = 0; form < 3; form++) {
                // 0: every row; 1: a sparse subset without normals; 2: every row and the planarity threshold
                const bool all = form != 1;
                const T minp = form == 2 ? thr : T(0);
                auto make = [&]() {
                    return std::make_shared<EL>(ratio, knn, method, box, minp, true, all, all, true, all, all, true, all, true, 23);
                };
                typename PM::DataPoints c(in), h(in), y(in);
                auto fd = make();
                fd->inPlaceFilter(c);
                CHECK(fd->ranOnDevice());
                const int kept = (int)c.getNbPoints();
                CHECK(kept > 0 && kept < n);
                const int rows = all ? 32 : 7, labels = all ? 8 : 3;
                CHECK((int)c.descriptorLabels.size() == drows + labels && (int)c.descriptors.rows() == drows + rows);
                CHECK(c.descriptorLabels[drows].text == (all ? "normals" : "eigValues") && c.descriptorLabels.back().text == "shapes");
                // the host form: the same DataPoints bit for bit
                setenv("PGSLAM_HOST_ELIPSOIDS", "1", 1);
                auto fh = make();
                fh->inPlaceFilter(h);
                unsetenv("PGSLAM_HOST_ELIPSOIDS");
                CHECK(!fh->ranOnDevice());
                CHECK(same_cloud<T>(h, c));
                // from YAML: the same filter, the same DataPoints
                std::ostringstream ys;
                ys.precision(17);
                ys << "- ElipsoidsDataPointsFilter:\n    ratio: " << (double)ratio << "\n    knn: " << knn << "\n    samplingMethod: " << method
                   << "\n    maxBoxDim: " << (double)box << "\n    minPlanarity: " << (double)minp << "\n    seed: 23\n    keepNormals: " << (all ? 1 : 0)
                   << "\n    keepDensities: " << (all ? 1 : 0) << "\n    keepEigenValues: 1\n    keepEigenVectors: " << (all ? 1 : 0)
                   << "\n    keepCovariances: " << (all ? 1 : 0) << "\n    keepWeights: 1\n    keepMeans: " << (all ? 1 : 0) << "\n    keepShapes: 1\n";
                std::istringstream yin(ys.str());
                typename PM::DataPointsFilters filters(yin);
                auto fy = std::dynamic_pointer_cast<EL>(filters.at(0));
                CHECK(fy && fy->minPlanarity == minp && fy->ratio == ratio && fy->maxBoxDim == box);
                filters.apply(y);
                CHECK(fy->ranOnDevice());
                CHECK(same_cloud<T>(y, c));
                if (form == 2) {
                    // the threshold dropped some boxes and kept others; every kept point's planarity passes it
                    typename PM::DataPoints z(in);
                    EL zero(ratio, knn, method, box, T(0), true, true, true, true, true, true, true, true, true, 23);
                    zero.inPlaceFilter(z);
                    CHECK(zero.ranOnDevice() && kept < (int)z.getNbPoints());
                    const int r0 = c.getDescriptorStartingRow("shapes");
                    for (int i = 0; i < kept; i++) CHECK(!(c.descriptors(r0, i) < thr));
                }
                runs++;
            }
        }
    {   // an argument the device refuses (knn beyond its range) falls back to the host recursion
        typename PM::DataPoints c = bare_corner<T>(700, 31);
        EL f(T(0.5), 2000, 1, inf, T(0), true, true, false, false, false, false, true, false, true, 1);
        f.inPlaceFilter(c);
        CHECK(!f.ranOnDevice() && c.getNbPoints() > 0 && c.descriptorExists("weights"));
    }
    std::printf("%s: ok  (%d runs: device form == host form == from YAML, bit for bit)\n", name, runs);
}

// The chain of the end-to-end run.  The checkers stop well below the bound that is asserted: a differential checker that lets the
// iteration end while it still moves 0.01 m a step (the other tests' chain) cannot promise 0.02 m from a start 0.4 m away.
static const char *kElipIcpYaml =
    "readingDataPointsFilters:\n  - IdentityDataPointsFilter\n"
    "referenceDataPointsFilters:\n  - ElipsoidsDataPointsFilter:\n      knn: 7\n      samplingMethod: 1\n      keepNormals: 1\n      keepWeights: 1\n"
    "      minPlanarity: %s\n"
    "matcher:\n  KDTreeMatcher:\n    knn: 1\n    epsilon: 0\n    maxDist: 2.0\n"
    "outlierFilters:\n  - TrimmedDistOutlierFilter:\n      ratio: 0.85\n"
    "errorMinimizer:\n  PointToPlaneErrorMinimizer\n"
    "transformationCheckers:\n  - CounterTransformationChecker:\n      maxIterationCount: 40\n"
    "  - DifferentialTransformationChecker:\n      minDiffRotErr: 0.0001\n      minDiffTransErr: 0.001\n      smoothLength: 3\n"
    "inspector:\n  NullInspector\nlogger:\n  NullLogger\n";

void run_icp(const char *path, const char *min_planarity)
{
    typedef float T;
    IMPORT_PGSLAM_TYPES(T)
    typedef PM::ElipsoidsDataPointsFilter EL;
    std::ifstream in(path, std::ios::binary);
    int n[2] = {0, 0};
    double Ti[16], Tt[16];
    in.read((char *)n, sizeof n); in.read((char *)Ti, sizeof Ti); in.read((char *)Tt, sizeof Tt);
    std::vector<float> rd(3 * (size_t)n[0]), rf(3 * (size_t)n[1]);
    in.read((char *)rd.data(), sizeof(float) * rd.size());
    in.read((char *)rf.data(), sizeof(float) * rf.size());
    CHECK(in.good() && n[0] > 0 && n[1] > 0);
    const DP reading = DP::fromXYZ(rd.data(), n[0], nullptr), reference = DP::fromXYZ(rf.data(), n[1], nullptr);
    Matrix init(4, 4), truth(4, 4);
    for (int r = 0; r < 4; r++) for (int c = 0; c < 4; c++) { init(r, c) = (T)Ti[4 * r + c]; truth(r, c) = (T)Tt[4 * r + c]; }
    PM::ICP icp;
    {
        std::vector<char> text(std::strlen(kElipIcpYaml) + std::strlen(min_planarity) + 1);
        std::snprintf(text.data(), text.size(), kElipIcpYaml, min_planarity);
        std::istringstream ys(text.data());
        icp.loadFromYaml(ys);
    }
    auto f = std::dynamic_pointer_cast<EL>(icp.referenceDataPointsFilters.at(0));
    CHECK(f && f->keepNormals && f->keepWeights && f->samplingMethod == 1 && f->knn == 7 && f->minPlanarity == (T)std::atof(min_planarity));
    const Matrix Tf = icp(reading, reference, init);
    CHECK(f->ranOnDevice());
    CHECK(icp.getPrefilteredReferencePtsCount() > 0 && (int)icp.getPrefilteredReferencePtsCount() < n[1]);
    const Matrix d = truth.inverse() * Tf, d0 = truth.inverse() * init;
    const double dt = std::sqrt((double)(d(0, 3) * d(0, 3) + d(1, 3) * d(1, 3) + d(2, 3) * d(2, 3)));
    const double dt0 = std::sqrt((double)(d0(0, 3) * d0(0, 3) + d0(1, 3) * d0(1, 3) + d0(2, 3) * d0(2, 3)));
    std::printf("ICP<float>, reference chain [Elipsoids{keepNormals, samplingMethod 1, minPlanarity %s}]: %d of %d reference points, |dt| %.3e m (from %.3e m)\n",
                min_planarity, (int)icp.getPrefilteredReferencePtsCount(), n[1], dt, dt0);
    CHECK(dt < 0.02);
}

int main(int argc, char **argv)
{
    run_forms<float>("Elipsoids<float>");
    run_forms<double>("Elipsoids<double>");
    if (argc == 3) run_icp(argv[1], argv[2]);
    std::puts("elipsoids gpu tests ok");
    return 0;
}
