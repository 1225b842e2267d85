// [EXT] SurfaceNormalDataPointsFilter{keepDensities} -> MaxDensityDataPointsFilter through the C++ drop-in on the device
// (include/pgicp_density.h).  From YAML, as float and as double, on a cloud that carries a descriptor row of its own, four ways:
//   fused      the pair as DataPointsFilters::apply finds it: one pgicp_normals_max_density_* call;
//   unfused    an IdentityDataPointsFilter between the two: pgicp_surface_densities_*, then pgicp_max_density_*;
//   knob       PGSLAM_HOST_MAX_DENSITY=1: the device's densities, the filter's host loop;
//   restated   the host arithmetic the drop-in had before the device form, written out here from the neighbour ids.
// The four leave the same features and the same descriptors by name, bit for bit; then an ICP runs against the filtered reference.
#include "common.hpp"
#include <cstring>

static void host_knob(bool on) { if (on) setenv("PGSLAM_HOST_MAX_DENSITY", "1", 1); else unsetenv("PGSLAM_HOST_MAX_DENSITY"); }

static std::string chain_yaml(int knn, double max_density, bool identity_between, const char *indent = "")
{
    char buf[512];
    std::snprintf(buf, sizeof buf,
                  "%s- SurfaceNormalDataPointsFilter:\n%s    knn: %d\n%s    keepDensities: 1\n%s    keepEigenValues: 1\n%s"
                  "%s- MaxDensityDataPointsFilter:\n%s    maxDensity: %.9g\n%s    seed: 7\n",
                  indent, indent, knn, indent, indent, identity_between ? (std::string(indent) + "- IdentityDataPointsFilter\n").c_str() : "",
                  indent, indent, max_density, indent);
    return buf;
}

template <typename T>
typename PointMatcher<T>::DataPoints make_cloud(int per_plane, unsigned long long seed)
{
    typedef PointMatcher<T> PM;
    const typename PM::DataPoints base = make_corner<T>(per_plane, seed, 0.003);
    typename PM::DataPoints c(base.features, base.featureLabels);           // (no normals: the chain makes them)
    const int n = (int)c.features.cols();
    typename PM::Matrix own(1, n);
    Lcg g(seed + 99);
    for (int i = 0; i < n; i++) own(0, i) = (T)(100.0 * g.next());
    c.addDescriptor("intensity", own);
    return c;
}

template <typename T>
bool same_bits(const pgslam_amd::Mat<T> &a, const pgslam_amd::Mat<T> &b)
{
    return a.rows() == b.rows() && a.cols() == b.cols() && (a.size() == 0 || std::memcmp(a.data(), b.data(), sizeof(T) * a.size()) == 0);
}

template <typename T>
void same_cloud(const typename PointMatcher<T>::DataPoints &a, const typename PointMatcher<T>::DataPoints &b)
{
    CHECK(same_bits<T>(a.features, b.features));
    CHECK(a.descriptorLabels.size() == b.descriptorLabels.size());
    for (size_t k = 0; k < a.descriptorLabels.size(); k++) {
        CHECK(a.descriptorLabels[k] == b.descriptorLabels[k]);
        CHECK(same_bits<T>(a.getDescriptorViewByName(a.descriptorLabels[k].text), b.getDescriptorViewByName(a.descriptorLabels[k].text)));
    }
}

// the drop-in's host arithmetic before the device form: densities from the neighbour ids, then MaxDensity's three passes
template <typename T>
typename PointMatcher<T>::DataPoints restated(const typename PointMatcher<T>::DataPoints &in, int knn, T maxDensity, unsigned long long seed)
{
    typedef PointMatcher<T> PM;
    typename PM::DataPoints c(in);
    const int n = (int)c.features.cols();
    typename PM::Matrix nrm(3, n), eig(3, n), dens(1, n);
    std::vector<int32_t> ids((size_t)n * knn);
    pgicp_ctx *ctx = pgslam_amd::default_context();
    PM::check(ctx, pgslam_amd::Abi<T>::normals_ids(ctx, c.features.data(), (int)c.features.rows(), n, knn, 1e300, nrm.data(), 3, eig.data(), ids.data()));
    for (int i = 0; i < n; i++) {
        const int32_t *nb = ids.data() + (size_t)i * knn;
        int cnt = 0;
        T sx = 0, sy = 0, sz = 0;
        for (int j = 0; j < knn; j++) if (nb[j] >= 0) { sx += c.features(0, nb[j]); sy += c.features(1, nb[j]); sz += c.features(2, nb[j]); cnt++; }
        T r2 = 0;
        if (cnt > 0) {
            const T mx = sx / (T)cnt, my = sy / (T)cnt, mz = sz / (T)cnt;
            for (int j = 0; j < knn; j++) if (nb[j] >= 0) {
                const T dx = c.features(0, nb[j]) - mx, dy = c.features(1, nb[j]) - my, dz = c.features(2, nb[j]) - mz;
                const T q = (dx * dx + dy * dy) + dz * dz;
                if (q > r2) r2 = q;
            }
        }
        const T r = std::sqrt(r2);
        dens(0, i) = (T)cnt / ((T)((4.0 / 3.0) * 3.14159265358979323846) * ((r * r) * r));
    }
    c.setDescriptor("normals", nrm);
    c.setDescriptor("densities", dens);
    c.setDescriptor("eigValues", eig);
    const int rd = c.getDescriptorStartingRow("densities");
    T last = c.descriptors(rd, 0);
    for (int i = 1; i < n; i++) if (c.descriptors(rd, i) > last) last = c.descriptors(rd, i);
    int saturated = 0;
    for (int i = 0; i < n; i++) saturated += c.descriptors(rd, i) == last;
    PM::compactColumns(c, [&](int j) {
        const T density = c.descriptors(rd, j);
        if (!(density > maxDensity)) return true;
        float accept = (float)(maxDensity / density);
        if (density == last) accept = accept * (float)(1 - saturated / n);
        return (double)(PM::RandomSamplingDataPointsFilter::mix(seed * 0x100000001B3ULL + (unsigned long long)j) >> 11) / 9007199254740992.0 < (double)accept;
    });
    return c;
}

template <typename T>
void run(const char *name)
{
    IMPORT_PGSLAM_TYPES(T)
    const int knn = 10;
    const double max_density = 150.0;
    const DP cloud = make_cloud<T>(1500, 31);
    const unsigned n = cloud.getNbPoints();
    DP out[3];
    for (int way = 0; way < 3; way++) {                // 0 fused, 1 unfused, 2 the knob
        host_knob(way == 2);
        std::istringstream in(chain_yaml(knn, max_density, way == 1));
        typename PM::DataPointsFilters filters(in);
        CHECK(filters.size() == (way == 1 ? 3u : 2u));
        auto md = std::dynamic_pointer_cast<typename PM::MaxDensityDataPointsFilter>(filters.back());
        CHECK(md);
        out[way] = cloud;
        filters.apply(out[way]);
        CHECK(md->onDevice == (way != 2));
        CHECK(md->ranOnDevice() == (way != 2));
    }
    host_knob(false);
    const DP ref = restated<T>(cloud, knn, (T)max_density, 7);
    CHECK(ref.getNbPoints() > 0 && ref.getNbPoints() < n);                 // the filter drops some points, not all
    CHECK(ref.descriptorLabels.size() == 4 && ref.descriptorLabels[0].text == "intensity" && ref.descriptorLabels[1].text == "normals" &&
          ref.descriptorLabels[2].text == "densities" && ref.descriptorLabels[3].text == "eigValues");
    for (int way = 0; way < 3; way++) same_cloud<T>(out[way], ref);

    // an ICP against the filtered reference: the chain as the reference filters of an ICP object, fused and with the knob
    TransformationPtr rigid = PM::get().REG(Transformation).create("RigidTransformation");
    const Matrix truth = pose<T>(0.04, -0.03, 0.0, 0.02);
    const DP rd = rigid->compute(make_corner<T>(1500, 32, 0.003), truth.inverse());
    const DP ref_in(cloud.features, cloud.featureLabels);
    Matrix res[2];
    for (int host = 0; host < 2; host++) {
        host_knob(host);
        typename PM::ICP icp;
        std::istringstream in("readingDataPointsFilters:\n  - IdentityDataPointsFilter\nreferenceDataPointsFilters:\n" + chain_yaml(knn, max_density, false, "  ") +
                              PGSLAM_TEST_CHAIN_TAIL);
        icp.loadFromYaml(in);
        auto md = std::dynamic_pointer_cast<typename PM::MaxDensityDataPointsFilter>(icp.referenceDataPointsFilters.at(1));
        CHECK(md);
        res[host] = icp(rd, ref_in);
        CHECK(md->onDevice == !host);
    }
    host_knob(false);
    CHECK(pose_diff(res[0], res[1]) == 0.0);
    const Matrix d = truth.inverse() * res[0];
    const double dt = std::sqrt((double)(d(0, 3) * d(0, 3) + d(1, 3) * d(1, 3) + d(2, 3) * d(2, 3)));
    CHECK(dt < 0.02);
    std::printf("%s: ok  (%u of %u points kept; fused == unfused == knob == restated; ICP |dt| %.2e m)\n", name, ref.getNbPoints(), n, dt);
}

int main()
{
    run<float>("DataPointsFilters<float>, SurfaceNormal{keepDensities} -> MaxDensity");
    run<double>("DataPointsFilters<double>, SurfaceNormal{keepDensities} -> MaxDensity");
    std::puts("density gpu tests ok");
    return 0;
}
