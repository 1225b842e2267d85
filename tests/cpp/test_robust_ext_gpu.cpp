// [EXT] RobustOutlierFilter's distanceType, berg and nbIterationForScale through the C++ drop-in on the device (the filter built in
// code: a YAML names upstream's defaults only): one ICP::operator()
// equals the C calls -- pgicp_set_params + pgicp_set_robust_ext + pgicp_align on a context of its own -- bit for bit; the object's
// context carries the setting and a chain without such settings takes it out again; the filter's own compute() is the stage-level
// call: berg's first scale, and point2plane refused.
#include "common.hpp"
#include <cstring>
#include <sstream>

#define RX_CHAIN(robust) \
    "matcher:\n  KDTreeMatcher:\n    knn: 1\n    maxDist: 1.0\n" \
    "outlierFilters:\n  - RobustOutlierFilter:\n" robust \
    "errorMinimizer:\n  PointToPlaneWithCovErrorMinimizer:\n    sensorStdDev: 0.01\n" \
    "transformationCheckers:\n  - CounterTransformationChecker:\n      maxIterationCount: 30\n" \
    "  - DifferentialTransformationChecker:\n      minDiffRotErr: 0.001\n      minDiffTransErr: 0.01\n      smoothLength: 3\n" \
    "inspector:\n  NullInspector\nlogger:\n  NullLogger\n"
// (the chain's other slots; its robust filter is replaced in code)
static const char *kBaseYaml = RX_CHAIN("      robustFct: cauchy\n      tuning: 0.05\n      approximation: 3.0\n");
static const char *kPlainYaml = RX_CHAIN("      robustFct: cauchy\n      tuning: 2.0\n      scaleEstimator: mad\n      approximation: 3.0\n");

// the chain of kBaseYaml with cauchy / tuning 0.05 / approximation 3 and the given settings of include/pgicp_robust.h
template <typename T, typename ICP_>
void load_ext(ICP_ &icp, const char *scale, const char *dist, int nb)
{
    std::istringstream in(kBaseYaml);
    icp.loadFromYaml(in);
    icp.outlierFilters[0] = std::make_shared<typename PointMatcher<T>::RobustOutlierFilter>(&icp, "cauchy", T(0.05), scale, T(3), dist, nb);
}

template <typename T>
void run(const char *name)
{
    IMPORT_PGSLAM_TYPES(T)
    using A = pgslam_amd::Abi<T>;
    TransformationPtr rigid = PM::get().REG(Transformation).create("RigidTransformation");
    const DP ref = make_corner<T>(1500, 21, 0.004);
    const Matrix truth = pose<T>(0.12, -0.08, 0.02, 0.03);
    const DP rd = rigid->compute(make_corner<T>(1500, 22, 0.004), truth.inverse());
    const int n = (int)rd.getNbPoints(), m = (int)ref.getNbPoints();
    double Ti[16], To[16];
    pgslam_amd::to_row_major16(Matrix(Matrix::Identity(4, 4)), Ti);

    typename PM::ICP icp;
    load_ext<T>(icp, "berg", "point2plane", 3);
    const Matrix Tres = icp(rd, ref);
    int on = 0;
    pgicp_robust_ext got;
    PM::check(icp.ctx, pgicp_get_robust_ext(icp.ctx, &on, &got));
    CHECK(on == 1 && got.distance_type == PGICP_ROBUST_DIST_POINT2PLANE && got.scale_estimator == PGICP_ROBUST_SCALE_BERG && got.nb_iteration_for_scale == 3);
    pgicp_params prm;
    PM::check(icp.ctx, pgicp_get_params(icp.ctx, &prm));
    CHECK(prm.robust_fct == PGICP_ROBUST_CAUCHY && prm.robust_tuning == (double)T(0.05) && prm.robust_approx == 3.0);

    // the same through the C ABI alone, on a context of its own
    pgicp_ctx *c = nullptr;
    CHECK(pgicp_ctx_create(0, &c) == PGICP_OK);
    PM::check(c, pgicp_set_params(c, &prm));
    const pgicp_robust_ext x = {PGICP_ROBUST_DIST_POINT2PLANE, PGICP_ROBUST_SCALE_BERG, 3};
    PM::check(c, pgicp_set_robust_ext(c, &x));
    int id = -1;
    PM::check(c, A::map_create(c, ref.xyzPtr(), ref.xyzStride(), ref.normalsPtr(), (int)ref.descriptors.rows(), m, 1, &id));
    pgicp_stats st;
    PM::check(c, A::align(c, id, rd.xyzPtr(), rd.xyzStride(), n, Ti, To, &st));
    const Matrix Tc = pgslam_amd::from_row_major16<T>(To);
    for (int i = 0; i < 4; i++) for (int j = 0; j < 4; j++) CHECK(std::memcmp(&Tres(i, j), &Tc(i, j), sizeof(T)) == 0);
    CHECK(st.iterations > 3 && st.converged);                              // (iterations beyond nb: the scale was held)
    CHECK(st.iterations == icp.lastStats.iterations && st.n_kept == icp.lastStats.n_kept);
    CHECK(std::memcmp(&st.residual, &icp.lastStats.residual, sizeof(double)) == 0 && std::memcmp(st.cov, icp.lastStats.cov, sizeof st.cov) == 0);
    // ... and without the setting the C context computes something else: the setting is what made the two agree
    PM::check(c, pgicp_set_robust_ext(c, nullptr));
    double To2[16];
    PM::check(c, A::align(c, id, rd.xyzPtr(), rd.xyzStride(), n, Ti, To2, &st));
    CHECK(std::memcmp(To, To2, sizeof To) != 0);
    const Matrix d = truth.inverse() * Tres;
    const double dt = std::sqrt((double)(d(0, 3) * d(0, 3) + d(1, 3) * d(1, 3) + d(2, 3) * d(2, 3)));
    CHECK(dt < 0.02);

    {   // the filter's own compute(): the stage-level call -- berg's first scale over the distances handed in
        typename PM::ICP stage;
        load_ext<T>(stage, "berg", "point2point", 3);
        typename PM::Matches mt(1, 5);
        const T d2[5] = {T(0.01), T(0.0625), T(0.25), T(0.04), T(0.09)};         // median 0.0625: s = T(1.9) * 0.25
        for (int j = 0; j < 5; j++) { mt.dists(0, j) = d2[j]; mt.ids(0, j) = j; }
        const typename PM::OutlierWeights w = stage.outlierFilters[0]->compute(rd, ref, mt);
        const T s = T(1.9) * T(0.25), s2 = s * s;
        for (int j = 0; j < 5; j++) {
            const T e2 = d2[j] / s2, want = T(1) / (T(1) + e2 / (T(1) * T(1)));
            CHECK(std::memcmp(&w(0, j), &want, sizeof(T)) == 0);
        }
        // point2plane: a bare array of distances has no planes
        load_ext<T>(stage, "berg", "point2plane", 3);
        bool thrown = false;
        try { stage.outlierFilters[0]->compute(rd, ref, mt); } catch (const std::runtime_error &e) { thrown = std::string(e.what()).find("no geometry") != std::string::npos; }
        CHECK(thrown);
    }
    {   // a chain without such settings takes the setting out of the same object's context
        std::istringstream inp(kPlainYaml);
        icp.loadFromYaml(inp);
        const Matrix Tp = icp(rd, ref);
        PM::check(icp.ctx, pgicp_get_robust_ext(icp.ctx, &on, &got));
        CHECK(on == 0);
        typename PM::ICP fresh;
        std::istringstream inf(kPlainYaml);
        fresh.loadFromYaml(inf);
        const Matrix Tf = fresh(rd, ref);
        for (int i = 0; i < 4; i++) for (int j = 0; j < 4; j++) CHECK(std::memcmp(&Tp(i, j), &Tf(i, j), sizeof(T)) == 0);
    }
    pgicp_ctx_destroy(c);
    std::printf("%s: ok  (%d iterations, |dt| %.2e m)\n", name, icp.lastStats.iterations, dt);
}

int main()
{
    run<float>("RobustOutlierFilter ext <float>");
    run<double>("RobustOutlierFilter ext <double>");
    std::puts("robust ext gpu tests ok");
    return 0;
}
