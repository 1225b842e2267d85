// [EXT] RobustOutlierFilter's distanceType, berg and nbIterationForScale in the C++ drop-in, without a device: the constructor takes
// each new setting and says what pgicp_set_robust_ext will be handed; scaleEstimator std, an
// unknown distanceType and a negative count are refused with the module's name in the message; a YAML keeps naming upstream's
// defaults only (the three settings are refused there by name, std and an unknown key too); point2plane against a reference
// without normals throws DataPoints::InvalidField before anything is built.
#include "common.hpp"
#include <limits>
#include <sstream>

#define RX_HEAD "matcher:\n  KDTreeMatcher:\n    knn: 1\n    maxDist: 1.0\noutlierFilters:\n  - RobustOutlierFilter:\n"
#define RX_TAIL(minimiser) "errorMinimizer:\n  " minimiser "\n"

template <typename PM>
std::shared_ptr<typename PM::RobustOutlierFilter> load(typename PM::ICP &icp, const std::string &params, const char *tail = RX_TAIL("PointToPlaneErrorMinimizer"))
{
    std::istringstream in(std::string(RX_HEAD) + params + tail);
    icp.loadFromYaml(in);
    CHECK(icp.outlierFilters.size() == 1);
    return std::dynamic_pointer_cast<typename PM::RobustOutlierFilter>(icp.outlierFilters[0]);
}

template <typename F>
std::string what_of(F f)
{
    try { f(); } catch (const std::runtime_error &e) { return e.what(); }
    return "";
}

template <typename T>
void run(const char *name)
{
    using PM = PointMatcher<T>;
    using RB = typename PM::RobustOutlierFilter;
    const T inf = std::numeric_limits<T>::infinity();
    {   // a YAML chain: the filter as it was, and nothing for pgicp_set_robust_ext to say
        typename PM::ICP icp;
        auto rb = load<PM>(icp, "      robustFct: cauchy\n");
        CHECK(rb && rb->distanceType == "point2point" && rb->scaleEstimator == "mad" && rb->nbIterationForScale == 0 && rb->asksNothing());
        CHECK(!icp.robustNeedsNormals());
        // each new setting on its own, through the constructor
        icp.outlierFilters[0] = std::make_shared<RB>(&icp, "tukey", T(1), "mad", inf, "point2plane");
        rb = std::dynamic_pointer_cast<RB>(icp.outlierFilters[0]);
        CHECK(rb->distCode() == PGICP_ROBUST_DIST_POINT2PLANE && !rb->asksNothing() && icp.robustNeedsNormals());
        icp.outlierFilters[0] = std::make_shared<RB>(&icp, "tukey", T(1), "mad", inf, "point2point", 3);
        rb = std::dynamic_pointer_cast<RB>(icp.outlierFilters[0]);
        CHECK(rb->nbIterationForScale == 3 && rb->distCode() == PGICP_ROBUST_DIST_POINT2POINT && !rb->asksNothing() && !icp.robustNeedsNormals());
        icp.outlierFilters[0] = std::make_shared<RB>(&icp, "cauchy", T(0.3), "berg");
        rb = std::dynamic_pointer_cast<RB>(icp.outlierFilters[0]);
        CHECK(rb->scaleCode() == PGICP_ROBUST_SCALE_BERG && !rb->asksNothing());
        CHECK(rb->tuning == T(0.3));                                     // (berg: what pgicp_params.robust_tuning carries is the target scale)
        pgicp_robust_ext x = rb->ext();
        CHECK(x.distance_type == 0 && x.scale_estimator == 2 && x.nb_iteration_for_scale == 0);
        // all of them, the usual robust point-to-plane chain
        RB all(&icp, "cauchy", T(0.2), "berg", T(2.5), "point2plane", 4);
        x = all.ext();
        CHECK(x.distance_type == PGICP_ROBUST_DIST_POINT2PLANE && x.scale_estimator == PGICP_ROBUST_SCALE_BERG && x.nb_iteration_for_scale == 4);
        CHECK(all.tuning == T(0.2) && all.approximation == T(2.5) && all.fctCode() == PGICP_ROBUST_CAUCHY);
    }
    {   // the constructor's refusals carry the module's name
        typename PM::ICP icp;
        std::string what = what_of([&] { RB f(&icp, "cauchy", T(1), "std"); });
        CHECK(what.find("RobustOutlierFilter") != std::string::npos && what.find("std") != std::string::npos && what.find("not offered") != std::string::npos);
        what = what_of([&] { RB f(&icp, "cauchy", T(1), "sigma"); });
        CHECK(what.find("RobustOutlierFilter") != std::string::npos && what.find("sigma") != std::string::npos);
        what = what_of([&] { RB f(&icp, "cauchy", T(1), "mad", inf, "point2line"); });
        CHECK(what.find("RobustOutlierFilter: unknown distanceType point2line") != std::string::npos);
        what = what_of([&] { RB f(&icp, "cauchy", T(1), "mad", inf, "point2point", -1); });
        CHECK(what.find("RobustOutlierFilter: nbIterationForScale") != std::string::npos);
    }
    {   // a YAML names upstream's defaults only: the three settings, std and an unknown key are refused by name
        typename PM::ICP icp;
        for (const char *key : {"distanceType: point2plane", "nbIterationForScale: 3", "scaleEstimator: berg", "scaleEstimator: std"}) {
            const std::string what = what_of([&] { load<PM>(icp, std::string("      ") + key + "\n"); });
            const std::string k(key);
            CHECK(what.find("RobustOutlierFilter") != std::string::npos && what.find(k.substr(0, k.find(':'))) != std::string::npos);
        }
        CHECK(what_of([&] { load<PM>(icp, "      nbIterationsForScale: 2\n"); }) == "RobustOutlierFilter: unknown parameter nbIterationsForScale");
        CHECK(load<PM>(icp, "      distanceType: point2point\n      nbIterationForScale: 0\n      scaleEstimator: none\n")->asksNothing());
    }
    {   // point2plane reads the reference's normals whatever the minimiser: a reference without them is an InvalidField
        typename PM::ICP icp;
        load<PM>(icp, "      robustFct: cauchy\n", RX_TAIL("PointToPointErrorMinimizer"));
        icp.outlierFilters[0] = std::make_shared<RB>(&icp, "cauchy", T(1), "mad", inf, "point2plane");
        const typename PM::DataPoints with = make_corner<T>(200, 3);
        const typename PM::DataPoints bare = PM::DataPoints::fromXYZ(with.xyzPtr(), (int)with.getNbPoints());
        CHECK(!bare.descriptorExists("normals"));
        bool thrown = false;
        try { icp(with, bare); } catch (const typename PM::DataPoints::InvalidField &e) {
            thrown = std::string(e.what()).find("RobustOutlierFilter") != std::string::npos && std::string(e.what()).find("normals") != std::string::npos;
        }
        CHECK(thrown);
        typename PM::ICPSequence seq;
        std::istringstream in(std::string(RX_HEAD) + "      robustFct: cauchy\n" + RX_TAIL("PointToPointErrorMinimizer"));
        seq.loadFromYaml(in);
        seq.outlierFilters[0] = std::make_shared<RB>(&seq, "cauchy", T(1), "mad", inf, "point2plane");
        thrown = false;
        try { seq.setMap(bare); } catch (const typename PM::DataPoints::InvalidField &) { thrown = true; }
        CHECK(thrown);
    }
    std::printf("%s: ok\n", name);
}

int main()
{
    run<float>("RobustOutlierFilter settings <float>");
    run<double>("RobustOutlierFilter settings <double>");
    std::puts("robust ext cpu tests ok");
    return 0;
}
