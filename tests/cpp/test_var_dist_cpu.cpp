// [EXT] KDTreeVarDistMatcher in the C++ drop-in, without a device: the YAML loads, members and defaults; maxDist and any other
// unknown key are refused by name; the message for an unknown matcher names both matchers.
#include "common.hpp"
#include <sstream>

#define VD_TAIL \
    "outlierFilters:\n  - TrimmedDistOutlierFilter:\n      ratio: 0.85\n" \
    "errorMinimizer:\n  PointToPlaneErrorMinimizer\n"

template <typename T>
void run(const char *name)
{
    using PM = PointMatcher<T>;
    {   // defaults
        typename PM::ICP icp;
        std::istringstream in("matcher:\n  KDTreeVarDistMatcher\n" VD_TAIL);
        icp.loadFromYaml(in);
        auto vd = std::dynamic_pointer_cast<typename PM::KDTreeVarDistMatcher>(icp.matcher);
        CHECK(vd);
        CHECK(vd->maxDistField == "maxSearchDist" && vd->knn == 1 && vd->epsilon == T(0) && vd->perPointRadii());
    }
    {   // every parameter
        typename PM::ICP icp;
        std::istringstream in("matcher:\n  KDTreeVarDistMatcher:\n    knn: 3\n    epsilon: 0.5\n    searchType: 1\n    maxDistField: gate\n" VD_TAIL);
        icp.loadFromYaml(in);
        auto vd = std::dynamic_pointer_cast<typename PM::KDTreeVarDistMatcher>(icp.matcher);
        CHECK(vd && vd->maxDistField == "gate" && vd->knn == 3 && vd->epsilon == T(0.5));
        // the other matcher still loads, and is not this one
        std::istringstream kd("matcher:\n  KDTreeMatcher:\n    knn: 2\n    maxDist: 1.5\n" VD_TAIL);
        icp.loadFromYaml(kd);
        CHECK(!std::dynamic_pointer_cast<typename PM::KDTreeVarDistMatcher>(icp.matcher));
        CHECK(icp.matcher->knn == 2 && icp.matcher->maxDist == T(1.5) && !icp.matcher->perPointRadii());
    }
    for (const char *key : {"maxDist", "radius", "maxDistfield"}) {
        typename PM::ICP icp;
        std::istringstream in(std::string("matcher:\n  KDTreeVarDistMatcher:\n    knn: 1\n    ") + key + ": 2.0\n" VD_TAIL);
        std::string what;
        try { icp.loadFromYaml(in); } catch (const std::runtime_error &e) { what = e.what(); }
        CHECK(what == std::string("KDTreeVarDistMatcher: unknown parameter ") + key);
    }
    {
        typename PM::ICP icp;
        std::istringstream in("matcher:\n  NullMatcher\n" VD_TAIL);
        std::string what;
        try { icp.loadFromYaml(in); } catch (const std::runtime_error &e) { what = e.what(); }
        CHECK(what.find("unsupported matcher NullMatcher") != std::string::npos);
        CHECK(what.find("KDTreeMatcher") != std::string::npos && what.find("KDTreeVarDistMatcher") != std::string::npos);
    }
    std::printf("%s: ok\n", name);
}

int main()
{
    run<float>("KDTreeVarDistMatcher YAML <float>");
    run<double>("KDTreeVarDistMatcher YAML <double>");
    std::puts("var dist cpu tests ok");
    return 0;
}
