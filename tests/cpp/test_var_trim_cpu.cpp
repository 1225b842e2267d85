// CPU-only checks of [EXT] VarTrimmedDistOutlierFilter in the C++ drop-in (no device needed): loadFromYaml accepts it with the
// members upstream spells, refuses what the statement refuses (include/pgicp.h, pgicp_set_var_trim), and lets it share the
// chain with MaxDist and SurfaceNormal outlier filters but not with a second quantile or robust filter.
#include "common.hpp"
#include <string>

template <typename T>
void var_trim_yaml()
{
    using PM = PointMatcher<T>;
    const std::string head = "matcher:\n  KDTreeMatcher:\n    knn: 1\noutlierFilters:\n";
    auto load = [&](typename PM::ICP &icp, const std::string &filters) {
        std::istringstream in(head + filters);
        icp.loadFromYaml(in);
    };
    auto refused = [&](const std::string &filters) {
        typename PM::ICP icp;
        try { load(icp, filters); } catch (const std::runtime_error &) { return true; }
        return false;
    };
    {
        typename PM::ICP icp;
        load(icp, "  - VarTrimmedDistOutlierFilter:\n      minRatio: 0.3\n      maxRatio: 0.95\n      lambda: 2.0\n");
        CHECK(icp.outlierFilters.size() == 1);
        auto vt = std::dynamic_pointer_cast<typename PM::VarTrimmedDistOutlierFilter>(icp.outlierFilters[0]);
        CHECK(vt && vt->minRatio == T(0.3) && vt->maxRatio == T(0.95) && vt->lambda == T(2.0));
    }
    {   // beside MaxDist and SurfaceNormal: the weights multiply
        typename PM::ICP icp;
        load(icp, "  - MaxDistOutlierFilter:\n      maxDist: 1.0\n"
                  "  - VarTrimmedDistOutlierFilter:\n      minRatio: 0.5\n      maxRatio: 1.0\n      lambda: 0\n"
                  "  - SurfaceNormalOutlierFilter:\n      maxAngle: 0.7\n");
        CHECK(icp.outlierFilters.size() == 3);
        auto vt = std::dynamic_pointer_cast<typename PM::VarTrimmedDistOutlierFilter>(icp.outlierFilters[1]);
        CHECK(vt && vt->minRatio == T(0.5) && vt->maxRatio == T(1.0) && vt->lambda == T(0));
    }
    const std::string ok = "  - VarTrimmedDistOutlierFilter:\n      minRatio: 0.3\n      maxRatio: 0.95\n      lambda: 2.0\n";
    // every parameter explicit
    CHECK(refused("  - VarTrimmedDistOutlierFilter:\n      maxRatio: 0.95\n      lambda: 2.0\n"));
    CHECK(refused("  - VarTrimmedDistOutlierFilter:\n      minRatio: 0.3\n      lambda: 2.0\n"));
    CHECK(refused("  - VarTrimmedDistOutlierFilter:\n      minRatio: 0.3\n      maxRatio: 0.95\n"));
    {   // the message names the missing key
        typename PM::ICP icp;
        std::string msg;
        try { load(icp, "  - VarTrimmedDistOutlierFilter:\n      minRatio: 0.3\n      maxRatio: 0.95\n"); } catch (const std::runtime_error &e) { msg = e.what(); }
        CHECK(msg.find("lambda") != std::string::npos);
    }
    CHECK(refused("  - VarTrimmedDistOutlierFilter:\n      minRatio: 0.3\n      maxRatio: 0.95\n      lambda: 2.0\n      ratio: 0.8\n"));
    // 0 < minRatio < maxRatio <= 1
    for (const char *r : {"      minRatio: 0\n      maxRatio: 0.9\n", "      minRatio: -0.1\n      maxRatio: 0.9\n",
                          "      minRatio: 0.5\n      maxRatio: 0.5\n", "      minRatio: 0.6\n      maxRatio: 0.5\n",
                          "      minRatio: 0.3\n      maxRatio: 1.1\n"})
        CHECK(refused(std::string("  - VarTrimmedDistOutlierFilter:\n") + r + "      lambda: 1\n"));
    // lambda finite and >= 0
    for (const char *l : {"-1", "inf", "nan"})
        CHECK(refused(std::string("  - VarTrimmedDistOutlierFilter:\n      minRatio: 0.3\n      maxRatio: 0.9\n      lambda: ") + l + "\n"));
    // one quantile / robust filter per chain
    CHECK(refused(ok + "  - TrimmedDistOutlierFilter:\n      ratio: 0.8\n"));
    CHECK(refused("  - TrimmedDistOutlierFilter:\n      ratio: 0.8\n" + ok));
    CHECK(refused(ok + "  - MedianDistOutlierFilter:\n      factor: 3\n"));
    CHECK(refused("  - RobustOutlierFilter:\n      robustFct: cauchy\n" + ok));
    CHECK(refused(ok + ok));
    {   // the refusal of an unsupported chain names the filter among the supported ones
        typename PM::ICP icp;
        std::string msg;
        try { load(icp, ok + "  - TrimmedDistOutlierFilter:\n      ratio: 0.8\n"); } catch (const std::runtime_error &e) { msg = e.what(); }
        CHECK(msg.find("VarTrimmedDistOutlierFilter") != std::string::npos);
    }
}

int main()
{
    var_trim_yaml<float>();
    var_trim_yaml<double>();
    std::puts("var trim cpu tests ok");
    return 0;
}
