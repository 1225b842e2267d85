// CPU-only checks of [EXT] GenericDescriptorOutlierFilter in the C++ drop-in (no device needed): loadFromYaml accepts it with
// the members upstream spells and refuses what the statement refuses (include/pgicp.h, pgicp_set_descriptor_filter: deviations
// c and d), and its stage-level compute() is the statement -- the same weights as tests/generic_descriptor_ref.py, printed
// for the Python test to compare bit for bit.
#include "common.hpp"
#include <cstdint>
#include <cstring>
#include <string>

template <typename T>
void yaml()
{
    using PM = PointMatcher<T>;
    const std::string head = "matcher:\n  KDTreeMatcher:\n    knn: 1\noutlierFilters:\n";
    auto load = [&](typename PM::ICP &icp, const std::string &filters) {
        std::istringstream in(head + filters);
        icp.loadFromYaml(in);
    };
    auto message = [&](const std::string &filters) -> std::string {
        typename PM::ICP icp;
        try { load(icp, filters); } catch (const std::runtime_error &e) { return e.what(); }
        return std::string();
    };
    auto refused = [&](const std::string &filters) { return !message(filters).empty(); };
    {   // hard mode, upstream's defaults for source and useLargerThan
        typename PM::ICP icp;
        load(icp, "  - TrimmedDistOutlierFilter:\n      ratio: 0.85\n"
                  "  - GenericDescriptorOutlierFilter:\n      descName: probabilityStatic\n      threshold: 0.5\n");
        CHECK(icp.outlierFilters.size() == 2);
        auto gd = std::dynamic_pointer_cast<typename PM::GenericDescriptorOutlierFilter>(icp.outlierFilters[1]);
        CHECK(gd && gd->descName == "probabilityStatic" && !gd->soft && gd->largerThan && gd->threshold == T(0.5));
        CHECK(gd->mode() == PGICP_DESC_FILTER_LARGER);
        CHECK(icp.descriptorName() == "probabilityStatic");
    }
    {   // every member spelled out; beside Robust, MaxDist and SurfaceNormal filters
        typename PM::ICP icp;
        load(icp, "  - RobustOutlierFilter:\n      robustFct: cauchy\n"
                  "  - GenericDescriptorOutlierFilter:\n      source: reference\n      descName: label\n      useSoftThreshold: 0\n"
                  "      useLargerThan: 0\n      threshold: 2.5\n"
                  "  - MaxDistOutlierFilter:\n      maxDist: 1.0\n"
                  "  - SurfaceNormalOutlierFilter:\n      maxAngle: 0.7\n");
        CHECK(icp.outlierFilters.size() == 4);
        auto gd = std::dynamic_pointer_cast<typename PM::GenericDescriptorOutlierFilter>(icp.outlierFilters[1]);
        CHECK(gd && !gd->soft && !gd->largerThan && gd->threshold == T(2.5) && gd->mode() == PGICP_DESC_FILTER_SMALLER);
    }
    {   // soft mode needs no threshold
        typename PM::ICP icp;
        load(icp, "  - GenericDescriptorOutlierFilter:\n      descName: w\n      useSoftThreshold: 1\n");
        auto gd = std::dynamic_pointer_cast<typename PM::GenericDescriptorOutlierFilter>(icp.outlierFilters[0]);
        CHECK(gd && gd->soft && gd->mode() == PGICP_DESC_FILTER_SOFT);
    }
    {   // without the filter the chain names no row
        typename PM::ICP icp;
        load(icp, "  - TrimmedDistOutlierFilter:\n      ratio: 0.85\n");
        CHECK(icp.descriptorName().empty() && icp.descriptorFilter() == nullptr);
    }
    const std::string ok = "  - GenericDescriptorOutlierFilter:\n      descName: probabilityStatic\n      threshold: 0.5\n";
    // (c) source: reading
    CHECK(message("  - GenericDescriptorOutlierFilter:\n      source: reading\n      descName: d\n      threshold: 0.5\n").find("source") != std::string::npos);
    // (d) descName, and threshold in hard mode
    CHECK(message("  - GenericDescriptorOutlierFilter:\n      threshold: 0.5\n").find("descName") != std::string::npos);
    CHECK(message("  - GenericDescriptorOutlierFilter:\n      descName: d\n").find("threshold") != std::string::npos);
    CHECK(message("  - GenericDescriptorOutlierFilter:\n      descName: d\n      useLargerThan: 0\n").find("threshold") != std::string::npos);
    // an unknown key
    CHECK(message(ok + "      ratio: 0.8\n").find("unknown parameter ratio") != std::string::npos);
    // a non-finite threshold
    for (const char *t : {"inf", "-inf", "nan"})
        CHECK(refused(std::string("  - GenericDescriptorOutlierFilter:\n      descName: d\n      threshold: ") + t + "\n"));
    // two filters
    CHECK(message(ok + ok).find("at most one") != std::string::npos);
    {   // the refusal of an unsupported chain names the filter among the supported ones (and still the others)
        const std::string msg = message(ok + "  - TrimmedDistOutlierFilter:\n      ratio: 0.8\n  - MedianDistOutlierFilter:\n      factor: 3\n");
        CHECK(msg.find("GenericDescriptorOutlierFilter") != std::string::npos);
        CHECK(msg.find("VarTrimmedDistOutlierFilter") != std::string::npos && msg.find("SurfaceNormalOutlierFilter") != std::string::npos);
    }
}

// compute() on hand-made Matches: knn x N ids with -1 entries, the reference's one-row descriptor; the weights are printed as
// hex bits ("W <mode> <T> <bits>...") for the Python test's comparison with the numpy statement
template <typename T>
void stage(const char *tname)
{
    using PM = PointMatcher<T>;
    typename PM::DataPoints ref;
    const int m = 6;
    ref.features = PM::Matrix::Zero(4, m);
    typename PM::Matrix d(2, m);
    const double vals[m] = {0.0, 0.25, 0.5, 0.75, 1.0 / 3.0, 2.0};
    for (int j = 0; j < m; j++) { d(0, j) = T(j); d(1, j) = (T)vals[j]; }
    ref.addDescriptor("other", d.block(0, 0, 1, m));
    ref.addDescriptor("probabilityStatic", d.block(1, 0, 1, m));
    typename PM::Matches mt(2, 5);
    const int ids[10] = {0, 5, -1, 3, 2, 2, 4, -1, 1, 3};      // column-major: point j's two neighbours at 2 j, 2 j + 1
    for (int e = 0; e < 10; e++) { mt.ids(e % 2, e / 2) = ids[e]; mt.dists(e % 2, e / 2) = T(0.01) * T(e); }
    struct Case { const char *name; bool soft, larger; double thr; };
    const Case cases[] = {{"larger", false, true, 0.5}, {"smaller", false, false, 0.5}, {"soft", true, true, 0.0}};
    for (const Case &c : cases) {
        typename PM::GenericDescriptorOutlierFilter f("probabilityStatic", c.soft, c.larger, (T)c.thr);
        const typename PM::OutlierWeights w = f.compute(ref, ref, mt);
        CHECK(w.rows() == 2 && w.cols() == 5);
        std::printf("W %s %s", c.name, tname);
        for (int e = 0; e < 10; e++) {
            const T v = w(e % 2, e / 2);
            if (sizeof(T) == 4) { uint32_t b; std::memcpy(&b, &v, 4); std::printf(" %08x", b); }
            else { uint64_t b; std::memcpy(&b, &v, 8); std::printf(" %016llx", (unsigned long long)b); }
        }
        std::printf("\n");
    }
    // refusals of the stage: a missing row, a row that is not one row
    {
        typename PM::GenericDescriptorOutlierFilter f("missing", false, true, T(0.5));
        bool threw = false;
        try { f.compute(ref, ref, mt); } catch (const std::runtime_error &) { threw = true; }
        CHECK(threw);
    }
    {
        typename PM::DataPoints r2;
        r2.features = PM::Matrix::Zero(4, m);
        r2.addDescriptor("two", d);
        typename PM::GenericDescriptorOutlierFilter f("two", false, true, T(0.5));
        bool threw = false;
        try { f.compute(r2, r2, mt); } catch (const std::runtime_error &) { threw = true; }
        CHECK(threw);
    }
    {   // soft mode: a maximum of 0 weighs everything 0 (deviation b)
        typename PM::DataPoints r3;
        r3.features = PM::Matrix::Zero(4, m);
        r3.addDescriptor("z", PM::Matrix::Zero(1, m));
        typename PM::GenericDescriptorOutlierFilter f("z", true, true, T(0));
        const typename PM::OutlierWeights w = f.compute(r3, r3, mt);
        for (int e = 0; e < 10; e++) CHECK(w(e % 2, e / 2) == T(0));
    }
}

int main()
{
    yaml<float>();
    yaml<double>();
    stage<float>("float32");
    stage<double>("float64");
    std::puts("generic descriptor cpu tests ok");
    return 0;
}
