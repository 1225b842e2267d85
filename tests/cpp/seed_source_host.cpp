// tests/test_seed_source_host.py: pgslam_amd/csrc/seed_source.hpp on the host -- may a seeded probe read the source context's state?
//   seed_source_host    one record that is seeded, then one field changed at a time; prints "seed source ok: N rows"
// Every row names what it changes and what the answer must be.
#include "seed_source.hpp"

#include <cstdio>
#include <functional>
#include <vector>

using pgicp::SeedSource;

static SeedSource good()
{
    SeedSource s;
    s.src_n = 2500; s.src_elem = 4; s.src_knn = 1; s.src_map = 0; s.src_device = 0; s.src_stamp = 5;
    s.n = 2500; s.elem = 4; s.device = 0; s.n_seg = 3; s.src_is_self = false;
    s.problems = 1; s.knn = 1; s.grid_matcher = true; s.normals_filter = false; s.desc_filter = false;
    s.map_used = true; s.map_stamp = 5;
    return s;
}

struct Row { const char *what; std::function<void(SeedSource &)> change; bool seeded; };

int main()
{
    const std::vector<Row> rows = {
        {"nothing changed", [](SeedSource &) {}, true},
        // the reading
        {"the source aligned one point more", [](SeedSource &s) { s.src_n = 2501; }, false},
        {"the source aligned one point fewer", [](SeedSource &s) { s.src_n = 2499; }, false},
        {"the caller's reading is one point longer", [](SeedSource &s) { s.n = 2501; }, false},
        {"the source's align was overwritten (n = -1)", [](SeedSource &s) { s.src_n = -1; }, false},
        {"overwritten, and the caller's n is -1 too", [](SeedSource &s) { s.src_n = -1; s.n = -1; }, false},
        // the cloud type
        {"the source aligned doubles, the caller probes floats", [](SeedSource &s) { s.src_elem = 8; }, false},
        {"the source aligned floats, the caller probes doubles", [](SeedSource &s) { s.elem = 8; }, false},
        {"both doubles", [](SeedSource &s) { s.src_elem = 8; s.elem = 8; }, true},
        {"the source has not aligned anything (element size 0)", [](SeedSource &s) { s.src_elem = 0; }, false},
        // the device
        {"the source is on device 1", [](SeedSource &s) { s.src_device = 1; }, false},
        {"the caller is on device 1", [](SeedSource &s) { s.device = 1; }, false},
        {"both on device 1", [](SeedSource &s) { s.src_device = 1; s.device = 1; }, true},
        // the source itself
        {"the caller names itself", [](SeedSource &s) { s.src_is_self = true; }, false},
        // the map
        {"the map's entry is not in use", [](SeedSource &s) { s.map_used = false; }, false},
        {"not in use, stamp 0", [](SeedSource &s) { s.map_used = false; s.map_stamp = 0; }, false},
        {"the source names no map (-1)", [](SeedSource &s) { s.src_map = -1; }, false},
        {"another entry of the table, same stamp", [](SeedSource &s) { s.src_map = 7; }, true},
        {"the align's stamp is older than the map's (the entry was reused)", [](SeedSource &s) { s.map_stamp = 6; }, false},
        {"much older", [](SeedSource &s) { s.map_stamp = 5000000000ULL; }, false},
        {"equal stamps, another value", [](SeedSource &s) { s.src_stamp = 5000000000ULL; s.map_stamp = 5000000000ULL; }, true},
        {"the align's stamp is newer than the map's", [](SeedSource &s) { s.src_stamp = 6; }, false},
        {"stamps that differ only above 32 bits", [](SeedSource &s) { s.src_stamp = 5 + (1ULL << 32); }, false},
        // the source's knn
        {"the source aligned with knn 2", [](SeedSource &s) { s.src_knn = 2; }, false},
        {"the source aligned with knn 3", [](SeedSource &s) { s.src_knn = 3; }, false},
        {"the source's knn was never recorded (0)", [](SeedSource &s) { s.src_knn = 0; }, false},
        // the segments
        {"no segment", [](SeedSource &s) { s.n_seg = 0; }, false},
        {"one segment", [](SeedSource &s) { s.n_seg = 1; }, true},
        {"16 segments", [](SeedSource &s) { s.n_seg = 16; }, true},
        {"17 segments", [](SeedSource &s) { s.n_seg = 17; }, false},
        {"-1 segments", [](SeedSource &s) { s.n_seg = -1; }, false},
        // the caller's chain
        {"a batch of two problems", [](SeedSource &s) { s.problems = 2; }, false},
        {"the caller's knn is 2", [](SeedSource &s) { s.knn = 2; }, false},
        {"the brute matcher", [](SeedSource &s) { s.grid_matcher = false; }, false},
        {"a SurfaceNormalOutlierFilter", [](SeedSource &s) { s.normals_filter = true; }, false},
        {"a GenericDescriptorOutlierFilter", [](SeedSource &s) { s.desc_filter = true; }, false},
    };
    int bad = 0, n_rows = 0;
    for (const Row &r : rows) {
        SeedSource s = good();
        r.change(s);
        const bool got = pgicp::seed_source_ok(s);
        if (got != r.seeded) { std::printf("%s: %s, expected %s\n", r.what, got ? "seeded" : "unseeded", r.seeded ? "seeded" : "unseeded"); ++bad; }
        ++n_rows;
    }
    if (bad) return 1;
    std::printf("seed source ok: %d rows\n", n_rows);
    return 0;
}
