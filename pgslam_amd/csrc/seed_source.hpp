// seed_source.hpp -- host code only, no HIP types: may pgicp_partial_chain_seeded take its seeds from the source context?
//
// The seeded probe reads ANOTHER context's device state: its reading order and the correspondences its last align call left, which
// are slots of the map that call matched against.  They mean something only while that very map is still the one in its table
// entry.  Table entries are reused (a new map gets the first free one), so "the entry is in use" says nothing: every map carries
// the stamp its context's counter had when it was created or adopted -- the counter moves with every create, destroy, transfer in
// and transfer out -- and the align call records the stamp of the map it ran against.  Equal stamps: the same map, untouched.
// Whatever is refused here is searched unseeded, as pgicp_partial_chain: never an error, never another result.
// (tests/cpp/seed_source_host.cpp walks the table.)
#pragma once

namespace pgicp {

constexpr int kSeedMaxSegs = 16;              // SeedSegs (kernels.hpp) holds this many keyframe segments

struct SeedSource {
    // what the source context's last align call left (problem 0): n < 0 -- none, or overwritten by a later call
    int src_n, src_elem, src_knn, src_map, src_device;
    unsigned long long src_stamp;
    // what the caller asks for: the reading, its cloud type, its device, the segments, and whether it names itself as the source
    int n, elem, device, n_seg;
    bool src_is_self;
    // the caller's chain: problems of the call, KDTreeMatcher.knn, the grid matcher, a SurfaceNormalOutlierFilter (the set-up
    // kernel does not carry the reading's normals), a GenericDescriptorOutlierFilter
    int problems, knn;
    bool grid_matcher, normals_filter, desc_filter;
    // the source's map table NOW, at entry src_map (src_map outside the table: not in use)
    bool map_used;
    unsigned long long map_stamp;
};

inline bool seed_source_ok(const SeedSource &s)
{
    if (s.problems != 1 || s.knn != 1 || !s.grid_matcher || s.normals_filter || s.desc_filter) return false;
    if (s.src_is_self) return false;                                  // the call overwrites what it would read
    if (s.src_device != s.device) return false;
    if (s.n_seg < 1 || s.n_seg > kSeedMaxSegs) return false;
    if (s.src_n < 0 || s.src_n != s.n) return false;                  // another reading (or none)
    if (s.src_elem != s.elem) return false;                           // the other cloud type: another State's arrays
    if (s.src_knn != 1) return false;                                 // knn slots per point: another layout
    if (s.src_map < 0 || !s.map_used) return false;
    return s.src_stamp == s.map_stamp;                                // older: the entry was reused; newer: cannot be -- refused too
}

}  // namespace pgicp
