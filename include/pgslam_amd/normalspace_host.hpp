// normalspace_host.hpp -- the host side of NormalSpaceDataPointsFilter (statement: include/pgicp_normalspace.h): the grid, the
// bucket of a normal, the sort key, the draw over the buckets' counts -- which the library runs between its two kernels -- and the
// whole filter in plain C++, which the C++ drop-in runs with no device or under PGSLAM_HOST_INPUT_STAGE=1.
// Header-only, no dependency beyond the standard library.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <utility>
#include <vector>

namespace pgslam_amd {
namespace normalspace {

constexpr int kMaxBuckets = 65536;
constexpr double kPi = 3.14159265358979323846;      // M_PI
constexpr int kRankBits = 24;                        // the bits of r_i under the bucket in the sort key

//! the SplitMix64 finaliser of RandomSamplingDataPointsFilter
inline unsigned long long mix(unsigned long long z)
{
    z += 0x9E3779B97F4A7C15ULL; z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL; z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}

struct Grid { int nPhi, nTheta, nbBucket; };

//! false: epsilon is outside the statement's bounds (finite, > 0, <= pi, nbBucket <= 65536)
inline bool make_grid(double epsilon, Grid &g)
{
    g = Grid{0, 0, 0};
    if (!std::isfinite(epsilon) || !(epsilon > 0.0) || !(epsilon <= kPi)) return false;
    const double np = std::ceil(2.0 * kPi / epsilon), nt = std::ceil(kPi / epsilon);
    if (!(np * nt <= (double)kMaxBuckets)) return false;
    g.nPhi = (int)np; g.nTheta = (int)nt; g.nbBucket = g.nPhi * g.nTheta;
    return true;
}

//! the bucket of a normal whose components are finite
inline int bucket_of(double nx, double ny, double nz, double epsilon, const Grid &g)
{
    const double z = std::max(std::min(nz, 1.0), -1.0);
    double theta = std::acos(z);
    double phi = std::fmod(std::atan2(ny, nx) + 2.0 * kPi, 2.0 * kPi);
    if (theta == kPi) theta = 0.0;
    if (phi == 2.0 * kPi) phi = 0.0;
    const int it = std::min((int)std::floor(theta / epsilon), g.nTheta - 1), ip = std::min((int)std::floor(phi / epsilon), g.nPhi - 1);
    return it * g.nPhi + ip;
}

//! r_i: the 24-bit rank of point i inside its bucket
inline unsigned long long rank_of(unsigned long long seed, unsigned long long i) { return mix(seed * 0x100000001B3ULL + i) >> 40; }
//! the sort key: ascending keys, ties by ascending index, are ascending (bucket, r_i, i)
inline unsigned long long key_of(int bucket, unsigned long long seed, unsigned long long i)
{
    return ((unsigned long long)bucket << kRankBits) | rank_of(seed, i);
}

//! The draw, over counts only: pick j is the rank[j]-th point, in the bucket's order, of bucket[j].  nb_sample <= the sum of the
//! counts.  The non-empty list is a Fenwick tree of 0 / 1 flags over the buckets: the r-th set flag by a descent, a flag cleared
//! when a bucket's last point is taken -- O((nb_sample + nbBucket) log nbBucket).
inline void draw(const int32_t *counts, int nb_bucket, int nb_sample, unsigned long long seed, std::vector<int32_t> &bucket, std::vector<int32_t> &rank)
{
    bucket.assign((size_t)nb_sample, 0);
    rank.assign((size_t)nb_sample, 0);
    int top = 1;
    while (top * 2 <= nb_bucket) top *= 2;
    std::vector<int32_t> tree((size_t)nb_bucket + 1, 0), taken((size_t)nb_bucket, 0);
    unsigned long long m = 0;
    for (int b = 0; b < nb_bucket; b++)
        if (counts[b] > 0) { tree[(size_t)b + 1] = 1; m++; }
    for (int k = 1; k <= nb_bucket; k++) {                              // the linear-time build
        const int up = k + (k & -k);
        if (up <= nb_bucket) tree[(size_t)up] += tree[(size_t)k];
    }
    const unsigned long long base = ~(seed * 0x100000001B3ULL);
    for (int j = 0; j < nb_sample; j++) {
        long long r = (long long)((mix(base + (unsigned long long)j) >> 11) % m);
        int pos = 0;                                                    // the largest prefix holding <= r set flags
        for (int step = top; step > 0; step >>= 1)
            if (pos + step <= nb_bucket && tree[(size_t)(pos + step)] <= r) { pos += step; r -= tree[(size_t)pos]; }
        const int b = pos;                                              // 0-based bucket: prefix `pos` ends just below it
        bucket[(size_t)j] = b;
        rank[(size_t)j] = taken[(size_t)b]++;
        if (taken[(size_t)b] == counts[b]) {
            for (int k = b + 1; k <= nb_bucket; k += k & -k) tree[(size_t)k]--;
            m--;
        }
    }
}

//! The filter: N(i, a) component a of normal i.  kept[j]: pick j's input index, bucket[j] its bucket; the no-op (nb_sample >= n)
//! gives 0 .. n-1 and -1.  false: a normal component is not finite (nothing written).  epsilon is within make_grid's bounds.
template <typename T, class GetN>
bool host_select(int n, GetN N, int nb_sample, double epsilon, unsigned long long seed, std::vector<int32_t> &kept, std::vector<int32_t> &bucket)
{
    kept.clear(); bucket.clear();
    if (n <= 0) return true;
    if (nb_sample >= n) {
        kept.resize((size_t)n); bucket.assign((size_t)n, -1);
        for (int i = 0; i < n; i++) kept[(size_t)i] = i;
        return true;
    }
    Grid g;
    if (!make_grid(epsilon, g)) return false;
    std::vector<std::pair<unsigned long long, int32_t>> kv((size_t)n);
    std::vector<int32_t> counts((size_t)g.nbBucket, 0);
    for (int i = 0; i < n; i++) {
        const T c[3] = {N(i, 0), N(i, 1), N(i, 2)};
        if (!std::isfinite(c[0]) || !std::isfinite(c[1]) || !std::isfinite(c[2])) return false;
        const int b = bucket_of((double)c[0], (double)c[1], (double)c[2], epsilon, g);
        counts[(size_t)b]++;
        kv[(size_t)i] = {key_of(b, seed, (unsigned long long)i), i};
    }
    std::sort(kv.begin(), kv.end());                                    // (key, index): a stable sort by key
    std::vector<int32_t> start((size_t)g.nbBucket + 1, 0), pb, pr;
    for (int b = 0; b < g.nbBucket; b++) start[(size_t)b + 1] = start[(size_t)b] + counts[(size_t)b];
    draw(counts.data(), g.nbBucket, nb_sample, seed, pb, pr);
    kept.resize((size_t)nb_sample);
    for (int j = 0; j < nb_sample; j++) kept[(size_t)j] = kv[(size_t)(start[(size_t)pb[(size_t)j]] + pr[(size_t)j])].second;
    bucket.swap(pb);
    return true;
}

}  // namespace normalspace
}  // namespace pgslam_amd
