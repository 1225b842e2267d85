// octree_host.hpp -- the host side of OctreeGridDataPointsFilter (statement: include/pgicp_octree.h): the root and the code
// length the library derives from the device's bounds, and the whole filter in plain C++ -- path codes, a stable sort, the leaf
// depth from prefix counts, the emission -- which the C++ drop-in runs with no device or under PGSLAM_HOST_INPUT_STAGE=1.
// Header-only, no dependency beyond the standard library.  Compile with -ffp-contract=off: the statement forbids contraction.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

namespace pgslam_amd {
namespace octree {

constexpr int kMaxDepth = 21;

//! the SplitMix64 finaliser of RandomSamplingDataPointsFilter
inline unsigned long long mix(unsigned long long z)
{
    z += 0x9E3779B97F4A7C15ULL; z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL; z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}

//! the root node and the levels a path code has: min(21, d_size)
template <typename T>
struct Root { T c[3], r; int levels; };

template <typename T>
Root<T> make_root(const T lo[3], const T hi[3], T max_size)
{
    Root<T> R;
    T emax = T(0);
    for (int a = 0; a < 3; a++) {
        const T e = hi[a] - lo[a];
        R.c[a] = lo[a] + e * T(0.5);
        if (a == 0 || e > emax) emax = e;
    }
    R.r = T(0.5) * emax;
    T r = R.r;
    int d = 0;
    while (d < kMaxDepth && !(r * T(2) <= max_size)) { r = r * T(0.5); d++; }
    R.levels = d;
    return R;
}

//! the path code of one point: R.levels digits of 3 bits, the level-l digit above the level-(l+1) digit
template <typename T>
unsigned long long path_code(const Root<T> &R, T x, T y, T z)
{
    const T p[3] = {x, y, z};
    T c[3] = {R.c[0], R.c[1], R.c[2]}, r = R.r;
    unsigned long long key = 0;
    for (int l = 0; l < R.levels; l++) {
        const T h = r * T(0.5);
        unsigned m = 0;
        for (int a = 0; a < 3; a++) {
            if (p[a] > c[a]) { m |= 1u << a; c[a] = c[a] + h; }
            else c[a] = c[a] - h;
        }
        key = (key << 3) | m;
        r = h;
    }
    return key;
}

//! the leaf depth of sorted position s: the smallest d in 0 .. levels whose d-prefix of key[s] is shared by <= max_pts keys, else
//! `levels`.  The count is non-increasing in d: a binary search over d, each probe a lower bound in key[0 .. s] and one look ahead.
inline int leaf_depth(const unsigned long long *key, int n, int s, int levels, int max_pts, int *leaf_start)
{
    const unsigned long long k = key[s];
    auto lower = [&](int sh) {                      // the first position whose sh-shifted key equals k's
        const unsigned long long p = k >> sh;
        int lo = 0, hi = s;
        while (lo < hi) { const int mid = lo + (hi - lo) / 2; if ((key[mid] >> sh) < p) lo = mid + 1; else hi = mid; }
        return lo;
    };
    int dlo = 0, dhi = levels;
    while (dlo < dhi) {
        const int d = (dlo + dhi) / 2, sh = 3 * (levels - d);
        const int L = lower(sh);
        const long long e = (long long)L + max_pts;
        const bool few = e >= n || (key[e] >> sh) != (k >> sh);
        if (few) dhi = d; else dlo = d + 1;
    }
    if (leaf_start) *leaf_start = lower(3 * (levels - dlo));
    return dlo;
}

template <typename T>
struct Result {
    std::vector<int32_t> kept, count, depth;        // a leaf: kept_idx, its points, its depth
    std::vector<T> xyz, desc;                       // 3 and drows values a leaf
};

//! the filter: X(i, a) coordinate a of point i, D(i, r) descriptor row r.  false: a coordinate is not finite (nothing written)
template <typename T, class GetX, class GetD>
bool host_filter(int n, GetX X, int drows, GetD D, int max_pts, T max_size, int method, unsigned long long seed, Result<T> &out)
{
    out = Result<T>();
    if (n <= 0) return true;
    T lo[3], hi[3];
    for (int a = 0; a < 3; a++) lo[a] = hi[a] = X(0, a) + T(0);
    for (int i = 0; i < n; i++)
        for (int a = 0; a < 3; a++) {
            const T x = X(i, a);
            if (!std::isfinite(x)) return false;
            if (x < lo[a]) lo[a] = x;
            if (x > hi[a]) hi[a] = x;
        }
    const Root<T> R = make_root<T>(lo, hi, max_size);
    std::vector<std::pair<unsigned long long, int32_t>> kv((size_t)n);
    for (int i = 0; i < n; i++) kv[(size_t)i] = {path_code<T>(R, X(i, 0), X(i, 1), X(i, 2)), i};
    std::sort(kv.begin(), kv.end());                // (key, index): a stable sort by key
    std::vector<unsigned long long> key((size_t)n);
    std::vector<int32_t> idx((size_t)n);
    for (int s = 0; s < n; s++) { key[(size_t)s] = kv[(size_t)s].first; idx[(size_t)s] = kv[(size_t)s].second; }
    kv.clear(); kv.shrink_to_fit();
    for (int s = 0; s < n;) {
        const int d = leaf_depth(key.data(), n, s, R.levels, max_pts, nullptr), sh = 3 * (R.levels - d);
        int e = s + 1;
        while (e < n && (key[(size_t)e] >> sh) == (key[(size_t)s] >> sh)) e++;
        const int c = e - s;
        if (d < R.levels) std::sort(idx.begin() + s, idx.begin() + e);       // a leaf above the last level: back to ascending index
        const int32_t *p = idx.data() + s;
        const int first = p[0];
        int keep = first;
        T cen[3] = {T(0), T(0), T(0)};
        if (method == 1) keep = p[(size_t)((mix(seed * 0x100000001B3ULL + (unsigned long long)first) >> 11) % (unsigned long long)c)];
        if (method >= 2) {
            for (int a = 0; a < 3; a++) {
                T sum = X(first, a);
                for (int k = 1; k < c; k++) sum += X(p[k], a);
                cen[a] = sum / (T)c;
            }
        }
        if (method == 3) {
            T best = T(0);
            for (int k = 0; k < c; k++) {
                const T dx = X(p[k], 0) - cen[0], dy = X(p[k], 1) - cen[1], dz = X(p[k], 2) - cen[2];
                const T dd = (dx * dx + dy * dy) + dz * dz;
                if (k == 0 || dd < best) { best = dd; keep = p[k]; }
            }
        }
        out.kept.push_back(keep);
        out.count.push_back(c);
        out.depth.push_back(d);
        for (int a = 0; a < 3; a++) out.xyz.push_back(method == 2 ? cen[a] : X(keep, a));
        for (int r = 0; r < drows; r++) {
            if (method == 2) {
                T sum = D(first, r);
                for (int k = 1; k < c; k++) sum += D(p[k], r);
                out.desc.push_back(sum / (T)c);
            } else
                out.desc.push_back(D(keep, r));
        }
        s = e;
    }
    return true;
}

}  // namespace octree
}  // namespace pgslam_amd
