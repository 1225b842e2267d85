// axis_quantile_host.hpp -- MaxQuantileOnAxisDataPointsFilter's statement (include/pgicp_quantile.h) in plain C++: the host form of
// the C++ drop-in's inPlaceFilter (a lone host cloud is not worth an upload) and the reference the device form is tested against.
#pragma once

#include <algorithm>
#include <cmath>
#include <limits>
#include <vector>

namespace pgslam_amd {
namespace axis_quantile {

// the statement's parameter ranges (upstream's)
inline bool dim_ok(int dim) { return dim >= 0 && dim <= 2; }
inline bool ratio_ok(double ratio) { return std::isfinite(ratio) && ratio >= 1e-7 && ratio <= 0.9999999; }

// NaN-last order: a NaN after +inf, all NaNs equal; -0 == +0 by the comparison itself
template <typename T>
inline bool less_nan_last(T a, T b)
{
    if (a != a) return false;
    if (b != b) return true;
    return a < b;
}

// k = (int)(T(n) * ratio), the product rounded in T with ratio held as T, clamped to n - 1 (n >= 1)
template <typename T>
inline int rank_of(int n, T ratio)
{
    const volatile T prod = (T)n * ratio;            // (volatile: rounded to T here, whatever the target's evaluation width)
    long long k = (long long)prod;
    if (k > (long long)n - 1) k = (long long)n - 1;
    return k < 0 ? 0 : (int)k;
}

template <typename T>
struct Result { T limit; int k; int below; };

// The limit of n values at `stride`, the rank and the number of values strictly below the limit.  The limit comes back canonical:
// +0 for either zero, the default quiet NaN for a NaN (and for n == 0).
template <typename T>
Result<T> select(const T *v, long long stride, int n, T ratio)
{
    Result<T> r{std::numeric_limits<T>::quiet_NaN(), 0, 0};
    if (n <= 0) return r;
    std::vector<T> w((size_t)n);
    for (int i = 0; i < n; i++) w[(size_t)i] = v[(long long)i * stride];
    r.k = rank_of<T>(n, ratio);
    std::nth_element(w.begin(), w.begin() + r.k, w.end(), less_nan_last<T>);
    const T lim = w[(size_t)r.k];
    if (lim != lim) return r;
    r.limit = lim == (T)0 ? (T)0 : lim;
    for (int i = 0; i < n; i++) r.below += v[(long long)i * stride] < r.limit ? 1 : 0;
    return r;
}

// the indices the filter keeps, ascending
template <typename T>
std::vector<int> kept_indices(const T *v, long long stride, int n, T ratio)
{
    std::vector<int> keep;
    if (n <= 0) return keep;
    const Result<T> r = select<T>(v, stride, n, ratio);
    keep.reserve((size_t)r.below);
    for (int i = 0; i < n; i++)
        if (v[(long long)i * stride] < r.limit) keep.push_back(i);
    return keep;
}

}  // namespace axis_quantile
}  // namespace pgslam_amd
