// surface_normals_host.hpp -- the statement of include/pgicp_normals_ext.h in plain C++: given a cloud and its neighbour table
// (the ids pgicp_surface_normals_* returns), the raw normals, the eigenvalues, the eigenvector columns, the mean distances, the
// matched ids and the smoothed normals.  A second statement for tests to hold the device against; NOT a fallback: the filter
// without a device refuses as it always did.  Header-only, no dependency beyond the standard library.  Compile it without
// floating-point contraction: no product here may be fused with a sum.
#pragma once

#include <cmath>
#include <cstdint>
#include <limits>
#include <vector>

namespace pgslam_amd {
namespace surface_normals {

//! cyclic Jacobi on a symmetric 3x3 in double: a -> diagonal, columns of v the eigenvectors (16 sweeps at most, pairs (0,1),
//! (0,2), (1,2), the rotation applied to the columns, then the rows, then v)
inline void jacobi3(double a[3][3], double v[3][3])
{
    for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) v[i][j] = i == j ? 1.0 : 0.0;
    for (int sweep = 0; sweep < 16; sweep++) {
        const double off = a[0][1] * a[0][1] + a[0][2] * a[0][2] + a[1][2] * a[1][2];
        if (off == 0.0) break;
        for (int p = 0; p < 2; p++)
            for (int q = p + 1; q < 3; q++) {
                if (a[p][q] == 0.0) continue;
                const double theta = (a[q][q] - a[p][p]) / (2.0 * a[p][q]);
                const double t = (theta >= 0.0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
                const double c = 1.0 / std::sqrt(t * t + 1.0), s = t * c;
                for (int r = 0; r < 3; r++) { const double x = a[r][p], y = a[r][q]; a[r][p] = c * x - s * y; a[r][q] = s * x + c * y; }
                for (int r = 0; r < 3; r++) { const double x = a[p][r], y = a[q][r]; a[p][r] = c * x - s * y; a[q][r] = s * x + c * y; }
                for (int r = 0; r < 3; r++) { const double x = v[r][p], y = v[r][q]; v[r][p] = c * x - s * y; v[r][q] = s * x + c * y; }
            }
    }
}

template <typename T>
struct Rows {
    std::vector<T> normals, eigValues, eigVectors, meanDists, matchedIds;      // 3, 3, 9, 1 and knn values a point
};

//! everything but the smoothing: xyz at `stride`, ids n x knn (-1 = none)
template <typename T>
Rows<T> rows(const T *xyz, int stride, int n, const int32_t *ids, int knn)
{
    Rows<T> o;
    o.normals.resize(3 * (size_t)n); o.eigValues.resize(3 * (size_t)n); o.eigVectors.resize(9 * (size_t)n);
    o.meanDists.resize((size_t)n); o.matchedIds.resize((size_t)n * knn);
    for (int i = 0; i < n; i++) {
        const int32_t *nb = ids + (size_t)i * knn;
        int cnt = 0;
        T sx = 0, sy = 0, sz = 0;
        for (int j = 0; j < knn; j++) {
            o.matchedIds[(size_t)i * knn + j] = nb[j] >= 0 ? (T)nb[j] : (T)-1;
            if (nb[j] < 0) continue;
            const T *p = xyz + (size_t)nb[j] * stride;
            sx += p[0]; sy += p[1]; sz += p[2]; cnt++;
        }
        T c00 = 0, c01 = 0, c02 = 0, c11 = 0, c12 = 0, c22 = 0, md = 0;
        if (cnt > 0) {
            const T mx = sx / (T)cnt, my = sy / (T)cnt, mz = sz / (T)cnt;
            for (int j = 0; j < knn; j++) {
                if (nb[j] < 0) continue;
                const T *p = xyz + (size_t)nb[j] * stride;
                const T dx = p[0] - mx, dy = p[1] - my, dz = p[2] - mz;
                c00 += dx * dx; c01 += dx * dy; c02 += dx * dz; c11 += dy * dy; c12 += dy * dz; c22 += dz * dz;
            }
            const T *q = xyz + (size_t)i * stride;
            const T dx = q[0] - mx, dy = q[1] - my, dz = q[2] - mz;
            md = std::sqrt((dx * dx + dy * dy) + dz * dz);
        }
        o.meanDists[(size_t)i] = md;
        double A[3][3] = {{(double)c00, (double)c01, (double)c02}, {(double)c01, (double)c11, (double)c12}, {(double)c02, (double)c12, (double)c22}};
        double V[3][3];
        jacobi3(A, V);
        const double ev[3] = {A[0][0], A[1][1], A[2][2]};
        int lo = 0, hi = 0;
        for (int k = 1; k < 3; k++) { if (ev[k] < ev[lo]) lo = k; if (ev[k] > ev[hi]) hi = k; }
        const int mid = 3 - lo - hi;
        const bool degenerate = lo == hi || !(ev[hi] > 0.0) || !(ev[mid] > 3.0 * (double)std::numeric_limits<T>::epsilon() * ev[hi]);
        T *vec = &o.eigVectors[9 * (size_t)i], *val = &o.eigValues[3 * (size_t)i];
        if (degenerate) {
            const T d[9] = {0, 1, 0, 0, 0, 1, 1, 0, 0};
            for (int k = 0; k < 9; k++) vec[k] = d[k];
            val[0] = 0; val[1] = 0; val[2] = 1;
        } else {
            const int col[3] = {lo, mid, hi};
            for (int c = 0; c < 3; c++) {
                for (int r = 0; r < 3; r++) vec[3 * c + r] = (T)V[r][col[c]];
                val[c] = (T)ev[col[c]];
            }
        }
        for (int r = 0; r < 3; r++) o.normals[3 * (size_t)i + r] = vec[r];
    }
    return o;
}

//! the smoothing step: nrm at `nstride`, ids n x knn (-1 = none; every other id in [0, n)); out packed, 3 a point
template <typename T>
std::vector<T> smooth(const T *nrm, int nstride, int n, const int32_t *ids, int knn)
{
    std::vector<T> out(3 * (size_t)n);
    for (int i = 0; i < n; i++) {
        const T *r = nrm + (size_t)i * nstride;
        T ax = 0, ay = 0, az = 0;
        for (int j = 0; j < knn; j++) {
            const int32_t id = ids[(size_t)i * knn + j];
            if (id < 0) continue;
            const T *p = nrm + (size_t)id * nstride;
            const T d = (r[0] * p[0] + r[1] * p[1]) + r[2] * p[2];
            if (d > T(0)) { ax += p[0]; ay += p[1]; az += p[2]; }
            else { ax -= p[0]; ay -= p[1]; az -= p[2]; }
        }
        const T len = std::sqrt((ax * ax + ay * ay) + az * az);
        const bool ok = len > T(0) && std::isfinite(len);
        out[3 * (size_t)i] = ok ? ax / len : r[0];
        out[3 * (size_t)i + 1] = ok ? ay / len : r[1];
        out[3 * (size_t)i + 2] = ok ? az / len : r[2];
    }
    return out;
}

}  // namespace surface_normals
}  // namespace pgslam_amd
