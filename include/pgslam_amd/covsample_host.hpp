// covsample_host.hpp -- the host side of CovarianceSamplingDataPointsFilter (statement: include/pgicp_covsample.h): the Jacobi of
// the frame, the per-point values, the lists' order and the greedy.  Shared by libpgicp.so (the host steps between its device
// passes) and by the C++ drop-in's host form, so that the two are the same code.  Every expression is written in the
// statement's order; the functions are compiled without contraction whatever the including file's flags.
#pragma once
#include "../pgicp_covsample.h"
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <unordered_set>
#include <vector>

#if defined(__clang__)
#define PGSLAM_COV_NOCONTRACT
#define PGSLAM_COV_BODY _Pragma("clang fp contract(off)")
#elif defined(__GNUC__)
#define PGSLAM_COV_NOCONTRACT __attribute__((optimize("fp-contract=off")))
#define PGSLAM_COV_BODY
#else
#define PGSLAM_COV_NOCONTRACT
#define PGSLAM_COV_BODY
#endif

namespace pgslam_amd {
namespace covsample {

// the 21 distinct sums of C in the order (a, b), a <= b, a-major
inline int tri(int a, int b) { return a * 6 - a * (a - 1) / 2 + (b - a); }

// cyclic Jacobi of a symmetric 6 x 6 matrix (full, row-major) in double: eigenvalues ascending (equal ones in the order the
// sweep left them), eigenvectors as the columns of X (column-major)
inline void jacobi6(const double Cin[36], double lambda[6], double X[36])
{
    double A[6][6], V[6][6];
    double frob = 0.0;
    for (int r = 0; r < 6; r++)
        for (int q = 0; q < 6; q++) { A[r][q] = Cin[6 * r + q]; V[r][q] = r == q ? 1.0 : 0.0; frob += A[r][q] * A[r][q]; }
    for (int sweep = 0; sweep < 60; sweep++) {
        double off = 0.0;
        for (int p = 0; p < 6; p++) for (int q = p + 1; q < 6; q++) off += A[p][q] * A[p][q];
        if (!(off > 1e-34 * frob)) break;
        for (int p = 0; p < 6; p++)
            for (int q = p + 1; q < 6; q++) {
                const double apq = A[p][q];
                if (apq == 0.0) continue;
                const double theta = (A[q][q] - A[p][p]) / (2.0 * apq);
                const double t = (theta >= 0.0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
                const double cs = 1.0 / std::sqrt(t * t + 1.0), sn = t * cs;
                for (int k = 0; k < 6; k++) {           // A <- A J
                    const double akp = A[k][p], akq = A[k][q];
                    A[k][p] = cs * akp - sn * akq;
                    A[k][q] = sn * akp + cs * akq;
                }
                for (int k = 0; k < 6; k++) {           // A <- J^T A
                    const double apk = A[p][k], aqk = A[q][k];
                    A[p][k] = cs * apk - sn * aqk;
                    A[q][k] = sn * apk + cs * aqk;
                }
                A[p][q] = 0.0; A[q][p] = 0.0;
                for (int k = 0; k < 6; k++) {
                    const double vkp = V[k][p], vkq = V[k][q];
                    V[k][p] = cs * vkp - sn * vkq;
                    V[k][q] = sn * vkp + cs * vkq;
                }
            }
    }
    int order[6] = {0, 1, 2, 3, 4, 5};
    std::stable_sort(order, order + 6, [&](int a, int b) { return A[a][a] < A[b][b]; });
    for (int k = 0; k < 6; k++) {
        lambda[k] = A[order[k]][order[k]];
        for (int r = 0; r < 6; r++) X[6 * k + r] = V[r][order[k]];
    }
}

// a cascaded sum (Knuth's two-sum, the rounding errors summed apart): the exact sum's rounding for any order of the terms
struct Cascade {
    double hi = 0.0, lo = 0.0;
    PGSLAM_COV_NOCONTRACT inline void add(double v)
    {
        PGSLAM_COV_BODY
        const double s = hi + v, bb = s - hi;
        lo += (hi - (s - bb)) + (v - bb);
        hi = s;
    }
    double value() const { return hi + lo; }
};

// the frame from its raw parts: c and L (values of T), the 21 sums of C
template <typename T>
void finish_frame(const double c[3], double L, const double sums[21], pgicp_cov_frame &f)
{
    double C[36];
    for (int a = 0; a < 6; a++) for (int b = a; b < 6; b++) { C[6 * a + b] = sums[tri(a, b)]; C[6 * b + a] = sums[tri(a, b)]; }
    for (int a = 0; a < 3; a++) f.center[a] = c[a];
    f.L = L;
    jacobi6(C, f.eigenvalues, f.basis);
    for (double &x : f.basis) x = (double)(T)x;
}

// what a point's values need of a frame, in T
template <typename T>
struct FrameT {
    T c[3], inv, X[36];
    explicit FrameT(const pgicp_cov_frame &f)
    {
        for (int a = 0; a < 3; a++) c[a] = (T)f.center[a];
        inv = T(1) / (T)f.L;
        for (int k = 0; k < 36; k++) X[k] = (T)f.basis[k];
    }
};

// f_i of a point
template <typename T>
PGSLAM_COV_NOCONTRACT inline void point_f(const T x[3], const T nr[3], const T c[3], T inv, T f[6])
{
    PGSLAM_COV_BODY
    const T px = x[0] - c[0], py = x[1] - c[1], pz = x[2] - c[2];
    const T cx = py * nr[2] - pz * nr[1], cy = pz * nr[0] - px * nr[2], cz = px * nr[1] - py * nr[0];
    f[0] = inv * cx; f[1] = inv * cy; f[2] = inv * cz; f[3] = nr[0]; f[4] = nr[1]; f[5] = nr[2];
}
// v_ik of a point, k = 0 .. 5
template <typename T>
PGSLAM_COV_NOCONTRACT inline void point_values(const T x[3], const T nr[3], const FrameT<T> &F, T v[6])
{
    PGSLAM_COV_BODY
    T f[6];
    point_f<T>(x, nr, F.c, F.inv, f);
    for (int k = 0; k < 6; k++) {
        const T *Xk = F.X + 6 * k;
        v[k] = std::fabs(((((f[0] * Xk[0] + f[1] * Xk[1]) + f[2] * Xk[2]) + f[3] * Xk[3]) + f[4] * Xk[4]) + f[5] * Xk[5]);
    }
}

// a candidate of a list: the point and its six values
template <typename T>
struct Cand { int32_t idx; T v[6]; };

// list k in its order: v_k descending, ties by ascending index
template <typename T>
void sort_list(std::vector<Cand<T>> &l, int k)
{
    std::sort(l.begin(), l.end(), [k](const Cand<T> &a, const Cand<T> &b) { return a.v[k] > b.v[k] || (a.v[k] == b.v[k] && a.idx < b.idx); });
}

// the greedy over six sorted lists (each its list's first min(n, nb_sample) entries): the picks in pick order
template <typename T>
PGSLAM_COV_NOCONTRACT inline void greedy(const std::vector<Cand<T>> lists[6], int nb_sample, std::vector<int32_t> &picks)
{
    PGSLAM_COV_BODY
    picks.clear();
    picks.reserve((size_t)nb_sample);
    std::unordered_set<int32_t> sampled;
    sampled.reserve(2 * (size_t)nb_sample);
    size_t head[6] = {0, 0, 0, 0, 0, 0};
    T t[6] = {0, 0, 0, 0, 0, 0};
    for (int s = 0; s < nb_sample; s++) {
        int k = 0;
        for (int kk = 1; kk < 6; kk++) if (t[k] > t[kk]) k = kk;
        const std::vector<Cand<T>> &l = lists[k];
        while (head[k] < l.size() && sampled.count(l[head[k]].idx)) head[k]++;
        if (head[k] >= l.size()) break;             // (the prefix bound: not reached with lists of min(n, nb_sample) entries)
        const Cand<T> &j = l[head[k]++];
        sampled.insert(j.idx);
        picks.push_back(j.idx);
        for (int m = 0; m < 6; m++) t[m] += j.v[m] * j.v[m];
    }
}

// The whole statement on the host, for a cloud reached through P(i, a) / N(i, a) (coordinate / normal component a of point i).
// frame(): false when an input is not finite or L is not > 0.  The double accumulations run in index order, those behind c and L
// cascaded.
template <typename T, class PF, class NF>
PGSLAM_COV_NOCONTRACT inline bool host_frame(int n, PF P, NF N, int torque_norm, pgicp_cov_frame &out)
{
    PGSLAM_COV_BODY
    Cascade s[3];
    T lo[3], hi[3];
    for (int a = 0; a < 3; a++) { lo[a] = P(0, a); hi[a] = lo[a]; }
    for (int i = 0; i < n; i++)
        for (int a = 0; a < 3; a++) {
            const T x = P(i, a);
            if (!std::isfinite(x) || !std::isfinite((T)N(i, a))) return false;
            s[a].add((double)x);
            if (x < lo[a]) lo[a] = x;
            if (x > hi[a]) hi[a] = x;
        }
    T c[3];
    for (int a = 0; a < 3; a++) c[a] = (T)(s[a].value() / (double)n);
    T L = T(1);
    if (torque_norm == 1) {
        Cascade sum;
        for (int i = 0; i < n; i++) {
            const T dx = P(i, 0) - c[0], dy = P(i, 1) - c[1], dz = P(i, 2) - c[2];
            sum.add((double)std::sqrt((dx * dx + dy * dy) + dz * dz));
        }
        L = (T)(sum.value() / (double)n);
    } else if (torque_norm == 2) {
        T e = hi[0] - lo[0];
        for (int a = 1; a < 3; a++) { const T ea = hi[a] - lo[a]; if (ea > e) e = ea; }
        L = T(0.5) * e;
    }
    if (!(L > T(0)) || !std::isfinite(L)) return false;
    const T inv = T(1) / L;
    double sums[21];
    for (double &x : sums) x = 0.0;
    for (int i = 0; i < n; i++) {
        const T x[3] = {P(i, 0), P(i, 1), P(i, 2)}, nr[3] = {N(i, 0), N(i, 1), N(i, 2)};
        T f[6];
        point_f<T>(x, nr, c, inv, f);
        int q = 0;
        for (int a = 0; a < 6; a++) for (int b = a; b < 6; b++) sums[q++] += (double)f[a] * (double)f[b];
    }
    const double cd[3] = {(double)c[0], (double)c[1], (double)c[2]};
    finish_frame<T>(cd, (double)L, sums, out);
    return true;
}

// the picks given the frame (nb_sample < n): every list's first nb_sample entries by a partial sort, then the greedy
template <typename T, class PF, class NF>
void host_select(int n, PF P, NF N, int nb_sample, const pgicp_cov_frame &frame, std::vector<int32_t> &picks)
{
    const FrameT<T> F(frame);
    std::vector<Cand<T>> all((size_t)n);
    for (int i = 0; i < n; i++) {
        const T x[3] = {P(i, 0), P(i, 1), P(i, 2)}, nr[3] = {N(i, 0), N(i, 1), N(i, 2)};
        all[(size_t)i].idx = i;
        point_values<T>(x, nr, F, all[(size_t)i].v);
    }
    const size_t m = (size_t)std::min(n, nb_sample);
    std::vector<Cand<T>> lists[6];
    for (int k = 0; k < 6; k++) {
        std::vector<Cand<T>> tmp(all);
        std::partial_sort(tmp.begin(), tmp.begin() + m, tmp.end(),
                          [k](const Cand<T> &a, const Cand<T> &b) { return a.v[k] > b.v[k] || (a.v[k] == b.v[k] && a.idx < b.idx); });
        lists[k].assign(tmp.begin(), tmp.begin() + m);
    }
    greedy<T>(lists, nb_sample, picks);
}

}  // namespace covsample
}  // namespace pgslam_amd
