// pointmatcher.hpp -- drop-in for the part of libpointmatcher's object model that
// pgslam drives on its ICP hot path, forwarding every numeric stage to the
// MI355X library through the C ABI of include/pgicp.h.
//
// Same spelling as PointMatcher<T> (reference src/pgslam/types.h:19-29 aliases
// it as PM): DataPoints, Matches, OutlierWeights, Transformation(s),
// DataPointsFilters, Matcher, OutlierFilters, ErrorMinimizer (+ErrorElements),
// TransformationCheckers, ICPChainBase, ICP, ICPSequence, ConvergenceError,
// PM::get().REG(Transformation).create("RigidTransformation").
// Call sites mirrored: Localizer.hpp:20,70,77,103,106,126,148,168,238,254,278,
// 309-347; LoopCloser.hpp:73,98,108,317,331,346-362; LocalMap.hpp:37,97,222.
//
// Header only; link with -lpgicp.  There is no CPU fallback: constructing an ICP
// object without a usable GPU throws.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <istream>
#include <limits>
#include <functional>
#include <initializer_list>
#include <memory>
#include <sstream>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <vector>

#include "../pgicp.h"
#include "../pgicp_noise.h"
#include "../pgicp_vardist.h"
#include "../pgicp_robust.h"
#include "../pgicp_density.h"
#include "../pgicp_covsample.h"
#include "covsample_host.hpp"
#include "../pgicp_octree.h"
#include "octree_host.hpp"
#include "../pgicp_normalspace.h"
#include "normalspace_host.hpp"
#include "../pgicp_normals_ext.h"
#include "../pgicp_quantile.h"
#include "../pgicp_ssn_ext.h"
#include "../pgicp_elipsoids.h"
#include "elipsoids_host.hpp"
#include "../pgicp_sensor_chain.h"
#include "sensor_chain_host.hpp"
#include "../pgicp_descriptor_filters.h"
#include "descriptor_filters_host.hpp"
#include "axis_quantile_host.hpp"
#include "matrix.hpp"
#include "yaml_lite.hpp"

namespace pgslam_amd {

// one lazily created context for objects that are not ICP chains (standalone
// RigidTransformation, LocalMap assembly); every ICP chain owns its own context
// and stream, as every pgslam worker owns its own ICP object.
inline pgicp_ctx *default_context(int device = 0)
{
    struct Holder {
        pgicp_ctx *c = nullptr;
        ~Holder() { if (c) pgicp_ctx_destroy(c); }
    };
    static thread_local Holder h;
    if (!h.c) {
        const int st = pgicp_ctx_create(device, &h.c);
        if (st != PGICP_OK) throw std::runtime_error("pgslam_amd: no usable MI355X device (pgicp_ctx_create failed, code " + std::to_string(st) + ")");
    }
    return h.c;
}

//! A device context made at FIRST USE: an ICP chain (and therefore a default-constructed pgslam facade, as the
//! reference's tests/instantiation.cpp constructs them) touches no GPU until it is asked to compute something.
struct LazyContext {
    int device = 0;
    int high_priority = 0;                      // pgicp_ctx_create_priority: a stream of the device's highest priority
    mutable pgicp_ctx *p = nullptr;
    explicit LazyContext(int d = 0, int prio = 0) : device(d), high_priority(prio) {}
    LazyContext(const LazyContext &) = delete;
    LazyContext &operator=(const LazyContext &) = delete;
    ~LazyContext() { destroy(); }
    bool made() const { return p != nullptr; }
    pgicp_ctx *get() const
    {
        if (!p) {
            const int st = high_priority ? pgicp_ctx_create_priority(device, 1, &p) : pgicp_ctx_create(device, &p);
            if (st != PGICP_OK) { p = nullptr; throw std::runtime_error(std::string("pgslam_amd: cannot create a device context: ") + pgicp_status_string(st)); }
        }
        return p;
    }
    operator pgicp_ctx *() const { return get(); }
    void destroy() { if (p) { pgicp_ctx_destroy(p); p = nullptr; } }
};

//! A cloud that stays in device memory between calls (pgicp_device_alloc): points as [n][xs], normals (optional) as [n][ns].
//! What a keyframe of the local map keeps (LocalMap.hpp:209-224 walks the keyframes at every rebuild; here the walk is one
//! device pass over resident clouds: pgicp_build_local_map with mem = PGICP_DEVICE) and what an assembled map is handed to
//! ICPSequence::setMap as.  Grow-only when reused as an assembly buffer.
template <typename T>
struct DeviceCloud {
    T *xyz = nullptr, *nrm = nullptr;
    int n = 0, xs = 3, ns = 3;
    size_t cap_x = 0, cap_n = 0;                    // elements allocated
    bool has_nrm = false;                           // the CURRENT contents carry normals (a reused buffer may hold an older cloud's)
    DeviceCloud() {}
    DeviceCloud(const DeviceCloud &) = delete;
    DeviceCloud &operator=(const DeviceCloud &) = delete;
    ~DeviceCloud() { release(); }
    void release()
    {
        if (xyz) pgicp_device_free(nullptr, xyz);
        if (nrm) pgicp_device_free(nullptr, nrm);
        xyz = nrm = nullptr; n = 0; cap_x = cap_n = 0; has_nrm = false;
    }
    static void fail(pgicp_ctx *c, int st, const char *what)
    {
        if (st != PGICP_OK) throw std::runtime_error(std::string(what) + ": " + pgicp_status_string(st) + " (" + pgicp_last_error(c) + ")");
    }
    //! room for `count` points (and normals) at the given strides; contents are undefined afterwards
    void reserve(pgicp_ctx *c, int count, int xstride, bool normals, int nstride)
    {
        const size_t need_x = (size_t)count * xstride, need_n = normals ? (size_t)count * nstride : 0;
        if (need_x > cap_x) {
            if (xyz) pgicp_device_free(c, xyz);
            xyz = nullptr; cap_x = 0;
            fail(c, pgicp_device_alloc(c, sizeof(T) * (need_x + need_x / 8), (void **)&xyz), "DeviceCloud: device allocation");
            cap_x = need_x + need_x / 8;
        }
        if (need_n > cap_n) {
            if (nrm) pgicp_device_free(c, nrm);
            nrm = nullptr; cap_n = 0;
            fail(c, pgicp_device_alloc(c, sizeof(T) * (need_n + need_n / 8), (void **)&nrm), "DeviceCloud: device allocation");
            cap_n = need_n + need_n / 8;
        }
        n = count; xs = xstride; ns = nstride; has_nrm = normals;
    }
    bool hasNormals() const { return has_nrm && nrm != nullptr && cap_n >= (size_t)n * ns && n > 0; }
    //! host -> device, strides kept as they are on the host (`x` holds (count - 1) * xstride + 3 elements at least)
    void upload(pgicp_ctx *c, const T *x, int xstride, const T *nr, int nstride, int count)
    {
        reserve(c, count, xstride, nr != nullptr, nstride);
        if (count <= 0) return;
        fail(c, pgicp_device_copy(c, xyz, x, sizeof(T) * ((size_t)(count - 1) * xstride + 3), PGICP_COPY_TO_DEVICE), "DeviceCloud: upload");
        if (nr) fail(c, pgicp_device_copy(c, nrm, nr, sizeof(T) * ((size_t)(count - 1) * nstride + 3), PGICP_COPY_TO_DEVICE), "DeviceCloud: upload");
    }
};

//! one of the two entry points of a pgicp_*_f32 / pgicp_*_f64 pair, by the cloud's scalar; any other T does not compile
template <typename T, typename F32, typename F64>
constexpr auto pick(F32 *f32, F64 *f64)
{
    static_assert(std::is_same<T, float>::value || std::is_same<T, double>::value, "pgslam_amd: T must be float or double");
    if constexpr (std::is_same<T, float>::value) return f32; else return f64;
}
//! the C ABI by scalar type: each forwarder fixes the memory (PGICP_HOST, or PGICP_DEVICE for *_dev), the packed output
//! strides and the optional arguments its callers leave out
template <typename T> struct Abi {
    static_assert(std::is_same<T, float>::value || std::is_same<T, double>::value, "pgslam_amd: T must be float or double");
    static int map_create(pgicp_ctx *c, const T *x, int xs, const T *n, int ns, int m, int center, int *id) { return pick<T>(pgicp_map_create_f32, pgicp_map_create_f64)(c, x, xs, n, ns, m, PGICP_HOST, center, id); }
    static int align(pgicp_ctx *c, int id, const T *r, int s, int n, const double *Ti, double *To, pgicp_stats *st) { return pick<T>(pgicp_align_f32, pgicp_align_f64)(c, id, r, s, n, PGICP_HOST, Ti, To, st); }
    static int align_dev(pgicp_ctx *c, int id, const T *r, int s, int n, const double *Ti, double *To, pgicp_stats *st) { return pick<T>(pgicp_align_f32, pgicp_align_f64)(c, id, r, s, n, PGICP_DEVICE, Ti, To, st); }
    static int align_nrm(pgicp_ctx *c, int id, const T *r, int s, int n, const T *nr, int ns, const double *Ti, double *To, pgicp_stats *st)
    {
        pgicp_problem p;
        std::memset(&p, 0, sizeof p);
        p.map_id = id; p.reading = r; p.stride = s; p.n = n; p.mem = PGICP_HOST; p.normals = nr; p.nstride = ns;
        std::memcpy(p.T_init, Ti, sizeof p.T_init);
        return pick<T>(pgicp_align_batch_f32, pgicp_align_batch_f64)(c, 1, &p, To, st);
    }
    static int upload(pgicp_ctx *c, const T *host, int stride, int n, const T **dev) { return pick<T>(pgicp_upload_f32, pgicp_upload_f64)(c, 1, &host, &stride, &n, PGICP_HOST, dev); }
    static int match(pgicp_ctx *c, int id, const T *r, int s, int n, int32_t *ids, T *d2) { return pick<T>(pgicp_match_f32, pgicp_match_f64)(c, id, r, s, n, PGICP_HOST, nullptr, ids, d2); }
    static int weights(pgicp_ctx *c, const T *d2, int n, T *w, T *lim, int *nf) { return pick<T>(pgicp_outlier_weights_f32, pgicp_outlier_weights_f64)(c, d2, n, PGICP_HOST, w, lim, nf); }
    static int stats(pgicp_ctx *c, int id, const T *r, int s, int n, const int32_t *ids, const T *w, double *ratio, double *res, double *sys) { return pick<T>(pgicp_error_stats_f32, pgicp_error_stats_f64)(c, id, r, s, n, PGICP_HOST, ids, w, ratio, res, sys); }
    static int map_create_batch(pgicp_ctx *c, int k, const T *const *x, const int *xs, const T *const *n, const int *ns, const int *m, int center, int *ids) { return pick<T>(pgicp_map_create_batch_f32, pgicp_map_create_batch_f64)(c, k, x, xs, n, ns, m, PGICP_HOST, center, ids); }
    static int normals(pgicp_ctx *c, const T *x, int xs, int n, int knn, double md, T *out, int os, T *eig) { return pick<T>(pgicp_surface_normals_f32, pgicp_surface_normals_f64)(c, x, xs, n, PGICP_HOST, knn, md, out, os, eig, nullptr, nullptr); }
    static int normals_ids(pgicp_ctx *c, const T *x, int xs, int n, int knn, double md, T *out, int os, T *eig, int32_t *ids) { return pick<T>(pgicp_surface_normals_f32, pgicp_surface_normals_f64)(c, x, xs, n, PGICP_HOST, knn, md, out, os, eig, ids, nullptr); }
    static int densities(pgicp_ctx *c, const T *x, int xs, int n, int knn, double md, T *out, int os, T *eig, T *dens) { return pick<T>(pgicp_surface_densities_f32, pgicp_surface_densities_f64)(c, x, xs, n, PGICP_HOST, knn, md, out, os, eig, dens); }
    static int normals_ext(pgicp_ctx *c, const T *x, int xs, int n, int knn, double md, int smooth, T *out, int os, T *eig, T *vec, T *mdist, T *mids, T *dens)
    { return pick<T>(pgicp_surface_normals_ext_f32, pgicp_surface_normals_ext_f64)(c, x, xs, n, PGICP_HOST, knn, md, smooth, out, os, eig, vec, mdist, mids, nullptr, nullptr, dens); }
    static int smooth_normals(pgicp_ctx *c, const T *nr, int ns, const int32_t *ids, int knn, int n, T *out, int os) { return pick<T>(pgicp_smooth_normals_f32, pgicp_smooth_normals_f64)(c, nr, ns, ids, knn, n, PGICP_HOST, out, os); }
    static int max_density(pgicp_ctx *c, const T *dens, int n, double md, uint64_t sd, int32_t *idx, int *n_out) { return pick<T>(pgicp_max_density_f32, pgicp_max_density_f64)(c, dens, n, PGICP_HOST, md, sd, idx, n_out); }
    static int normals_max_density(pgicp_ctx *c, const T *x, int xs, int n, int knn, double md, double dmax, uint64_t sd, const T *d, int dr, T *ox, T *on,
                                   T *oe, T *odn, T *od, int32_t *idx, int *n_out)
    { return pick<T>(pgicp_normals_max_density_f32, pgicp_normals_max_density_f64)(c, x, xs, n, PGICP_HOST, knn, md, dmax, sd, d, dr, ox, on, 3, oe, odn, od, idx, n_out); }
    static int sampling_normals(pgicp_ctx *c, const T *x, int xs, int n, int knn, double r, int m, double box, uint64_t sd, const T *d, int dr, int avg,
                                T *ox, T *on, T *od, int32_t *idx, int *n_out)
    { return pick<T>(pgicp_sampling_surface_normal_f32, pgicp_sampling_surface_normal_f64)(c, x, xs, n, PGICP_HOST, knn, r, m, box, sd, d, dr, avg, ox, 3, on, 3, od, idx, n_out, nullptr); }
    static int sampling_normals_ext(pgicp_ctx *c, const T *x, int xs, int n, int knn, double r, int m, double box, uint64_t sd, const T *d, int dr, int avg,
                                    T *ox, T *on, T *od, int32_t *idx, int *n_out, T *eig, T *vec, T *dens)
    { return pick<T>(pgicp_sampling_surface_normal_ext_f32, pgicp_sampling_surface_normal_ext_f64)(c, x, xs, n, PGICP_HOST, knn, r, m, box, sd, d, dr, avg, ox, 3, on, 3, od, idx, n_out, nullptr, eig, vec, dens); }
    static int elipsoids(pgicp_ctx *c, const T *x, int xs, int n, int knn, double r, int m, double box, double minp, uint64_t sd, const T *d, int dr, int avg,
                         T *ox, T *on, T *od, int32_t *idx, int *n_out, T *eig, T *vec, T *dens, T *cov, T *wgt, T *mean, T *shp)
    { return pick<T>(pgicp_elipsoids_f32, pgicp_elipsoids_f64)(c, x, xs, n, PGICP_HOST, knn, r, m, box, sd, d, dr, avg, ox, 3, on, 3, od, idx, n_out, nullptr, eig, vec, dens, minp, cov, wgt, mean, shp); }
    static int sensor_chain(pgicp_ctx *c, const T *x, int xs, int n, int knn, double md, int kn, int ke, int kd, int ns, const pgicp_chain_stage *st, const T *d, int dr,
                            T *ox, T *on, T *oe, T *odn, T *oobs, T *onoise, T *od, int32_t *idx, int *n_out)
    { return pick<T>(pgicp_sensor_chain_f32, pgicp_sensor_chain_f64)(c, x, xs, n, PGICP_HOST, knn, md, kn, ke, kd, ns, st, d, dr, ox, on, 3, oe, odn, oobs, onoise, od, idx, n_out); }
    static int sensor_chain_ext(pgicp_ctx *c, const T *x, int xs, int n, int knn, double md, int kn, int ke, int kd, int ns, const pgicp_chain_stage *st, const T *d, int dr,
                                const pgicp_chain_out &o, int *n_out)
    { return pick<T>(pgicp_sensor_chain_ext_f32, pgicp_sensor_chain_ext_f64)(c, x, xs, n, PGICP_HOST, knn, md, kn, ke, kd, ns, st, d, dr, &o, n_out); }
    static int covariance_sampling(pgicp_ctx *c, const T *x, int xs, const T *nr, int ns, int n, int nb, int tn, int32_t *idx, int *n_out, pgicp_cov_frame *fr)
    { return pick<T>(pgicp_covariance_sampling_f32, pgicp_covariance_sampling_f64)(c, x, xs, nr, ns, n, PGICP_HOST, nb, tn, nullptr, 0, nullptr, nullptr, 3, nullptr, idx, n_out, fr); }
    static int normal_space(pgicp_ctx *c, const T *x, int xs, const T *nr, int ns, int n, int nb, double eps, unsigned long long seed, int32_t *idx, int *n_out)
    { return pick<T>(pgicp_normal_space_sampling_f32, pgicp_normal_space_sampling_f64)(c, x, xs, nr, ns, n, PGICP_HOST, nb, eps, seed, nullptr, 0, nullptr, nullptr, 3, nullptr, idx, nullptr, n_out); }
    static int octree_grid(pgicp_ctx *c, const T *x, int xs, int n, int mp, double ms, int method, unsigned long long seed, const T *d, int dr, T *ox, T *od, int32_t *idx, int *n_out)
    { return pick<T>(pgicp_octree_grid_f32, pgicp_octree_grid_f64)(c, x, xs, n, PGICP_HOST, mp, ms, method, seed, d, dr, ox, 3, od, idx, nullptr, nullptr, n_out); }
    static int voxel_grid(pgicp_ctx *c, const T *x, int xs, int n, const double *v, int cen, const T *d, int dr, int avg, T *ox, T *od, int32_t *idx, int *n_out)
    { return pick<T>(pgicp_voxel_grid_f32, pgicp_voxel_grid_f64)(c, x, xs, n, PGICP_HOST, v, cen, d, dr, avg, ox, 3, od, idx, nullptr, n_out); }
    static int partial(pgicp_ctx *c, int id, const T *r, int s, int n, const double *Tm, double *ratio, double *res) { return pick<T>(pgicp_partial_chain_f32, pgicp_partial_chain_f64)(c, id, r, s, n, PGICP_HOST, Tm, ratio, res); }
    static int partial_dev(pgicp_ctx *c, int id, const T *r, int s, int n, const double *Tm, double *ratio, double *res) { return pick<T>(pgicp_partial_chain_f32, pgicp_partial_chain_f64)(c, id, r, s, n, PGICP_DEVICE, Tm, ratio, res); }
    static int partial_seeded_dev(pgicp_ctx *c, int id, const T *r, int s, int n, const double *Tm, pgicp_ctx *src, int ns, const int32_t *a, const int32_t *b, double *ratio, double *res) { return pick<T>(pgicp_partial_chain_seeded_f32, pgicp_partial_chain_seeded_f64)(c, id, r, s, n, PGICP_DEVICE, Tm, src, ns, a, b, ratio, res); }
    static int transform(pgicp_ctx *c, const double *Tm, const T *in, int is, T *out, int os, int n, int ro) { return pick<T>(pgicp_transform_f32, pgicp_transform_f64)(c, Tm, in, is, out, os, n, ro, PGICP_HOST); }
    static int local_map(pgicp_ctx *c, int k, const T *const *x, const T *const *n, const int *sx, const int *sn, const int *cnt, const double *Ts, T *ox, int os, T *on, int ons) { return pick<T>(pgicp_build_local_map_f32, pgicp_build_local_map_f64)(c, k, x, n, sx, sn, cnt, Ts, ox, os, on, ons, PGICP_HOST); }
    static int local_map_dev(pgicp_ctx *c, int k, const T *const *x, const T *const *n, const int *sx, const int *sn, const int *cnt, const double *Ts, T *ox, int os, T *on, int ons) { return pick<T>(pgicp_build_local_map_f32, pgicp_build_local_map_f64)(c, k, x, n, sx, sn, cnt, Ts, ox, os, on, ons, PGICP_DEVICE); }
    static int map_create_dev(pgicp_ctx *c, const T *x, int xs, const T *n, int ns, int m, int center, int *id) { return pick<T>(pgicp_map_create_f32, pgicp_map_create_f64)(c, x, xs, n, ns, m, PGICP_DEVICE, center, id); }
    static int transform_dev(pgicp_ctx *c, const double *T16, const T *in, int is, T *out, int os, int n, int rotate_only) { return pick<T>(pgicp_transform_f32, pgicp_transform_f64)(c, T16, in, is, out, os, n, rotate_only, PGICP_DEVICE); }
    static int arm_radii(pgicp_ctx *c, int k, const T *const *rows, const int *strides, const int *n) { return pick<T>(pgicp_arm_reading_radii_f32, pgicp_arm_reading_radii_f64)(c, k, rows, strides, n, PGICP_HOST); }
    static int arm_noise(pgicp_ctx *c, int k, const T *const *rows, const int *strides, const int *n) { return pick<T>(pgicp_arm_reading_noise_f32, pgicp_arm_reading_noise_f64)(c, k, rows, strides, n, PGICP_HOST); }
    static int set_values(pgicp_ctx *c, int id, const T *v, int stride) { return pick<T>(pgicp_map_set_values_f32, pgicp_map_set_values_f64)(c, id, v, stride, PGICP_HOST); }
    static int map_create_batch_dev(pgicp_ctx *c, int k, const T *const *x, const int *xs, const T *const *n, const int *ns, const int *m, int center, int *ids) { return pick<T>(pgicp_map_create_batch_f32, pgicp_map_create_batch_f64)(c, k, x, xs, n, ns, m, PGICP_DEVICE, center, ids); }
    static int align_residual_batch(pgicp_ctx *c, int k, const pgicp_problem *p, double *To, pgicp_stats *st, double *residual) { return pick<T>(pgicp_align_residual_batch_f32, pgicp_align_residual_batch_f64)(c, k, p, To, st, residual, nullptr, nullptr); }
    static int filter_cloud(pgicp_ctx *c, int nf, const pgicp_filter *f, const T *x, int xs, const T *d, int dr, int n, const double *T16, int r0, int r1, T *ox, T *od, int *n_out, const T **dev)
    { return pick<T>(pgicp_filter_cloud_f32, pgicp_filter_cloud_f64)(c, nf, f, x, xs, d, dr, n, T16, r0, r1, ox, od, nullptr, n_out, dev); }
    static int filter_cloud_dev(pgicp_ctx *c, int nf, const pgicp_filter *f, const T *x, int xs, int n, int32_t *dropped, int cap, int *n_dropped, int *n_out, const T **dev)
    { return pick<T>(pgicp_filter_cloud_dev_f32, pgicp_filter_cloud_dev_f64)(c, nf, f, x, xs, n, dropped, cap, n_dropped, n_out, dev); }
};

}  // namespace pgslam_amd

template <typename T>
struct PointMatcher {
    typedef T ScalarType;
    typedef pgslam_amd::Mat<T> Matrix;
    typedef pgslam_amd::Mat<int> IntMatrix;
    typedef Matrix TransformationParameters;
    typedef Matrix OutlierWeights;
    using A = pgslam_amd::Abi<T>;

    //! what libpointmatcher throws when a stage cannot proceed; pgslam never catches it
    struct ConvergenceError : std::runtime_error {
        explicit ConvergenceError(const std::string &r) : std::runtime_error(r) {}
    };
    static void check(pgicp_ctx *c, int st)
    {
        if (st == PGICP_OK) return;
        const std::string msg = c ? pgicp_last_error(c) : "pgicp error";
        if (st == PGICP_ERR_NO_MATCH || st == PGICP_ERR_NAN || st == PGICP_ERR_BOUND) throw ConvergenceError(msg);
        if (st == PGICP_ERR_NOT_RIGID) throw std::runtime_error("RigidTransformation: " + msg);
        throw std::runtime_error("pgicp (" + std::to_string(st) + "): " + msg);
    }

    // ------------------------------------------------------------------ DataPoints
    struct DataPoints {
        struct Label {
            std::string text;
            size_t span;
            Label(const std::string &t = "", size_t s = 0) : text(t), span(s) {}
            bool operator==(const Label &o) const { return text == o.text && span == o.span; }
        };
        struct Labels : std::vector<Label> {
            bool contains(const std::string &t) const { for (auto &l : *this) if (l.text == t) return true; return false; }
            size_t totalDim() const { size_t d = 0; for (auto &l : *this) d += l.span; return d; }
        };
        //! [EXT] DataPoints::InvalidField: a filter asks for a descriptor the cloud does not carry, or carries in another shape
        struct InvalidField : std::runtime_error { explicit InvalidField(const std::string &m) : std::runtime_error(m) {} };
        Matrix features;          //!< (dim+1) x N homogeneous coordinates, column major: one point = 4 contiguous values
        Labels featureLabels;
        Matrix descriptors;       //!< D x N
        Labels descriptorLabels;

        DataPoints() {}
        DataPoints(const Matrix &f, const Labels &fl) : features(f), featureLabels(fl) {}
        DataPoints(const Matrix &f, const Labels &fl, const Matrix &d, const Labels &dl) : features(f), featureLabels(fl), descriptors(d), descriptorLabels(dl) {}
        //! convenience: N x 3 points (+ optional N x 3 normals), row i = point i
        static DataPoints fromXYZ(const T *xyz, int n, const T *normals = nullptr)
        {
            DataPoints dp;
            dp.features = Matrix(4, n);
            for (int i = 0; i < n; i++) { for (int a = 0; a < 3; a++) dp.features(a, i) = xyz[3 * i + a]; dp.features(3, i) = T(1); }
            dp.featureLabels.push_back(Label("x", 1)); dp.featureLabels.push_back(Label("y", 1));
            dp.featureLabels.push_back(Label("z", 1)); dp.featureLabels.push_back(Label("pad", 1));
            if (normals) {
                dp.descriptors = Matrix(3, n);
                for (int i = 0; i < n; i++) for (int a = 0; a < 3; a++) dp.descriptors(a, i) = normals[3 * i + a];
                dp.descriptorLabels.push_back(Label("normals", 3));
            }
            return dp;
        }
        unsigned getNbPoints() const { return (unsigned)features.cols(); }
        unsigned getEuclideanDim() const { return features.rows() > 0 ? (unsigned)features.rows() - 1 : 0; }
        bool descriptorExists(const std::string &name) const { return descriptorLabels.contains(name); }
        int getDescriptorStartingRow(const std::string &name) const
        {
            int row = 0;
            for (auto &l : descriptorLabels) { if (l.text == name) return row; row += (int)l.span; }
            throw std::runtime_error("DataPoints: descriptor " + name + " not found");
        }
        int getDescriptorDimension(const std::string &name) const
        {
            for (auto &l : descriptorLabels) if (l.text == name) return (int)l.span;
            return 0;
        }
        //! copy of the rows of one descriptor (Eigen returns a block view; reads are equivalent)
        Matrix getDescriptorViewByName(const std::string &name) const
        {
            return descriptors.block(getDescriptorStartingRow(name), 0, getDescriptorDimension(name), descriptors.cols());
        }
        void addDescriptor(const std::string &name, const Matrix &d)
        {
            if (d.cols() != features.cols()) throw std::runtime_error("DataPoints::addDescriptor: wrong number of points");
            if (descriptorExists(name)) throw std::runtime_error("DataPoints::addDescriptor: " + name + " exists");
            const int old = descriptors.rows();
            Matrix nd(old + d.rows(), features.cols());
            for (int j = 0; j < features.cols(); j++) {
                for (int i = 0; i < old; i++) nd(i, j) = descriptors(i, j);
                for (int i = 0; i < d.rows(); i++) nd(old + i, j) = d(i, j);
            }
            descriptors = nd;
            descriptorLabels.push_back(Label(name, d.rows()));
        }
        //! what a filter that "allocates" a descriptor does upstream (DataPoints::allocateDescriptors): a descriptor of that name and
        //! span that already exists is REUSED -- its rows are overwritten --, one of another span is an error, a new one is appended
        void setDescriptor(const std::string &name, const Matrix &d)
        {
            if (!descriptorExists(name)) { addDescriptor(name, d); return; }
            if (d.cols() != features.cols()) throw std::runtime_error("DataPoints::setDescriptor: wrong number of points");
            if (getDescriptorDimension(name) != (int)d.rows()) throw std::runtime_error("DataPoints::setDescriptor: " + name + " exists with another dimension");
            const int r0 = getDescriptorStartingRow(name);
            for (int j = 0; j < features.cols(); j++) for (int i = 0; i < d.rows(); i++) descriptors(r0 + i, j) = d(i, j);
        }
        //! append dp; only descriptors present in BOTH clouds (same name and span) are kept
        void concatenate(const DataPoints &dp)
        {
            if (features.cols() == 0) { *this = dp; return; }
            if (dp.features.rows() != features.rows()) throw std::runtime_error("DataPoints::concatenate: feature dimensions differ");
            const int n0 = features.cols(), n1 = dp.features.cols();
            Matrix f(features.rows(), n0 + n1);
            std::memcpy(f.data(), features.data(), sizeof(T) * features.size());
            std::memcpy(f.data() + features.size(), dp.features.data(), sizeof(T) * dp.features.size());
            Labels keep;
            int rows = 0;
            for (auto &l : descriptorLabels)
                if (dp.descriptorLabels.contains(l.text) && dp.getDescriptorDimension(l.text) == (int)l.span) { keep.push_back(l); rows += (int)l.span; }
            Matrix d(rows, n0 + n1);
            int r = 0;
            for (auto &l : keep) {
                const int a = getDescriptorStartingRow(l.text), b = dp.getDescriptorStartingRow(l.text);
                for (int k = 0; k < (int)l.span; k++) {
                    for (int j = 0; j < n0; j++) d(r + k, j) = descriptors(a + k, j);
                    for (int j = 0; j < n1; j++) d(r + k, n0 + j) = dp.descriptors(b + k, j);
                }
                r += (int)l.span;
            }
            features = f; descriptors = d; descriptorLabels = keep;
        }
        // (pointer, stride) views handed to the C ABI
        const T *xyzPtr() const { return features.data(); }
        int xyzStride() const { return features.rows(); }
        const T *normalsPtr() const { return descriptorExists("normals") ? descriptors.data() + getDescriptorStartingRow("normals") : nullptr; }
        int normalsStride() const { return descriptors.rows(); }
    };

    // ------------------------------------------------------------------ Matches
    struct Matches {
        typedef Matrix Dists;
        typedef IntMatrix Ids;
        static constexpr int InvalidId = -1;
        static T InvalidDist() { return std::numeric_limits<T>::infinity(); }
        Dists dists;      //!< knn x N SQUARED distances
        Ids ids;          //!< knn x N indices into the reference
        Matches() {}
        Matches(int knn, int n) : dists(knn, n), ids(knn, n) {}
    };

    // ------------------------------------------------------------------ Transformation
    struct Transformation {
        virtual ~Transformation() {}
        virtual DataPoints compute(const DataPoints &input, const TransformationParameters &parameters) const = 0;
        virtual bool checkParameters(const TransformationParameters &parameters) const = 0;
    };
    struct RigidTransformation : Transformation {
        const pgslam_amd::LazyContext *ctx;          // the owning chain's context (made at first use), or none
        explicit RigidTransformation(const pgslam_amd::LazyContext *c = nullptr) : ctx(c) {}
        bool checkParameters(const TransformationParameters &p) const override
        {
            double e = 0;
            for (int i = 0; i < 3; i++)
                for (int j = 0; j < 3; j++) {
                    double s = 0;
                    for (int k = 0; k < 3; k++) s += (double)p(k, i) * (double)p(k, j);
                    e = std::max(e, std::fabs(s - (i == j ? 1.0 : 0.0)));
                }
            return e < 1e-3;
        }
        //! features' = T * features; the normals / observationDirections descriptors are rotated
        DataPoints compute(const DataPoints &input, const TransformationParameters &parameters) const override
        {
            pgicp_ctx *c = ctx ? ctx->get() : pgslam_amd::default_context();
            DataPoints out(input);
            double Tm[16];
            pgslam_amd::to_row_major16(parameters, Tm);
            const int n = (int)input.getNbPoints();
            if (n == 0) return out;
            // `out` is a copy of `input`: transformed in place (the call uploads its data once, not input AND output)
            check(c, A::transform(c, Tm, out.features.data(), out.features.rows(), out.features.data(), out.features.rows(), n, 0));
            for (const char *name : {"normals", "observationDirections"}) {
                if (!input.descriptorExists(name) || input.getDescriptorDimension(name) != 3) continue;
                const int row = input.getDescriptorStartingRow(name);
                check(c, A::transform(c, Tm, out.descriptors.data() + row, out.descriptors.rows(), out.descriptors.data() + row,
                                      out.descriptors.rows(), n, 1));
            }
            return out;
        }
    };
    struct Transformations : std::vector<std::shared_ptr<Transformation>> {
        //! LoopCloser.hpp:352 -- temp_icp.transformations.apply(reading, T)
        void apply(DataPoints &cloud, const TransformationParameters &parameters) const
        {
            DataPoints t(cloud);
            for (auto &tr : *this) t = tr->compute(t, parameters);
            cloud = t;
        }
    };

    // ------------------------------------------------------------------ DataPointsFilters
    struct DataPointsFilter {
        virtual ~DataPointsFilter() {}
        virtual void init() {}
        virtual void inPlaceFilter(DataPoints &cloud) = 0;
        //! the filter as an entry of pgicp_filter_cloud's list (the device pass keeps the points this host version keeps);
        //! false: the filter has no device form (it adds descriptors, or needs neighbours)
        virtual bool deviceSpec(pgicp_filter &) const { return false; }
        //! the same for a filter whose entry depends on the cloud it is about to see (a descriptor's row)
        virtual bool deviceSpec(pgicp_filter &f, const DataPoints &) const { return deviceSpec(f); }
        //! called once after a device pass that stood in for inPlaceFilter (filters whose parameters evolve from cloud to cloud)
        virtual void afterDevicePass() {}
    };
    struct IdentityDataPointsFilter : DataPointsFilter {
        void inPlaceFilter(DataPoints &) override {}
        bool deviceSpec(pgicp_filter &f) const override { std::memset(&f, 0, sizeof f); f.type = PGICP_FILTER_IDENTITY; return true; }
    };
    //! keeps the columns for which `keep(j)` holds, in order (features and descriptors)
    template <typename Pred>
    static void compactColumns(DataPoints &c, Pred keep)
    {
        const int n = (int)c.features.cols();
        int k = 0;
        for (int j = 0; j < n; j++) {
            if (!keep(j)) continue;
            if (k != j) {
                for (int i = 0; i < c.features.rows(); i++) c.features(i, k) = c.features(i, j);
                for (int i = 0; i < c.descriptors.rows(); i++) c.descriptors(i, k) = c.descriptors(i, j);
            }
            k++;
        }
        c.features.conservativeResize(c.features.rows(), k);
        if (c.descriptors.rows()) c.descriptors.conservativeResize(c.descriptors.rows(), k);
    }
    //! the build's seeded draw for item j, uniform in [0, 1): SplitMix64's finaliser of seed and index (reproducible, not
    //! rand()-parity); what every sampling filter compares with its probability
    static unsigned long long mix64(unsigned long long z)
    {
        z += 0x9E3779B97F4A7C15ULL; z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL; z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
        return z ^ (z >> 31);
    }
    static double seededDraw(unsigned long long seed, int j) { return (double)(mix64(seed * 0x100000001B3ULL + (unsigned long long)j) >> 11) / 9007199254740992.0; }
    //! keeps the columns idx[0 .. kept) (ascending), in order
    static void keepColumns(DataPoints &c, const int32_t *idx, int kept)
    {
        int k = 0;
        compactColumns(c, [&](int j) { if (k < kept && idx[k] == j) { k++; return true; } return false; });
    }
    //! the columns idx[0 .. kept), in that order (features and descriptors)
    static void gatherColumns(DataPoints &c, const int32_t *idx, int kept)
    {
        const int frows = (int)c.features.rows(), drows = (int)c.descriptors.rows();
        Matrix f(frows, kept), d(drows, kept);
        for (int o = 0; o < kept; o++) {
            const int i = idx[o];
            for (int r = 0; r < frows; r++) f(r, o) = c.features(r, i);
            for (int r = 0; r < drows; r++) d(r, o) = c.descriptors(r, i);
        }
        c.features = f;
        c.descriptors = d;
    }
    //! one column per idx[0 .. kept): rows 0-2 from `ox` (3 a point), rows 3.. of point idx[o], descriptors from `od` (drows a point)
    static void assemble(DataPoints &c, const T *ox, const T *od, const int32_t *idx, int kept)
    {
        const int frows = (int)c.features.rows(), drows = (int)c.descriptors.rows();
        Matrix f(frows, kept), d(drows, kept);
        for (int o = 0; o < kept; o++) {
            const int i = idx[o];
            for (int r = 0; r < 3; r++) f(r, o) = ox[3 * (size_t)o + r];
            for (int r = 3; r < frows; r++) f(r, o) = c.features(r, i);
            for (int r = 0; r < drows; r++) d(r, o) = od[(size_t)drows * o + r];
        }
        c.features = f;
        if (drows > 0) c.descriptors = d;
    }
    //! What the filters with a device form AND a host form of one statement share.  `ctx` is made when the filter first runs on
    //! the device, not when a YAML file is read (so the filter is not copyable); ranOnDevice(): which of the two forms the last
    //! inPlaceFilter took; deviceWanted(knob): a device is present and the environment does not say <knob>=1.
    struct DeviceBackedDataPointsFilter : DataPointsFilter {
        pgslam_amd::LazyContext ctx;
        bool onDevice = false;
        DeviceBackedDataPointsFilter() {}
        DeviceBackedDataPointsFilter(const DeviceBackedDataPointsFilter &) = delete;
        DeviceBackedDataPointsFilter &operator=(const DeviceBackedDataPointsFilter &) = delete;
        bool ranOnDevice() const { return onDevice; }
        static bool deviceWanted(const char *knob)
        {
            static const bool have_device = pgicp_device_count() > 0;
            const char *v = std::getenv(knob);
            return have_device && !(v && std::strcmp(v, "1") == 0);
        }
        //! the output buffers are kept from call to call and only grow (a 1 M-point map: no fresh pages)
        template <typename V> static void grow(V &v, size_t n) { if (v.size() < n) v.resize(n); }
        static void need3D(const DataPoints &c, const char *filter)
        {
            if (c.features.rows() != 4) throw std::runtime_error(std::string(filter) + ": only 3-D clouds (4 feature rows) are supported");
        }
        static void needNormals(const DataPoints &c, const char *filter)
        {
            if (!c.descriptorExists("normals") || c.getDescriptorDimension("normals") != 3)
                throw std::runtime_error(std::string(filter) + ": Error, cannot find normals in descriptors.");
        }
        //! What a box filter's device call returned (SamplingSurfaceNormal, Elipsoids), made into what its host recursion leaves: the
        //! kept columns in input order, rows 0-2 from the device (the box mean with samplingMethod 1, row 3 then 1), the other
        //! feature rows gathered, the descriptors compacted or averaged
        static void takeKept(DataPoints &c, const std::vector<int32_t> &idx, int kept, const Matrix &ox, const Matrix &od, int samplingMethod)
        {
            const int frows = (int)c.features.rows(), drows = (int)c.descriptors.rows();
            Matrix f(frows, kept), d(drows, kept);
            for (int o = 0; o < kept; o++) {
                const int i = idx[o];
                for (int r = 0; r < 3; r++) f(r, o) = ox(r, o);
                for (int r = 3; r < frows; r++) f(r, o) = c.features(r, i);
                if (samplingMethod != 0 && frows > 3) f(3, o) = T(1);
                for (int r = 0; r < drows; r++) d(r, o) = od(r, o);
            }
            c.features = f;
            if (drows > 0) c.descriptors = d;
        }
        //! a row that came packed from the device cut to its first `kept` columns, the kept points' (a row not asked for has none)
        static void head(Matrix &m, int kept)
        {
            Matrix h(m.rows(), m.cols() > 0 ? kept : 0);
            for (int o = 0; o < (int)h.cols(); o++) for (int r = 0; r < (int)m.rows(); r++) h(r, o) = m(r, o);
            m = h;
        }
    };
    //! [EXT] MaxDistDataPointsFilter{maxDist, dim} / MinDistDataPointsFilter{minDist, dim} (DataPointsFilters/MaxDist.cpp, MinDist.cpp):
    //! dim = -1: keeps points whose distance to the origin -- features.col(i).head(3).norm() in T -- is below |maxDist| (above
    //! |minDist|), strictly; dim = 0..2: keeps features(dim, i) < maxDist (> minDist).  A NaN fails either comparison.
    struct DistLimitDataPointsFilter : DataPointsFilter {
        T limit; bool keepInside; int dim;
        DistLimitDataPointsFilter(T l, bool inside, int d = -1) : limit(l), keepInside(inside), dim(d) {}
        bool deviceSpec(pgicp_filter &f) const override
        {
            std::memset(&f, 0, sizeof f);
            f.type = keepInside ? PGICP_FILTER_MAX_DIST : PGICP_FILTER_MIN_DIST; f.p[0] = (double)limit; f.p[1] = (double)(dim + 1);
            return true;
        }
        void inPlaceFilter(DataPoints &c) override
        {
            const T al = limit < (T)0 ? -limit : limit;
            compactColumns(c, [&](int j) {
                if (dim >= 0) return keepInside ? c.features(dim, j) < limit : c.features(dim, j) > limit;
                const T x = c.features(0, j), y = c.features(1, j), z = c.features(2, j);
                const T r = std::sqrt((x * x + y * y) + z * z);          // Eigen's .norm() of the three coordinates, in T
                return keepInside ? r < al : r > al;
            });
        }
    };
    //! [EXT] MaxQuantileOnAxisDataPointsFilter{dim, ratio} (DataPointsFilters/MaxQuantileOnAxis.cpp, restated as recalled in
    //! pgicp_quantile.h): keeps the points whose coordinate `dim` lies strictly below the k-th smallest one, k = (int)(T(n) * ratio)
    //! in T.  The host form is axis_quantile_host.hpp's statement (a lone host cloud is not worth an upload); as an entry of a
    //! device list (deviceSpec) the same cut is an exact radix select on the device.
    struct MaxQuantileOnAxisDataPointsFilter : DataPointsFilter {
        int dim; T ratio;
        explicit MaxQuantileOnAxisDataPointsFilter(int d = 0, T r = (T)0.5) : dim(d), ratio(r)
        {
            if (!pgslam_amd::axis_quantile::dim_ok(d)) throw std::runtime_error("MaxQuantileOnAxisDataPointsFilter: dim must be 0, 1 or 2");
            if (!pgslam_amd::axis_quantile::ratio_ok((double)r) || !(r > (T)0 && r < (T)1))
                throw std::runtime_error("MaxQuantileOnAxisDataPointsFilter: ratio must be in [1e-7, 0.9999999]");
        }
        bool deviceSpec(pgicp_filter &f) const override
        {
            std::memset(&f, 0, sizeof f);
            f.type = PGICP_FILTER_MAX_QUANTILE_ON_AXIS; f.p[0] = (double)dim; f.p[1] = (double)ratio;
            return true;
        }
        void inPlaceFilter(DataPoints &c) override
        {
            const int n = (int)c.features.cols();
            if (n == 0) return;
            if (c.features.rows() <= dim) throw std::runtime_error("MaxQuantileOnAxisDataPointsFilter: the cloud has no coordinate `dim`");
            const auto r = pgslam_amd::axis_quantile::select<T>(c.features.data() + dim, (long long)c.features.rows(), n, ratio);
            compactColumns(c, [&](int j) { return c.features(dim, j) < r.limit; });
        }
    };
    //! [EXT] BoundingBoxDataPointsFilter{xMin..zMax, removeInside}: a point is inside when every coordinate lies
    //! strictly between its bounds; removeInside = 1 (the default) drops the inside, 0 keeps only the inside
    struct BoundingBoxDataPointsFilter : DataPointsFilter {
        T lo[3], hi[3]; bool removeInside;
        BoundingBoxDataPointsFilter(const T l[3], const T h[3], bool rm) : removeInside(rm) { for (int a = 0; a < 3; a++) { lo[a] = l[a]; hi[a] = h[a]; } }
        bool deviceSpec(pgicp_filter &f) const override
        {
            std::memset(&f, 0, sizeof f);
            f.type = PGICP_FILTER_BOUNDING_BOX;
            for (int a = 0; a < 3; a++) { f.p[a] = (double)lo[a]; f.p[3 + a] = (double)hi[a]; }
            f.p[6] = removeInside ? 1.0 : 0.0;
            return true;
        }
        void inPlaceFilter(DataPoints &c) override
        {
            compactColumns(c, [&](int j) {
                bool in = true;
                for (int a = 0; a < 3; a++) in = in && lo[a] < c.features(a, j) && c.features(a, j) < hi[a];
                return in != removeInside;
            });
        }
    };
    //! [EXT] RemoveNaNDataPointsFilter: drops points with a NaN coordinate
    struct RemoveNaNDataPointsFilter : DataPointsFilter {
        bool deviceSpec(pgicp_filter &f) const override { std::memset(&f, 0, sizeof f); f.type = PGICP_FILTER_REMOVE_NAN; return true; }
        void inPlaceFilter(DataPoints &c) override
        {
            compactColumns(c, [&](int j) {
                for (int i = 0; i < c.features.rows(); i++) if (c.features(i, j) != c.features(i, j)) return false;
                return true;
            });
        }
    };
    //! [EXT] ObservationDirectionDataPointsFilter{x, y, z}: descriptor observationDirections = sensor position - point
    struct ObservationDirectionDataPointsFilter : DataPointsFilter {
        T c0[3];
        ObservationDirectionDataPointsFilter(T x, T y, T z) { c0[0] = x; c0[1] = y; c0[2] = z; }
        void inPlaceFilter(DataPoints &c) override
        {
            const int n = (int)c.features.cols();
            Matrix d(3, n);
            for (int j = 0; j < n; j++) {
                const T x[3] = {c.features(0, j), c.features(1, j), c.features(2, j)};
                T o[3];
                pgslam_amd::sensor_chain::observation_direction<T>(c0, x, o);
                for (int a = 0; a < 3; a++) d(a, j) = o[a];
            }
            c.addDescriptor("observationDirections", d);
        }
    };
    //! [EXT] OrientNormalsDataPointsFilter{towardCenter}: flips every normal that points away from (towardCenter = 1)
    //! or toward (0) the sensor; needs the normals and observationDirections descriptors
    struct OrientNormalsDataPointsFilter : DataPointsFilter {
        bool towardCenter;
        explicit OrientNormalsDataPointsFilter(bool t) : towardCenter(t) {}
        void inPlaceFilter(DataPoints &c) override
        {
            if (!c.descriptorExists("normals")) throw std::runtime_error("OrientNormalsDataPointsFilter: cannot find normals in descriptors");
            if (!c.descriptorExists("observationDirections")) throw std::runtime_error("OrientNormalsDataPointsFilter: cannot find observation directions in descriptors");
            const int rn = c.getDescriptorStartingRow("normals"), ro = c.getDescriptorStartingRow("observationDirections");
            const int n = (int)c.features.cols();
            for (int j = 0; j < n; j++) {
                const T nv[3] = {c.descriptors(rn, j), c.descriptors(rn + 1, j), c.descriptors(rn + 2, j)};
                const T ov[3] = {c.descriptors(ro, j), c.descriptors(ro + 1, j), c.descriptors(ro + 2, j)};
                if (pgslam_amd::sensor_chain::orient_flips<T>(nv, ov, towardCenter))
                    for (int a = 0; a < 3; a++) c.descriptors(rn + a, j) = -c.descriptors(rn + a, j);
            }
        }
    };
    //! [EXT] ShadowDataPointsFilter{eps} (DataPointsFilters/Shadow.cpp as restated in oracle/icp_oracle.c: orc_shadow_keep): keeps a
    //! point while |normal.normalized() . position.normalized()| > sin(eps) -- drops surfaces seen at a grazing angle from the sensor's
    //! origin.  Needs the normals descriptor; host side (it reads a descriptor the device input stage does not carry).
    struct ShadowDataPointsFilter : DataPointsFilter {
        T epsAngle, eps;
        explicit ShadowDataPointsFilter(T e) : epsAngle(e), eps(pgslam_amd::sensor_chain::shadow_threshold<T>(e)) {}
        void inPlaceFilter(DataPoints &c) override
        {
            if (!c.descriptorExists("normals")) throw std::runtime_error("ShadowDataPointsFilter: cannot find normals in descriptors");
            const int rn = c.getDescriptorStartingRow("normals");
            compactColumns(c, [&](int j) {
                const T nv[3] = {c.descriptors(rn, j), c.descriptors(rn + 1, j), c.descriptors(rn + 2, j)};
                const T x[3] = {c.features(0, j), c.features(1, j), c.features(2, j)};
                return pgslam_amd::sensor_chain::shadow_keep<T>(nv, x, eps);
            });
        }
    };
    //! [EXT] FixStepSamplingDataPointsFilter{startStep, endStep, stepMult} (DataPointsFilters/FixStepSampling.cpp): keeps points
    //! phase, phase + step, ...; after every cloud step *= stepMult, clamped at endStep in the direction of travel; init() goes back
    //! to startStep.  Upstream draws phase = rand() % step from the C library's global generator -- like RandomSampling there is
    //! nothing to be bit-exact against; here the phase is 0 (documented as NOT parity with upstream's sample, same density).
    struct FixStepSamplingDataPointsFilter : DataPointsFilter {
        double startStep, endStep, stepMult, step;
        explicit FixStepSamplingDataPointsFilter(double s, double e = -1, double m = 1) : startStep(s < 1 ? 1 : s), endStep(e < 1 ? startStep : e), stepMult(m), step(startStep) {}
        void init() override { step = startStep; }
        bool deviceSpec(pgicp_filter &f) const override { std::memset(&f, 0, sizeof f); f.type = PGICP_FILTER_FIX_STEP; f.p[0] = (double)(int)step; return true; }
        void afterDevicePass() override { advance(); }
        void advance()
        {
            const double delta = startStep * stepMult - startStep;
            step *= stepMult;
            if (delta < 0 && step < endStep) step = endStep;
            if (delta > 0 && step > endStep) step = endStep;
        }
        void inPlaceFilter(DataPoints &c) override
        {
            const int iStep = (int)step;
            compactColumns(c, [&](int j) { return j % iStep == 0; });
            advance();
        }
    };
    //! [EXT] RandomSamplingDataPointsFilter{prob}: upstream keeps a point when rand() / RAND_MAX < prob -- the C library's
    //! global generator, so no two runs (or platforms) agree and there is nothing to be bit-exact against.  Here the draw is
    //! a build-owned counter-based generator (SplitMix64 of seed and point index): the sample is reproducible, has the same
    //! distribution, and is documented as NOT bit-parity with upstream.  `seed` is an extra, optional parameter.
    struct RandomSamplingDataPointsFilter : DataPointsFilter {
        T prob; unsigned long long seed;
        RandomSamplingDataPointsFilter(T p, unsigned long long s) : prob(p), seed(s) {}
        bool deviceSpec(pgicp_filter &f) const override
        {
            if (seed >= (1ULL << 53)) return false;              // (the seed crosses the ABI as a double)
            std::memset(&f, 0, sizeof f);
            f.type = PGICP_FILTER_RANDOM_SAMPLING; f.p[0] = (double)prob; f.p[1] = (double)seed;
            return true;
        }
        static unsigned long long mix(unsigned long long z) { return mix64(z); }
        void inPlaceFilter(DataPoints &c) override
        {
            compactColumns(c, [&](int j) { return seededDraw(seed, j) < (double)prob; });
        }
    };
    //! [EXT] MaxPointCountDataPointsFilter{maxCount, seed} (DataPointsFilters/MaxPointCount.cpp as of the libpointmatcher pgslam was
    //! written against): when more than maxCount points arrive, a random sample with prob = T(maxCount) / T(N) -- about maxCount
    //! points survive.  The draw is RandomSampling's build-owned one (not rand()-parity, see there).
    struct MaxPointCountDataPointsFilter : DataPointsFilter {
        unsigned maxCount; unsigned long long seed;
        MaxPointCountDataPointsFilter(unsigned m, unsigned long long s) : maxCount(m < 1 ? 1 : m), seed(s) {}
        bool deviceSpec(pgicp_filter &f) const override
        {
            if (seed >= (1ULL << 53)) return false;
            std::memset(&f, 0, sizeof f);
            f.type = PGICP_FILTER_MAX_POINT_COUNT; f.p[0] = (double)maxCount; f.p[1] = (double)seed;
            return true;
        }
        void inPlaceFilter(DataPoints &c) override
        {
            const int n = (int)c.features.cols();
            if (!((double)n > (double)maxCount)) return;
            const double prob = (double)((T)maxCount / (T)n);
            compactColumns(c, [&](int j) { return seededDraw(seed, j) < prob; });
        }
    };
    //! [EXT] SurfaceNormalDataPointsFilter{knn, maxDist, epsilon, keepNormals, keepEigenValues}: normals (and,
    //! on request, eigenvalues) of every point from its knn neighbours, computed on the device by
    //! pgicp_surface_normals_*; the descriptors are appended as libpointmatcher appends them.  keepEigenVectors (`eigVectors`, 9
    //! rows: three columns in ascending-eigenvalue order), keepMatchedIds (`matchedIds`, knn rows, -1 = none), keepMeanDist
    //! (`meanDists`) and smoothNormals go through pgicp_surface_normals_ext_*; their statement, with its marked deviations from
    //! upstream, is in include/pgicp_normals_ext.h.
    struct SurfaceNormalDataPointsFilter : DataPointsFilter {
        int knn = 5; T maxDist = std::numeric_limits<T>::infinity(); bool keepNormals = true, keepEigenValues = false, keepDensities = false;
        bool keepEigenVectors = false, keepMatchedIds = false, keepMeanDist = false, smoothNormals = false;
        pgslam_amd::LazyContext ctx;                 // made when the filter first runs, not when a YAML file is read
        SurfaceNormalDataPointsFilter(int k, T md, bool kn, bool ke, bool kd = false, bool kev = false, bool kmi = false, bool kmd = false, bool sm = false)
            : knn(k), maxDist(md), keepNormals(kn), keepEigenValues(ke), keepDensities(kd), keepEigenVectors(kev), keepMatchedIds(kmi), keepMeanDist(kmd), smoothNormals(sm)
        {
            if (sm && !kn) throw std::runtime_error("SurfaceNormalDataPointsFilter: smoothNormals needs keepNormals (there is nothing to smooth into)");
        }
        //! an output only pgicp_surface_normals_ext_* makes
        bool wantsExt() const { return keepEigenVectors || keepMatchedIds || keepMeanDist || smoothNormals; }
        SurfaceNormalDataPointsFilter(const SurfaceNormalDataPointsFilter &) = delete;
        SurfaceNormalDataPointsFilter &operator=(const SurfaceNormalDataPointsFilter &) = delete;
        void inPlaceFilter(DataPoints &c) override
        {
            const int n = (int)c.features.cols();
            if (n == 0 || (!keepNormals && !keepEigenValues && !keepDensities && !wantsExt())) return;
            Matrix nrm(3, n), eig(3, n);
            const double md = std::isfinite((double)maxDist) ? (double)maxDist : 1e300;
            if (wantsExt()) {
                // upstream's order: normals, densities, eigValues, eigVectors, matchedIds, meanDists
                if (knn < (keepDensities ? 3 : 1) || knn > 32) throw std::runtime_error("SurfaceNormalDataPointsFilter: knn must be in [1, 32], in [3, 32] with keepDensities");
                Matrix dens(1, keepDensities ? n : 0), vec(9, keepEigenVectors ? n : 0), ids(knn, keepMatchedIds ? n : 0), dist(1, keepMeanDist ? n : 0);
                check(ctx, pgslam_amd::Abi<T>::normals_ext(ctx, c.features.data(), (int)c.features.rows(), n, knn, md, smoothNormals ? 1 : 0,
                                                           keepNormals ? nrm.data() : nullptr, 3, keepEigenValues ? eig.data() : nullptr,
                                                           keepEigenVectors ? vec.data() : nullptr, keepMeanDist ? dist.data() : nullptr,
                                                           keepMatchedIds ? ids.data() : nullptr, keepDensities ? dens.data() : nullptr));
                if (keepNormals) c.setDescriptor("normals", nrm);
                if (keepDensities) c.setDescriptor("densities", dens);
                if (keepEigenValues) c.setDescriptor("eigValues", eig);
                if (keepEigenVectors) c.setDescriptor("eigVectors", vec);
                if (keepMatchedIds) c.setDescriptor("matchedIds", ids);
                if (keepMeanDist) c.setDescriptor("meanDists", dist);
                return;
            }
            if (keepDensities) {
                // [EXT] computeDensity: neighbours found / volume of the sphere that holds them around their MEAN, in T (the oracle's
                // orc_densities) -- an epilogue of the device's normals kernel (pgicp_surface_densities_*): no id table comes back
                if (knn < 3 || knn > 32) throw std::runtime_error("SurfaceNormalDataPointsFilter: keepDensities needs knn in [3, 32]");
                Matrix dens(1, n);
                check(ctx, pgslam_amd::Abi<T>::densities(ctx, c.features.data(), (int)c.features.rows(), n, knn, md, keepNormals ? nrm.data() : nullptr, 3,
                                                         keepEigenValues ? eig.data() : nullptr, dens.data()));
                if (keepNormals) c.setDescriptor("normals", nrm);
                c.setDescriptor("densities", dens);
            } else {
                check(ctx, pgslam_amd::Abi<T>::normals(ctx, c.features.data(), (int)c.features.rows(), n, knn, md, nrm.data(), 3,
                                                       keepEigenValues ? eig.data() : nullptr));
                if (keepNormals) c.setDescriptor("normals", nrm);
            }
            if (keepEigenValues) c.setDescriptor("eigValues", eig);
        }
    };
    //! eigen-decomposition of a symmetric 3x3 (cyclic Jacobi in double): ev[k], columns V[.][k]
    static void symEigen3(double A[3][3], double V[3][3], double ev[3])
    {
        for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) V[i][j] = i == j ? 1.0 : 0.0;
        for (int sweep = 0; sweep < 50; sweep++) {
            const double off = A[0][1] * A[0][1] + A[0][2] * A[0][2] + A[1][2] * A[1][2];
            if (off == 0.0) break;
            for (int p = 0; p < 2; p++)
                for (int q = p + 1; q < 3; q++) {
                    if (A[p][q] == 0.0) continue;
                    const double theta = (A[q][q] - A[p][p]) / (2.0 * A[p][q]);
                    const double t = (theta >= 0.0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
                    const double cs = 1.0 / std::sqrt(t * t + 1.0), sn = t * cs;
                    for (int r = 0; r < 3; r++) { const double a = A[r][p], b = A[r][q]; A[r][p] = cs * a - sn * b; A[r][q] = sn * a + cs * b; }
                    for (int r = 0; r < 3; r++) { const double a = A[p][r], b = A[q][r]; A[p][r] = cs * a - sn * b; A[q][r] = sn * a + cs * b; }
                    for (int r = 0; r < 3; r++) { const double a = V[r][p], b = V[r][q]; V[r][p] = cs * a - sn * b; V[r][q] = sn * a + cs * b; }
                }
        }
        for (int i = 0; i < 3; i++) ev[i] = A[i][i];
    }
    //! The host form of the box filters (SamplingSurfaceNormalDataPointsFilter, ElipsoidsDataPointsFilter), the statement the device
    //! kernels restate bit for bit (pgslam_amd/csrc/k_ssn.inc): the cloud is cut at the median of its widest carried side, ordered by
    //! (coordinate, index), until a range holds at most knn points; such a box's extent, mean and scatter are summed in T in box
    //! order and decomposed in double; a box larger than maxBoxDim, of rank < 2 or (minPlanarity > 0) of a planarity below
    //! minPlanarity is dropped; a fused box keeps every point with probability `ratio` (samplingMethod 0) or its first point, moved
    //! to its mean, the existing descriptors averaged (samplingMethod 1).  rowsOf(i) says where kept point i's rows of its box go
    //! (elipsoids_host.hpp's assemble_rows writes them; the density is pgicp_density.h's statement over the members around the
    //! box's mean).  Returns the keep flag of every point; c's columns are not compacted yet.
    struct BoxPointRows { pgslam_amd::elipsoids::Rows<T> rows; T *dens = nullptr; };
    template <typename RowsOf>
    static std::vector<char> boxFilterHost(DataPoints &c, int knn, int samplingMethod, T maxBoxDim, T minPlanarity, T ratio, unsigned long long seed,
                                           bool averageExistingDescriptors, bool wantDensity, bool wantShape, RowsOf rowsOf)
    {
        namespace eh = pgslam_amd::elipsoids;
        const int n = (int)c.features.cols(), drows = (int)c.descriptors.rows();
        std::vector<int> idx(n);
        for (int i = 0; i < n; i++) idx[i] = i;
        std::vector<char> keep(n, 0);
        struct Range { int first, last; T lo[3], hi[3]; };
        std::vector<Range> stack;
        Range all{0, n, {c.features(0, 0), c.features(1, 0), c.features(2, 0)}, {c.features(0, 0), c.features(1, 0), c.features(2, 0)}};
        for (int i = 0; i < n; i++)
            for (int a = 0; a < 3; a++) { const T v = c.features(a, i); if (v < all.lo[a]) all.lo[a] = v; if (v > all.hi[a]) all.hi[a] = v; }
        stack.push_back(all);
        Matrix merged(drows > 0 ? drows : 1, 1);
        while (!stack.empty()) {
            const Range R = stack.back();
            stack.pop_back();
            const int count = R.last - R.first;
            if (count > knn) {
                int cut = 0;
                for (int a = 1; a < 3; a++) if (R.hi[a] - R.lo[a] > R.hi[cut] - R.lo[cut]) cut = a;
                std::sort(idx.begin() + R.first, idx.begin() + R.last, [&](int i, int j) {
                    const T x = c.features(cut, i), y = c.features(cut, j);
                    return x < y || (x == y && i < j);
                });
                const int right = count / 2, left = count - right;
                const T cv = c.features(cut, idx[R.first + left]);
                Range L = R, G = R;
                L.last = R.first + left; L.hi[cut] = cv;
                G.first = R.first + left; G.lo[cut] = cv;
                stack.push_back(G);                  // (the left half is taken first; boxes are independent of one another)
                stack.push_back(L);
                continue;
            }
            // ---- a box
            T lo[3], hi[3], sum[3] = {0, 0, 0};
            for (int a = 0; a < 3; a++) { lo[a] = c.features(a, idx[R.first]); hi[a] = lo[a]; }
            for (int k = R.first; k < R.last; k++)
                for (int a = 0; a < 3; a++) { const T v = c.features(a, idx[k]); if (v < lo[a]) lo[a] = v; if (v > hi[a]) hi[a] = v; sum[a] += v; }
            T box = hi[0] - lo[0];
            if (hi[1] - lo[1] > box) box = hi[1] - lo[1];
            if (hi[2] - lo[2] > box) box = hi[2] - lo[2];
            if (box > maxBoxDim) continue;
            const T mean[3] = {sum[0] / (T)count, sum[1] / (T)count, sum[2] / (T)count};
            const T mx = mean[0], my = mean[1], mz = mean[2];
            T c00 = 0, c01 = 0, c02 = 0, c11 = 0, c12 = 0, c22 = 0;
            for (int k = R.first; k < R.last; k++) {
                const int i = idx[k];
                const T dx = c.features(0, i) - mx, dy = c.features(1, i) - my, dz = c.features(2, i) - mz;
                c00 += dx * dx; c01 += dx * dy; c02 += dx * dz; c11 += dy * dy; c12 += dy * dz; c22 += dz * dz;
            }
            double A[3][3] = {{(double)c00, (double)c01, (double)c02}, {(double)c01, (double)c11, (double)c12}, {(double)c02, (double)c12, (double)c22}}, V[3][3], ev[3];
            symEigen3(A, V, ev);
            int l = 0, h = 0;
            for (int k = 1; k < 3; k++) { if (ev[k] < ev[l]) l = k; if (ev[k] > ev[h]) h = k; }
            const int mid = 3 - l - h;
            if (l == h || !(ev[h] > 0.0) || !(ev[mid] > 3.0 * (double)std::numeric_limits<T>::epsilon() * ev[h])) continue;   // rank < 2
            // include/pgicp_elipsoids.h: the shape values and the planarity drop, before the draw
            eh::Shape<T> shape{};
            if (minPlanarity > T(0) || wantShape) {
                shape = eh::shape_of<T>(ev, l, mid, h);
                if (eh::dropped_by_planarity<T>(shape, minPlanarity)) continue;
            }
            // include/pgicp_ssn_ext.h: the box's density
            T boxDens = 0;
            if (wantDensity) {
                T r2 = 0;
                for (int k = R.first; k < R.last; k++) {
                    const int i = idx[k];
                    const T dx = c.features(0, i) - mx, dy = c.features(1, i) - my, dz = c.features(2, i) - mz;
                    const T q = (dx * dx + dy * dy) + dz * dz;
                    if (q > r2) r2 = q;
                }
                const T r = std::sqrt(r2);
                boxDens = (T)count / ((T)((4.0 / 3.0) * 3.14159265358979323846) * ((r * r) * r));
            }
            const T scatter[6] = {c00, c01, c02, c11, c12, c22};
            auto rowsTo = [&](int i) {
                keep[i] = 1;
                const BoxPointRows o = rowsOf(i);
                eh::assemble_rows<T>(count, mean, scatter, ev, V, l, mid, h, shape, o.rows);
                if (o.dens) *o.dens = boxDens;
            };
            if (samplingMethod == 0) {
                for (int k = R.first; k < R.last; k++)
                    if (seededDraw(seed, idx[k]) < (double)ratio) rowsTo(idx[k]);
            } else {
                const int i = idx[R.first];
                rowsTo(i);
                if (drows > 0 && averageExistingDescriptors) {
                    for (int r = 0; r < drows; r++) merged(r, 0) = 0;
                    for (int k = R.first; k < R.last; k++) for (int r = 0; r < drows; r++) merged(r, 0) += c.descriptors(r, idx[k]);
                    for (int r = 0; r < drows; r++) c.descriptors(r, i) = merged(r, 0) / (T)count;
                }
                c.features(0, i) = mx; c.features(1, i) = my; c.features(2, i) = mz;
                if (c.features.rows() > 3) c.features(3, i) = T(1);
            }
        }
        return keep;
    }
    //! [EXT] SamplingSurfaceNormalDataPointsFilter{ratio, knn, samplingMethod, maxBoxDim, averageExistingDescriptors, keepNormals}
    //! (DataPointsFilters/SamplingSurfaceNormal.cpp; upstream's setDefault() reference filter): the cloud is cut at the median of
    //! its widest dimension until a range holds at most knn points; each such box gets ONE normal (PCA of its points) and keeps
    //! every point with probability `ratio` (samplingMethod 0) or one point moved to its mean, the existing descriptors
    //! averaged (samplingMethod 1); boxes larger than maxBoxDim or of rank < 2 are dropped; the kept points stay in cloud order.
    //! The statement is the oracle's (oracle/icp_oracle.c orc_sampling_surface_normal, which says what is upstream's and what
    //! cannot be: nth_element's arrangement -> a sort on (coordinate, index); rand() -> the seeded draw; EigenSolver -> Jacobi).
    //! It runs once per keyframe / map, on the reference (Localizer.hpp:314-315), and per loop-closure candidate: on the device
    //! (pgicp_sampling_surface_normal_*, the same bits) when there is one, unless PGSLAM_HOST_SAMPLING_NORMALS=1 or the device
    //! refuses the cloud (a NaN or infinite coordinate, an out-of-range knn); then the host recursion (boxFilterHost, above).
    //! keepDensities (`densities`, 1 row), keepEigenValues (`eigValues`, 3 rows, ascending) and keepEigenVectors (`eigVectors`, 9 rows:
    //! three columns in that order) append the kept point's BOX's values after `normals`, in upstream's order; they go through
    //! pgicp_sampling_surface_normal_ext_*, and the host recursion computes them by the same statement (include/pgicp_ssn_ext.h,
    //! with its marked deviations from upstream), so the two forms agree bit for bit.  From YAML keepEigenValues and
    //! keepEigenVectors load; `keepDensities: 1` is still refused there (a constructed filter carries densities).
    struct SamplingSurfaceNormalDataPointsFilter : DeviceBackedDataPointsFilter {
        using DeviceBackedDataPointsFilter::ctx; using DeviceBackedDataPointsFilter::onDevice;
        T ratio; int knn, samplingMethod; T maxBoxDim; bool averageExistingDescriptors, keepNormals; unsigned long long seed;
        bool keepDensities, keepEigenValues, keepEigenVectors;
        SamplingSurfaceNormalDataPointsFilter(T r = T(0.5), int k = 7, int method = 0, T box = std::numeric_limits<T>::infinity(), bool avg = true,
                                              bool kn = true, unsigned long long sd = 1, bool kd = false, bool ke = false, bool kev = false)
            : ratio(r), knn(k), samplingMethod(method), maxBoxDim(box), averageExistingDescriptors(avg), keepNormals(kn), seed(sd),
              keepDensities(kd), keepEigenValues(ke), keepEigenVectors(kev) {}
        //! an output only pgicp_sampling_surface_normal_ext_* makes
        bool wantsExt() const { return keepDensities || keepEigenValues || keepEigenVectors; }
        //! upstream's order after `normals`: densities, eigValues, eigVectors (each overwritten when it exists)
        void setExtDescriptors(DataPoints &c, const Matrix &dens, const Matrix &eig, const Matrix &vec) const
        {
            if (keepDensities) c.setDescriptor("densities", dens);
            if (keepEigenValues) c.setDescriptor("eigValues", eig);
            if (keepEigenVectors) c.setDescriptor("eigVectors", vec);
        }
        //! the device form; false (the cloud untouched) when the device refuses the arguments
        bool deviceFilter(DataPoints &c)
        {
            const int n = (int)c.features.cols(), frows = (int)c.features.rows(), drows = (int)c.descriptors.rows();
            Matrix ox(3, n), on(3, n), od(drows > 0 ? drows : 1, n);
            Matrix dens(1, keepDensities ? n : 0), eig(3, keepEigenValues ? n : 0), vec(9, keepEigenVectors ? n : 0);
            std::vector<int32_t> idx((size_t)n);
            int kept = 0;
            const int st = !wantsExt()
                ? pgslam_amd::Abi<T>::sampling_normals(ctx, c.features.data(), frows, n, knn, (double)ratio, samplingMethod, (double)maxBoxDim,
                                                                (uint64_t)seed, drows > 0 ? c.descriptors.data() : nullptr, drows,
                                                                averageExistingDescriptors ? 1 : 0, ox.data(), on.data(), drows > 0 ? od.data() : nullptr,
                                                                idx.data(), &kept)
                : pgslam_amd::Abi<T>::sampling_normals_ext(ctx, c.features.data(), frows, n, knn, (double)ratio, samplingMethod, (double)maxBoxDim,
                                                           (uint64_t)seed, drows > 0 ? c.descriptors.data() : nullptr, drows,
                                                           averageExistingDescriptors ? 1 : 0, ox.data(), on.data(), drows > 0 ? od.data() : nullptr,
                                                           idx.data(), &kept, keepEigenValues ? eig.data() : nullptr,
                                                           keepEigenVectors ? vec.data() : nullptr, keepDensities ? dens.data() : nullptr);
            if (st == PGICP_ERR_ARG) return false;
            check(ctx, st);
            this->takeKept(c, idx, kept, ox, od, samplingMethod);
            this->head(on, kept);
            if (keepNormals) c.setDescriptor("normals", on);
            if (wantsExt()) {
                this->head(dens, kept); this->head(eig, kept); this->head(vec, kept);
                setExtDescriptors(c, dens, eig, vec);
            }
            return true;
        }
        void inPlaceFilter(DataPoints &c) override
        {
            onDevice = false;
            const int n = (int)c.features.cols();
            if (n == 0) return;
            if (this->deviceWanted("PGSLAM_HOST_SAMPLING_NORMALS") && deviceFilter(c)) { onDevice = true; return; }
            Matrix nrm(3, n);
            Matrix dens(1, keepDensities ? n : 0), eig(3, keepEigenValues ? n : 0), vec(9, keepEigenVectors ? n : 0);
            const std::vector<char> keep = boxFilterHost(c, knn, samplingMethod, maxBoxDim, T(0), ratio, seed, averageExistingDescriptors,
                                                         keepDensities, false, [&](int i) {
                BoxPointRows o;               // (a matrix column is contiguous)
                o.rows.normal = &nrm(0, i);
                if (keepEigenValues) o.rows.eig = &eig(0, i);
                if (keepEigenVectors) o.rows.vec = &vec(0, i);
                if (keepDensities) o.dens = &dens(0, i);
                return o;
            });
            if (keepNormals) c.setDescriptor("normals", nrm);
            if (wantsExt()) setExtDescriptors(c, dens, eig, vec);
            compactColumns(c, [&](int j) { return keep[j] != 0; });
        }
    };
    //! [EXT] ElipsoidsDataPointsFilter{ratio, knn, samplingMethod, maxBoxDim, minPlanarity, averageExistingDescriptors, keepNormals,
    //! keepDensities, keepEigenValues, keepEigenVectors, keepCovariances, keepWeights, keepMeans, keepShapes} (DataPointsFilters/
    //! Elipsoids.cpp): SamplingSurfaceNormalDataPointsFilter's tree, every box summarised as an ellipsoid; a box whose planarity is below
    //! minPlanarity (> 0) is dropped.  The statement, with its marked deviations from upstream, is in include/pgicp_elipsoids.h; the
    //! shape values, the planarity test and the row assembly are elipsoids_host.hpp's, which the device kernel shares.  The descriptors
    //! are appended in this order, each only when asked, each overwriting a descriptor of the same name: `normals` (3), `densities` (1),
    //! `eigValues` (3, ascending), `eigVectors` (9), `covariance` (9, the scatter sums, not normalised), `weights` (1, the box's count),
    //! `means` (3), `shapes` (3: planarity, cylindricality, sphericality).  3-D clouds.  On the device (pgicp_elipsoids_*, the same bits)
    //! when there is one, unless PGSLAM_HOST_ELIPSOIDS=1 or the device refuses the arguments; then the host recursion (boxFilterHost,
    //! the one SamplingSurfaceNormal runs).  No deviceSpec: a chain that holds it takes the per-filter path (it changes values).
    //! maxTimeWindow: this DataPoints carries no times, so only +inf (the default) is accepted.  From YAML keepNormals must be given.
    struct ElipsoidsDataPointsFilter : DeviceBackedDataPointsFilter {
        using DeviceBackedDataPointsFilter::ctx; using DeviceBackedDataPointsFilter::onDevice;
        T ratio; int knn, samplingMethod; T maxBoxDim, minPlanarity; bool averageExistingDescriptors, keepNormals;
        bool keepDensities, keepEigenValues, keepEigenVectors, keepCovariances, keepWeights, keepMeans, keepShapes;
        unsigned long long seed; T maxTimeWindow;
        ElipsoidsDataPointsFilter(T r = T(0.5), int k = 7, int method = 0, T box = std::numeric_limits<T>::infinity(), T minPlan = T(0), bool avg = true,
                                  bool kn = true, bool kd = false, bool ke = false, bool kev = false, bool kc = false, bool kw = false, bool km = false,
                                  bool ks = false, unsigned long long sd = 1, T timeWindow = std::numeric_limits<T>::infinity())
            : ratio(r), knn(k), samplingMethod(method), maxBoxDim(box), minPlanarity(minPlan), averageExistingDescriptors(avg), keepNormals(kn),
              keepDensities(kd), keepEigenValues(ke), keepEigenVectors(kev), keepCovariances(kc), keepWeights(kw), keepMeans(km), keepShapes(ks),
              seed(sd), maxTimeWindow(timeWindow)
        {
            if (!pgslam_amd::elipsoids::min_planarity_ok((double)minPlan)) throw std::runtime_error("ElipsoidsDataPointsFilter: minPlanarity must be finite and in [0, 1]");
            if (!(timeWindow == std::numeric_limits<T>::infinity()))
                throw std::runtime_error("ElipsoidsDataPointsFilter: maxTimeWindow is not supported (the cloud carries no times): leave it out or give inf");
        }
        //! the rows of every input point (filled for the kept ones), one matrix a row, empty when not asked for
        struct RowSet {
            Matrix nrm, dens, eig, vec, cov, wgt, mean, shp;
            RowSet(const ElipsoidsDataPointsFilter &f, int n)
                : nrm(3, n), dens(1, f.keepDensities ? n : 0), eig(3, f.keepEigenValues ? n : 0), vec(9, f.keepEigenVectors ? n : 0),
                  cov(9, f.keepCovariances ? n : 0), wgt(1, f.keepWeights ? n : 0), mean(3, f.keepMeans ? n : 0), shp(3, f.keepShapes ? n : 0) {}
        };
        //! the order of the statement (each overwritten when it exists)
        void setDescriptors(DataPoints &c, const RowSet &s) const
        {
            if (keepNormals) c.setDescriptor("normals", s.nrm);
            if (keepDensities) c.setDescriptor("densities", s.dens);
            if (keepEigenValues) c.setDescriptor("eigValues", s.eig);
            if (keepEigenVectors) c.setDescriptor("eigVectors", s.vec);
            if (keepCovariances) c.setDescriptor("covariance", s.cov);
            if (keepWeights) c.setDescriptor("weights", s.wgt);
            if (keepMeans) c.setDescriptor("means", s.mean);
            if (keepShapes) c.setDescriptor("shapes", s.shp);
        }
        //! the device form; false (the cloud untouched) when the device refuses the arguments
        bool deviceFilter(DataPoints &c)
        {
            const int n = (int)c.features.cols(), frows = (int)c.features.rows(), drows = (int)c.descriptors.rows();
            Matrix ox(3, n), od(drows > 0 ? drows : 1, n);
            RowSet s(*this, n);
            std::vector<int32_t> idx((size_t)n);
            int kept = 0;
            auto out = [](Matrix &m) { return m.cols() > 0 ? m.data() : nullptr; };
            const int st = pgslam_amd::Abi<T>::elipsoids(ctx, c.features.data(), frows, n, knn, (double)ratio, samplingMethod, (double)maxBoxDim,
                                                         (double)minPlanarity, (uint64_t)seed, drows > 0 ? c.descriptors.data() : nullptr, drows,
                                                         averageExistingDescriptors ? 1 : 0, ox.data(), keepNormals ? s.nrm.data() : nullptr,
                                                         drows > 0 ? od.data() : nullptr, idx.data(), &kept, out(s.eig), out(s.vec), out(s.dens),
                                                         out(s.cov), out(s.wgt), out(s.mean), out(s.shp));
            if (st == PGICP_ERR_ARG) return false;
            check(ctx, st);
            this->takeKept(c, idx, kept, ox, od, samplingMethod);
            for (Matrix *m : {&s.nrm, &s.dens, &s.eig, &s.vec, &s.cov, &s.wgt, &s.mean, &s.shp}) this->head(*m, kept);
            setDescriptors(c, s);
            return true;
        }
        void inPlaceFilter(DataPoints &c) override
        {
            onDevice = false;
            const int n = (int)c.features.cols();
            if (n == 0) return;
            this->need3D(c, "ElipsoidsDataPointsFilter");
            if (this->deviceWanted("PGSLAM_HOST_ELIPSOIDS") && deviceFilter(c)) { onDevice = true; return; }
            RowSet s(*this, n);
            const std::vector<char> keep = boxFilterHost(c, knn, samplingMethod, maxBoxDim, minPlanarity, ratio, seed, averageExistingDescriptors,
                                                         keepDensities, keepShapes, [&](int i) {
                BoxPointRows o;               // (a matrix column is contiguous)
                o.rows.normal = &s.nrm(0, i);
                if (keepEigenValues) o.rows.eig = &s.eig(0, i);
                if (keepEigenVectors) o.rows.vec = &s.vec(0, i);
                if (keepCovariances) o.rows.cov = &s.cov(0, i);
                if (keepWeights) o.rows.weight = &s.wgt(0, i);
                if (keepMeans) o.rows.mean = &s.mean(0, i);
                if (keepShapes) o.rows.shape = &s.shp(0, i);
                if (keepDensities) o.dens = &s.dens(0, i);
                return o;
            });
            setDescriptors(c, s);
            compactColumns(c, [&](int j) { return keep[j] != 0; });
        }
    };
    //! [EXT] VoxelGridDataPointsFilter{vSizeX, vSizeY, vSizeZ, useCentroid, averageExistingDescriptors} (DataPointsFilters/
    //! VoxelGrid.cpp): one point per non-empty voxel of a grid anchored at the cloud's minimum -- the voxel's centroid (summed in
    //! ascending index) or centre, row 3 and further feature rows the voxel's first point's, the descriptors averaged or the first
    //! point's -- in ascending first-point index.  The statement, with its marked deviations, is in include/pgicp.h
    //! (pgicp_voxel_grid_*).  3-D clouds only.  On the device (the same bits) when there is one, unless PGSLAM_HOST_VOXEL_GRID=1
    //! or the device refuses the cloud; then the host form below, which sorts (key, index) instead of allocating the dense
    //! grid.  No deviceSpec: a chain that holds it takes the per-filter path (it changes values, pgicp_filter_cloud only drops
    //! points).  From YAML the three sizes come together or not at all (upstream fills a missing one with 1 m; here one or two
    //! sizes alone are refused).
    struct VoxelGridDataPointsFilter : DeviceBackedDataPointsFilter {
        using DeviceBackedDataPointsFilter::ctx; using DeviceBackedDataPointsFilter::onDevice;
        T vSizeX, vSizeY, vSizeZ; bool useCentroid, averageExistingDescriptors;
        std::vector<T> oxBuf, odBuf;                 // the device form's outputs, kept from call to call (a 1 M-point map: no fresh pages)
        std::vector<int32_t> idxBuf;
        VoxelGridDataPointsFilter(T vx = T(1), T vy = T(1), T vz = T(1), bool cen = true, bool avg = true)
            : vSizeX(vx), vSizeY(vy), vSizeZ(vz), useCentroid(cen), averageExistingDescriptors(avg)
        {
            for (T v : {vx, vy, vz})
                if (!(v > T(0)) || !std::isfinite(v)) throw std::runtime_error("VoxelGridDataPointsFilter: vSizeX, vSizeY and vSizeZ must be finite and > 0");
        }
        //! the device form; false (the cloud untouched) when the device refuses the arguments
        bool deviceFilter(DataPoints &c)
        {
            const int n = (int)c.features.cols(), frows = (int)c.features.rows(), drows = (int)c.descriptors.rows();
            this->grow(oxBuf, 3 * (size_t)n);
            this->grow(odBuf, (size_t)drows * n);
            this->grow(idxBuf, (size_t)n);
            const double v[3] = {(double)vSizeX, (double)vSizeY, (double)vSizeZ};
            int kept = 0;
            const int st = pgslam_amd::Abi<T>::voxel_grid(ctx, c.features.data(), frows, n, v, useCentroid ? 1 : 0, drows > 0 ? c.descriptors.data() : nullptr,
                                                          drows, averageExistingDescriptors ? 1 : 0, oxBuf.data(), drows > 0 ? odBuf.data() : nullptr,
                                                          idxBuf.data(), &kept);
            if (st == PGICP_ERR_ARG) return false;
            check(ctx, st);
            assemble(c, oxBuf.data(), odBuf.data(), idxBuf.data(), kept);
            return true;
        }
        //! the host form: the same statement, with a sort of (key, index) for the dense voxel array
        void hostFilter(DataPoints &c)
        {
            const int n = (int)c.features.cols(), drows = (int)c.descriptors.rows();
            const T v[3] = {vSizeX, vSizeY, vSizeZ};
            T lo[3], hi[3], minB[3];
            unsigned long long nd[3];
            for (int a = 0; a < 3; a++) { lo[a] = c.features(a, 0); hi[a] = lo[a]; }
            for (int i = 0; i < n; i++)
                for (int a = 0; a < 3; a++) {
                    const T x = c.features(a, i);
                    if (!std::isfinite(x))
                        throw std::runtime_error("VoxelGridDataPointsFilter: a coordinate is NaN or infinite (put a RemoveNaNDataPointsFilter ahead of it)");
                    if (x < lo[a]) lo[a] = x;
                    if (x > hi[a]) hi[a] = x;
                }
            for (int a = 0; a < 3; a++) {
                minB[a] = lo[a] / v[a];
                const T maxB = hi[a] / v[a];
                const T d = (T(1) + maxB) - minB[a];
                if (!(d < T(2147483648.0)))
                    throw std::runtime_error("VoxelGridDataPointsFilter: the grid is too fine (a numDiv >= 2^31; a RemoveNaNDataPointsFilter or a bounding box ahead of it may help)");
                nd[a] = (unsigned long long)(unsigned)d;
            }
            if ((unsigned __int128)(nd[0] * nd[1]) * nd[2] >= ((unsigned __int128)1 << 62))
                throw std::runtime_error("VoxelGridDataPointsFilter: the grid is too fine (numDivX numDivY numDivZ >= 2^62; a RemoveNaNDataPointsFilter or a bounding box ahead of it may help)");
            std::vector<std::pair<unsigned long long, int>> kv((size_t)n);
            for (int i = 0; i < n; i++) {
                unsigned long long ia[3];
                for (int a = 0; a < 3; a++) ia[a] = (unsigned long long)(unsigned)std::floor(c.features(a, i) / v[a] - minB[a]);
                kv[i] = {ia[0] + ia[1] * nd[0] + ia[2] * (nd[0] * nd[1]), i};
            }
            std::sort(kv.begin(), kv.end());
            struct Vox { int first, start, count; };
            std::vector<Vox> vox;
            for (int s = 0; s < n; s++) {
                if (s == 0 || kv[s].first != kv[s - 1].first) vox.push_back({kv[s].second, s, 0});
                vox.back().count++;
            }
            std::sort(vox.begin(), vox.end(), [](const Vox &a, const Vox &b) { return a.first < b.first; });
            const int kept = (int)vox.size();
            Matrix ox(3, kept), od(drows > 0 ? drows : 1, kept);
            std::vector<int32_t> idx((size_t)kept);
            for (int o = 0; o < kept; o++) {
                const Vox &V = vox[o];
                const int i = V.first;
                idx[o] = i;
                const T cnt = (T)V.count;
                if (useCentroid) {
                    for (int a = 0; a < 3; a++) {
                        T sum = c.features(a, i);
                        for (int k = 1; k < V.count; k++) sum += c.features(a, kv[V.start + k].second);
                        ox(a, o) = V.count == 1 ? sum : sum / cnt;
                    }
                } else {
                    const unsigned long long key = kv[V.start].first, pl = nd[0] * nd[1];
                    const unsigned long long k = key / pl, j = (key - k * pl) / nd[0], ii = key - k * pl - j * nd[0];
                    const unsigned long long ia[3] = {ii, j, k};
                    for (int a = 0; a < 3; a++) { const T b = minB[a] + (T)ia[a], m = b * v[a]; ox(a, o) = m + v[a] / T(2); }
                }
                for (int r = 0; r < drows; r++) {
                    T sum = c.descriptors(r, i);
                    if (averageExistingDescriptors) {
                        for (int k = 1; k < V.count; k++) sum += c.descriptors(r, kv[V.start + k].second);
                        if (V.count > 1) sum = sum / cnt;
                    }
                    od(r, o) = sum;
                }
            }
            assemble(c, ox.data(), od.data(), idx.data(), kept);
        }
        void inPlaceFilter(DataPoints &c) override
        {
            onDevice = false;
            this->need3D(c, "VoxelGridDataPointsFilter");
            if (c.features.cols() == 0) return;
            if (this->deviceWanted("PGSLAM_HOST_VOXEL_GRID") && deviceFilter(c)) { onDevice = true; return; }
            hostFilter(c);
        }
    };
    //! [EXT] CovarianceSamplingDataPointsFilter{nbSample, torqueNorm} (DataPointsFilters/CovarianceSampling.cpp): the stability
    //! sampler of Gelfand et al. 2003 -- the nbSample points that best constrain the six degrees of freedom of the point-to-plane
    //! solve, in pick order.  Needs the `normals` descriptor.  The statement, with its marked deviations, is in
    //! include/pgicp_covsample.h.  3-D clouds only.  On the device (pgicp_covariance_sampling_*) when there is one, unless
    //! PGSLAM_HOST_INPUT_STAGE=1; else the host form of the same statement (covsample_host.hpp): the same picks bit for bit given
    //! the same frame -- the host form sums its frame in index order, the device in a tree, so the two frames may differ in
    //! their last bits.  No deviceSpec: a chain that holds it takes the per-filter path (the picks come in pick order,
    //! pgicp_filter_cloud only drops points).  lastFrame: the last inPlaceFilter's frame.
    struct CovarianceSamplingDataPointsFilter : DeviceBackedDataPointsFilter {
        using DeviceBackedDataPointsFilter::ctx; using DeviceBackedDataPointsFilter::onDevice;
        enum TorqueNormMethod { L1 = 0, Lavg = 1, Lmax = 2 };
        std::size_t nbSample; TorqueNormMethod normalizationMethod;
        pgicp_cov_frame lastFrame{};
        std::vector<int32_t> idxBuf;
        explicit CovarianceSamplingDataPointsFilter(std::size_t nb = 5000, int torqueNorm = 1) : nbSample(nb), normalizationMethod((TorqueNormMethod)torqueNorm)
        {
            if (nb < 1 || nb > 2147483647u) throw std::runtime_error("CovarianceSamplingDataPointsFilter: nbSample must be in [1, INT_MAX]");
            if (torqueNorm < 0 || torqueNorm > 2) throw std::runtime_error("CovarianceSamplingDataPointsFilter: torqueNorm must be 0 (L = 1), 1 (Lavg) or 2 (Lmax)");
        }
        //! the picks of the host form given a frame (nbSample < the cloud's size)
        void hostPicks(const DataPoints &c, const pgicp_cov_frame &frame, std::vector<int32_t> &picks) const
        {
            const int rn = c.getDescriptorStartingRow("normals");
            pgslam_amd::covsample::host_select<T>((int)c.features.cols(), [&](int i, int a) { return c.features(a, i); },
                                                  [&](int i, int a) { return c.descriptors(rn + a, i); }, (int)nbSample, frame, picks);
        }
        void hostFilter(DataPoints &c)
        {
            const int n = (int)c.features.cols(), rn = c.getDescriptorStartingRow("normals");
            if (!pgslam_amd::covsample::host_frame<T>(n, [&](int i, int a) { return c.features(a, i); }, [&](int i, int a) { return c.descriptors(rn + a, i); },
                                                      (int)normalizationMethod, lastFrame))
                throw std::runtime_error("CovarianceSamplingDataPointsFilter: a coordinate or a normal component is NaN or infinite, or every point lies at the mean "
                                         "(put a RemoveNaNDataPointsFilter ahead of it)");
            std::vector<int32_t> picks;
            hostPicks(c, lastFrame, picks);
            gatherColumns(c, picks.data(), (int)picks.size());
        }
        void deviceFilter(DataPoints &c)
        {
            const int n = (int)c.features.cols(), frows = (int)c.features.rows(), drows = (int)c.descriptors.rows();
            const int rn = c.getDescriptorStartingRow("normals");
            this->grow(idxBuf, nbSample);
            int kept = 0;
            check(ctx, pgslam_amd::Abi<T>::covariance_sampling(ctx, c.features.data(), frows, c.descriptors.data() + rn, drows, n, (int)nbSample,
                                                               (int)normalizationMethod, idxBuf.data(), &kept, &lastFrame));
            gatherColumns(c, idxBuf.data(), kept);
        }
        void inPlaceFilter(DataPoints &c) override
        {
            onDevice = false;
            this->needNormals(c, "CovarianceSamplingDataPointsFilter");
            this->need3D(c, "CovarianceSamplingDataPointsFilter");
            if ((std::size_t)c.features.cols() <= nbSample) return;                 // the no-op: the cloud as it is
            if (this->deviceWanted("PGSLAM_HOST_INPUT_STAGE")) { deviceFilter(c); onDevice = true; return; }
            hostFilter(c);
        }
    };
    //! [EXT] OctreeGridDataPointsFilter{maxPointByNode, maxSizeByNode, samplingMethod, buildParallel} (DataPointsFilters/
    //! OctreeGrid.cpp): one point per non-empty leaf of an octree over the cloud -- the leaf's first point (0), a seeded random one
    //! (1), its centroid (2: descriptors averaged, further feature rows the first point's) or its medoid (3) -- in depth-first leaf
    //! order.  The statement, with its marked deviations, is in include/pgicp_octree.h.  3-D clouds only.  On the device
    //! (pgicp_octree_grid_*, the same bits) when there is one, unless PGSLAM_HOST_INPUT_STAGE=1; else the host form of the same
    //! statement (octree_host.hpp).  No deviceSpec: a chain that holds it takes the per-filter path (it reorders points).
    //! `seed` (method 1) is a build-owned extra parameter, as RandomSampling's.  From YAML maxPointByNode or maxSizeByNode must be
    //! given (neither: the defaults keep every distinct point, refused as an omission).
    struct OctreeGridDataPointsFilter : DeviceBackedDataPointsFilter {
        using DeviceBackedDataPointsFilter::ctx; using DeviceBackedDataPointsFilter::onDevice;
        enum SamplingMethod { FIRST_PTS = 0, RAND_PTS = 1, CENTROID = 2, MEDOID = 3 };
        std::size_t maxPointByNode; T maxSizeByNode; SamplingMethod samplingMethod; bool buildParallel; unsigned long long seed;
        std::vector<T> oxBuf, odBuf;                 // the device form's outputs, kept from call to call
        std::vector<int32_t> idxBuf;
        explicit OctreeGridDataPointsFilter(std::size_t maxPts = 1, T maxSize = T(0), int method = 0, bool parallel = true, unsigned long long seed_ = 1)
            : maxPointByNode(maxPts), maxSizeByNode(maxSize), samplingMethod((SamplingMethod)method), buildParallel(parallel), seed(seed_)
        {
            if (maxPts < 1 || maxPts > 2147483647u) throw std::runtime_error("OctreeGridDataPointsFilter: maxPointByNode must be in [1, INT_MAX]");
            if (!(maxSize >= T(0)) || !std::isfinite(maxSize)) throw std::runtime_error("OctreeGridDataPointsFilter: maxSizeByNode must be finite and >= 0");
            if (method < 0 || method > 3) throw std::runtime_error("OctreeGridDataPointsFilter: samplingMethod must be 0 (first), 1 (random), 2 (centroid) or 3 (medoid)");
            if (seed_ >= (1ULL << 53)) throw std::runtime_error("OctreeGridDataPointsFilter: seed must be in [0, 2^53)");
        }
        void deviceFilter(DataPoints &c)
        {
            const int n = (int)c.features.cols(), frows = (int)c.features.rows(), drows = (int)c.descriptors.rows();
            this->grow(oxBuf, 3 * (size_t)n);
            this->grow(odBuf, (size_t)drows * n);
            this->grow(idxBuf, (size_t)n);
            int kept = 0;
            const int st = pgslam_amd::Abi<T>::octree_grid(ctx, c.features.data(), frows, n, (int)maxPointByNode, (double)maxSizeByNode, (int)samplingMethod, seed,
                                                           drows > 0 ? c.descriptors.data() : nullptr, drows, oxBuf.data(), drows > 0 ? odBuf.data() : nullptr,
                                                           idxBuf.data(), &kept);
            if (st == PGICP_ERR_ARG)
                throw std::runtime_error("OctreeGridDataPointsFilter: a coordinate is NaN or infinite (put a RemoveNaNDataPointsFilter ahead of it)");
            check(ctx, st);
            assemble(c, oxBuf.data(), odBuf.data(), idxBuf.data(), kept);
        }
        void hostFilter(DataPoints &c)
        {
            const int n = (int)c.features.cols(), drows = (int)c.descriptors.rows();
            pgslam_amd::octree::Result<T> res;
            if (!pgslam_amd::octree::host_filter<T>(n, [&](int i, int a) { return c.features(a, i); }, drows, [&](int i, int r) { return c.descriptors(r, i); },
                                                    (int)maxPointByNode, maxSizeByNode, (int)samplingMethod, seed, res))
                throw std::runtime_error("OctreeGridDataPointsFilter: a coordinate is NaN or infinite (put a RemoveNaNDataPointsFilter ahead of it)");
            assemble(c, res.xyz.data(), res.desc.data(), res.kept.data(), (int)res.kept.size());
        }
        void inPlaceFilter(DataPoints &c) override
        {
            onDevice = false;
            this->need3D(c, "OctreeGridDataPointsFilter");
            if (c.features.cols() == 0) return;
            if (this->deviceWanted("PGSLAM_HOST_INPUT_STAGE")) { deviceFilter(c); onDevice = true; return; }
            hostFilter(c);
        }
    };
    //! [EXT] NormalSpaceDataPointsFilter{nbSample, epsilon, seed} (DataPointsFilters/NormalSpace.cpp): normal-space sampling
    //! (Rusinkiewicz & Levoy 2001) -- the normals bucketed on the sphere by steps of epsilon radians, each pick uniform over the
    //! non-empty buckets and then a random point of that bucket, in pick order.  Needs the `normals` descriptor.  The statement,
    //! with its marked deviations, is in include/pgicp_normalspace.h.  3-D clouds only.  On the device
    //! (pgicp_normal_space_sampling_*) when there is one, unless PGSLAM_HOST_INPUT_STAGE=1; else the host form of the same
    //! statement (normalspace_host.hpp): the same picks.  No deviceSpec: a chain that holds it takes the per-filter path (the
    //! picks come in pick order).  `seed` is a build-owned extra parameter, as RandomSampling's.  From YAML nbSample must be given
    //! (upstream's default of 5000 bears no relation to the cloud's size).
    struct NormalSpaceDataPointsFilter : DeviceBackedDataPointsFilter {
        using DeviceBackedDataPointsFilter::ctx; using DeviceBackedDataPointsFilter::onDevice;
        std::size_t nbSample; double epsilon; unsigned long long seed;        // (epsilon: a double in both precisions, as the statement reads it)
        std::vector<int32_t> idxBuf;
        explicit NormalSpaceDataPointsFilter(std::size_t nb = 5000, double eps = 0.09, unsigned long long seed_ = 1) : nbSample(nb), epsilon(eps), seed(seed_)
        {
            pgslam_amd::normalspace::Grid g;
            if (nb < 1 || nb > 2147483647u) throw std::runtime_error("NormalSpaceDataPointsFilter: nbSample must be in [1, INT_MAX]");
            if (!pgslam_amd::normalspace::make_grid(eps, g))
                throw std::runtime_error("NormalSpaceDataPointsFilter: epsilon must be finite, > 0, <= pi and give at most 65536 buckets (about 1 degree or more)");
            if (seed_ >= (1ULL << 53)) throw std::runtime_error("NormalSpaceDataPointsFilter: seed must be in [0, 2^53)");
        }
        void hostFilter(DataPoints &c)
        {
            const int n = (int)c.features.cols(), rn = c.getDescriptorStartingRow("normals");
            std::vector<int32_t> picks, buckets;
            if (!pgslam_amd::normalspace::host_select<T>(n, [&](int i, int a) { return c.descriptors(rn + a, i); }, (int)nbSample, epsilon, seed, picks, buckets))
                throw std::runtime_error("NormalSpaceDataPointsFilter: a normal component is NaN or infinite (put a RemoveNaNDataPointsFilter ahead of it)");
            gatherColumns(c, picks.data(), (int)picks.size());
        }
        void deviceFilter(DataPoints &c)
        {
            const int n = (int)c.features.cols(), frows = (int)c.features.rows(), drows = (int)c.descriptors.rows();
            const int rn = c.getDescriptorStartingRow("normals");
            this->grow(idxBuf, nbSample);
            int kept = 0;
            const int st = pgslam_amd::Abi<T>::normal_space(ctx, c.features.data(), frows, c.descriptors.data() + rn, drows, n, (int)nbSample, epsilon, seed,
                                                            idxBuf.data(), &kept);
            if (st == PGICP_ERR_ARG)
                throw std::runtime_error("NormalSpaceDataPointsFilter: a normal component is NaN or infinite (put a RemoveNaNDataPointsFilter ahead of it)");
            check(ctx, st);
            gatherColumns(c, idxBuf.data(), kept);
        }
        void inPlaceFilter(DataPoints &c) override
        {
            onDevice = false;
            this->needNormals(c, "NormalSpaceDataPointsFilter");
            this->need3D(c, "NormalSpaceDataPointsFilter");
            if ((std::size_t)c.features.cols() <= nbSample) return;                 // the no-op: the cloud as it is
            if (this->deviceWanted("PGSLAM_HOST_INPUT_STAGE")) { deviceFilter(c); onDevice = true; return; }
            hostFilter(c);
        }
    };
    //! [EXT] MaxDensityDataPointsFilter{maxDensity} (DataPointsFilters/MaxDensity.cpp): needs the `densities` descriptor
    //! (SurfaceNormalDataPointsFilter{keepDensities: 1}); keeps a point at or below maxDensity, a denser one with probability
    //! maxDensity / density -- times (1 - nbSaturatedPts / nbPointsIn) in INTEGER arithmetic for points at the cloud's largest
    //! density, as upstream writes it.  The draw is the build's seeded one (not rand()-parity, see RandomSampling).  On the device
    //! (pgicp_max_density_*, the same bits) when there is one, unless PGSLAM_HOST_MAX_DENSITY=1 or the parameters are ones
    //! the device call refuses (maxDensity not > 0, a seed >= 2^53); then the host loop.  ranOnDevice(): which of the two the last inPlaceFilter (or fused pass) took.
    struct MaxDensityDataPointsFilter : DeviceBackedDataPointsFilter {
        using DeviceBackedDataPointsFilter::ctx; using DeviceBackedDataPointsFilter::onDevice;
        T maxDensity; unsigned long long seed;
        std::vector<T> densBuf;                      // the device form's buffers, kept from call to call
        std::vector<int32_t> idxBuf;
        explicit MaxDensityDataPointsFilter(T d = T(10), unsigned long long s = 1) : maxDensity(d), seed(s) {}
        //! what pgicp_max_density_* refuses, checked here: every other refusal of the device call is an error and throws
        bool deviceTakesParameters() const { return maxDensity > T(0) && seed < (1ULL << 53); }
        //! the device form (pgicp_max_density_*); false (the cloud untouched) for parameters the device call refuses
        bool deviceFilter(DataPoints &c)
        {
            if (!deviceTakesParameters()) return false;
            const int n = (int)c.features.cols(), rd = c.getDescriptorStartingRow("densities");
            this->grow(densBuf, (size_t)n);
            this->grow(idxBuf, (size_t)n);
            for (int i = 0; i < n; i++) densBuf[(size_t)i] = c.descriptors(rd, i);
            int kept = 0;
            check(ctx, pgslam_amd::Abi<T>::max_density(ctx, densBuf.data(), n, (double)maxDensity, (uint64_t)seed, idxBuf.data(), &kept));
            keepColumns(c, idxBuf.data(), kept);
            return true;
        }
        //! the host form: upstream's three passes
        void hostFilter(DataPoints &c)
        {
            const int n = (int)c.features.cols();
            const int rd = c.getDescriptorStartingRow("densities");
            T last = c.descriptors(rd, 0);
            for (int i = 1; i < n; i++) if (c.descriptors(rd, i) > last) last = c.descriptors(rd, i);
            int saturated = 0;
            for (int i = 0; i < n; i++) saturated += c.descriptors(rd, i) == last;
            compactColumns(c, [&](int j) {
                const T density = c.descriptors(rd, j);
                if (!(density > maxDensity)) return true;
                float accept = (float)(maxDensity / density);
                if (density == last) accept = accept * (float)(1 - saturated / n);
                return seededDraw(seed, j) < (double)accept;
            });
        }
        void inPlaceFilter(DataPoints &c) override
        {
            onDevice = false;
            if (!c.descriptorExists("densities")) throw std::runtime_error("MaxDensityDataPointsFilter: Error, no densities found in descriptors.");
            const int n = (int)c.features.cols();
            if (n == 0) return;
            if (this->deviceWanted("PGSLAM_HOST_MAX_DENSITY") && deviceFilter(c)) { onDevice = true; return; }
            hostFilter(c);
        }
        //! SurfaceNormalDataPointsFilter{keepDensities} directly ahead of this filter (DataPointsFilters::apply): both as ONE device
        //! pass (pgicp_normals_max_density_*) -- one upload of the cloud, one download of the kept points, the same bits as the two
        //! filters one after the other.  false: nothing was done (no device, the knob, a cloud that already carries one of the
        //! descriptors the pair writes -- setDescriptor would reuse its rows --, or parameters or coordinates the device call
        //! refuses, checked here) and the caller applies the two filters as before; any other refusal of the call throws.
        bool fusedWith(SurfaceNormalDataPointsFilter &sn, DataPoints &c)
        {
            const int n = (int)c.features.cols(), frows = (int)c.features.rows(), drows = (int)c.descriptors.rows();
            if (n == 0 || frows < 3 || !sn.keepDensities || sn.wantsExt() || !this->deviceWanted("PGSLAM_HOST_MAX_DENSITY") || !deviceTakesParameters() || sn.knn < 3 || sn.knn > 32) return false;
            for (const char *name : {"normals", "densities", "eigValues"}) if (c.descriptorExists(name)) return false;
            // (a coordinate that is not finite: the device refuses the cloud, and the unfused pair says so as it always did)
            for (int i = 0; i < n; i++)
                if (!std::isfinite(c.features(0, i)) || !std::isfinite(c.features(1, i)) || !std::isfinite(c.features(2, i))) return false;
            const bool kn = sn.keepNormals, ke = sn.keepEigenValues;
            Matrix ox(frows, n), on(3, kn ? n : 0), oe(3, ke ? n : 0), od(1, n), oc(drows, drows > 0 ? n : 0);
            this->grow(idxBuf, (size_t)n);
            const double md = std::isfinite((double)sn.maxDist) ? (double)sn.maxDist : 1e300;
            int kept = 0;
            const int st = pgslam_amd::Abi<T>::normals_max_density(sn.ctx, c.features.data(), frows, n, sn.knn, md, (double)maxDensity, (uint64_t)seed,
                                                                   drows > 0 ? c.descriptors.data() : nullptr, drows, ox.data(), kn ? on.data() : nullptr,
                                                                   ke ? oe.data() : nullptr, od.data(), drows > 0 ? oc.data() : nullptr, idxBuf.data(), &kept);
            check(sn.ctx, st);
            // rows 0-2 from the device, further feature rows the kept points' own; descriptors: the carried rows, then normals,
            // densities, eigValues -- the order the unfused pair appends them in
            const int nd = drows + (kn ? 3 : 0) + 1 + (ke ? 3 : 0);
            Matrix f(frows, kept), d(nd, kept);
            for (int o = 0; o < kept; o++) {
                const int i = idxBuf[(size_t)o];
                for (int r = 0; r < 3; r++) f(r, o) = ox(r, o);
                for (int r = 3; r < frows; r++) f(r, o) = c.features(r, i);
                int q = 0;
                for (int r = 0; r < drows; r++) d(q++, o) = oc(r, o);
                if (kn) for (int r = 0; r < 3; r++) d(q++, o) = on(r, o);
                d(q++, o) = od(0, o);
                if (ke) for (int r = 0; r < 3; r++) d(q++, o) = oe(r, o);
            }
            c.features = f;
            c.descriptors = d;
            if (kn) c.descriptorLabels.push_back(typename DataPoints::Label("normals", 3));
            c.descriptorLabels.push_back(typename DataPoints::Label("densities", 1));
            if (ke) c.descriptorLabels.push_back(typename DataPoints::Label("eigValues", 3));
            onDevice = true;
            return true;
        }
    };
    //! [EXT] SimpleSensorNoiseDataPointsFilter{sensorType, gain} (DataPointsFilters/SimpleSensorNoise.cpp, restated as recalled):
    //! adds the one-row descriptor `simpleSensorNoise` = gain * max(minRadius, beamAngle * |p| + beamConst) -- sensorType 0 Sick
    //! LMS-1xx, 1 Hokuyo URG-04LX, 2 Hokuyo UTM-30LX, 4 Sick Tim3xx -- or gain * |p|^2 * 0.5 * 0.00285 for 3 (Kinect / Xtion);
    //! ErrorMinimizer::getOverlap() reads it (Localizer.hpp:278, LoopCloser.hpp:331).  oracle: orc_simple_sensor_noise
    struct SimpleSensorNoiseDataPointsFilter : DataPointsFilter {
        int sensorType; T gain;
        explicit SimpleSensorNoiseDataPointsFilter(int t = 0, T g = T(1)) : sensorType(t), gain(g)
        {
            if (t < 0 || t > 4) throw std::runtime_error("SimpleSensorNoiseDataPointsFilter: sensorType must be 0 ... 4");
        }
        void inPlaceFilter(DataPoints &c) override
        {
            pgslam_amd::sensor_chain::NoiseModel<T> model;
            pgslam_amd::sensor_chain::noise_model<T>(sensorType, gain, model);          // (the constructor has checked the type)
            const int n = (int)c.features.cols();
            Matrix noise(1, n);
            for (int i = 0; i < n; i++) {
                const T x[3] = {c.features(0, i), c.features(1, i), c.features(2, i)};
                noise(0, i) = pgslam_amd::sensor_chain::noise_value<T>(model, x);
            }
            c.setDescriptor("simpleSensorNoise", noise);
        }
    };
    //! the row of descriptor `name`, which must exist with `span` rows: DataPoints::InvalidField otherwise, worded as upstream words it
    static int descriptorRowOf(const DataPoints &c, const std::string &name, int span, const char *filter)
    {
        if (!c.descriptorExists(name)) throw typename DataPoints::InvalidField(std::string(filter) + ": Error, cannot find " + name + " in descriptors.");
        if (c.getDescriptorDimension(name) != span)
            throw typename DataPoints::InvalidField(std::string(filter) + ": Error, descriptor " + name + " must have " + std::to_string(span) + (span == 1 ? " row." : " rows."));
        return c.getDescriptorStartingRow(name);
    }
    //! [EXT] IncidenceAngleDataPointsFilter (DataPointsFilters/IncidenceAngle.cpp, restated as recalled in
    //! include/pgicp_descriptor_filters.h): adds the one-row descriptor `incidenceAngles`, the angle between a point's normal and its
    //! observation direction -- descriptor_filters_host.hpp's incidence_angle, which the device stage calls too.  Needs `normals` and
    //! `observationDirections`, 3 rows each.  Elementwise: alone it runs on the host, inside a sensor-chain run on the device.
    struct IncidenceAngleDataPointsFilter : DataPointsFilter {
        void inPlaceFilter(DataPoints &c) override
        {
            const int rn = descriptorRowOf(c, "normals", 3, "IncidenceAngleDataPointsFilter"), ro = descriptorRowOf(c, "observationDirections", 3, "IncidenceAngleDataPointsFilter");
            const int n = (int)c.features.cols();
            Matrix a(1, n);
            for (int j = 0; j < n; j++) {
                const T nv[3] = {c.descriptors(rn, j), c.descriptors(rn + 1, j), c.descriptors(rn + 2, j)};
                const T ov[3] = {c.descriptors(ro, j), c.descriptors(ro + 1, j), c.descriptors(ro + 2, j)};
                a(0, j) = pgslam_amd::descriptor_filters::incidence_angle<T>(nv, ov);
            }
            c.setDescriptor("incidenceAngles", a);
        }
    };
    //! [EXT] SphericalityDataPointsFilter{keepUnstructureness, keepStructureness} (DataPointsFilters/Sphericality.cpp, restated as
    //! recalled): from `eigValues` (3 rows) the one-row descriptors `sphericality` and, when asked for, `unstructureness` and
    //! `structureness`, appended in that order -- descriptor_filters_host.hpp's sphericality
    struct SphericalityDataPointsFilter : DataPointsFilter {
        bool keepUnstructureness, keepStructureness;
        explicit SphericalityDataPointsFilter(bool ku = false, bool ks = false) : keepUnstructureness(ku), keepStructureness(ks) {}
        void inPlaceFilter(DataPoints &c) override
        {
            const int re = descriptorRowOf(c, "eigValues", 3, "SphericalityDataPointsFilter");
            const int n = (int)c.features.cols();
            Matrix sph(1, n), uns(1, n), str(1, n);
            for (int j = 0; j < n; j++) {
                const T e[3] = {c.descriptors(re, j), c.descriptors(re + 1, j), c.descriptors(re + 2, j)};
                pgslam_amd::descriptor_filters::sphericality<T>(e, sph(0, j), uns(0, j), str(0, j));
            }
            c.setDescriptor("sphericality", sph);
            if (keepUnstructureness) c.setDescriptor("unstructureness", uns);
            if (keepStructureness) c.setDescriptor("structureness", str);
        }
    };
    //! [EXT] CutAtDescriptorThresholdDataPointsFilter{descName, useLargerThan, threshold} (DataPointsFilters/CutAtDescriptorThreshold.cpp,
    //! restated as recalled): drops the points whose one-row descriptor `descName` lies above the threshold (useLargerThan) or below
    //! it -- descriptor_filters_host.hpp's cut_keep; a NaN is never kept.  Order is kept; features and descriptors travel.  On the
    //! device it is an entry of pgicp_filter_cloud's list (its row is the cloud's, so the spec needs the cloud) and a stage of a
    //! sensor-chain run.
    struct CutAtDescriptorThresholdDataPointsFilter : DataPointsFilter {
        std::string descName; bool useLargerThan; T threshold;
        CutAtDescriptorThresholdDataPointsFilter(const std::string &name, bool larger, T thr) : descName(name), useLargerThan(larger), threshold(thr) {}
        void inPlaceFilter(DataPoints &c) override
        {
            const int r = descriptorRowOf(c, descName, 1, "CutAtDescriptorThresholdDataPointsFilter");
            compactColumns(c, [&](int j) { return pgslam_amd::descriptor_filters::cut_keep<T>(c.descriptors(r, j), threshold, useLargerThan); });
        }
        //! (no descriptor of that name and one row, or no cloud to look at: no device form -- the host path runs, and throws)
        using DataPointsFilter::deviceSpec;
        bool deviceSpec(pgicp_filter &f, const DataPoints &c) const override
        {
            if (!c.descriptorExists(descName) || c.getDescriptorDimension(descName) != 1) return false;
            std::memset(&f, 0, sizeof f);
            f.type = PGICP_FILTER_CUT_AT_DESCRIPTOR; f.p[0] = (double)c.getDescriptorStartingRow(descName); f.p[1] = useLargerThan ? 1.0 : 0.0; f.p[2] = (double)threshold;
            return true;
        }
    };
    struct DataPointsFilters : std::vector<std::shared_ptr<DataPointsFilter>> {
        DataPointsFilters() {}
        //! Localizer.hpp:77 -- a YAML list of filters
        explicit DataPointsFilters(std::istream &in)
        {
            std::stringstream ss;
            ss << "filters:\n" << in.rdbuf();          // a bare sequence: give it a section name
            const auto chain = pgslam_amd::yaml_lite::parse(ss);
            if (chain.has("filters")) load(chain.sections.at("filters"));
        }
        static std::string supportedNames()
        {
            return " (supported: Identity, MinDist, MaxDist, DistanceLimit, MaxQuantileOnAxis, BoundingBox, RemoveNaN, SurfaceNormal, "
                   "SamplingSurfaceNormal, Elipsoids, VoxelGrid, OctreeGrid, MaxDensity, CovarianceSampling, NormalSpace, ObservationDirection, OrientNormals, Shadow, IncidenceAngle, Sphericality, CutAtDescriptorThreshold, FixStepSampling, RandomSampling, MaxPointCount "
                   "(seeded samplers, not rand()-parity))";
        }
        //! refuses a module that carries a parameter outside `names` (only the filters that always refused one call it)
        static void allowOnly(const pgslam_amd::yaml_lite::Module &m, std::initializer_list<const char *> names)
        {
            for (auto &kv : m.params)
                if (std::none_of(names.begin(), names.end(), [&](const char *k) { return kv.first == k; }))
                    throw std::runtime_error(m.name + ": unknown parameter " + kv.first);
        }
        void load(const std::vector<pgslam_amd::yaml_lite::Module> &mods)
        {
            using pgslam_amd::yaml_lite::to_double;
            for (auto &m : mods) {
                // parameter `k` as a number, `def` when the module does not give it
                auto get = [&](const char *k, const char *def) { return to_double(m.params.count(k) ? m.params.at(k) : std::string(def), m.name); };
                if (m.name == "IdentityDataPointsFilter") this->push_back(std::make_shared<IdentityDataPointsFilter>());
                else if (m.name == "MaxDistDataPointsFilter" || m.name == "MinDistDataPointsFilter") {
                    const int dim = (int)get("dim", "-1");
                    if (dim < -1 || dim > 2) throw std::runtime_error(m.name + ": dim must be -1 (radius), 0, 1 or 2");
                    const T lim = (T)to_double(m.params.count("maxDist") ? m.params.at("maxDist") : m.params.count("minDist") ? m.params.at("minDist") : "1", m.name);
                    this->push_back(std::make_shared<DistLimitDataPointsFilter>(lim, m.name == "MaxDistDataPointsFilter", dim));
                } else if (m.name == "DistanceLimitDataPointsFilter") {
                    // upstream's newer spelling of Min/MaxDist: removeInside = 1 keeps what MinDist keeps, 0 what MaxDist keeps
                    allowOnly(m, {"dim", "dist", "removeInside"});
                    const int dim = (int)get("dim", "-1");
                    if (dim < -1 || dim > 2) throw std::runtime_error(m.name + ": dim must be -1 (radius), 0, 1 or 2");
                    const double ri = get("removeInside", "1");
                    if (ri != 0.0 && ri != 1.0) throw std::runtime_error(m.name + ": removeInside must be 0 or 1");
                    this->push_back(std::make_shared<DistLimitDataPointsFilter>((T)get("dist", "1"), /*keepInside=*/ri == 0.0, dim));
                } else if (m.name == "MaxQuantileOnAxisDataPointsFilter") {
                    allowOnly(m, {"dim", "ratio"});
                    // upstream's default ratio of 0.5 drops half of every scan: as a bare list entry that is an omission far more
                    // often than a choice, so, as VoxelGrid, OctreeGrid and NormalSpace refuse their bare forms, it is refused
                    if (!m.params.count("ratio"))
                        throw std::runtime_error("DataPointsFilters: unsupported filter '" + m.name + "' without ratio: the default (0.5) drops half of "
                                                 "every scan, give ratio (in [1e-7, 0.9999999])" + supportedNames());
                    const double dim = get("dim", "0"), ratio = get("ratio", "0.5");
                    if (dim != 0.0 && dim != 1.0 && dim != 2.0) throw std::runtime_error(m.name + ": dim must be 0, 1 or 2");
                    if (!pgslam_amd::axis_quantile::ratio_ok(ratio) || !((T)ratio > (T)0 && (T)ratio < (T)1))
                        throw std::runtime_error(m.name + ": ratio must be in [1e-7, 0.9999999]");
                    this->push_back(std::make_shared<MaxQuantileOnAxisDataPointsFilter>((int)dim, (T)ratio));
                } else if (m.name == "SurfaceNormalDataPointsFilter") {
                    // (epsilon > 0 allows an approximate neighbour search upstream; the exact search here meets every allowance)
                    if (!(get("epsilon", "0") >= 0.0)) throw std::runtime_error(m.name + ": epsilon must be >= 0");
                    const int knn = (int)get("knn", "5");
                    if (knn < 3 || knn > 32) throw std::runtime_error(m.name + ": knn must be in [3, 32]");
                    if (get("smoothNormals", "0") != 0.0 && get("keepNormals", "1") == 0.0)
                        throw std::runtime_error(m.name + ": smoothNormals needs keepNormals (there is nothing to smooth into)");
                    this->push_back(std::make_shared<SurfaceNormalDataPointsFilter>(knn, (T)get("maxDist", "inf"),
                                                                                     get("keepNormals", "1") != 0.0,
                                                                                     get("keepEigenValues", "0") != 0.0,
                                                                                     get("keepDensities", "0") != 0.0,
                                                                                     get("keepEigenVectors", "0") != 0.0,
                                                                                     get("keepMatchedIds", "0") != 0.0,
                                                                                     get("keepMeanDist", "0") != 0.0,
                                                                                     get("smoothNormals", "0") != 0.0));
                } else if (m.name == "SamplingSurfaceNormalDataPointsFilter") {
                    // (a constructed filter carries densities; from YAML the key stays refused)
                    if (get("keepDensities", "0") != 0.0) throw std::runtime_error(m.name + ": keepDensities is not supported");
                    const double ratio = get("ratio", "0.5"), seed = get("seed", "1");
                    const int knn = (int)get("knn", "7"), method = (int)get("samplingMethod", "0");
                    if (!(ratio > 0.0 && ratio < 1.0) || knn < 3 || (method != 0 && method != 1) || !(seed >= 0.0 && seed < 9007199254740992.0))
                        throw std::runtime_error(m.name + ": ratio must be in (0, 1), knn >= 3, samplingMethod 0 or 1, seed in [0, 2^53)");
                    this->push_back(std::make_shared<SamplingSurfaceNormalDataPointsFilter>((T)ratio, knn, method, (T)get("maxBoxDim", "inf"),
                                                                                             get("averageExistingDescriptors", "1") != 0.0,
                                                                                             get("keepNormals", "1") != 0.0, (unsigned long long)seed,
                                                                                             false, get("keepEigenValues", "0") != 0.0,
                                                                                             get("keepEigenVectors", "0") != 0.0));
                } else if (m.name == "ElipsoidsDataPointsFilter") {
                    allowOnly(m, {"ratio", "knn", "samplingMethod", "maxBoxDim", "minPlanarity", "maxTimeWindow", "averageExistingDescriptors", "keepNormals",
                                  "keepDensities", "keepEigenValues", "keepEigenVectors", "keepCovariances", "keepWeights", "keepMeans", "keepShapes", "seed"});
                    // upstream's default of keepNormals is not pinned here: as VarTrimmedDistOutlierFilter asks for every parameter, it is
                    // asked for rather than guessed
                    if (!m.params.count("keepNormals")) throw std::runtime_error(m.name + ": give keepNormals (0 or 1) explicitly");
                    // (this DataPoints carries no times)
                    if (!(get("maxTimeWindow", "inf") == std::numeric_limits<double>::infinity()))
                        throw std::runtime_error(m.name + ": maxTimeWindow is not supported (the cloud carries no times): leave it out or give inf");
                    const double ratio = get("ratio", "0.5"), seed = get("seed", "1"), minPlan = get("minPlanarity", "0");
                    const int knn = (int)get("knn", "7"), method = (int)get("samplingMethod", "0");
                    if (!(ratio > 0.0 && ratio < 1.0) || knn < 3 || (method != 0 && method != 1) || !(seed >= 0.0 && seed < 9007199254740992.0))
                        throw std::runtime_error(m.name + ": ratio must be in (0, 1), knn >= 3, samplingMethod 0 or 1, seed in [0, 2^53)");
                    if (!pgslam_amd::elipsoids::min_planarity_ok(minPlan)) throw std::runtime_error(m.name + ": minPlanarity must be finite and in [0, 1]");
                    this->push_back(std::make_shared<ElipsoidsDataPointsFilter>((T)ratio, knn, method, (T)get("maxBoxDim", "inf"), (T)minPlan,
                                                                                 get("averageExistingDescriptors", "1") != 0.0, get("keepNormals", "1") != 0.0,
                                                                                 get("keepDensities", "0") != 0.0, get("keepEigenValues", "0") != 0.0,
                                                                                 get("keepEigenVectors", "0") != 0.0, get("keepCovariances", "0") != 0.0,
                                                                                 get("keepWeights", "0") != 0.0, get("keepMeans", "0") != 0.0,
                                                                                 get("keepShapes", "0") != 0.0, (unsigned long long)seed));
                } else if (m.name == "VoxelGridDataPointsFilter") {
                    allowOnly(m, {"vSizeX", "vSizeY", "vSizeZ", "useCentroid", "averageExistingDescriptors"});
                    // the three sizes are given together or not at all (1 m each, upstream's defaults): one or two sizes alone would
                    // leave the others at 1 m -- a grid of 0.1 x 1 x 1 m from `vSizeX: 0.1`, which is a typo far more often than a
                    // choice -- so, as VarTrimmedDistOutlierFilter asks for every parameter, that is refused rather than guessed
                    const int given = (int)m.params.count("vSizeX") + (int)m.params.count("vSizeY") + (int)m.params.count("vSizeZ");
                    if (given != 0 && given != 3)
                        throw std::runtime_error(m.name + ": give vSizeX, vSizeY and vSizeZ together (or none of them: 1 m each)");
                    const double vx = get("vSizeX", "1"), vy = get("vSizeY", "1"), vz = get("vSizeZ", "1");
                    for (double vs : {vx, vy, vz})
                        if (!(vs > 0.0) || !std::isfinite(vs) || !((T)vs > T(0)) || !std::isfinite((T)vs))
                            throw std::runtime_error(m.name + ": vSizeX, vSizeY and vSizeZ must be finite and > 0");
                    this->push_back(std::make_shared<VoxelGridDataPointsFilter>((T)vx, (T)vy, (T)vz, get("useCentroid", "1") != 0.0,
                                                                                get("averageExistingDescriptors", "1") != 0.0));
                } else if (m.name == "CovarianceSamplingDataPointsFilter") {
                    allowOnly(m, {"nbSample", "torqueNorm"});
                    const double nb = get("nbSample", "5000"), tn = get("torqueNorm", "1");
                    if (!(nb >= 1.0 && nb <= 2147483647.0) || nb != std::floor(nb) || (tn != 0.0 && tn != 1.0 && tn != 2.0))
                        throw std::runtime_error(m.name + ": nbSample must be an integer in [1, INT_MAX], torqueNorm 0, 1 or 2");
                    this->push_back(std::make_shared<CovarianceSamplingDataPointsFilter>((std::size_t)nb, (int)tn));
                } else if (m.name == "OctreeGridDataPointsFilter") {
                    allowOnly(m, {"maxPointByNode", "maxSizeByNode", "samplingMethod", "buildParallel", "seed"});
                    // with neither limit given the defaults hold (maxPointByNode 1, maxSizeByNode 0): one leaf a distinct point -- the
                    // cloud comes back whole, reordered, only coincident points merged.  As a list entry that is an omission far more
                    // often than a choice, so, as VoxelGrid refuses one or two sizes alone, that form is refused rather than run
                    if (!m.params.count("maxPointByNode") && !m.params.count("maxSizeByNode"))
                        throw std::runtime_error("DataPointsFilters: unsupported filter '" + m.name + "' without maxPointByNode or maxSizeByNode: the defaults "
                                                 "(1 and 0) keep every distinct point, give at least one of the two" + supportedNames());
                    const double mp = get("maxPointByNode", "1"), ms = get("maxSizeByNode", "0"), sm = get("samplingMethod", "0"), seed = get("seed", "1");
                    if (!(mp >= 1.0 && mp <= 2147483647.0) || mp != std::floor(mp) || !(ms >= 0.0) || !std::isfinite(ms) || !std::isfinite((T)ms) ||
                        (sm != 0.0 && sm != 1.0 && sm != 2.0 && sm != 3.0) || !(seed >= 0.0 && seed < 9007199254740992.0))
                        throw std::runtime_error(m.name + ": maxPointByNode must be an integer in [1, INT_MAX], maxSizeByNode finite and >= 0, "
                                                          "samplingMethod 0, 1, 2 or 3, seed in [0, 2^53)");
                    // (buildParallel: accepted and ignored, the result does not depend on it)
                    this->push_back(std::make_shared<OctreeGridDataPointsFilter>((std::size_t)mp, (T)ms, (int)sm, get("buildParallel", "1") != 0.0,
                                                                                  (unsigned long long)seed));
                } else if (m.name == "NormalSpaceDataPointsFilter") {
                    allowOnly(m, {"nbSample", "epsilon", "seed"});
                    // upstream's default of 5000 bears no relation to the cloud's size: as a list entry without nbSample it is an
                    // omission far more often than a choice, so, as VoxelGrid and OctreeGrid refuse their bare forms, it is refused
                    if (!m.params.count("nbSample"))
                        throw std::runtime_error("DataPointsFilters: unsupported filter '" + m.name + "' without nbSample: the default (5000) bears no relation "
                                                 "to the cloud's size, give nbSample (an integer >= 1)" + supportedNames());
                    const double nb = get("nbSample", "5000"), eps = get("epsilon", "0.09"), seed = get("seed", "1");
                    pgslam_amd::normalspace::Grid g;
                    if (!(nb >= 1.0 && nb <= 2147483647.0) || nb != std::floor(nb) || !pgslam_amd::normalspace::make_grid(eps, g) ||
                        !(seed >= 0.0 && seed < 9007199254740992.0))
                        throw std::runtime_error(m.name + ": nbSample must be an integer in [1, INT_MAX], epsilon finite, > 0, <= pi and of at most 65536 "
                                                          "buckets (about 1 degree or more), seed in [0, 2^53)");
                    this->push_back(std::make_shared<NormalSpaceDataPointsFilter>((std::size_t)nb, eps, (unsigned long long)seed));
                } else if (m.name == "MaxDensityDataPointsFilter") {
                    const double md = get("maxDensity", "10"), seed = get("seed", "1");
                    if (!(md > 0.0) || !(seed >= 0.0 && seed < 9007199254740992.0)) throw std::runtime_error(m.name + ": maxDensity must be positive, seed in [0, 2^53)");
                    this->push_back(std::make_shared<MaxDensityDataPointsFilter>((T)md, (unsigned long long)seed));
                } else if (m.name == "SimpleSensorNoiseDataPointsFilter") {
                    const double st = get("sensorType", "0"), gain = get("gain", "1");
                    if (st != std::floor(st) || st < 0.0 || st > 4.0 || !(gain >= 1.0)) throw std::runtime_error(m.name + ": sensorType must be 0 ... 4, gain >= 1");
                    this->push_back(std::make_shared<SimpleSensorNoiseDataPointsFilter>((int)st, (T)gain));
                } else if (m.name == "BoundingBoxDataPointsFilter") {
                    const T lo[3] = {(T)get("xMin", "-1"), (T)get("yMin", "-1"), (T)get("zMin", "-1")}, hi[3] = {(T)get("xMax", "1"), (T)get("yMax", "1"), (T)get("zMax", "1")};
                    this->push_back(std::make_shared<BoundingBoxDataPointsFilter>(lo, hi, (T)get("removeInside", "1") != (T)0));
                } else if (m.name == "RemoveNaNDataPointsFilter") {
                    this->push_back(std::make_shared<RemoveNaNDataPointsFilter>());
                } else if (m.name == "ObservationDirectionDataPointsFilter") {
                    this->push_back(std::make_shared<ObservationDirectionDataPointsFilter>((T)get("x", "0"), (T)get("y", "0"), (T)get("z", "0")));
                } else if (m.name == "OrientNormalsDataPointsFilter") {
                    this->push_back(std::make_shared<OrientNormalsDataPointsFilter>(get("towardCenter", "1") != 0.0));
                } else if (m.name == "ShadowDataPointsFilter") {
                    const double e = get("eps", "0.1");
                    if (!(e >= 0.0 && e <= 3.14159265358979323846)) throw std::runtime_error(m.name + ": eps must be in [0, pi]");
                    this->push_back(std::make_shared<ShadowDataPointsFilter>((T)e));
                } else if (m.name == "IncidenceAngleDataPointsFilter") {
                    allowOnly(m, {});
                    this->push_back(std::make_shared<IncidenceAngleDataPointsFilter>());
                } else if (m.name == "SphericalityDataPointsFilter") {
                    allowOnly(m, {"keepUnstructureness", "keepStructureness"});
                    const double ku = get("keepUnstructureness", "0"), ks = get("keepStructureness", "0");
                    if ((ku != 0.0 && ku != 1.0) || (ks != 0.0 && ks != 1.0)) throw std::runtime_error(m.name + ": keepUnstructureness and keepStructureness must be 0 or 1");
                    this->push_back(std::make_shared<SphericalityDataPointsFilter>(ku != 0.0, ks != 0.0));
                } else if (m.name == "CutAtDescriptorThresholdDataPointsFilter") {
                    allowOnly(m, {"descName", "useLargerThan", "threshold"});
                    // upstream's defaults ("none" and 1) cut nothing meaningful: as VarTrimmedDistOutlierFilter asks for its parameters,
                    // the name and the threshold are asked for rather than guessed
                    for (const char *k : {"descName", "threshold"})
                        if (!m.params.count(k)) throw std::runtime_error(m.name + ": parameter " + k + " must be given");
                    const double lt = get("useLargerThan", "1"), thr = get("threshold", "1");
                    if (lt != 0.0 && lt != 1.0) throw std::runtime_error(m.name + ": useLargerThan must be 0 or 1");
                    if (m.params.at("descName").empty()) throw std::runtime_error(m.name + ": descName must name a descriptor");
                    this->push_back(std::make_shared<CutAtDescriptorThresholdDataPointsFilter>(m.params.at("descName"), lt != 0.0, (T)thr));
                } else if (m.name == "FixStepSamplingDataPointsFilter") {
                    const double start = get("startStep", "10"), end = get("endStep", "10"), mult = get("stepMult", "1");
                    if (!(start >= 1.0 && start <= 2147483647.0) || !(end >= 1.0 && end <= 2147483647.0) || !(mult > 0.0))
                        throw std::runtime_error(m.name + ": startStep and endStep must be in [1, INT_MAX], stepMult positive");
                    this->push_back(std::make_shared<FixStepSamplingDataPointsFilter>(start, m.params.count("endStep") ? end : start, mult));
                } else if (m.name == "RandomSamplingDataPointsFilter") {
                    const double prob = get("prob", "0.75"), seed = get("seed", "1");
                    if (!(prob >= 0.0 && prob <= 1.0) || !(seed >= 0.0 && seed < 9007199254740992.0)) throw std::runtime_error(m.name + ": prob must be in [0, 1], seed in [0, 2^53)");
                    this->push_back(std::make_shared<RandomSamplingDataPointsFilter>((T)prob, (unsigned long long)seed));
                } else if (m.name == "MaxPointCountDataPointsFilter") {
                    const double mc = get("maxCount", "1000"), seed = get("seed", "1");
                    if (!(mc >= 1.0 && mc <= 2147483647.0) || !(seed >= 0.0 && seed < 9007199254740992.0)) throw std::runtime_error(m.name + ": maxCount must be in [1, INT_MAX], seed in [0, 2^53)");
                    this->push_back(std::make_shared<MaxPointCountDataPointsFilter>((unsigned)mc, (unsigned long long)seed));
                } else
                    throw std::runtime_error("DataPointsFilters: unsupported filter '" + m.name + "'" + supportedNames());
            }
        }
        void init() { for (auto &f : *this) f->init(); }
        size_t lastFused = 0;
        //! A sensor-chain RUN starting at filter k (include/pgicp_sensor_chain.h, include/pgicp_descriptor_filters.h): the longest
        //! contiguous sub-list from k made of one SurfaceNormalDataPointsFilter (no ext output, knn in [3, 32]) and ObservationDirection,
        //! OrientNormals, Shadow, MaxDensity, SimpleSensorNoise, IncidenceAngle, Sphericality, each at most once, and up to four
        //! CutAtDescriptorThreshold, that the device call accepts -- only ObservationDirection and SimpleSensorNoise may stand ahead of
        //! the SurfaceNormal (they read coordinates, and nothing ahead of the head drops points); OrientNormals and IncidenceAngle need
        //! keepNormals and the run's ObservationDirection before them, Shadow keepNormals, MaxDensity keepDensities and parameters the
        //! device takes, Sphericality keepEigenValues, a cut a descName that names a row the run has made by then or a one-row
        //! descriptor `cloud` carries (null: no cloud to look at) -- and that holds at least one of the filters which otherwise run on
        //! the host.  Returns the run's length, 0 when there is none at k.  Needs no device.
        struct ChainRunState {
            SurfaceNormalDataPointsFilter *sn = nullptr;
            SphericalityDataPointsFilter *sph = nullptr;
            bool obs = false, orient = false, shadow = false, md = false, noise = false, inc = false;
            int cuts = 0;
            //! PGICP_CHAIN_ROW_* of a row the run has made so far, -1: none of that name
            int rowMade(const std::string &name) const
            {
                if (name == "densities") return sn && sn->keepDensities ? PGICP_CHAIN_ROW_DENSITIES : -1;
                if (name == "incidenceAngles") return inc ? PGICP_CHAIN_ROW_INCIDENCE_ANGLES : -1;
                if (name == "sphericality") return sph ? PGICP_CHAIN_ROW_SPHERICALITY : -1;
                if (name == "unstructureness") return sph && sph->keepUnstructureness ? PGICP_CHAIN_ROW_UNSTRUCTURENESS : -1;
                if (name == "structureness") return sph && sph->keepStructureness ? PGICP_CHAIN_ROW_STRUCTURENESS : -1;
                if (name == "simpleSensorNoise") return noise ? PGICP_CHAIN_ROW_SIMPLE_SENSOR_NOISE : -1;
                return -1;
            }
            //! takes filter f into the run; false: the run ends ahead of it
            bool take(DataPointsFilter *f, const DataPoints *cloud)
            {
                if (auto *s = dynamic_cast<SurfaceNormalDataPointsFilter *>(f)) {
                    if (sn || s->wantsExt() || s->knn < 3 || s->knn > 32) return false;
                    sn = s;
                } else if (dynamic_cast<ObservationDirectionDataPointsFilter *>(f)) {
                    if (obs) return false;
                    obs = true;
                } else if (dynamic_cast<SimpleSensorNoiseDataPointsFilter *>(f)) {
                    if (noise) return false;
                    noise = true;
                } else if (dynamic_cast<OrientNormalsDataPointsFilter *>(f)) {
                    if (orient || !sn || !sn->keepNormals || !obs) return false;
                    orient = true;
                } else if (dynamic_cast<ShadowDataPointsFilter *>(f)) {
                    if (shadow || !sn || !sn->keepNormals) return false;
                    shadow = true;
                } else if (auto *m = dynamic_cast<MaxDensityDataPointsFilter *>(f)) {
                    if (md || !sn || !sn->keepDensities || !m->deviceTakesParameters()) return false;
                    md = true;
                } else if (dynamic_cast<IncidenceAngleDataPointsFilter *>(f)) {
                    if (inc || !sn || !sn->keepNormals || !obs) return false;
                    inc = true;
                } else if (auto *p = dynamic_cast<SphericalityDataPointsFilter *>(f)) {
                    if (sph || !sn || !sn->keepEigenValues) return false;
                    sph = p;
                } else if (auto *p = dynamic_cast<CutAtDescriptorThresholdDataPointsFilter *>(f)) {
                    if (cuts == PGICP_CHAIN_EXT_MAX_CUTS || !sn) return false;
                    if (rowMade(p->descName) < 0 && !(cloud && cloud->descriptorExists(p->descName) && cloud->getDescriptorDimension(p->descName) == 1)) return false;
                    cuts++;
                } else
                    return false;
                return true;
            }
            bool ext() const { return inc || sph || cuts > 0; }
        };
        size_t sensorChainRunAt(size_t k, const DataPoints *cloud = nullptr) const
        {
            ChainRunState r;
            size_t j = k;
            while (j < this->size() && r.take((*this)[j].get(), cloud)) j++;
            if (!r.sn || !(r.obs || r.orient || r.shadow || r.noise || r.ext())) return 0;
            return j - k;
        }
        //! the number of filters the last apply() ran inside one pgicp_sensor_chain_* / pgicp_sensor_chain_ext_* call; 0 when it ran none
        size_t lastFusedRun() const { return lastFused; }
        //! The run [k, k + len) as ONE device call: one upload of the cloud, one download of the kept points; the cloud ends in the
        //! state filter-by-filter application leaves (the same labels in the same order, the same bytes).  false: nothing was done
        //! (no device, PGSLAM_HOST_SENSOR_CHAIN=1, an empty cloud or one of fewer than 3 feature rows, a cloud that already carries a
        //! descriptor the run writes -- setDescriptor would reuse its rows --, or arguments the device call refuses, e.g. a
        //! coordinate that is not finite) and the caller applies the filters one by one as before; any other failure throws.
        bool applySensorChain(size_t k, size_t len, DataPoints &c)
        {
            const int n = (int)c.features.cols(), frows = (int)c.features.rows(), drows = (int)c.descriptors.rows();
            if (n == 0 || frows < 3 || len > PGICP_CHAIN_EXT_MAX_STAGES + 1 || !DeviceBackedDataPointsFilter::deviceWanted("PGSLAM_HOST_SENSOR_CHAIN")) return false;
            SurfaceNormalDataPointsFilter *sn = nullptr;
            MaxDensityDataPointsFilter *mdf = nullptr;
            std::vector<pgicp_chain_stage> stages;
            ChainRunState made;                              // (what the run has made when a cut looks for its row)
            for (size_t j = k; j < k + len; j++) {
                DataPointsFilter *f = (*this)[j].get();
                pgicp_chain_stage s;
                std::memset(&s, 0, sizeof s);
                if (auto *p = dynamic_cast<CutAtDescriptorThresholdDataPointsFilter *>(f)) {
                    s.type = PGICP_CHAIN_CUT_AT_DESCRIPTOR; s.p[0] = (double)made.rowMade(p->descName); s.p[1] = p->useLargerThan ? 1.0 : 0.0; s.p[2] = (double)p->threshold;
                    if (s.p[0] < 0.0) {
                        if (!c.descriptorExists(p->descName) || c.getDescriptorDimension(p->descName) != 1) return false;
                        s.p[0] = (double)PGICP_CHAIN_ROW_DESC; s.p[3] = (double)c.getDescriptorStartingRow(p->descName);
                    }
                }
                if (!made.take(f, &c)) return false;
                if (s.type) { stages.push_back(s); continue; }
                if (auto *p = dynamic_cast<SurfaceNormalDataPointsFilter *>(f)) { sn = p; continue; }
                else if (dynamic_cast<IncidenceAngleDataPointsFilter *>(f)) s.type = PGICP_CHAIN_INCIDENCE_ANGLE;
                else if (auto *p = dynamic_cast<SphericalityDataPointsFilter *>(f)) { s.type = PGICP_CHAIN_SPHERICALITY; s.p[0] = p->keepUnstructureness ? 1.0 : 0.0; s.p[1] = p->keepStructureness ? 1.0 : 0.0; }
                else if (auto *p = dynamic_cast<ObservationDirectionDataPointsFilter *>(f)) { s.type = PGICP_CHAIN_OBSERVATION_DIRECTION; for (int a = 0; a < 3; a++) s.p[a] = (double)p->c0[a]; }
                else if (auto *p = dynamic_cast<SimpleSensorNoiseDataPointsFilter *>(f)) { s.type = PGICP_CHAIN_SIMPLE_SENSOR_NOISE; s.p[0] = (double)p->sensorType; s.p[1] = (double)p->gain; }
                else if (auto *p = dynamic_cast<OrientNormalsDataPointsFilter *>(f)) { s.type = PGICP_CHAIN_ORIENT_NORMALS; s.p[0] = p->towardCenter ? 1.0 : 0.0; }
                else if (auto *p = dynamic_cast<ShadowDataPointsFilter *>(f)) { s.type = PGICP_CHAIN_SHADOW; s.p[0] = (double)p->epsAngle; }
                else if (auto *p = dynamic_cast<MaxDensityDataPointsFilter *>(f)) { mdf = p; s.type = PGICP_CHAIN_MAX_DENSITY; s.p[0] = (double)p->maxDensity; s.p[1] = (double)p->seed; }
                else return false;
                stages.push_back(s);
            }
            if (!sn || (!made.ext() && stages.size() > PGICP_CHAIN_MAX_STAGES)) return false;
            const bool kn = sn->keepNormals, ke = sn->keepEigenValues, kd = sn->keepDensities;
            const bool obs = made.obs, noise = made.noise, inc = made.inc, sph = made.sph != nullptr;
            const bool uns = sph && made.sph->keepUnstructureness, str = sph && made.sph->keepStructureness;
            // the labels the run appends, in the order the filters append them one by one (SurfaceNormal: normals, densities, eigValues)
            typename DataPoints::Labels added;
            for (size_t j = k; j < k + len; j++) {
                DataPointsFilter *f = (*this)[j].get();
                if (dynamic_cast<SurfaceNormalDataPointsFilter *>(f)) {
                    if (kn) added.push_back(typename DataPoints::Label("normals", 3));
                    if (kd) added.push_back(typename DataPoints::Label("densities", 1));
                    if (ke) added.push_back(typename DataPoints::Label("eigValues", 3));
                } else if (dynamic_cast<ObservationDirectionDataPointsFilter *>(f)) added.push_back(typename DataPoints::Label("observationDirections", 3));
                else if (dynamic_cast<SimpleSensorNoiseDataPointsFilter *>(f)) added.push_back(typename DataPoints::Label("simpleSensorNoise", 1));
                else if (dynamic_cast<IncidenceAngleDataPointsFilter *>(f)) added.push_back(typename DataPoints::Label("incidenceAngles", 1));
                else if (dynamic_cast<SphericalityDataPointsFilter *>(f)) {
                    added.push_back(typename DataPoints::Label("sphericality", 1));
                    if (uns) added.push_back(typename DataPoints::Label("unstructureness", 1));
                    if (str) added.push_back(typename DataPoints::Label("structureness", 1));
                }
            }
            for (auto &l : added) if (c.descriptorExists(l.text)) return false;
            Matrix ox(frows, n), on(3, kn ? n : 0), oe(3, ke ? n : 0), od(1, kd ? n : 0), oo(3, obs ? n : 0), oz(1, noise ? n : 0), oc(drows, drows > 0 ? n : 0);
            Matrix oi(1, inc ? n : 0), os(1, sph ? n : 0), ou(1, uns ? n : 0), ot(1, str ? n : 0);
            std::vector<int32_t> idx((size_t)n);
            const double md = std::isfinite((double)sn->maxDist) ? (double)sn->maxDist : 1e300;
            int kept = 0;
            // (a run without one of the three descriptor filters takes the call it always took)
            int st;
            if (made.ext()) {
                const auto ptr = [](Matrix &m, bool want) { return want ? (void *)m.data() : nullptr; };
                pgicp_chain_out o;
                o.xyz = ox.data(); o.nrm = ptr(on, kn); o.nstride = 3; o.eig = ptr(oe, ke); o.dens = ptr(od, kd); o.obs = ptr(oo, obs); o.noise = ptr(oz, noise);
                o.desc = ptr(oc, drows > 0); o.incidence = ptr(oi, inc); o.sphericality = ptr(os, sph); o.unstructureness = ptr(ou, uns);
                o.structureness = ptr(ot, str); o.kept_idx = idx.data();
                st = pgslam_amd::Abi<T>::sensor_chain_ext(sn->ctx, c.features.data(), frows, n, sn->knn, md, kn, ke, kd, (int)stages.size(), stages.data(),
                                                          drows > 0 ? c.descriptors.data() : nullptr, drows, o, &kept);
            } else
                st = pgslam_amd::Abi<T>::sensor_chain(sn->ctx, c.features.data(), frows, n, sn->knn, md, kn, ke, kd, (int)stages.size(), stages.data(),
                                                      drows > 0 ? c.descriptors.data() : nullptr, drows, ox.data(), kn ? on.data() : nullptr,
                                                      ke ? oe.data() : nullptr, kd ? od.data() : nullptr, obs ? oo.data() : nullptr,
                                                      noise ? oz.data() : nullptr, drows > 0 ? oc.data() : nullptr, idx.data(), &kept);
            if (st == PGICP_ERR_ARG) return false;
            check(sn->ctx, st);
            int nd = drows;
            for (auto &l : added) nd += (int)l.span;
            std::vector<const Matrix *> rows;               // the call's output behind each added label
            for (auto &l : added)
                rows.push_back(l.text == "normals" ? &on : l.text == "densities" ? &od : l.text == "eigValues" ? &oe : l.text == "observationDirections" ? &oo :
                               l.text == "simpleSensorNoise" ? &oz : l.text == "incidenceAngles" ? &oi : l.text == "sphericality" ? &os : l.text == "unstructureness" ? &ou : &ot);
            Matrix f(frows, kept), d(nd, kept);
            for (int o = 0; o < kept; o++) {
                const int i = idx[(size_t)o];
                for (int r = 0; r < 3; r++) f(r, o) = ox(r, o);
                for (int r = 3; r < frows; r++) f(r, o) = c.features(r, i);
                int q = 0;
                for (int r = 0; r < drows; r++) d(q++, o) = oc(r, o);
                for (size_t a = 0; a < added.size(); a++)
                    for (int r = 0; r < (int)added[a].span; r++) d(q++, o) = (*rows[a])(r, o);
            }
            c.features = f;
            c.descriptors = d;
            for (auto &l : added) c.descriptorLabels.push_back(l);
            if (mdf) mdf->onDevice = true;
            return true;
        }
        //! the filters in order.  Two patterns are fused: a sensor-chain run (sensorChainRunAt) goes as one device call
        //! (applySensorChain) when it can, and SurfaceNormalDataPointsFilter{keepDensities} directly followed by
        //! MaxDensityDataPointsFilter runs as one device pass (MaxDensityDataPointsFilter::fusedWith); every other list as before
        void apply(DataPoints &cloud)
        {
            lastFused = 0;
            for (size_t k = 0; k < this->size(); k++) {
                if (const size_t run = sensorChainRunAt(k, &cloud)) {
                    if (applySensorChain(k, run, cloud)) { lastFused = run; k += run - 1; continue; }
                }
                if (k + 1 < this->size()) {
                    auto *sn = dynamic_cast<SurfaceNormalDataPointsFilter *>((*this)[k].get());
                    auto *md = dynamic_cast<MaxDensityDataPointsFilter *>((*this)[k + 1].get());
                    if (sn && md && sn->keepDensities && md->fusedWith(*sn, cloud)) { k++; continue; }
                }
                (*this)[k]->inPlaceFilter(cloud);
            }
        }
        //! every filter of the list has a device form (and the list fits pgicp_filter_cloud): the list as its argument.  `cloud`: the
        //! cloud the pass is about to see, for the filters whose entry names one of its rows (without it they have no device form)
        bool deviceSpecs(std::vector<pgicp_filter> &out, const DataPoints *cloud = nullptr) const
        {
            out.clear();
            if (this->size() > PGICP_MAX_FILTERS) return false;
            for (auto &f : *this) { pgicp_filter s; if (!(cloud ? f->deviceSpec(s, *cloud) : f->deviceSpec(s))) return false; out.push_back(s); }
            return true;
        }
        bool allIdentity() const
        {
            for (auto &f : *this) if (!std::dynamic_pointer_cast<IdentityDataPointsFilter>(f)) return false;
            return true;
        }
    };
    //! Localizer.hpp:103-106 in ONE device pass (pgicp_filter_cloud): filters.apply(cloud), in place, then
    //! cloud = RigidTransformation::compute(cloud, T).  `dev` receives the device address of the resulting features (a reading
    //! that needs no second upload; valid for the next three calls on `c`).  false: some filter has no device form, nothing
    //! was done (the caller applies the host filters and the transformation one after the other).
    static bool filterAndTransformOnDevice(pgicp_ctx *c, const DataPointsFilters &filters, DataPoints &cloud, const TransformationParameters &Tm,
                                           const T **dev = nullptr)
    {
        std::vector<pgicp_filter> specs;
        const int n = (int)cloud.getNbPoints();
        if (n == 0 || cloud.features.rows() < 3 || !filters.deviceSpecs(specs, &cloud)) return false;
        RigidTransformation check_t;
        if (!check_t.checkParameters(Tm)) throw std::runtime_error("RigidTransformation: the transformation is not rigid");
        double T16[16];
        pgslam_amd::to_row_major16(Tm, T16);
        const int drows = (int)cloud.descriptors.rows();
        const int r0 = cloud.descriptorExists("normals") && cloud.getDescriptorDimension("normals") == 3 ? cloud.getDescriptorStartingRow("normals") : -1;
        const int r1 = cloud.descriptorExists("observationDirections") && cloud.getDescriptorDimension("observationDirections") == 3
                           ? cloud.getDescriptorStartingRow("observationDirections") : -1;
        int kept = 0;
        const T *d = nullptr;
        T *const desc = drows ? cloud.descriptors.data() : nullptr;
        check(c, A::filter_cloud(c, (int)specs.size(), specs.data(), cloud.features.data(), (int)cloud.features.rows(), desc, drows, n, T16, r0, r1,
                                 cloud.features.data(), desc, &kept, &d));
        for (auto &f : filters) f->afterDevicePass();               // (a FixStep filter's step moves on, as after inPlaceFilter)
        cloud.features.conservativeResize(cloud.features.rows(), kept);
        if (drows) cloud.descriptors.conservativeResize(drows, kept);
        if (dev) *dev = d;
        return true;
    }

    //! closes the gaps of the dropped columns (ascending indices) in features and descriptors: what the filters' compactColumns
    //! leaves, as a few block moves
    static void compactByDropped(DataPoints &c, const std::vector<int32_t> &dropped)
    {
        const int n = (int)c.features.cols();
        if (dropped.empty()) return;
        const size_t fr = (size_t)c.features.rows(), dr = (size_t)c.descriptors.rows();
        T *f = c.features.data(), *d = dr ? c.descriptors.data() : nullptr;
        int dst = dropped[0];
        for (size_t k = 0; k < dropped.size(); k++) {
            const int from = dropped[k] + 1, to = k + 1 < dropped.size() ? dropped[k + 1] : n;      // the kept run [from, to)
            if (to > from) {
                std::memmove(f + (size_t)dst * fr, f + (size_t)from * fr, sizeof(T) * fr * (size_t)(to - from));
                if (d) std::memmove(d + (size_t)dst * dr, d + (size_t)from * dr, sizeof(T) * dr * (size_t)(to - from));
                dst += to - from;
            }
        }
        c.features.conservativeResize(c.features.rows(), dst);
        if (dr) c.descriptors.conservativeResize((int)dr, dst);
    }
    //! The device half of filterAndTransformOnDevice for a cloud that needs NO transformation (`Tm` the identity): the filters run
    //! on the uploaded features, `dev` / `kept` describe the filtered device copy, `dropped` lists what the HOST cloud still holds
    //! too much (ascending) -- the caller applies compactByDropped(cloud, dropped) when it suits it, e.g. on another thread while
    //! the ICP runs on the device copy.  false: not applicable (a transformation, a filter without a device form, more than 4 096
    //! points dropped): nothing was done, the caller takes filterAndTransformOnDevice.
    static bool filterOnDeviceDeferred(pgicp_ctx *c, const DataPointsFilters &filters, const DataPoints &cloud, const TransformationParameters &Tm,
                                       const T **dev, int *kept, std::vector<int32_t> &dropped)
    {
        std::vector<pgicp_filter> specs;
        const int n = (int)cloud.getNbPoints();
        if (n == 0 || cloud.features.rows() < 3 || !filters.deviceSpecs(specs)) return false;
        for (int i = 0; i < 4; i++) for (int j = 0; j < 4; j++) if (Tm(i, j) != (i == j ? T(1) : T(0))) return false;
        dropped.resize(4096);
        int nd = 0;
        check(c, A::filter_cloud_dev(c, (int)specs.size(), specs.data(), cloud.features.data(), (int)cloud.features.rows(), n, dropped.data(),
                                     (int)dropped.size(), &nd, kept, dev));
        if (nd > (int)dropped.size()) { dropped.clear(); return false; }       // (the filters' state has not moved: afterDevicePass was not called)
        dropped.resize((size_t)nd);
        for (auto &f : filters) f->afterDevicePass();
        return true;
    }

    struct ICPChainBase;

    // ------------------------------------------------------------------ Matcher
    struct Matcher {
        ICPChainBase *chain;
        int knn = 1; T epsilon = 0; T maxDist = std::numeric_limits<T>::infinity();
        int mapId = -1; int mapSize = 0;
        explicit Matcher(ICPChainBase *c) : chain(c) {}
        virtual ~Matcher() { release(); }
        void release() { if (mapId >= 0 && chain && chain->ctx.made()) { pgicp_map_destroy(chain->ctx, mapId); mapId = -1; } }
        //! Localizer.hpp:317, LoopCloser.hpp:356 -- index over the cloud AS GIVEN (not centred)
        virtual void init(const DataPoints &filteredReference) { initImpl(filteredReference, 0); }
        void initImpl(const DataPoints &ref, int center)
        {
            release();
            chain->pushParams();
            check(chain->ctx, A::map_create(chain->ctx, ref.xyzPtr(), ref.xyzStride(), ref.normalsPtr(), ref.normalsStride(), (int)ref.getNbPoints(), center, &mapId));
            mapSize = (int)ref.getNbPoints();
            chain->setMapValues(ref, mapId);          // (a GenericDescriptorOutlierFilter's row of the reference; nothing without one)
        }
        //! the same over a cloud that is in device memory already (DeviceCloud): no upload
        void initDevice(const pgslam_amd::DeviceCloud<T> &ref, int center)
        {
            release();
            chain->pushParams();
            if (chain->descriptorFilter())
                throw std::logic_error("Matcher: a GenericDescriptorOutlierFilter needs the reference's descriptors; a device cloud carries xyz and normals only");
            check(chain->ctx, A::map_create_dev(chain->ctx, ref.xyz, ref.xs, ref.hasNormals() ? ref.nrm : nullptr, ref.ns, ref.n, center, &mapId));
            mapSize = ref.n;
        }
        //! Localizer.hpp:328, LoopCloser.hpp:358
        virtual Matches findClosests(const DataPoints &filteredReading)
        {
            if (mapId < 0) throw std::runtime_error("Matcher::findClosests: init() was not called");
            const int n = (int)filteredReading.getNbPoints();
            Matches m(knn < 1 ? 1 : knn, n);                  // knn x N, column-major: [point][neighbour], as the ABI writes them
            takeRadii(filteredReading);
            chain->pushParams();
            armRadii(filteredReading);
            check(chain->ctx, A::match(chain->ctx, mapId, filteredReading.xyzPtr(), filteredReading.xyzStride(), n, m.ids.data(), m.dists.data()));
            return m;
        }
        //! A matcher with one search radius per reading point (KDTreeVarDistMatcher).  Every call that matches a host reading goes
        //! takeRadii(reading) -- the row is looked at and its largest value becomes maxDist --, pushParams(), armRadii(reading) --
        //! the row is handed to the next matching call of the context --, then the call.  Nothing for KDTreeMatcher.
        virtual bool perPointRadii() const { return false; }
        virtual void takeRadii(const DataPoints &) {}
        virtual void armRadii(const DataPoints &) const {}
        //! a reading that lives in device memory carries coordinates only: refused by a matcher that reads a descriptor of it
        virtual void refuseDeviceReading() const {}
    };
    //! [EXT] KDTreeVarDistMatcher{knn, epsilon, searchType, maxDistField} (Matchers/KDTree.cpp's second matcher): every reading point
    //! has its own search radius, the one-row descriptor `maxDistField` of the reading (default "maxSearchDist") after the reading
    //! filters, which carry descriptor rows along.  The statement is include/pgicp_vardist.h's: the neighbours of point i are the knn
    //! nearest among those with d2 <= r_i * r_i (the product in T); a negative or NaN radius is refused, +inf cuts nothing.  The
    //! context's max_dist is the row's largest value (+inf if any is).  It has no maxDist parameter (upstream has none).
    struct KDTreeVarDistMatcher : Matcher {
        std::string maxDistField = "maxSearchDist";
        explicit KDTreeVarDistMatcher(ICPChainBase *c) : Matcher(c) {}
        bool perPointRadii() const override { return true; }
        //! the row of `reading`: throws, naming the field, when the descriptor is missing or is not one row
        int row(const DataPoints &reading) const
        {
            if (!reading.descriptorExists(maxDistField))
                throw std::runtime_error("KDTreeVarDistMatcher: the reading has no descriptor " + maxDistField);
            if (reading.getDescriptorDimension(maxDistField) != 1)
                throw std::runtime_error("KDTreeVarDistMatcher: descriptor " + maxDistField + " must have one row, it has " +
                                         std::to_string(reading.getDescriptorDimension(maxDistField)));
            return (int)reading.getDescriptorStartingRow(maxDistField);
        }
        void takeRadii(const DataPoints &reading) override
        {
            const int r = row(reading);
            T largest = T(0);
            for (int j = 0; j < (int)reading.getNbPoints(); j++) {
                const T v = reading.descriptors(r, j);
                if (v > largest) largest = v;             // (+inf: the largest; a NaN is left to the consuming call, which refuses it)
            }
            this->maxDist = largest;
        }
        void armRadii(const DataPoints &reading) const override
        {
            const T *rowp = reading.descriptors.data() + row(reading);
            const int stride = (int)reading.descriptors.rows(), n = (int)reading.getNbPoints();
            check(this->chain->ctx, A::arm_radii(this->chain->ctx, 1, &rowp, &stride, &n));
        }
        void refuseDeviceReading() const override
        {
            throw std::runtime_error("KDTreeVarDistMatcher: the reading is a device cloud, which carries no descriptor " + maxDistField +
                                     "; pass the host cloud");
        }
    };

    // ------------------------------------------------------------------ OutlierFilters
    struct OutlierFilter {
        virtual ~OutlierFilter() {}
        virtual OutlierWeights compute(const DataPoints &reading, const DataPoints &reference, const Matches &input) = 0;
    };
    struct TrimmedDistOutlierFilter : OutlierFilter {
        ICPChainBase *chain; T ratio;
        TrimmedDistOutlierFilter(ICPChainBase *c, T r) : chain(c), ratio(r) {}
        OutlierWeights compute(const DataPoints &, const DataPoints &, const Matches &input) override
        {
            OutlierWeights w(input.dists.rows(), input.dists.cols());
            chain->pushParams();
            T lim; int nf;
            check(chain->ctx, A::weights(chain->ctx, input.dists.data(), (int)input.dists.size(), w.data(), &lim, &nf));
            return w;
        }
    };
    //! [EXT] VarTrimmedDistOutlierFilter{minRatio, maxRatio, lambda}: a TrimmedDist filter whose ratio is chosen at every call --
    //! the trim that minimises the fractional RMSD of the sorted residuals over [minRatio, maxRatio] (OutlierFiltersImpl.cpp,
    //! optimizeInlierRatio; the statement and its marked deviations: include/pgicp.h, pgicp_set_var_trim).  Every parameter must
    //! be given (upstream's defaults are not pinned here); 0 < minRatio < maxRatio <= 1, lambda finite and >= 0.  It takes the
    //! quantile slot (no TrimmedDist / MedianDist / Robust filter beside it).  Inside an ICP run the device applies it; this
    //! stage-level call is pgicp_outlier_weights under the same setting.
    struct VarTrimmedDistOutlierFilter : OutlierFilter {
        ICPChainBase *chain; T minRatio, maxRatio, lambda;
        VarTrimmedDistOutlierFilter(ICPChainBase *c, T mn, T mx, T l) : chain(c), minRatio(mn), maxRatio(mx), lambda(l)
        {
            if (!(minRatio > T(0) && minRatio < maxRatio && maxRatio <= T(1)))
                throw std::runtime_error("VarTrimmedDistOutlierFilter: need 0 < minRatio < maxRatio <= 1");
            if (!(lambda >= T(0)) || !std::isfinite((double)lambda))
                throw std::runtime_error("VarTrimmedDistOutlierFilter: lambda must be finite and >= 0");
        }
        OutlierWeights compute(const DataPoints &, const DataPoints &, const Matches &input) override
        {
            OutlierWeights w(input.dists.rows(), input.dists.cols());
            chain->pushParams();
            T lim; int nf;
            check(chain->ctx, A::weights(chain->ctx, input.dists.data(), (int)input.dists.size(), w.data(), &lim, &nf));
            return w;
        }
        //! the ratio the last call chose (upstream logs it as "Optimized ratio")
        double lastRatio() const { double r = 0.0; check(chain->ctx, pgicp_last_var_trim_ratio(chain->ctx, 0, &r)); return r; }
    };
    //! [EXT] MedianDistOutlierFilter{factor}: limit = factor * getDistsQuantile(0.5) on the SQUARED match distances, weight 1
    //! while dist <= limit (OutlierFiltersImpl.cpp as restated in oracle/icp_oracle.c: orc_median_weights).  On the device
    //! it is the trimmed filter's exact order statistic at ratio 0.5, scaled (pgicp_params.quantile_scale).
    struct MedianDistOutlierFilter : OutlierFilter {
        ICPChainBase *chain; T factor;
        MedianDistOutlierFilter(ICPChainBase *c, T f) : chain(c), factor(f) {}
        OutlierWeights compute(const DataPoints &, const DataPoints &, const Matches &input) override
        {
            OutlierWeights w(input.dists.rows(), input.dists.cols());
            chain->pushParams();
            T lim; int nf;
            check(chain->ctx, A::weights(chain->ctx, input.dists.data(), (int)input.dists.size(), w.data(), &lim, &nf));
            return w;
        }
    };
    //! [EXT] RobustOutlierFilter{robustFct, tuning, scaleEstimator, nbIterationForScale, distanceType, approximation}: an
    //! M-estimator weight per pair from e2 = dist / scale^2 (OutlierFiltersImpl.cpp as restated in oracle/icp_oracle.c:
    //! orc_robust_weights), scale = sqrt(median absolute deviation of the finite squared distances), 1, or berg's (scaleEstimator
    //! berg: `tuning` is the target scale and the weight function runs with tuning 1).  distanceType point2plane weighs by the
    //! squared distance from the matched point's plane; nbIterationForScale n > 0 estimates the scale in the first n iterations
    //! of an ICP and holds it afterwards (the statement and its marked deviation: include/pgicp_robust.h).  No TrimmedDist /
    //! MedianDist filter beside it, knn 1; scaleEstimator std is not offered.  These three are the constructor's: loadFromYaml keeps
    //! refusing them by name, a YAML names upstream's defaults only.  Inside an ICP run the device applies it
    //! (pgicp_params.robust_*, pgicp_set_robust_ext); this stage-level call is pgicp_outlier_weights under the same settings: one
    //! pass is iteration 1, and a bare array of distances has no planes -- point2plane is refused there.
    struct RobustOutlierFilter : OutlierFilter {
        ICPChainBase *chain; std::string robustFct, scaleEstimator; T tuning, approximation;
        std::string distanceType;
        int nbIterationForScale;
        RobustOutlierFilter(ICPChainBase *c, const std::string &fct = "cauchy", T tun = T(1), const std::string &scale = "mad",
                            T approx = std::numeric_limits<T>::infinity(), const std::string &dist = "point2point", int nbIter = 0)
            : chain(c), robustFct(fct), scaleEstimator(scale), tuning(tun), approximation(approx), distanceType(dist), nbIterationForScale(nbIter)
        {
            fctCode(); scaleCode(); distCode();
            if (!(tuning > T(0))) throw std::runtime_error("RobustOutlierFilter: tuning must be positive");
            if (nbIterationForScale < 0) throw std::runtime_error("RobustOutlierFilter: nbIterationForScale must be >= 0");
        }
        int distCode() const
        {
            if (distanceType == "point2point") return PGICP_ROBUST_DIST_POINT2POINT;
            if (distanceType == "point2plane") return PGICP_ROBUST_DIST_POINT2PLANE;
            throw std::runtime_error("RobustOutlierFilter: unknown distanceType " + distanceType + " (point2point, point2plane)");
        }
        //! what pgicp_set_robust_ext is handed; asksNothing(): the filter as pgicp_params alone describes it
        pgicp_robust_ext ext() const { pgicp_robust_ext x = {distCode(), scaleCode(), nbIterationForScale}; return x; }
        bool asksNothing() const { return distCode() == PGICP_ROBUST_DIST_POINT2POINT && scaleCode() != PGICP_ROBUST_SCALE_BERG && nbIterationForScale == 0; }
        int fctCode() const
        {
            static const char *names[] = {"cauchy", "welsch", "sc", "gm", "tukey", "huber", "L1"};
            for (int k = 0; k < 7; k++) if (robustFct == names[k]) return PGICP_ROBUST_CAUCHY + k;
            throw std::runtime_error("RobustOutlierFilter: unknown robustFct " + robustFct + " (cauchy, welsch, sc, gm, tukey, huber, L1)");
        }
        int scaleCode() const
        {
            if (scaleEstimator == "mad") return PGICP_ROBUST_SCALE_MAD;
            if (scaleEstimator == "none") return PGICP_ROBUST_SCALE_NONE;
            if (scaleEstimator == "berg") return PGICP_ROBUST_SCALE_BERG;
            if (scaleEstimator == "std") throw std::runtime_error("RobustOutlierFilter: scaleEstimator std is not offered (mad, none, berg): its treatment of pairs without a neighbour is not pinned here");
            throw std::runtime_error("RobustOutlierFilter: scaleEstimator " + scaleEstimator + " is not supported (mad, none, berg)");
        }
        OutlierWeights compute(const DataPoints &, const DataPoints &, const Matches &input) override
        {
            OutlierWeights w(input.dists.rows(), input.dists.cols());
            chain->pushParams();
            T lim; int nf;
            check(chain->ctx, A::weights(chain->ctx, input.dists.data(), (int)input.dists.size(), w.data(), &lim, &nf));
            return w;
        }
    };
    //! [EXT] MaxDistOutlierFilter{maxDist}: weight 1 while the squared match distance is <= maxDist^2, else 0
    struct MaxDistOutlierFilter : OutlierFilter {
        T maxDist;
        explicit MaxDistOutlierFilter(T d) : maxDist(d) {}
        OutlierWeights compute(const DataPoints &, const DataPoints &, const Matches &input) override
        {
            OutlierWeights w(input.dists.rows(), input.dists.cols());
            const T lim = maxDist * maxDist;
            for (int j = 0; j < w.cols(); j++) for (int i = 0; i < w.rows(); i++) w(i, j) = input.dists(i, j) <= lim ? T(1) : T(0);
            return w;
        }
    };
    //! [EXT] SurfaceNormalOutlierFilter{maxAngle}: weight 0 when the angle between the (normalised) normals of a reading
    //! point and of its matched reference point exceeds maxAngle, or the match is invalid; ones when either cloud has no
    //! `normals` descriptor.  Inside an ICP run the device applies it (pgicp_params.normal_max_angle); this
    //! host version serves the stage-level call of the partial chains (Localizer.hpp:330, LoopCloser.hpp:360).
    struct SurfaceNormalOutlierFilter : OutlierFilter {
        T maxAngle;
        explicit SurfaceNormalOutlierFilter(T a) : maxAngle(a) {}
        OutlierWeights compute(const DataPoints &reading, const DataPoints &reference, const Matches &input) override
        {
            OutlierWeights w = OutlierWeights::Constant(input.ids.rows(), input.ids.cols(), T(1));
            if (!reading.descriptorExists("normals") || !reference.descriptorExists("normals")) return w;
            const int rr = reading.getDescriptorStartingRow("normals"), rf = reference.getDescriptorStartingRow("normals");
            const T eps = std::cos(maxAngle);
            auto normalized = [](T &x, T &y, T &z) { const T zz = (x * x + y * y) + z * z; if (zz > T(0)) { const T s = std::sqrt(zz); x = x / s; y = y / s; z = z / s; } };
            for (int j = 0; j < w.cols(); j++) {
                T ax = reading.descriptors(rr, j), ay = reading.descriptors(rr + 1, j), az = reading.descriptors(rr + 2, j);
                normalized(ax, ay, az);
                for (int i = 0; i < w.rows(); i++) {
                    const int id = input.ids(i, j);
                    if (id < 0) { w(i, j) = T(0); continue; }
                    T bx = reference.descriptors(rf, id), by = reference.descriptors(rf + 1, id), bz = reference.descriptors(rf + 2, id);
                    normalized(bx, by, bz);
                    if (((ax * bx + ay * by) + az * bz) < eps) w(i, j) = T(0);
                }
            }
            return w;
        }
    };
    //! [EXT] GenericDescriptorOutlierFilter{source, descName, useSoftThreshold, useLargerThan, threshold}: a weight per pair from the
    //! one-row descriptor `descName` of the reference at the pair's neighbour (OutlierFiltersImpl.cpp; the statement and its marked
    //! deviations: include/pgicp.h, pgicp_set_descriptor_filter).  Hard: desc > threshold (useLargerThan 1) or desc < threshold,
    //! strict, 1 / 0; soft: desc / its maximum over the pairs.  Only `source: reference`; descName, and threshold in hard mode,
    //! must be given.  Inside an ICP run the device applies it (the matcher's map carries the row: pgicp_map_set_values); this
    //! host version serves the stage-level call of the partial chains, from Matches.ids and the reference's descriptor.
    struct GenericDescriptorOutlierFilter : OutlierFilter {
        std::string descName; bool soft; bool largerThan; T threshold;
        GenericDescriptorOutlierFilter(const std::string &name, bool s, bool larger, T thr) : descName(name), soft(s), largerThan(larger), threshold(thr)
        {
            if (descName.empty()) throw std::runtime_error("GenericDescriptorOutlierFilter: descName must be given");
            if (!soft && !std::isfinite((double)threshold)) throw std::runtime_error("GenericDescriptorOutlierFilter: threshold must be finite");
        }
        int mode() const { return soft ? PGICP_DESC_FILTER_SOFT : largerThan ? PGICP_DESC_FILTER_LARGER : PGICP_DESC_FILTER_SMALLER; }
        //! the reference's row `descName` (throws when it is missing or is not one row)
        int row(const DataPoints &reference) const
        {
            if (!reference.descriptorExists(descName))
                throw std::runtime_error("GenericDescriptorOutlierFilter: the reference has no descriptor '" + descName + "'");
            if (reference.getDescriptorDimension(descName) != 1)
                throw std::runtime_error("GenericDescriptorOutlierFilter: the descriptor '" + descName + "' has more than one row");
            return reference.getDescriptorStartingRow(descName);
        }
        OutlierWeights compute(const DataPoints &, const DataPoints &reference, const Matches &input) override
        {
            const int r = row(reference);
            OutlierWeights w = OutlierWeights::Constant(input.ids.rows(), input.ids.cols(), T(0));
            T mx = T(0);
            for (int j = 0; j < w.cols(); j++)
                for (int i = 0; i < w.rows(); i++) {
                    const int id = input.ids(i, j);
                    if (id < 0) continue;                         // (deviation a: no neighbour weighs 0, outside the maximum)
                    const T v = reference.descriptors(r, id);
                    if (!std::isfinite((double)v)) throw std::runtime_error("GenericDescriptorOutlierFilter: a value is not finite");
                    if (soft) {
                        if (v < T(0)) throw std::runtime_error("GenericDescriptorOutlierFilter: soft mode needs values >= 0");
                        w(i, j) = v;
                        if (v > mx) mx = v;
                    } else w(i, j) = (largerThan ? v > threshold : v < threshold) ? T(1) : T(0);
                }
            if (soft) {
                if (!(mx > T(0))) return OutlierWeights::Constant(w.rows(), w.cols(), T(0));       // (deviation b)
                for (int j = 0; j < w.cols(); j++) for (int i = 0; i < w.rows(); i++) w(i, j) = w(i, j) / mx;
            }
            return w;
        }
    };
    struct OutlierFilters : std::vector<std::shared_ptr<OutlierFilter>> {
        //! Localizer.hpp:330, LoopCloser.hpp:360 -- element-wise product of the filters' weights
        OutlierWeights compute(const DataPoints &reading, const DataPoints &reference, const Matches &input)
        {
            if (this->empty()) return OutlierWeights::Constant(input.ids.rows(), input.ids.cols(), T(1));
            OutlierWeights w = (*this)[0]->compute(reading, reference, input);
            for (size_t k = 1; k < this->size(); k++) {
                const OutlierWeights o = (*this)[k]->compute(reading, reference, input);
                for (int j = 0; j < w.cols(); j++) for (int i = 0; i < w.rows(); i++) w(i, j) *= o(i, j);
            }
            return w;
        }
    };

    // ------------------------------------------------------------------ ErrorMinimizer
    struct ErrorMinimizer {
        //! the matched, weighted pairs (Localizer.hpp:332): compaction of the non-zero-weight matches
        struct ErrorElements {
            DataPoints reading, reference;
            OutlierWeights weights;
            Matches matches;
            int nbRejectedMatches = 0, nbRejectedPoints = 0;
            T pointUsedRatio = 0, weightedPointUsedRatio = 0;
            ErrorElements() {}
            ErrorElements(const DataPoints &requestedPts, const DataPoints &sourcePts, const OutlierWeights &outlierWeights, const Matches &m)
            {
                const int knn = outlierWeights.rows(), n = outlierWeights.cols();
                int kept = 0; double wsum = 0;
                for (int k = 0; k < knn; k++) for (int i = 0; i < n; i++) if (outlierWeights(k, i) != T(0)) { kept++; wsum += (double)outlierWeights(k, i); }
                if (kept == 0) throw ConvergenceError("ErrorMnimizer: no point to minimize");
                reading.features = Matrix(requestedPts.features.rows(), kept); reading.featureLabels = requestedPts.featureLabels;
                reading.descriptors = Matrix(requestedPts.descriptors.rows(), kept); reading.descriptorLabels = requestedPts.descriptorLabels;
                reference.features = Matrix(sourcePts.features.rows(), kept); reference.featureLabels = sourcePts.featureLabels;
                reference.descriptors = Matrix(sourcePts.descriptors.rows(), kept); reference.descriptorLabels = sourcePts.descriptorLabels;
                weights = OutlierWeights(1, kept); matches = Matches(1, kept);
                int j = 0;
                for (int k = 0; k < knn; k++)
                    for (int i = 0; i < n; i++) {
                        if (outlierWeights(k, i) == T(0)) continue;
                        const int id = m.ids(k, i);
                        for (int r = 0; r < reading.features.rows(); r++) reading.features(r, j) = requestedPts.features(r, i);
                        for (int r = 0; r < reading.descriptors.rows(); r++) reading.descriptors(r, j) = requestedPts.descriptors(r, i);
                        for (int r = 0; r < reference.features.rows(); r++) reference.features(r, j) = sourcePts.features(r, id);
                        for (int r = 0; r < reference.descriptors.rows(); r++) reference.descriptors(r, j) = sourcePts.descriptors(r, id);
                        weights(0, j) = outlierWeights(k, i); matches.ids(0, j) = id; matches.dists(0, j) = m.dists(k, i);
                        j++;
                    }
                nbRejectedMatches = knn * n - kept;
                pointUsedRatio = (T)((double)kept / (double)(knn * n));
                weightedPointUsedRatio = (T)(wsum / (double)(knn * n));
            }
        };
        ICPChainBase *chain;
        T sensorStdDev = T(0.01);
        bool withCov = false;
        bool pointToPoint = false;       //!< PointToPointErrorMinimizer (Kabsch); else PointToPlane(WithCov)
        bool force4DOF = false;          //!< PointToPlane[WithCov]ErrorMinimizer{force4DOF: 1}: rotation about z + translation only
        // state of the last ICP run / compute()
        T lastOverlap = 0; T lastResidual = 0; Matrix lastCov = Matrix::Zero(6, 6);
        explicit ErrorMinimizer(ICPChainBase *c) : chain(c) {}
        virtual ~ErrorMinimizer() {}
        //! Localizer.hpp:278, LoopCloser.hpp:331: weightedPointUsedRatio of the last error elements (pgslam's own clouds carry no
        //! simpleSensorNoise descriptor -- SURVEY.md A.7); for a reading that does (and, with the point-to-plane minimizer, `normals`
        //! too: ErrorMinimizers/PointToPlane.cpp) the share of the last error elements whose distance lies below mean + noise
        //! (ICPChainBase::sensorNoiseOverlap; oracle: orc_sensor_noise_overlap)
        T getOverlap() const { return lastOverlap; }
        T getWeightedPointUsedRatio() const { return lastRatio; }
        T lastRatio = 0;
        //! Localizer.hpp:238, LoopCloser.hpp:108: 6x6 Censi covariance, order [x y z rx ry rz]; zeros without "WithCov"
        Matrix getCovariance() const { return withCov ? lastCov : Matrix::Zero(6, 6); }
        //! LoopCloser.hpp:362: sum w (n.(p-q))^2 -- `reference` must be the cloud given to matcher->init
        T getResidualError(const DataPoints &filteredReading, const DataPoints &, const OutlierWeights &w, const Matches &m) const
        {
            double ratio, res;
            if (!chain->matcher || chain->matcher->mapId < 0) throw std::runtime_error("getResidualError: matcher->init() was not called");
            // pgicp_error_stats reads n x knn ids and weights with the CONTEXT's knn: push the chain's parameters and refuse
            // matches made under another knn (an out-of-bounds host read otherwise -- ADVICE round 4)
            chain->pushParams();
            const int K = chain->matcher->knn < 1 ? 1 : chain->matcher->knn, n = (int)filteredReading.getNbPoints();
            if (m.ids.rows() != K || w.rows() != K || m.ids.cols() != n || w.cols() != n)
                throw std::runtime_error("getResidualError: matches / weights are not knn x N of this chain's matcher");
            check(chain->ctx, A::stats(chain->ctx, chain->matcher->mapId, filteredReading.xyzPtr(), filteredReading.xyzStride(),
                                       (int)filteredReading.getNbPoints(), m.ids.data(), w.data(), &ratio, &res, nullptr));
            return (T)res;
        }
    };

    // ------------------------------------------------------------------ TransformationCheckers
    struct TransformationChecker { virtual ~TransformationChecker() {} std::string name; };
    struct CounterTransformationChecker : TransformationChecker { int maxIterationCount = 40; };
    struct DifferentialTransformationChecker : TransformationChecker { T minDiffRotErr = T(0.001), minDiffTransErr = T(0.001); int smoothLength = 3; };
    //! [EXT] BoundTransformationChecker{maxRotationNorm, maxTranslationNorm}: ConvergenceError when the accumulated correction
    //! leaves the bound
    struct BoundTransformationChecker : TransformationChecker { T maxRotationNorm = T(1), maxTranslationNorm = T(1); };
    struct TransformationCheckers : std::vector<std::shared_ptr<TransformationChecker>> {};

    // ------------------------------------------------------------------ ICP chain
    struct ICPChainBase {
        DataPointsFilters readingDataPointsFilters, readingStepDataPointsFilters, referenceDataPointsFilters;
        Transformations transformations;
        std::shared_ptr<Matcher> matcher;
        OutlierFilters outlierFilters;
        std::shared_ptr<ErrorMinimizer> errorMinimizer;
        TransformationCheckers transformationCheckers;
        pgslam_amd::LazyContext ctx;                 // the chain's device context and stream, made at first use
        pgicp_stats lastStats;
        //! Observer of every completed alignment (not part of libpointmatcher; its `inspector` slot sees iterations, not
        //! calls): the filtered reading, the filtered reference the index was built on, the initial guess, the result and
        //! the device statistics.  Used to record ICP calls of a SLAM run for replay through the CPU oracle.
        std::function<void(const DataPoints &, const DataPoints &, const TransformationParameters &, const TransformationParameters &,
                           const pgicp_stats &)> onAlign;
        const DataPoints *currentReference = nullptr;
        //! optional gate of the observer: asked once per completed alignment BEFORE the observer's arguments are made; false
        //! skips the observer for that call (a map that lives only in device memory is downloaded for the observer's sake)
        std::function<bool()> onAlignWanted;
        //! the host copy of a device-resident reference, made when an observer asks for it (ICPSequence::setMap(DeviceCloud))
        std::function<DataPoints()> lazyReference;
        DataPoints lazyReferenceCloud;
        const DataPoints *observedReference()
        {
            if (currentReference) return currentReference;
            if (!lazyReference) return nullptr;
            lazyReferenceCloud = lazyReference();
            lazyReference = nullptr;
            currentReference = &lazyReferenceCloud;
            return currentReference;
        }

        explicit ICPChainBase(int device = 0) : ctx(device)
        {
            std::memset(&lastStats, 0, sizeof lastStats);
            // (upstream's constructor leaves the chain EMPTY -- an ICP object used without setDefault() / loadFromYaml() has no
            // matcher there; here it starts with the default matcher / outlier filter / minimiser / checkers and no data-point
            // filters, so that members can be set one by one; setDefault() is upstream's, data-point filters included)
            setDefaultWithoutDataPointsFilters();
        }
        ICPChainBase(const ICPChainBase &) = delete;
        ICPChainBase &operator=(const ICPChainBase &) = delete;
        virtual ~ICPChainBase()
        {
            matcher.reset();
            ctx.destroy();
        }
        void cleanup()
        {
            readingDataPointsFilters.clear(); readingStepDataPointsFilters.clear(); referenceDataPointsFilters.clear();
            transformations.clear(); outlierFilters.clear(); transformationCheckers.clear();
            matcher.reset(); errorMinimizer.reset();
        }
        //! libpointmatcher defaults ([EXT] ICP.cpp ICPChaineBase::setDefault): RandomSamplingDataPointsFilter on the
        //! reading, SamplingSurfaceNormalDataPointsFilter on the reference (where the default point-to-plane minimiser gets its
        //! normals from), KDTreeMatcher, TrimmedDist 0.85, PointToPlane, Counter(40) + Differential
        virtual void setDefault()
        {
            setDefaultWithoutDataPointsFilters();
            readingDataPointsFilters.push_back(std::make_shared<RandomSamplingDataPointsFilter>(T(0.75), 1ULL));
            referenceDataPointsFilters.push_back(std::make_shared<SamplingSurfaceNormalDataPointsFilter>());
        }
        void setDefaultWithoutDataPointsFilters()
        {
            cleanup();
            transformations.push_back(std::make_shared<RigidTransformation>(&ctx));
            matcher = std::make_shared<Matcher>(this);
            outlierFilters.push_back(std::make_shared<TrimmedDistOutlierFilter>(this, T(0.85)));
            errorMinimizer = std::make_shared<ErrorMinimizer>(this);
            transformationCheckers.push_back(std::make_shared<CounterTransformationChecker>());
            transformationCheckers.push_back(std::make_shared<DifferentialTransformationChecker>());
        }
        //! Localizer.hpp:70,311; LoopCloser.hpp:73,348
        virtual void loadFromYaml(std::istream &in)
        {
            using pgslam_amd::yaml_lite::to_double;
            const auto y = pgslam_amd::yaml_lite::parse(in);
            cleanup();
            transformations.push_back(std::make_shared<RigidTransformation>(&ctx));
            if (y.has("readingDataPointsFilters")) readingDataPointsFilters.load(y.sections.at("readingDataPointsFilters"));
            if (y.has("readingStepDataPointsFilters")) {
                // step filters are applied ONCE here (they are pure functions of the cloud); upstream's random sampler draws
                // a fresh sample in every iteration, which one fixed subsample does not reproduce (overlap and covariance
                // would be those of the subsample): refused in this slot, never silently approximated
                for (auto &m : y.sections.at("readingStepDataPointsFilters"))
                    if (m.name == "RandomSamplingDataPointsFilter")
                        throw std::runtime_error("loadFromYaml: RandomSamplingDataPointsFilter is not supported in readingStepDataPointsFilters "
                                                 "(per-iteration resampling); use it in readingDataPointsFilters");
                readingStepDataPointsFilters.load(y.sections.at("readingStepDataPointsFilters"));
            }
            if (y.has("referenceDataPointsFilters")) referenceDataPointsFilters.load(y.sections.at("referenceDataPointsFilters"));
            matcher = std::make_shared<Matcher>(this);
            if (y.has("matcher") && !y.sections.at("matcher").empty() && y.sections.at("matcher")[0].name == "KDTreeVarDistMatcher") {
                auto vd = std::make_shared<KDTreeVarDistMatcher>(this);
                for (auto &kv : y.sections.at("matcher")[0].params) {
                    if (kv.first == "knn") vd->knn = (int)to_double(kv.second, "knn");
                    else if (kv.first == "epsilon") vd->epsilon = (T)to_double(kv.second, "epsilon");
                    else if (kv.first == "searchType") {}      // both search types return the same neighbours here
                    else if (kv.first == "maxDistField") vd->maxDistField = kv.second;
                    else throw std::runtime_error("KDTreeVarDistMatcher: unknown parameter " + kv.first);
                }
                matcher = vd;
            } else if (y.has("matcher") && !y.sections.at("matcher").empty()) {
                const auto &m = y.sections.at("matcher")[0];
                if (m.name != "KDTreeMatcher") throw std::runtime_error("loadFromYaml: unsupported matcher " + m.name + " (KDTreeMatcher, KDTreeVarDistMatcher)");
                for (auto &kv : m.params) {
                    if (kv.first == "knn") matcher->knn = (int)to_double(kv.second, "knn");
                    else if (kv.first == "epsilon") matcher->epsilon = (T)to_double(kv.second, "epsilon");
                    else if (kv.first == "maxDist") matcher->maxDist = (T)to_double(kv.second, "maxDist");
                    else if (kv.first == "searchType") {}      // both search types return the same neighbours here
                    else throw std::runtime_error("KDTreeMatcher: unknown parameter " + kv.first);
                }
            }
            // the chain multiplies its filters' weights (A.4): one QUANTILE filter (TrimmedDist or MedianDist) and / or one
            // MaxDist filter, in any order
            if (y.has("outlierFilters")) {
                int n_trim = 0, n_max = 0, n_nrm = 0, n_gd = 0;
                for (auto &m : y.sections.at("outlierFilters")) {
                    if (m.name == "GenericDescriptorOutlierFilter") {
                        if (n_gd++) throw std::runtime_error("GenericDescriptorOutlierFilter: at most one per chain");
                        std::string source = "reference", name;
                        bool soft = false, larger = true, hasThr = false;
                        T thr = T(0);
                        for (auto &kv : m.params) {
                            if (kv.first == "source") source = kv.second;
                            else if (kv.first == "descName") name = kv.second;
                            else if (kv.first == "useSoftThreshold") soft = to_double(kv.second, "useSoftThreshold") != 0.0;
                            else if (kv.first == "useLargerThan") larger = to_double(kv.second, "useLargerThan") != 0.0;
                            else if (kv.first == "threshold") { thr = (T)to_double(kv.second, "threshold"); hasThr = true; }
                            else throw std::runtime_error("GenericDescriptorOutlierFilter: unknown parameter " + kv.first);
                        }
                        // (deviation c: upstream's reading source reads the reading's descriptor at the reference's index)
                        if (source != "reference") throw std::runtime_error("GenericDescriptorOutlierFilter: source " + source + " is not supported (reference)");
                        if (name.empty()) throw std::runtime_error("GenericDescriptorOutlierFilter: parameter descName must be given");
                        if (!soft && !hasThr) throw std::runtime_error("GenericDescriptorOutlierFilter: parameter threshold must be given (hard mode)");
                        outlierFilters.push_back(std::make_shared<GenericDescriptorOutlierFilter>(name, soft, larger, thr));
                        continue;
                    }
                    if (m.name == "SurfaceNormalOutlierFilter" && n_nrm++ == 0) {
                        outlierFilters.push_back(std::make_shared<SurfaceNormalOutlierFilter>(m.params.count("maxAngle") ? (T)to_double(m.params.at("maxAngle"), "maxAngle") : T(1.57)));
                        continue;
                    }
                    if (m.name == "TrimmedDistOutlierFilter" && n_trim++ == 0)
                        outlierFilters.push_back(std::make_shared<TrimmedDistOutlierFilter>(this, m.params.count("ratio") ? (T)to_double(m.params.at("ratio"), "ratio") : T(0.85)));
                    else if (m.name == "MedianDistOutlierFilter" && n_trim++ == 0) {
                        const T f = m.params.count("factor") ? (T)to_double(m.params.at("factor"), "factor") : T(3);
                        if (!(f > T(0))) throw std::runtime_error("MedianDistOutlierFilter: factor must be positive");
                        outlierFilters.push_back(std::make_shared<MedianDistOutlierFilter>(this, f));
                    } else if (m.name == "RobustOutlierFilter" && n_trim++ == 0) {
                        std::string fct = "cauchy", scale = "mad", dtype = "point2point";
                        T tun = T(1), approx = std::numeric_limits<T>::infinity();
                        int nbIter = 0;
                        for (auto &kv : m.params) {
                            if (kv.first == "robustFct") fct = kv.second;
                            else if (kv.first == "scaleEstimator") scale = kv.second;
                            else if (kv.first == "distanceType") dtype = kv.second;
                            else if (kv.first == "tuning") tun = (T)to_double(kv.second, "tuning");
                            else if (kv.first == "approximation") approx = (T)to_double(kv.second, "approximation");
                            else if (kv.first == "nbIterationForScale") nbIter = (int)to_double(kv.second, "nbIterationForScale");
                            else throw std::runtime_error("RobustOutlierFilter: unknown parameter " + kv.first);
                        }
                        // A YAML still names upstream's defaults only (tests/cpp/test_dropin_cpu.cpp pins these refusals): the filter's
                        // other settings -- include/pgicp_robust.h -- are given to its constructor, which a chain built in code calls.
                        if (dtype != "point2point") throw std::runtime_error("RobustOutlierFilter: distanceType " + dtype + " is not supported in a YAML (point2point; the constructor takes point2plane)");
                        if (nbIter != 0) throw std::runtime_error("RobustOutlierFilter: nbIterationForScale must be 0 in a YAML (the constructor takes a count)");
                        if (scale == "berg") throw std::runtime_error("RobustOutlierFilter: scaleEstimator berg is not supported in a YAML (mad, none; the constructor takes berg)");
                        outlierFilters.push_back(std::make_shared<RobustOutlierFilter>(this, fct, tun, scale, approx));
                    } else if (m.name == "VarTrimmedDistOutlierFilter" && n_trim++ == 0) {
                        // (every parameter explicit: upstream's defaults are not pinned here -- refuse rather than guess)
                        for (auto &kv : m.params)
                            if (kv.first != "minRatio" && kv.first != "maxRatio" && kv.first != "lambda")
                                throw std::runtime_error("VarTrimmedDistOutlierFilter: unknown parameter " + kv.first);
                        for (const char *k : {"minRatio", "maxRatio", "lambda"})
                            if (!m.params.count(k)) throw std::runtime_error(std::string("VarTrimmedDistOutlierFilter: parameter ") + k + " must be given");
                        outlierFilters.push_back(std::make_shared<VarTrimmedDistOutlierFilter>(this, (T)to_double(m.params.at("minRatio"), "minRatio"),
                                                                                               (T)to_double(m.params.at("maxRatio"), "maxRatio"),
                                                                                               (T)to_double(m.params.at("lambda"), "lambda")));
                    } else if (m.name == "MaxDistOutlierFilter" && n_max++ == 0)
                        outlierFilters.push_back(std::make_shared<MaxDistOutlierFilter>(m.params.count("maxDist") ? (T)to_double(m.params.at("maxDist"), "maxDist") : T(1)));
                    else
                        throw std::runtime_error("loadFromYaml: unsupported outlier filter chain at " + m.name +
                                                 " (supported: one of TrimmedDistOutlierFilter, VarTrimmedDistOutlierFilter, MedianDistOutlierFilter or RobustOutlierFilter, and / or one MaxDistOutlierFilter, "
                                                 "and / or one SurfaceNormalOutlierFilter, and / or one GenericDescriptorOutlierFilter)");
                }
            } else outlierFilters.push_back(std::make_shared<TrimmedDistOutlierFilter>(this, T(0.85)));
            errorMinimizer = std::make_shared<ErrorMinimizer>(this);
            if (y.has("errorMinimizer") && !y.sections.at("errorMinimizer").empty()) {
                const auto &m = y.sections.at("errorMinimizer")[0];
                if (m.name == "PointToPlaneWithCovErrorMinimizer") errorMinimizer->withCov = true;
                else if (m.name == "PointToPointErrorMinimizer") errorMinimizer->pointToPoint = true;
                // [EXT] PointToPointWithCovErrorMinimizer{sensorStdDev}: the point-to-point solve + the covariance estimate (the
                // body of PointToPlaneWithCov's, read from the reference's normals) -- what a point-to-point pgslam configuration
                // needs, its optimiser refuses the base class's zero covariance (Optimizer.hpp:94,109)
                else if (m.name == "PointToPointWithCovErrorMinimizer") { errorMinimizer->pointToPoint = true; errorMinimizer->withCov = true; }
                else if (m.name != "PointToPlaneErrorMinimizer") throw std::runtime_error("loadFromYaml: unsupported error minimizer " + m.name);
                for (auto &kv : m.params) {
                    if (kv.first == "sensorStdDev") errorMinimizer->sensorStdDev = (T)to_double(kv.second, "sensorStdDev");
                    else if (kv.first == "force4DOF" && !errorMinimizer->pointToPoint) errorMinimizer->force4DOF = !(kv.second == "0" || kv.second == "false");
                    else if ((kv.first == "force2D" || kv.first == "force4DOF") && (kv.second == "0" || kv.second == "false")) {}
                    else throw std::runtime_error(m.name + ": unsupported parameter " + kv.first);
                }
            }
            if (y.has("transformationCheckers"))
                for (auto &m : y.sections.at("transformationCheckers")) {
                    if (m.name == "CounterTransformationChecker") {
                        auto c = std::make_shared<CounterTransformationChecker>();
                        if (m.params.count("maxIterationCount")) c->maxIterationCount = (int)to_double(m.params.at("maxIterationCount"), "maxIterationCount");
                        transformationCheckers.push_back(c);
                    } else if (m.name == "DifferentialTransformationChecker") {
                        auto c = std::make_shared<DifferentialTransformationChecker>();
                        if (m.params.count("minDiffRotErr")) c->minDiffRotErr = (T)to_double(m.params.at("minDiffRotErr"), "minDiffRotErr");
                        if (m.params.count("minDiffTransErr")) c->minDiffTransErr = (T)to_double(m.params.at("minDiffTransErr"), "minDiffTransErr");
                        if (m.params.count("smoothLength")) c->smoothLength = (int)to_double(m.params.at("smoothLength"), "smoothLength");
                        transformationCheckers.push_back(c);
                    } else if (m.name == "BoundTransformationChecker") {
                        auto c = std::make_shared<BoundTransformationChecker>();
                        if (m.params.count("maxRotationNorm")) c->maxRotationNorm = (T)to_double(m.params.at("maxRotationNorm"), "maxRotationNorm");
                        if (m.params.count("maxTranslationNorm")) c->maxTranslationNorm = (T)to_double(m.params.at("maxTranslationNorm"), "maxTranslationNorm");
                        transformationCheckers.push_back(c);
                    } else
                        throw std::runtime_error("loadFromYaml: unsupported transformation checker " + m.name);
                }
            else {
                transformationCheckers.push_back(std::make_shared<CounterTransformationChecker>());
                transformationCheckers.push_back(std::make_shared<DifferentialTransformationChecker>());
            }
        }
        //! chain objects -> pgicp_params.  `readingHasNormals`: a SurfaceNormalOutlierFilter only acts when both clouds carry
        //! the `normals` descriptor (else its weights are all ones: it is left out of the device chain for that call)
        void pushParams(bool readingHasNormals = false)
        {
            pgicp_params p;
            pgicp_default_params(&p);
            pgicp_params cur;
            pgicp_get_params(ctx, &cur);
            p.matcher = cur.matcher; p.grid_cell = cur.grid_cell; p.check_every = cur.check_every;
            if (matcher) { p.knn = matcher->knn; p.epsilon = (double)matcher->epsilon; p.max_dist = (double)matcher->maxDist; }
            p.trim_ratio = 1.0;                    // no TrimmedDist filter in the chain: every finite pair passes it
            p.outlier_max_dist = 0.0;
            const VarTrimmedDistOutlierFilter *vt = nullptr;
            const RobustOutlierFilter *rx = nullptr;
            for (auto &f : outlierFilters) {
                if (auto v = std::dynamic_pointer_cast<VarTrimmedDistOutlierFilter>(f)) vt = v.get();
                if (auto t = std::dynamic_pointer_cast<TrimmedDistOutlierFilter>(f)) { p.trim_ratio = (double)t->ratio; p.quantile_scale = 1.0; }
                if (auto md = std::dynamic_pointer_cast<MedianDistOutlierFilter>(f)) { p.trim_ratio = 0.5; p.quantile_scale = (double)md->factor; }
                if (auto m = std::dynamic_pointer_cast<MaxDistOutlierFilter>(f)) p.outlier_max_dist = (double)m->maxDist;
                if (auto rb = std::dynamic_pointer_cast<RobustOutlierFilter>(f)) {
                    if (p.robust_fct != PGICP_ROBUST_NONE) throw std::runtime_error("ICP chain: more than one RobustOutlierFilter");
                    // (berg is not a value of pgicp_params.robust_scale: it travels through pgicp_set_robust_ext below)
                    p.robust_fct = rb->fctCode(); p.robust_scale = rb->scaleCode() == PGICP_ROBUST_SCALE_BERG ? PGICP_ROBUST_SCALE_MAD : rb->scaleCode();
                    p.robust_tuning = (double)rb->tuning;
                    rx = rb.get();
                    p.robust_approx = std::isfinite((double)rb->approximation) ? (double)rb->approximation : 0.0;
                }
            }
            if (errorMinimizer) {
                p.sensor_std_dev = (double)errorMinimizer->sensorStdDev;
                p.error_minimizer = errorMinimizer->pointToPoint ? (errorMinimizer->withCov ? PGICP_MINIMIZER_POINT_TO_POINT_WITH_COV : PGICP_MINIMIZER_POINT_TO_POINT)
                                    : errorMinimizer->force4DOF ? PGICP_MINIMIZER_POINT_TO_PLANE_4DOF : PGICP_MINIMIZER_POINT_TO_PLANE;
            }
            for (auto &f : outlierFilters)
                if (auto sn = std::dynamic_pointer_cast<SurfaceNormalOutlierFilter>(f))
                    p.normal_max_angle = readingHasNormals ? (double)sn->maxAngle : 0.0;
            bool hasCounter = false, hasDiff = false;
            for (auto &c : transformationCheckers) {
                if (auto bc = std::dynamic_pointer_cast<BoundTransformationChecker>(c)) {
                    p.bound_max_rot = (double)bc->maxRotationNorm; p.bound_max_trans = (double)bc->maxTranslationNorm;
                }
                if (auto cc = std::dynamic_pointer_cast<CounterTransformationChecker>(c)) { p.max_iters = cc->maxIterationCount; hasCounter = true; }
                if (auto dc = std::dynamic_pointer_cast<DifferentialTransformationChecker>(c)) {
                    p.min_diff_rot = (double)dc->minDiffRotErr; p.min_diff_trans = (double)dc->minDiffTransErr; p.smooth_length = dc->smoothLength; hasDiff = true;
                }
            }
            if (!hasCounter) p.max_iters = 1 << 20;
            if (!hasDiff) { p.min_diff_rot = 0; p.min_diff_trans = 0; }
            check(ctx, pgicp_set_params(ctx, &p));
            if (vt) { const double q[3] = {(double)vt->minRatio, (double)vt->maxRatio, (double)vt->lambda}; check(ctx, pgicp_set_var_trim(ctx, q)); }
            else check(ctx, pgicp_set_var_trim(ctx, nullptr));
            // RobustOutlierFilter's distanceType / berg / nbIterationForScale (pgicp_robust.h); a chain without such settings: off
            if (rx && !rx->asksNothing()) { const pgicp_robust_ext x = rx->ext(); check(ctx, pgicp_set_robust_ext(ctx, &x)); }
            else check(ctx, pgicp_set_robust_ext(ctx, nullptr));
            if (const GenericDescriptorOutlierFilter *gd = descriptorFilter()) check(ctx, pgicp_set_descriptor_filter(ctx, gd->mode(), (double)gd->threshold));
            else check(ctx, pgicp_set_descriptor_filter(ctx, PGICP_DESC_FILTER_OFF, 0.0));
        }
        //! LoopCloser.hpp:317
        bool getMaxNumIterationsReached() const { return lastStats.max_iter_reached != 0; }
        unsigned getPrefilteredReadingPtsCount() const { return prefilteredReadingPtsCount; }
        unsigned getPrefilteredReferencePtsCount() const { return prefilteredReferencePtsCount; }

    protected:
        unsigned prefilteredReadingPtsCount = 0, prefilteredReferencePtsCount = 0;
        void storeStats(const pgicp_stats &s)
        {
            lastStats = s;
            errorMinimizer->lastOverlap = (T)s.overlap;
            errorMinimizer->lastRatio = (T)s.overlap;
            errorMinimizer->lastResidual = (T)s.residual;
            Matrix cov(6, 6);
            for (int i = 0; i < 6; i++) for (int j = 0; j < 6; j++) cov(i, j) = (T)s.cov[i * 6 + j];
            errorMinimizer->lastCov = cov;
        }
    public:
        //! does getOverlap() of this chain take the sensor-noise branch for `reading`? (upstream: the reading carries
        //! `simpleSensorNoise` -- and `normals` when the minimizer is point-to-plane)
        bool sensorNoiseApplies(const DataPoints &reading) const
        {
            return errorMinimizer && reading.descriptorExists("simpleSensorNoise") && (errorMinimizer->pointToPoint || reading.descriptorExists("normals"));
        }
    protected:
        //! getOverlap()'s sensor-noise branch (pgicp_noise.h): the reading's `simpleSensorNoise` row is handed to the NEXT align call
        //! of the context (pgicp_arm_reading_noise: copied inside the call, so the host cloud is read here, BEFORE the align is
        //! started, and never while it runs); the device then forms the share of the last error elements below mean + noise(point)
        //! with the chain's own combined weights -- Robust, SurfaceNormal and GenericDescriptor filters included.  Returns whether
        //! the branch applies (and the call is armed).
        bool armSensorNoise(const DataPoints &reading) const
        {
            if (!sensorNoiseApplies(reading)) return false;
            const T *row = reading.descriptors.data() + reading.getDescriptorStartingRow("simpleSensorNoise");
            const int stride = (int)reading.descriptors.rows(), n = (int)reading.getNbPoints();
            check(ctx, A::arm_noise(ctx, 1, &row, &stride, &n));
            return true;
        }
        //! ... and the result for problem `problem` of the armed align call that has just returned
        T sensorNoiseOverlap(int problem) const
        {
            double overlap = 0.0;
            int nb = 0;
            check(ctx, pgicp_last_noise_overlap(ctx, problem, &overlap, &nb));
            if (nb == 0) throw ConvergenceError("PointToPlaneErrorMinimizer: no element to minimize");
            return (T)overlap;
        }
    public:
        //! A reading whose filtered copy is on its way to (or already in) device memory: pgicp_upload_* started the
        //! transfer on the context's COPY stream and returned at once.  Not part of libpointmatcher; it is how a caller
        //! that already holds the next scan (LocalizerMT.hpp:27-40: it is queued while the current one aligns) lets the
        //! transfer overlap the running ICP.  Valid until the second-next uploadReading() on the same chain.
        struct DeviceReading {
            const T *dev = nullptr;
            std::shared_ptr<DataPoints> filtered;         // the host copy after the chain's reading filters (what was uploaded)
            //! points and stride of the device copy when they are known without looking at `filtered` (-1: ask it) -- a host copy whose
            //! gaps are still being closed on another thread must not be read (Localizer's deferred host compaction)
            int n = -1, stride = -1;
            int points() const { return n >= 0 ? n : (int)filtered->getNbPoints(); }
            int xyzStride() const { return stride >= 0 ? stride : filtered->xyzStride(); }
            explicit operator bool() const { return dev != nullptr; }
        };
        //! a device copy of a cloud may stand for the cloud itself in operator(): the chain's reading filters change nothing
        //! and no outlier filter looks at the reading's descriptors
        //! a RobustOutlierFilter with distanceType point2plane reads the reference's normals, whatever the minimiser
        bool robustNeedsNormals() const
        {
            for (auto &f : outlierFilters)
                if (auto rb = std::dynamic_pointer_cast<RobustOutlierFilter>(f)) if (rb->distCode() == PGICP_ROBUST_DIST_POINT2PLANE) return true;
            return false;
        }
        static void robustNormalsMissing() { throw typename DataPoints::InvalidField("RobustOutlierFilter: Error, cannot find normals in descriptors (distanceType point2plane)."); }
        //! the chain's GenericDescriptorOutlierFilter, or null
        const GenericDescriptorOutlierFilter *descriptorFilter() const
        {
            for (auto &f : outlierFilters) if (auto g = std::dynamic_pointer_cast<GenericDescriptorOutlierFilter>(f)) return g.get();
            return nullptr;
        }
        //! its descName ("" without the filter): the row a local map built for this chain must carry (BuildLocalMapCloud)
        std::string descriptorName() const { const GenericDescriptorOutlierFilter *g = descriptorFilter(); return g ? g->descName : std::string(); }
        //! the map `mapId` made from `ref` gets the filter's row of it (pgicp_map_set_values, a view of the column-major matrix:
        //! stride = rows); throws when the row is missing or is not one row.  Nothing without the filter.
        void setMapValues(const DataPoints &ref, int mapId)
        {
            const GenericDescriptorOutlierFilter *gd = descriptorFilter();
            if (!gd || ref.getNbPoints() == 0) return;
            const int r = gd->row(ref);
            check(ctx, A::set_values(ctx, mapId, ref.descriptors.data() + r, (int)ref.descriptors.rows()));
        }
        bool hasNormalFilter() const
        {
            for (auto &f : outlierFilters) if (std::dynamic_pointer_cast<SurfaceNormalOutlierFilter>(f)) return true;
            return false;
        }
        bool deviceReadingEquivalent() const
        {
            return !hasNormalFilter() && readingDataPointsFilters.allIdentity() && readingStepDataPointsFilters.allIdentity();
        }
        DeviceReading uploadReading(const DataPoints &readingIn)
        {
            DeviceReading r;
            r.filtered = std::make_shared<DataPoints>(readingIn);
            readingDataPointsFilters.init();
            readingDataPointsFilters.apply(*r.filtered);
            readingStepDataPointsFilters.init();
            readingStepDataPointsFilters.apply(*r.filtered);          // (applied once: see alignOnMap)
            check(ctx, A::upload(ctx, r.filtered->xyzPtr(), r.filtered->xyzStride(), (int)r.filtered->getNbPoints(), &r.dev));
            return r;
        }
    protected:
        TransformationParameters alignOnMap(const DeviceReading &r, const TransformationParameters &T_init)
        {
            // a device reading is coordinates only: a chain whose SurfaceNormalOutlierFilter compares the READING's normals must be
            // given the host cloud (refused, never run without the filter -- ADVICE round 4)
            if (hasNormalFilter() && r.filtered && r.filtered->normalsPtr() != nullptr)
                throw std::logic_error("ICP: a SurfaceNormalOutlierFilter needs the reading's normals; pass the host cloud, not a device reading");
            matcher->refuseDeviceReading();
            prefilteredReadingPtsCount = (unsigned)r.points();
            double Ti[16], To[16];
            pgslam_amd::to_row_major16(T_init, Ti);
            pgicp_stats st;
            pushParams();
            // a host copy whose gaps may still be closing (r.n >= 0) has no row that may be read: such a reading cannot take the
            // sensor-noise branch and is refused (only the labels are looked at, which the compaction leaves alone); the facade
            // does not defer the compaction of a cloud that carries `simpleSensorNoise`, GraphLocalizer::PreProcessOn
            if (r.n >= 0 && r.filtered && sensorNoiseApplies(*r.filtered))
                throw std::logic_error("ICP: a deferred device reading carries simpleSensorNoise; finish its host compaction and pass it with n = -1");
            const bool noisy = r.n < 0 && r.filtered && armSensorNoise(*r.filtered);
            // (the call makes its stream wait, on the device, for the upload; the host does not)
            const int rc = A::align_dev(ctx, matcher->mapId, r.dev, r.xyzStride(), r.points(), Ti, To, &st);
            storeStats(st);
            check(ctx, rc);
            if (noisy) errorMinimizer->lastOverlap = sensorNoiseOverlap(0);
            const TransformationParameters T_out = pgslam_amd::from_row_major16<T>(To);
            if (onAlign && (currentReference || lazyReference) && (!onAlignWanted || onAlignWanted()))
                if (const DataPoints *ref = observedReference()) onAlign(*r.filtered, *ref, T_init, T_out, st);
            return T_out;
        }
        TransformationParameters alignOnMap(const DataPoints &readingIn, const TransformationParameters &T_init)
        {
            DataPoints reading(readingIn);
            readingDataPointsFilters.init();
            readingDataPointsFilters.apply(reading);
            prefilteredReadingPtsCount = reading.getNbPoints();
            // [EXT] readingStepDataPointsFilters (Localizer.hpp:325-326) act on the filtered reading in ITS OWN frame at every
            // iteration, before the iteration's transform is applied; every filter restated here is a pure function of the
            // cloud, so the step filters give the same cloud in every iteration: they are applied once, here (the random
            // sampler, whose upstream version draws a new sample per iteration, is refused in this slot by loadFromYaml)
            readingStepDataPointsFilters.init();
            readingStepDataPointsFilters.apply(reading);
            double Ti[16], To[16];
            pgslam_amd::to_row_major16(T_init, Ti);
            pgicp_stats st;
            std::memset(&st, 0, sizeof st);
            bool normalFilter = false;
            for (auto &f : outlierFilters) normalFilter = normalFilter || std::dynamic_pointer_cast<SurfaceNormalOutlierFilter>(f) != nullptr;
            const bool withNormals = normalFilter && reading.normalsPtr() != nullptr;
            matcher->takeRadii(reading);
            pushParams(withNormals);
            matcher->armRadii(reading);
            const bool noisy = armSensorNoise(reading);
            const int rc = withNormals ? A::align_nrm(ctx, matcher->mapId, reading.xyzPtr(), reading.xyzStride(), (int)reading.getNbPoints(),
                                                      reading.normalsPtr(), reading.normalsStride(), Ti, To, &st)
                                       : A::align(ctx, matcher->mapId, reading.xyzPtr(), reading.xyzStride(), (int)reading.getNbPoints(), Ti, To, &st);
            storeStats(st);
            check(ctx, rc);
            if (noisy) errorMinimizer->lastOverlap = sensorNoiseOverlap(0);
            const TransformationParameters T_out = pgslam_amd::from_row_major16<T>(To);
            if (onAlign && (currentReference || lazyReference) && (!onAlignWanted || onAlignWanted()))
                if (const DataPoints *ref = observedReference()) onAlign(reading, *ref, T_init, T_out, st);
            return T_out;
        }
    };

    struct ICP : ICPChainBase {
        explicit ICP(int device = 0) : ICPChainBase(device) {}
        TransformationParameters operator()(const DataPoints &readingIn, const DataPoints &referenceIn) { return (*this)(readingIn, referenceIn, Matrix::Identity(4, 4)); }
        //! LoopCloser.hpp:98 -- reference filters, mean-centring, index build, loop
        TransformationParameters operator()(const DataPoints &readingIn, const DataPoints &referenceIn, const TransformationParameters &initialTransformationParameters)
        {
            return compute(readingIn, referenceIn, initialTransformationParameters);
        }
        TransformationParameters compute(const DataPoints &readingIn, const DataPoints &referenceIn, const TransformationParameters &T_init)
        {
            DataPoints reference(referenceIn);
            this->referenceDataPointsFilters.init();
            this->referenceDataPointsFilters.apply(reference);
            this->prefilteredReferencePtsCount = reference.getNbPoints();
            if (!reference.descriptorExists("normals") && this->robustNeedsNormals()) this->robustNormalsMissing();
            if (!reference.descriptorExists("normals") && !(this->errorMinimizer && this->errorMinimizer->pointToPoint && !this->errorMinimizer->withCov))
                throw std::runtime_error("PointToPlaneErrorMinimizer: the reference has no 'normals' descriptor");
            this->matcher->initImpl(reference, 1);
            this->currentReference = &reference;
            struct Reset { const DataPoints *&p; ~Reset() { p = nullptr; } } reset{this->currentReference};
            return this->alignOnMap(readingIn, T_init);
        }
        //! ICP::operator() for clouds that are in device memory already: mean-centring + index build of `reference` in place,
        //! the loop on the device copy of the reading (`reading.filtered` = its host cloud: sizes, the observer's copy).  Only for
        //! a chain whose filters change nothing (deviceReadingEquivalent, identity reference filters); `hostReference` makes the
        //! host copy of the reference when an observer asks for it.
        TransformationParameters computeOnDevice(const typename ICPChainBase::DeviceReading &reading, const pgslam_amd::DeviceCloud<T> &reference,
                                                 const TransformationParameters &T_init, std::function<DataPoints()> hostReference)
        {
            if (!this->referenceDataPointsFilters.allIdentity() || !this->deviceReadingEquivalent())
                throw std::logic_error("ICP::computeOnDevice: the chain filters its clouds or reads their descriptors");
            if (!reference.hasNormals() && this->robustNeedsNormals()) this->robustNormalsMissing();
            if (!reference.hasNormals() && !(this->errorMinimizer && this->errorMinimizer->pointToPoint && !this->errorMinimizer->withCov))
                throw std::runtime_error("PointToPlaneErrorMinimizer: the reference has no 'normals' descriptor");
            this->prefilteredReferencePtsCount = reference.n;
            this->matcher->initDevice(reference, 1);
            this->currentReference = nullptr;
            this->lazyReference = hostReference;
            struct Reset { std::function<DataPoints()> &f; const DataPoints *&p; ~Reset() { f = nullptr; p = nullptr; } } reset{this->lazyReference, this->currentReference};
            return this->alignOnMap(reading, T_init);
        }
    };

    struct ICPSequence : ICP {
        explicit ICPSequence(int device = 0) : ICP(device) {}
        bool hasMap() const { return mapPointCloud.getNbPoints() != 0 || mapOnDevice; }
        //! a map that is in device memory already (the localizer assembles it there from resident keyframe clouds) may stand
        //! for setMap(cloud): the chain's reference filters change nothing
        bool deviceMapEquivalent() const { return this->referenceDataPointsFilters.allIdentity() && !this->descriptorFilter(); }
        //! setMap for such a map: mean-centre + index build, no cloud crosses PCIe.  `hostCopy` makes the host cloud if an
        //! observer (onAlign) or getPrefilteredMap() asks for it.
        bool setMap(const pgslam_amd::DeviceCloud<T> &deviceCloud, std::function<DataPoints()> hostCopy)
        {
            if (!deviceMapEquivalent()) throw std::logic_error("ICPSequence::setMap(DeviceCloud): the chain has reference filters");
            if (!deviceCloud.hasNormals() && this->robustNeedsNormals()) this->robustNormalsMissing();
            if (!deviceCloud.hasNormals() && !(this->errorMinimizer && this->errorMinimizer->pointToPoint && !this->errorMinimizer->withCov))
                throw std::runtime_error("PointToPlaneErrorMinimizer: the map has no 'normals' descriptor");
            mapPointCloud = DataPoints();
            this->prefilteredReferencePtsCount = deviceCloud.n;
            this->matcher->initDevice(deviceCloud, 1);
            mapOnDevice = true;
            this->currentReference = nullptr;
            this->lazyReference = hostCopy;
            return true;
        }
        //! Localizer.hpp:148,168,254 -- copy, reference filters, mean-centre, build the index; stays resident in HBM
        bool setMap(const DataPoints &inputCloud)
        {
            mapPointCloud = inputCloud;
            this->referenceDataPointsFilters.init();
            this->referenceDataPointsFilters.apply(mapPointCloud);
            this->prefilteredReferencePtsCount = mapPointCloud.getNbPoints();
            if (!mapPointCloud.descriptorExists("normals") && this->robustNeedsNormals()) this->robustNormalsMissing();
            if (!mapPointCloud.descriptorExists("normals") && !(this->errorMinimizer && this->errorMinimizer->pointToPoint && !this->errorMinimizer->withCov))
                throw std::runtime_error("PointToPlaneErrorMinimizer: the map has no 'normals' descriptor");
            this->matcher->initImpl(mapPointCloud, 1);
            this->currentReference = &mapPointCloud;
            this->lazyReference = nullptr;
            mapOnDevice = false;
            return true;
        }
        void clearMap() { mapPointCloud = DataPoints(); this->currentReference = nullptr; this->lazyReference = nullptr; mapOnDevice = false; this->matcher->release(); }
        const DataPoints &getPrefilteredMap()
        {
            if (mapOnDevice) if (const DataPoints *ref = this->observedReference()) return *ref;
            return mapPointCloud;
        }
        TransformationParameters operator()(const DataPoints &cloudIn) { return (*this)(cloudIn, Matrix::Identity(4, 4)); }
        //! Localizer.hpp:126.  Without a map the first cloud becomes the map and identity is returned
        TransformationParameters operator()(const DataPoints &cloudIn, const TransformationParameters &initialTransformationParameters)
        {
            if (!hasMap()) { setMap(cloudIn); return Matrix::Identity(4, 4); }
            return this->alignOnMap(cloudIn, initialTransformationParameters);
        }
        //! the same against a reading whose upload was started earlier (ICPChainBase::uploadReading): needs a map
        TransformationParameters operator()(const typename ICPChainBase::DeviceReading &reading, const TransformationParameters &initialTransformationParameters)
        {
            if (!hasMap()) throw std::runtime_error("ICPSequence: a device reading needs a map (setMap)");
            return this->alignOnMap(reading, initialTransformationParameters);
        }
    private:
        DataPoints mapPointCloud;
        bool mapOnDevice = false;
    };

    // ------------------------------------------------------------------ registrar (PM::get().REG(Transformation).create(...))
    struct TransformationRegistrarT {
        std::shared_ptr<Transformation> create(const std::string &name) const
        {
            if (name == "RigidTransformation") return std::make_shared<RigidTransformation>();
            throw std::runtime_error("Registrar: unknown transformation " + name);
        }
    };
    TransformationRegistrarT TransformationRegistrar;
    static PointMatcher &get() { static PointMatcher pm; return pm; }
};

// libpointmatcher's own spelling (pointmatcher/Registrar.h defines this macro for its users: `PM::get().REG(Transformation)
// .create("RigidTransformation")`, Localizer.hpp:24, LoopCloser.hpp:27): a drop-in header has to provide it, short as it is.
#ifndef REG
#define REG(name) name##Registrar
#endif
