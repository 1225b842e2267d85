// api_box.inc -- part of pgicp_api.cpp (one translation unit): the box filters' three entries, pgicp_sampling_surface_normal_*
// (SamplingSurfaceNormalDataPointsFilter), pgicp_sampling_surface_normal_ext_* (include/pgicp_ssn_ext.h) and pgicp_elipsoids_*
// (include/pgicp_elipsoids.h).  One body: an entry is its name, the per-box rows it offers and whether it has a planarity drop.

namespace {

struct BoxEntry { const char *name; unsigned offered; bool planarity; };
constexpr BoxEntry kSamplingNormals{"pgicp_sampling_surface_normal", 0, false};
constexpr BoxEntry kSamplingNormalsExt{"pgicp_sampling_surface_normal_ext", kBoxRowsExt, false};
constexpr BoxEntry kElipsoids{"pgicp_elipsoids", kBoxRowsAll, true};

// `out`: the caller's pointers of the rows beyond the normals (host or device memory as `mem` says; a null one is not asked for;
// out.box is not read)
template <typename T>
int box_filter(pgicp_ctx *c, const BoxEntry &e, const T *xyz, int stride, int n, int mem, int knn, double ratio, int method, double max_box_dim,
               uint64_t seed, const T *desc, int drows, int average, T *out_xyz, int out_stride, T *out_nrm, int nrm_stride, T *out_desc,
               int32_t *kept_idx, int *n_out, int *n_boxes, double min_planarity, const BoxOut<T> &out)
{
    const std::string name = e.name;
    // min_planarity finite and in [0, 1]
    if (!c || n < 0 || (n > 0 && !xyz) || stride < 3 || knn < 3 || knn > kSsnMaxKnn || (method != 0 && method != 1) ||
        (mem != PGICP_HOST && mem != PGICP_DEVICE) || !n_out || (n > 0 && !out_xyz) || out_stride < 3 ||
        (out_nrm && nrm_stride < 3) || (desc && (drows <= 0 || !out_desc)) || 3LL * n + 1 > 0x7FFFFFFFLL ||
        (e.planarity && !pgslam_amd::elipsoids::min_planarity_ok(min_planarity)))
        return fail(c, PGICP_ERR_ARG, name + ": bad argument (3 <= knn <= 1024, sampling_method 0 or 1" +
                                          (e.planarity ? ", min_planarity in [0, 1])" : ")"));
    *n_out = 0;
    if (n_boxes) *n_boxes = 0;
    if (n == 0) return PGICP_OK;
    HIPC(c, hipSetDevice(c->device));
    UploadUse uu(c);
    const int dr = desc ? drows : 0;
    // x: the rows as the kernels see them (device memory); per offered row its bit, its values a point, where the caller wants it
    BoxOut<T> x = out;
    const struct { unsigned bit; int width; T *host; T **dev; } rows[] = {
        {kBoxEig, 3, out.eig, &x.eig},        {kBoxVec, 9, out.eigvec, &x.eigvec},     {kBoxDens, 1, out.dens, &x.dens},     {kBoxCov, 9, out.cov, &x.cov},
        {kBoxWeight, 1, out.weights, &x.weights}, {kBoxMean, 3, out.means, &x.means}, {kBoxShape, 3, out.shapes, &x.shapes}};
    // scratch of the build and the per-box rows the entry offers, then (host memory) the inputs' device copies and the outputs packed
    SsnScratch w;
    XFER(c, carve_buf(c, c->dpf_work, [&](Carve &cv) { w = ssn_scratch<T>(cv, n); x.box = box_scratch<T>(cv, n, e.offered, out); }));
    HIPC(c, c->dpf_stat.ensure(4 * sizeof(int)));
    CloudIn<T> in;
    T *d_ox = out_xyz, *d_on = out_nrm, *d_od = out_desc;
    int32_t *d_oi = kept_idx;
    int os = out_stride, ns = nrm_stride;
    if (mem == PGICP_HOST) {
        XFER(c, carve_buf(c, c->dpf_io, [&](Carve &cv) {
            in.carve(cv, stride, n, dr);
            d_ox = cv.take<T>(3 * (size_t)n);
            d_on = cv.take<T>(3 * (size_t)n, out_nrm);
            d_od = cv.take<T>((size_t)dr * n, desc);
            d_oi = cv.take<int32_t>((size_t)n);
            for (const auto &r : rows)
                if (e.offered & r.bit) *r.dev = cv.take<T>(r.width * (size_t)n, r.host);
        }));
        os = 3; ns = 3;
    }
    XFER(c, upload_cloud<T>(c, mem, xyz, stride, n, desc, dr, in));
    int *cnt = c->dpf_stat.as<int>();
    {
        ProfScope ps(c, PGICP_PROF_NORMALS, n);
        if (launch_box_filter<T>(c->stream, in.xyz, stride, n, knn, method, (T)ratio, (T)max_box_dim, (T)min_planarity, (unsigned long long)seed, in.desc,
                                 dr, average ? 1 : 0, w, d_ox, os, d_on, ns, d_od, d_oi, cnt, x) != 0)
            return fail(c, PGICP_ERR_ARG, name + ": n out of range");
    }
    int h[4] = {0, 0, 0, 0};
    XFER(c, read_back(c, h, cnt, sizeof h));
    // (a NaN makes the comparison of the statement no strict weak order; an infinity makes a carried side inf - inf: refused,
    // and the outputs are void)
    if (h[2]) return fail(c, PGICP_ERR_ARG, name + ": a coordinate is NaN or infinite");
    const int kept = h[3];
    if (mem == PGICP_HOST && kept > 0) {
        RowSpread<T> late;
        XFER(c, fetch_rows3<T>(c, out_xyz, out_stride, d_ox, kept, late));
        XFER(c, fetch_rows3<T>(c, out_nrm, nrm_stride, d_on, kept, late));
        if (desc) XFER(c, d2h(c, out_desc, d_od, sizeof(T) * (size_t)dr * kept));
        if (kept_idx) XFER(c, d2h(c, kept_idx, d_oi, sizeof(int32_t) * (size_t)kept));
        for (const auto &r : rows)
            if (r.host) XFER(c, d2h(c, r.host, *r.dev, sizeof(T) * r.width * (size_t)kept));
        XFER(c, late.land(c));
    }
    *n_out = kept;
    if (n_boxes) *n_boxes = h[1];
    return PGICP_OK;
}

}  // namespace

extern "C" {

int pgicp_sampling_surface_normal_f32(pgicp_ctx *c, const float *xyz, int stride, int n, int mem, int knn, double ratio, int sampling_method,
                                      double max_box_dim, uint64_t seed, const float *desc, int drows, int average_descriptors, float *out_xyz,
                                      int out_stride, float *out_nrm, int nrm_stride, float *out_desc, int32_t *kept_idx, int *n_out, int *n_boxes)
{ return box_filter<float>(c, kSamplingNormals, xyz, stride, n, mem, knn, ratio, sampling_method, max_box_dim, seed, desc, drows, average_descriptors, out_xyz,
                           out_stride, out_nrm, nrm_stride, out_desc, kept_idx, n_out, n_boxes, 0.0, {}); }
int pgicp_sampling_surface_normal_f64(pgicp_ctx *c, const double *xyz, int stride, int n, int mem, int knn, double ratio, int sampling_method,
                                      double max_box_dim, uint64_t seed, const double *desc, int drows, int average_descriptors, double *out_xyz,
                                      int out_stride, double *out_nrm, int nrm_stride, double *out_desc, int32_t *kept_idx, int *n_out, int *n_boxes)
{ return box_filter<double>(c, kSamplingNormals, xyz, stride, n, mem, knn, ratio, sampling_method, max_box_dim, seed, desc, drows, average_descriptors, out_xyz,
                            out_stride, out_nrm, nrm_stride, out_desc, kept_idx, n_out, n_boxes, 0.0, {}); }

int pgicp_sampling_surface_normal_ext_f32(pgicp_ctx *c, const float *xyz, int stride, int n, int mem, int knn, double ratio, int sampling_method,
                                          double max_box_dim, uint64_t seed, const float *desc, int drows, int average_descriptors, float *out_xyz,
                                          int out_stride, float *out_nrm, int nrm_stride, float *out_desc, int32_t *kept_idx, int *n_out, int *n_boxes,
                                          float *out_eig, float *out_eigvec, float *out_dens)
{ return box_filter<float>(c, kSamplingNormalsExt, xyz, stride, n, mem, knn, ratio, sampling_method, max_box_dim, seed, desc, drows, average_descriptors,
                           out_xyz, out_stride, out_nrm, nrm_stride, out_desc, kept_idx, n_out, n_boxes, 0.0, {out_eig, out_eigvec, out_dens}); }
int pgicp_sampling_surface_normal_ext_f64(pgicp_ctx *c, const double *xyz, int stride, int n, int mem, int knn, double ratio, int sampling_method,
                                          double max_box_dim, uint64_t seed, const double *desc, int drows, int average_descriptors, double *out_xyz,
                                          int out_stride, double *out_nrm, int nrm_stride, double *out_desc, int32_t *kept_idx, int *n_out, int *n_boxes,
                                          double *out_eig, double *out_eigvec, double *out_dens)
{ return box_filter<double>(c, kSamplingNormalsExt, xyz, stride, n, mem, knn, ratio, sampling_method, max_box_dim, seed, desc, drows, average_descriptors,
                            out_xyz, out_stride, out_nrm, nrm_stride, out_desc, kept_idx, n_out, n_boxes, 0.0, {out_eig, out_eigvec, out_dens}); }

int pgicp_elipsoids_f32(pgicp_ctx *c, const float *xyz, int stride, int n, int mem, int knn, double ratio, int sampling_method, double max_box_dim,
                        uint64_t seed, const float *desc, int drows, int average_descriptors, float *out_xyz, int out_stride, float *out_nrm,
                        int nrm_stride, float *out_desc, int32_t *kept_idx, int *n_out, int *n_boxes, float *out_eig, float *out_eigvec, float *out_dens,
                        double min_planarity, float *out_cov, float *out_weights, float *out_means, float *out_shapes)
{ return box_filter<float>(c, kElipsoids, xyz, stride, n, mem, knn, ratio, sampling_method, max_box_dim, seed, desc, drows, average_descriptors, out_xyz,
                           out_stride, out_nrm, nrm_stride, out_desc, kept_idx, n_out, n_boxes, min_planarity,
                           {out_eig, out_eigvec, out_dens, out_cov, out_weights, out_means, out_shapes}); }
int pgicp_elipsoids_f64(pgicp_ctx *c, const double *xyz, int stride, int n, int mem, int knn, double ratio, int sampling_method, double max_box_dim,
                        uint64_t seed, const double *desc, int drows, int average_descriptors, double *out_xyz, int out_stride, double *out_nrm,
                        int nrm_stride, double *out_desc, int32_t *kept_idx, int *n_out, int *n_boxes, double *out_eig, double *out_eigvec,
                        double *out_dens, double min_planarity, double *out_cov, double *out_weights, double *out_means, double *out_shapes)
{ return box_filter<double>(c, kElipsoids, xyz, stride, n, mem, knn, ratio, sampling_method, max_box_dim, seed, desc, drows, average_descriptors, out_xyz,
                            out_stride, out_nrm, nrm_stride, out_desc, kept_idx, n_out, n_boxes, min_planarity,
                            {out_eig, out_eigvec, out_dens, out_cov, out_weights, out_means, out_shapes}); }

}  // extern "C"
