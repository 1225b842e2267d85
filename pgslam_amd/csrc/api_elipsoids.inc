// api_elipsoids.inc -- part of pgicp_api.cpp (one translation unit): pgicp_elipsoids_* (include/pgicp_elipsoids.h).
// sampling_surface_normal_ext (api_ssn_ext.inc) with the planarity drop and four more outputs; the older entries' paths are not touched.

namespace {

template <typename T>
int elipsoids(pgicp_ctx *c, const T *xyz, int stride, int n, int mem, int knn, double ratio, int method, double max_box_dim, uint64_t seed,
              const T *desc, int drows, int average, T *out_xyz, int out_stride, T *out_nrm, int nrm_stride, T *out_desc, int32_t *kept_idx,
              int *n_out, int *n_boxes, T *out_eig, T *out_eigvec, T *out_dens, double min_planarity, T *out_cov, T *out_weights, T *out_means,
              T *out_shapes)
{
    // accepted and refused as pgicp_sampling_surface_normal_*; min_planarity finite and in [0, 1]
    if (!c || n < 0 || (n > 0 && !xyz) || stride < 3 || knn < 3 || knn > kSsnMaxKnn || (method != 0 && method != 1) ||
        (mem != PGICP_HOST && mem != PGICP_DEVICE) || !n_out || (n > 0 && !out_xyz) || out_stride < 3 ||
        (out_nrm && nrm_stride < 3) || (desc && (drows <= 0 || !out_desc)) || 3LL * n + 1 > 0x7FFFFFFFLL ||
        !pgslam_amd::elipsoids::min_planarity_ok(min_planarity))
        return fail(c, PGICP_ERR_ARG, "pgicp_elipsoids: bad argument (3 <= knn <= 1024, sampling_method 0 or 1, min_planarity in [0, 1])");
    *n_out = 0;
    if (n_boxes) *n_boxes = 0;
    if (n == 0) return PGICP_OK;
    HIPC(c, hipSetDevice(c->device));
    UploadUse uu(c);
    const int dr = desc ? drows : 0;
    ElipOut<T> x{};
    x.eig = out_eig; x.eigvec = out_eigvec; x.dens = out_dens; x.cov = out_cov; x.weights = out_weights; x.means = out_means; x.shapes = out_shapes;
    // scratch of the build and the per-box rows that are asked for, then (host memory) the inputs' device copies and the outputs packed
    SsnScratch w;
    XFER(c, carve_buf(c, c->dpf_work, [&](Carve &cv) { w = ssn_scratch<T>(cv, n); x.box = elip_scratch<T>(cv, n, x); }));
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
            x.eig = cv.take<T>(3 * (size_t)n, out_eig);
            x.eigvec = cv.take<T>(9 * (size_t)n, out_eigvec);
            x.dens = cv.take<T>((size_t)n, out_dens);
            x.cov = cv.take<T>(9 * (size_t)n, out_cov);
            x.weights = cv.take<T>((size_t)n, out_weights);
            x.means = cv.take<T>(3 * (size_t)n, out_means);
            x.shapes = cv.take<T>(3 * (size_t)n, out_shapes);
        }));
        os = 3; ns = 3;
    }
    XFER(c, upload_cloud<T>(c, mem, xyz, stride, n, desc, dr, in));
    int *cnt = c->dpf_stat.as<int>();
    {
        ProfScope ps(c, PGICP_PROF_NORMALS, n);
        if (launch_elipsoids<T>(c->stream, in.xyz, stride, n, knn, method, (T)ratio, (T)max_box_dim, (T)min_planarity, (unsigned long long)seed, in.desc,
                                dr, average ? 1 : 0, w, d_ox, os, d_on, ns, d_od, d_oi, cnt, x) != 0)
            return fail(c, PGICP_ERR_ARG, "pgicp_elipsoids: n out of range");
    }
    int h[4] = {0, 0, 0, 0};
    XFER(c, read_back(c, h, cnt, sizeof h));
    if (h[2]) return fail(c, PGICP_ERR_ARG, "pgicp_elipsoids: a coordinate is NaN or infinite");
    const int kept = h[3];
    if (mem == PGICP_HOST && kept > 0) {
        RowSpread<T> late;
        XFER(c, fetch_rows3<T>(c, out_xyz, out_stride, d_ox, kept, late));
        XFER(c, fetch_rows3<T>(c, out_nrm, nrm_stride, d_on, kept, late));
        if (desc) XFER(c, d2h(c, out_desc, d_od, sizeof(T) * (size_t)dr * kept));
        if (kept_idx) XFER(c, d2h(c, kept_idx, d_oi, sizeof(int32_t) * (size_t)kept));
        if (out_eig) XFER(c, d2h(c, out_eig, x.eig, sizeof(T) * 3 * (size_t)kept));
        if (out_eigvec) XFER(c, d2h(c, out_eigvec, x.eigvec, sizeof(T) * 9 * (size_t)kept));
        if (out_dens) XFER(c, d2h(c, out_dens, x.dens, sizeof(T) * (size_t)kept));
        if (out_cov) XFER(c, d2h(c, out_cov, x.cov, sizeof(T) * 9 * (size_t)kept));
        if (out_weights) XFER(c, d2h(c, out_weights, x.weights, sizeof(T) * (size_t)kept));
        if (out_means) XFER(c, d2h(c, out_means, x.means, sizeof(T) * 3 * (size_t)kept));
        if (out_shapes) XFER(c, d2h(c, out_shapes, x.shapes, sizeof(T) * 3 * (size_t)kept));
        XFER(c, late.land(c));
    }
    *n_out = kept;
    if (n_boxes) *n_boxes = h[1];
    return PGICP_OK;
}

}  // namespace

extern "C" {

int pgicp_elipsoids_f32(pgicp_ctx *c, const float *xyz, int stride, int n, int mem, int knn, double ratio, int sampling_method, double max_box_dim,
                        uint64_t seed, const float *desc, int drows, int average_descriptors, float *out_xyz, int out_stride, float *out_nrm,
                        int nrm_stride, float *out_desc, int32_t *kept_idx, int *n_out, int *n_boxes, float *out_eig, float *out_eigvec, float *out_dens,
                        double min_planarity, float *out_cov, float *out_weights, float *out_means, float *out_shapes)
{ return elipsoids<float>(c, xyz, stride, n, mem, knn, ratio, sampling_method, max_box_dim, seed, desc, drows, average_descriptors, out_xyz, out_stride,
                          out_nrm, nrm_stride, out_desc, kept_idx, n_out, n_boxes, out_eig, out_eigvec, out_dens, min_planarity, out_cov, out_weights,
                          out_means, out_shapes); }
int pgicp_elipsoids_f64(pgicp_ctx *c, const double *xyz, int stride, int n, int mem, int knn, double ratio, int sampling_method, double max_box_dim,
                        uint64_t seed, const double *desc, int drows, int average_descriptors, double *out_xyz, int out_stride, double *out_nrm,
                        int nrm_stride, double *out_desc, int32_t *kept_idx, int *n_out, int *n_boxes, double *out_eig, double *out_eigvec,
                        double *out_dens, double min_planarity, double *out_cov, double *out_weights, double *out_means, double *out_shapes)
{ return elipsoids<double>(c, xyz, stride, n, mem, knn, ratio, sampling_method, max_box_dim, seed, desc, drows, average_descriptors, out_xyz, out_stride,
                           out_nrm, nrm_stride, out_desc, kept_idx, n_out, n_boxes, out_eig, out_eigvec, out_dens, min_planarity, out_cov, out_weights,
                           out_means, out_shapes); }

}  // extern "C"
