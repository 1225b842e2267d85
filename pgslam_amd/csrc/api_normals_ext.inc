// api_normals_ext.inc -- part of pgicp_api.cpp (one translation unit): pgicp_surface_normals_ext_*, pgicp_smooth_normals_*
// (include/pgicp_normals_ext.h).

namespace {

template <typename T>
int surface_normals_ext(pgicp_ctx *c, const T *xyz, int stride, int n, int mem, int knn, double max_dist, int smooth, T *out_nrm, int out_stride,
                        T *out_eig, T *out_eigvec, T *out_mean_dist, T *out_matched, int32_t *out_ids, T *out_d2, T *out_dens)
{
    // accepted and refused as the call it stands for: pgicp_surface_densities_* with out_dens, pgicp_surface_normals_* without
    const bool as_dens = out_dens != nullptr;
    if (!c || n < 0 || (n > 0 && !xyz) || stride < 3 || (out_nrm && out_stride < 3) || knn > 32 || !(max_dist > 0) ||
        (mem != PGICP_HOST && mem != PGICP_DEVICE) || (smooth != 0 && smooth != 1) || (smooth && !out_nrm) ||
        (as_dens ? knn < 3 : (knn < 1 || n == 0 || !xyz)))
        return fail(c, PGICP_ERR_ARG, "pgicp_surface_normals_ext: bad argument (1 <= knn <= 32, 3 <= knn and n >= 0 with out_dens, else n >= 1; "
                                      "max_dist > 0, smooth 0 or 1 and only with out_nrm)");
    if (sizeof(T) == 4 && out_matched && n > PGICP_NORMALS_EXT_MAX_IDS_F32)
        return fail(c, PGICP_ERR_ARG, "pgicp_surface_normals_ext_f32: out_matched_ids holds indices as floats: n must not exceed 2^24");
    if (n == 0) return PGICP_OK;
    HIPC(c, hipSetDevice(c->device));
    TempMap<T> tm(c);
    { const int st = map_create<T>(c, xyz, stride, nullptr, 0, n, mem, 0, &tm.id); if (st) return st; }   // uncentred: coordinates stay exact
    State<T> &S = state<T>(c);
    const size_t n1 = (size_t)n, nk = (size_t)n * knn;
    // work: what the smoothing pass reads, in slot order (the raw normals, the points' indices, the neighbours' slots)
    NormalsExtOut<T> x{};
    if (smooth)
        XFER(c, carve_buf(c, c->dpf_work, [&](Carve &cv) {
            x.raw = cv.take<T>(3 * n1);
            x.self = cv.take<int>(n1);
            x.nb = cv.take<int>(nk);
        }));
    T *d_nrm = out_nrm, *d_eig = out_eig, *d_d2 = out_d2, *d_dens = out_dens;
    int32_t *d_ids = out_ids;
    x.eigvec = out_eigvec; x.mean_dist = out_mean_dist; x.matched = out_matched;
    int ds = out_stride;
    if (mem == PGICP_HOST) {
        // io: every requested output, packed
        XFER(c, carve_buf(c, c->dpf_io, [&](Carve &cv) {
            d_nrm = cv.take<T>(3 * n1, out_nrm);
            d_eig = cv.take<T>(3 * n1, out_eig);
            x.eigvec = cv.take<T>(9 * n1, out_eigvec);
            x.mean_dist = cv.take<T>(n1, out_mean_dist);
            x.matched = cv.take<T>(nk, out_matched);
            d_ids = cv.take<int32_t>(nk, out_ids);
            d_d2 = cv.take<T>(nk, out_d2);
            d_dens = cv.take<T>(n1, out_dens);
        }));
        ds = 3;
    }
    {
        ProfScope ps(c, PGICP_PROF_NORMALS, n);
        if (launch_surface_normals_ext<T>(c->stream, S.d_maps.template as<MapDev<T>>(), map_index<T>(c, tm.id), n, knn, (T)max_dist,
                                          std::numeric_limits<T>::epsilon(), smooth ? nullptr : d_nrm, ds, d_eig, d_ids, d_d2, d_dens, x) != 0)
            return fail(c, PGICP_ERR_ARG, "pgicp_surface_normals_ext: knn > 32");
        // the table is the kernel's own (no flag); row s is slot s, its result goes to the point's own index
        if (smooth) launch_smooth_normals<T>(c->stream, x.raw, 3, x.nb, 1, (long long)n, knn, n, x.self, d_nrm, ds, nullptr);
    }
    RowSpread<T> late;
    if (mem == PGICP_HOST) {
        XFER(c, fetch_rows3<T>(c, out_nrm, out_stride, d_nrm, n, late));
        if (out_eig) XFER(c, d2h(c, out_eig, d_eig, sizeof(T) * 3 * n1));
        if (out_eigvec) XFER(c, d2h(c, out_eigvec, x.eigvec, sizeof(T) * 9 * n1));
        if (out_mean_dist) XFER(c, d2h(c, out_mean_dist, x.mean_dist, sizeof(T) * n1));
        if (out_matched) XFER(c, d2h(c, out_matched, x.matched, sizeof(T) * nk));
        if (out_ids) XFER(c, d2h(c, out_ids, d_ids, sizeof(int32_t) * nk));
        if (out_d2) XFER(c, d2h(c, out_d2, d_d2, sizeof(T) * nk));
        if (out_dens) XFER(c, d2h(c, out_dens, d_dens, sizeof(T) * n1));
    }
    XFER(c, late.land(c));
    HIPC(c, hipGetLastError());
    return PGICP_OK;
}

template <typename T>
int smooth_normals(pgicp_ctx *c, const T *nrm, int nstride, const int32_t *ids, int knn, int n, int mem, T *out_nrm, int out_stride)
{
    if (!c || n < 0 || (n > 0 && (!nrm || !ids || !out_nrm)) || nstride < 3 || out_stride < 3 || knn < 1 ||
        (mem != PGICP_HOST && mem != PGICP_DEVICE) || (long long)n * knn > 0x7FFFFFFFLL)
        return fail(c, PGICP_ERR_ARG, "pgicp_smooth_normals: bad argument (n >= 0, knn >= 1, strides >= 3, n * knn < 2^31)");
    if (n == 0) return PGICP_OK;
    HIPC(c, hipSetDevice(c->device));
    UploadUse uu(c);
    const size_t n1 = (size_t)n, nk = (size_t)n * knn, in_vals = (n1 - 1) * nstride + 3;
    HIPC(c, c->dpf_stat.ensure(sizeof(int)));
    int *flag = c->dpf_stat.as<int>();
    const T *d_nrm = nrm;
    const int32_t *d_ids = ids;
    T *d_out = out_nrm;
    int os = out_stride;
    if (mem == PGICP_HOST) {
        T *s_nrm = nullptr;
        int32_t *s_ids = nullptr;
        XFER(c, carve_buf(c, c->dpf_io, [&](Carve &cv) {
            s_nrm = cv.take<T>(in_vals);
            s_ids = cv.take<int32_t>(nk);
            d_out = cv.take<T>(3 * n1);
        }));
        XFER(c, h2d(c, s_nrm, nrm, sizeof(T) * in_vals));
        XFER(c, h2d(c, s_ids, ids, sizeof(int32_t) * nk));
        d_nrm = s_nrm; d_ids = s_ids; os = 3;
    } else {
        uu.touch(nrm);
        uu.touch(ids);
    }
    launch_smooth_normals<T>(c->stream, d_nrm, nstride, d_ids, (long long)knn, 1, knn, n, nullptr, d_out, os, flag);
    int bad = 0;
    XFER(c, read_back(c, &bad, flag, sizeof bad));          // the one sync: the flag
    if (bad) return fail(c, PGICP_ERR_ARG, "pgicp_smooth_normals: an id is outside [-1, n)");
    if (mem == PGICP_HOST) {
        RowSpread<T> late;
        XFER(c, fetch_rows3<T>(c, out_nrm, out_stride, d_out, n, late));
        XFER(c, late.land(c));
    }
    return PGICP_OK;
}

}  // namespace

extern "C" {

int pgicp_surface_normals_ext_f32(pgicp_ctx *ctx, const float *xyz, int stride, int n, int mem, int knn, double max_dist, int smooth,
                                  float *out_nrm, int out_stride, float *out_eig, float *out_eigvec, float *out_mean_dist,
                                  float *out_matched_ids, int32_t *out_ids, float *out_d2, float *out_dens)
{
    return surface_normals_ext<float>(ctx, xyz, stride, n, mem, knn, max_dist, smooth, out_nrm, out_stride, out_eig, out_eigvec, out_mean_dist,
                                      out_matched_ids, out_ids, out_d2, out_dens);
}
int pgicp_surface_normals_ext_f64(pgicp_ctx *ctx, const double *xyz, int stride, int n, int mem, int knn, double max_dist, int smooth,
                                  double *out_nrm, int out_stride, double *out_eig, double *out_eigvec, double *out_mean_dist,
                                  double *out_matched_ids, int32_t *out_ids, double *out_d2, double *out_dens)
{
    return surface_normals_ext<double>(ctx, xyz, stride, n, mem, knn, max_dist, smooth, out_nrm, out_stride, out_eig, out_eigvec, out_mean_dist,
                                       out_matched_ids, out_ids, out_d2, out_dens);
}
int pgicp_smooth_normals_f32(pgicp_ctx *ctx, const float *nrm, int nstride, const int32_t *ids, int knn, int n, int mem, float *out_nrm,
                             int out_stride)
{ return smooth_normals<float>(ctx, nrm, nstride, ids, knn, n, mem, out_nrm, out_stride); }
int pgicp_smooth_normals_f64(pgicp_ctx *ctx, const double *nrm, int nstride, const int32_t *ids, int knn, int n, int mem, double *out_nrm,
                             int out_stride)
{ return smooth_normals<double>(ctx, nrm, nstride, ids, knn, n, mem, out_nrm, out_stride); }

}  // extern "C"
