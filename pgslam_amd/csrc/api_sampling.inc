// api_sampling.inc -- part of pgicp_api.cpp (one translation unit): pgicp_sampling_surface_normal_* (SamplingSurfaceNormalDataPointsFilter).
template <typename T>
int sampling_surface_normal(pgicp_ctx *c, const T *xyz, int stride, int n, int mem, int knn, double ratio, int method, double max_box_dim,
                            uint64_t seed, const T *desc, int drows, int average, T *out_xyz, int out_stride, T *out_nrm, int nrm_stride,
                            T *out_desc, int32_t *kept_idx, int *n_out, int *n_boxes)
{
    if (!c || n < 0 || (n > 0 && !xyz) || stride < 3 || knn < 3 || knn > kSsnMaxKnn || (method != 0 && method != 1) ||
        (mem != PGICP_HOST && mem != PGICP_DEVICE) || !n_out || (n > 0 && !out_xyz) || out_stride < 3 ||
        (out_nrm && nrm_stride < 3) || (desc && (drows <= 0 || !out_desc)) || 3LL * n + 1 > 0x7FFFFFFFLL)
        return fail(c, PGICP_ERR_ARG, "pgicp_sampling_surface_normal: bad argument (3 <= knn <= 1024, sampling_method 0 or 1)");
    *n_out = 0;
    if (n_boxes) *n_boxes = 0;
    if (n == 0) return PGICP_OK;
    HIPC(c, hipSetDevice(c->device));
    UploadUse uu(c);
    const int dr = desc ? drows : 0;
    // scratch of the build, then (host memory) the inputs' device copies and the outputs packed: 3 values a point
    SsnScratch w;
    XFER(c, carve_buf(c, c->dpf_work, [&](Carve &cv) { w = ssn_scratch<T>(cv, n); }));
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
        }));
        os = 3; ns = 3;
    }
    XFER(c, upload_cloud<T>(c, mem, xyz, stride, n, desc, dr, in));
    int *cnt = c->dpf_stat.as<int>();
    {
        ProfScope ps(c, PGICP_PROF_NORMALS, n);
        if (launch_sampling_normals<T>(c->stream, in.xyz, stride, n, knn, method, (T)ratio, (T)max_box_dim, (unsigned long long)seed, in.desc, dr,
                                       average ? 1 : 0, w, d_ox, os, d_on, ns, d_od, d_oi, cnt) != 0)
            return fail(c, PGICP_ERR_ARG, "pgicp_sampling_surface_normal: n out of range");
    }
    int h[4] = {0, 0, 0, 0};
    XFER(c, read_back(c, h, cnt, sizeof h));
    // (a NaN makes the comparison of the statement no strict weak order; an infinity makes a carried side inf - inf: refused,
    // and the outputs are void)
    if (h[2]) return fail(c, PGICP_ERR_ARG, "pgicp_sampling_surface_normal: a coordinate is NaN or infinite");
    const int kept = h[3];
    if (mem == PGICP_HOST && kept > 0) {
        RowSpread<T> late;
        XFER(c, fetch_rows3<T>(c, out_xyz, out_stride, d_ox, kept, late));
        XFER(c, fetch_rows3<T>(c, out_nrm, nrm_stride, d_on, kept, late));
        if (desc) XFER(c, d2h(c, out_desc, d_od, sizeof(T) * (size_t)dr * kept));
        if (kept_idx) XFER(c, d2h(c, kept_idx, d_oi, sizeof(int32_t) * (size_t)kept));
        XFER(c, late.land(c));
    }
    *n_out = kept;
    if (n_boxes) *n_boxes = h[1];
    return PGICP_OK;
}
