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
    auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
    // scratch of the build, then (host memory) the inputs' and outputs' device copies
    size_t sz[kSsnArrays];
    const size_t work = sampling_normals_scratch(n, (int)sizeof(T), sz);
    const size_t b_in = up(sizeof(T) * ((size_t)(n - 1) * stride + 3)), b_din = up(sizeof(T) * (size_t)dr * n),
                 b_ox = up(sizeof(T) * 3 * (size_t)n), b_on = up(sizeof(T) * 3 * (size_t)n), b_od = b_din, b_oi = up(sizeof(int) * (size_t)n);
    HIPC(c, c->ssn_work.ensure(work + 256));
    if (mem == PGICP_HOST) HIPC(c, c->ssn_io.ensure(b_in + b_din + b_ox + b_on + b_od + b_oi));
    HIPC(c, c->ssn_cnt.ensure(4 * sizeof(int)));
    SsnScratch w;
    {
        char *p = (char *)c->ssn_work.p;
        void **slots[kSsnArrays] = {&w.keys[0], &w.keys[1], (void **)&w.lst[0], (void **)&w.lst[1], (void **)&w.flag[0], (void **)&w.flag[1],
                                    (void **)&w.scan, (void **)&w.bsum, (void **)&w.seg_of[0], (void **)&w.seg_of[1], (void **)&w.side,
                                    &w.seg[0], &w.seg[1], &w.boxes, (void **)&w.keep, (void **)&w.box_of, &w.bnrm, &w.bmean, (void **)&w.pos};
        for (int k = 0; k < kSsnArrays; k++) { *slots[k] = p; p += sz[k]; }
    }
    const T *d_xyz = xyz, *d_desc = desc;
    int d_stride = stride;
    T *d_ox = out_xyz, *d_on = out_nrm, *d_od = out_desc;
    int32_t *d_oi = kept_idx;
    int os = out_stride, ns = nrm_stride;
    if (mem == PGICP_HOST) {
        char *p = (char *)c->ssn_io.p;
        XFER(c, h2d(c, p, xyz, sizeof(T) * ((size_t)(n - 1) * stride + 3)));
        d_xyz = (const T *)p;
        if (desc) { XFER(c, h2d(c, p + b_in, desc, sizeof(T) * (size_t)dr * n)); d_desc = (const T *)(p + b_in); }
        d_ox = (T *)(p + b_in + b_din);                      // the outputs packed: 3 values a point
        d_on = out_nrm ? (T *)(p + b_in + b_din + b_ox) : nullptr;
        d_od = desc ? (T *)(p + b_in + b_din + b_ox + b_on) : nullptr;
        d_oi = (int32_t *)(p + b_in + b_din + b_ox + b_on + b_od);
        os = 3; ns = 3;
    } else {
        uu.touch(xyz);
        if (desc) uu.touch(desc);
    }
    int *cnt = c->ssn_cnt.as<int>();
    {
        ProfScope ps(c, PGICP_PROF_NORMALS, n);
        if (launch_sampling_normals<T>(c->stream, d_xyz, d_stride, n, knn, method, (T)ratio, (T)max_box_dim, (unsigned long long)seed, d_desc, dr,
                                       average ? 1 : 0, w, d_ox, os, d_on, ns, d_od, d_oi, cnt) != 0)
            return fail(c, PGICP_ERR_ARG, "pgicp_sampling_surface_normal: n out of range");
    }
    int h[4] = {0, 0, 0, 0};
    XFER(c, d2h(c, h, cnt, sizeof h));
    HIPC(c, stream_sync(c));
    HIPC(c, hipGetLastError());
    // (a NaN makes the comparison of the statement no strict weak order; an infinity makes a carried side inf - inf: refused,
    // and the outputs are void)
    if (h[2]) return fail(c, PGICP_ERR_ARG, "pgicp_sampling_surface_normal: a coordinate is NaN or infinite");
    const int kept = h[3];
    if (mem == PGICP_HOST && kept > 0) {
        std::vector<T> tx, tn;
        T *hx = out_xyz, *hn = out_nrm;
        if (out_stride != 3) { tx.resize(3 * (size_t)kept); hx = tx.data(); }
        if (out_nrm && nrm_stride != 3) { tn.resize(3 * (size_t)kept); hn = tn.data(); }
        XFER(c, d2h(c, hx, d_ox, sizeof(T) * 3 * (size_t)kept));
        if (out_nrm) XFER(c, d2h(c, hn, d_on, sizeof(T) * 3 * (size_t)kept));
        if (desc) XFER(c, d2h(c, out_desc, d_od, sizeof(T) * (size_t)dr * kept));
        if (kept_idx) XFER(c, d2h(c, kept_idx, d_oi, sizeof(int32_t) * (size_t)kept));
        HIPC(c, stream_sync(c));
        for (size_t k = 0; k < tx.size() / 3; k++) std::memcpy(out_xyz + k * out_stride, hx + 3 * k, 3 * sizeof(T));
        for (size_t k = 0; k < tn.size() / 3; k++) std::memcpy(out_nrm + k * nrm_stride, hn + 3 * k, 3 * sizeof(T));
    }
    *n_out = kept;
    if (n_boxes) *n_boxes = h[1];
    return PGICP_OK;
}
