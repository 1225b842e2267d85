// api_covsample.inc -- part of pgicp_api.cpp (one translation unit): pgicp_covariance_sampling_* and
// pgicp_covariance_sampling_framed_* (include/pgicp_covsample.h).  The host steps between the device passes -- the Jacobi, the
// lists' order, the greedy -- are include/pgslam_amd/covsample_host.hpp, which the C++ drop-in's host form shares.

namespace {

namespace cvs = pgslam_amd::covsample;

// frame_in: the framed call (the frame's passes are skipped; no coordinates, normals or descriptors come out)
template <typename T>
int covariance_sampling(pgicp_ctx *c, const char *who, const T *xyz, int stride, const T *nrm, int nstride, int n, int mem, int nb_sample,
                        int torque_norm, const pgicp_cov_frame *frame_in, const T *desc, int drows, T *out_xyz, T *out_nrm, int out_nstride,
                        T *out_desc, int32_t *kept_idx, int *n_out, pgicp_cov_frame *frame_out)
{
    const std::string name(who);
    if (!c || n < 0 || (n > 0 && (!xyz || !nrm)) || stride < 3 || nstride < 3 || (out_nrm && out_nstride < 3) || nb_sample < 1 ||
        torque_norm < 0 || torque_norm > 2 || (mem != PGICP_HOST && mem != PGICP_DEVICE) || !n_out || (desc && (drows <= 0 || !out_desc)) ||
        6LL * n + 2 > 0x7FFFFFFFLL)
        return fail(c, PGICP_ERR_ARG, name + ": bad argument (n >= 0, nb_sample >= 1, torque_norm 0 .. 2, strides >= 3, out_desc with desc)");
    if (frame_in) {
        bool ok = frame_in->L > 0 && std::isfinite((T)frame_in->L) && (T)frame_in->L > (T)0;
        for (double x : frame_in->center) ok = ok && std::isfinite((T)x);
        for (double x : frame_in->basis) ok = ok && std::isfinite((T)x);
        if (!ok) return fail(c, PGICP_ERR_ARG, name + ": the frame's L is not > 0, or a value of the frame is not finite in T");
    }
    *n_out = 0;
    if (frame_out) *frame_out = pgicp_cov_frame{};
    if (n == 0) return PGICP_OK;
    HIPC(c, hipSetDevice(c->device));
    UploadUse uu(c);
    const int dr = desc ? drows : 0;
    const bool noop = nb_sample >= n;
    const int m = noop ? n : nb_sample;
    CovScratch w;
    XFER(c, carve_buf(c, c->dpf_work, [&](Carve &cv) { w = cov_scratch<T>(cv, n, m); }));
    HIPC(c, c->dpf_stat.ensure(sizeof(CovStat)));
    CovStat *stat = c->dpf_stat.as<CovStat>();
    CloudIn<T> in;
    const T *d_nrm = nrm;
    T *d_ox = out_xyz, *d_on = out_nrm, *d_od = out_desc;
    int32_t *d_oi = kept_idx;
    int ons = out_nstride;
    if (mem == PGICP_HOST) {
        // io: the cloud, its normals and descriptors as uploaded, then the outputs (coordinates at `stride`, the rest packed)
        XFER(c, carve_buf(c, c->dpf_io, [&](Carve &cv) {
            in.carve(cv, stride, n, dr);
            d_nrm = cv.take<T>((size_t)(n - 1) * nstride + 3);
            d_ox = cv.take<T>((size_t)(m - 1) * stride + 3, out_xyz);
            d_on = cv.take<T>(3 * (size_t)m, out_nrm);
            d_od = cv.take<T>((size_t)dr * m, desc);
            d_oi = cv.take<int32_t>((size_t)m, kept_idx);
        }));
        ons = 3;
        XFER(c, h2d(c, (void *)d_nrm, nrm, sizeof(T) * ((size_t)(n - 1) * nstride + 3)));
    } else
        uu.touch(nrm);
    XFER(c, upload_cloud<T>(c, mem, xyz, stride, n, desc, dr, in));
    const int *d_picks = nullptr;
    if (!noop) {
        HIPC(c, hipMemsetAsync(stat, 0, sizeof(CovStat), c->stream));
        CovStat h;
        pgicp_cov_frame frame;
        if (frame_in) frame = *frame_in;
        else {
            launch_cov_frame<T>(c->stream, in.xyz, stride, d_nrm, nstride, n, torque_norm, w, stat);
            XFER(c, read_back(c, &h, stat, sizeof h));                                  // sync 1: the frame's raw sums
            if (h.r1[3] > 0) return fail(c, PGICP_ERR_ARG, name + ": a coordinate or a normal component is NaN or infinite");
            if (!((T)h.L > (T)0) || !std::isfinite((T)h.L))
                return fail(c, PGICP_ERR_ARG, name + ": L is not > 0 (every point lies at the mean)");
            cvs::finish_frame<T>(h.c, h.L, h.sums, frame);
        }
        const cvs::FrameT<T> Fh(frame);
        CovFrameDev<T> F;
        for (int a = 0; a < 3; a++) F.c[a] = Fh.c[a];
        F.inv = Fh.inv;
        for (int k = 0; k < 36; k++) F.X[k] = Fh.X[k];
        launch_cov_select<T>(c->stream, in.xyz, stride, d_nrm, nstride, n, F, m, w, stat);
        std::vector<int32_t> ci(6 * (size_t)m);
        std::vector<T> cval(36 * (size_t)m);
        XFER(c, d2h(c, ci.data(), w.cand_idx, sizeof(int32_t) * ci.size()));
        XFER(c, d2h(c, cval.data(), w.cand_v, sizeof(T) * cval.size()));
        XFER(c, read_back(c, &h, stat, sizeof h));                                      // sync 2: six lists of m candidates
        if (h.bad) return fail(c, PGICP_ERR_ARG, name + ": a coordinate or a normal component is NaN or infinite");
        std::vector<cvs::Cand<T>> lists[6];
        for (int k = 0; k < 6; k++) {
            if (h.cursor[k] != m) return fail(c, PGICP_ERR_HIP, name + ": internal error: a list's selection is not nb_sample long");
            lists[k].resize((size_t)m);
            for (int s = 0; s < m; s++) {
                cvs::Cand<T> &cd = lists[k][(size_t)s];
                const size_t o = (size_t)k * m + s;
                cd.idx = ci[o];
                for (int q = 0; q < 6; q++) cd.v[q] = cval[o * 6 + q];
            }
            cvs::sort_list<T>(lists[k], k);
        }
        std::vector<int32_t> picks;
        cvs::greedy<T>(lists, m, picks);
        if ((int)picks.size() != m) return fail(c, PGICP_ERR_HIP, name + ": internal error: the greedy ran out of candidates");
        XFER(c, h2d(c, w.picks, picks.data(), sizeof(int32_t) * (size_t)m));
        d_picks = w.picks;
        if (frame_out) *frame_out = frame;
    }
    launch_gather_rows<T>(c->stream, d_picks, nullptr, nullptr, m, n, in.xyz, stride, d_nrm, nstride, in.desc, dr, d_ox, stride, d_on, ons, d_od, d_oi, nullptr);
    if (mem == PGICP_HOST) {
        RowSpread<T> late;
        XFER(c, fetch_rows3<T>(c, out_xyz, stride, d_ox, m, late, stride));
        XFER(c, fetch_rows3<T>(c, out_nrm, out_nstride, d_on, m, late));
        if (desc) XFER(c, d2h(c, out_desc, d_od, sizeof(T) * (size_t)dr * m));
        if (kept_idx) XFER(c, d2h(c, kept_idx, d_oi, sizeof(int32_t) * (size_t)m));
        XFER(c, late.land(c));
    } else
        HIPC(c, stream_sync(c));
    HIPC(c, hipGetLastError());
    *n_out = m;
    return PGICP_OK;
}

}  // namespace

extern "C" {

int pgicp_covariance_sampling_f32(pgicp_ctx *ctx, const float *xyz, int stride, const float *nrm, int nstride, int n, int mem, int nb_sample,
                                  int torque_norm, const float *desc, int drows, float *out_xyz, float *out_nrm, int out_nstride, float *out_desc,
                                  int32_t *kept_idx, int *n_out, pgicp_cov_frame *frame_out)
{
    return covariance_sampling<float>(ctx, "pgicp_covariance_sampling", xyz, stride, nrm, nstride, n, mem, nb_sample, torque_norm, nullptr, desc, drows,
                                      out_xyz, out_nrm, out_nstride, out_desc, kept_idx, n_out, frame_out);
}
int pgicp_covariance_sampling_f64(pgicp_ctx *ctx, const double *xyz, int stride, const double *nrm, int nstride, int n, int mem, int nb_sample,
                                  int torque_norm, const double *desc, int drows, double *out_xyz, double *out_nrm, int out_nstride,
                                  double *out_desc, int32_t *kept_idx, int *n_out, pgicp_cov_frame *frame_out)
{
    return covariance_sampling<double>(ctx, "pgicp_covariance_sampling", xyz, stride, nrm, nstride, n, mem, nb_sample, torque_norm, nullptr, desc, drows,
                                       out_xyz, out_nrm, out_nstride, out_desc, kept_idx, n_out, frame_out);
}
int pgicp_covariance_sampling_framed_f32(pgicp_ctx *ctx, const float *xyz, int stride, const float *nrm, int nstride, int n, int mem, int nb_sample,
                                         const pgicp_cov_frame *frame, int32_t *kept_idx, int *n_out)
{
    if (!frame) return fail(ctx, PGICP_ERR_ARG, "pgicp_covariance_sampling_framed: no frame");
    return covariance_sampling<float>(ctx, "pgicp_covariance_sampling_framed", xyz, stride, nrm, nstride, n, mem, nb_sample, 0, frame, nullptr, 0,
                                      nullptr, nullptr, 3, nullptr, kept_idx, n_out, nullptr);
}
int pgicp_covariance_sampling_framed_f64(pgicp_ctx *ctx, const double *xyz, int stride, const double *nrm, int nstride, int n, int mem, int nb_sample,
                                         const pgicp_cov_frame *frame, int32_t *kept_idx, int *n_out)
{
    if (!frame) return fail(ctx, PGICP_ERR_ARG, "pgicp_covariance_sampling_framed: no frame");
    return covariance_sampling<double>(ctx, "pgicp_covariance_sampling_framed", xyz, stride, nrm, nstride, n, mem, nb_sample, 0, frame, nullptr, 0,
                                       nullptr, nullptr, 3, nullptr, kept_idx, n_out, nullptr);
}

}  // extern "C"
