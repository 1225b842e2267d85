// api_quantile.inc -- part of pgicp_api.cpp (one translation unit): pgicp_axis_quantile_* (include/pgicp_quantile.h): the list
// entry's selection (k_axisquantile.inc) over a whole cloud.  The entry itself runs inside launch_filter_cloud; its checks are
// filter_specs' (api_filters_uploads.inc).

namespace {

template <typename T>
int axis_quantile(pgicp_ctx *c, const T *feat, int stride, int n, int mem, int dim, double ratio, T *limit, int *k_out, int *below)
{
    if (!c || n < 0 || (n > 0 && !feat) || stride < 3 || (mem != PGICP_HOST && mem != PGICP_DEVICE) || !axis_quantile_args_ok<T>(dim, ratio))
        return fail(c, PGICP_ERR_ARG, "pgicp_axis_quantile: bad argument (n >= 0, stride >= 3, dim in {0, 1, 2}, ratio finite and in (0, 1) as T)");
    if (limit) *limit = std::numeric_limits<T>::quiet_NaN();
    if (k_out) *k_out = 0;
    if (below) *below = 0;
    if (n == 0) return PGICP_OK;
    HIPC(c, hipSetDevice(c->device));
    UploadUse uu(c);
    HIPC(c, c->dpf_work.ensure(axis_quantile_scratch_bytes(n, sizeof(T))));
    const AqScratch w = axis_quantile_scratch(c->dpf_work.p, n, sizeof(T));
    const T *d_feat = feat;
    if (mem == PGICP_HOST) {
        const size_t vals = (size_t)(n - 1) * stride + 3;
        HIPC(c, c->dpf_io.ensure(sizeof(T) * vals));
        XFER(c, h2d(c, c->dpf_io.p, feat, sizeof(T) * vals));
        d_feat = c->dpf_io.as<T>();
    } else
        uu.touch(feat);
    launch_axis_quantile<T>(c->stream, d_feat, stride, dim, n, nullptr, (T)ratio, w);
    AqResult r;
    XFER(c, read_back(c, &r, w.result, sizeof r));
    if (limit) std::memcpy(limit, &r.limit_bits, sizeof(T));        // (T's bits in the low bytes: little-endian hosts only, as the rest)
    if (k_out) *k_out = r.k;
    if (below) *below = r.below;
    return PGICP_OK;
}

}  // namespace

extern "C" {

int pgicp_axis_quantile_f32(pgicp_ctx *ctx, const float *feat, int stride, int n, int mem, int dim, double ratio, float *limit, int *k_out,
                            int *below)
{
    return axis_quantile<float>(ctx, feat, stride, n, mem, dim, ratio, limit, k_out, below);
}
int pgicp_axis_quantile_f64(pgicp_ctx *ctx, const double *feat, int stride, int n, int mem, int dim, double ratio, double *limit, int *k_out,
                            int *below)
{
    return axis_quantile<double>(ctx, feat, stride, n, mem, dim, ratio, limit, k_out, below);
}

}  // extern "C"
