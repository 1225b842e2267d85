// api_octree.inc -- part of pgicp_api.cpp (one translation unit): pgicp_octree_grid_* (include/pgicp_octree.h).  The root and the
// levels of a path code come from include/pgslam_amd/octree_host.hpp, which the C++ drop-in's host form shares.

namespace {

template <typename T>
int octree_grid(pgicp_ctx *c, const T *xyz, int stride, int n, int mem, int max_pts, double max_size, int method, unsigned long long seed, const T *desc,
                int drows, T *out_xyz, int out_stride, T *out_desc, int32_t *kept_idx, int32_t *out_count, int32_t *out_depth, int *n_out)
{
    const T ms = (T)max_size;
    if (!c || n < 0 || (n > 0 && !xyz) || stride < 3 || (mem != PGICP_HOST && mem != PGICP_DEVICE) || !n_out || (out_xyz && out_stride < 3) ||
        (desc && (drows <= 0 || !out_desc)) || (long long)n + 2 > 0x7FFFFFFFLL || max_pts < 1 || !(ms >= (T)0) || !std::isfinite(ms) || method < 0 ||
        method > 3 || seed >= (1ULL << 53))
        return fail(c, PGICP_ERR_ARG,
                    "pgicp_octree_grid: bad argument (n >= 0, max_point_by_node >= 1, max_size_by_node finite and >= 0, sampling_method 0 .. 3, "
                    "seed < 2^53, strides >= 3, out_desc with desc)");
    *n_out = 0;
    if (n == 0) return PGICP_OK;
    HIPC(c, hipSetDevice(c->device));
    UploadUse uu(c);
    const int dr = desc ? drows : 0;
    OctScratch w;
    XFER(c, carve_buf(c, c->dpf_work, [&](Carve &cv) { w = oct_scratch(cv, n); }));
    CloudIn<T> in;
    T *d_ox = out_xyz, *d_od = out_desc;
    int32_t *d_oi = kept_idx, *d_oc = out_count, *d_odp = out_depth;
    int os = out_stride;
    if (mem == PGICP_HOST) {
        // io: the cloud and its descriptors as uploaded, then the outputs packed
        XFER(c, carve_buf(c, c->dpf_io, [&](Carve &cv) {
            in.carve(cv, stride, n, dr);
            d_ox = cv.take<T>(3 * (size_t)n, out_xyz);
            d_od = cv.take<T>((size_t)dr * n, desc);
            d_oi = cv.take<int32_t>((size_t)n, kept_idx);
            d_oc = cv.take<int32_t>((size_t)n, out_count);
            d_odp = cv.take<int32_t>((size_t)n, out_depth);
        }));
        os = 3;
    }
    XFER(c, upload_cloud<T>(c, mem, xyz, stride, n, desc, dr, in));
    VoxStat *stat;
    T lo[3], hi[3];
    XFER(c, cloud_bounds<T>(c, "pgicp_octree_grid", in.xyz, stride, n, &stat, lo, hi));
    const OctRoot<T> R = pgslam_amd::octree::make_root<T>(lo, hi, ms);
    {
        ProfScope ps(c, PGICP_PROF_NORMALS, n);
        launch_octree_grid<T>(c->stream, in.xyz, stride, n, R, max_pts, method, seed, in.desc, dr, w, d_ox, os, d_od, d_oi, d_oc, d_odp, stat);
    }
    return fetch_kept<T>(c, mem, stat, out_xyz, out_stride, d_ox, out_desc, d_od, dr, {{kept_idx, d_oi}, {out_count, d_oc}, {out_depth, d_odp}}, n_out);
}

}  // namespace

extern "C" {

int pgicp_octree_grid_f32(pgicp_ctx *ctx, const float *xyz, int stride, int n, int mem, int max_point_by_node, double max_size_by_node,
                          int sampling_method, unsigned long long seed, const float *desc, int drows, float *out_xyz, int out_stride, float *out_desc,
                          int32_t *kept_idx, int32_t *out_count, int32_t *out_depth, int *n_out)
{
    return octree_grid<float>(ctx, xyz, stride, n, mem, max_point_by_node, max_size_by_node, sampling_method, seed, desc, drows, out_xyz, out_stride,
                              out_desc, kept_idx, out_count, out_depth, n_out);
}
int pgicp_octree_grid_f64(pgicp_ctx *ctx, const double *xyz, int stride, int n, int mem, int max_point_by_node, double max_size_by_node,
                          int sampling_method, unsigned long long seed, const double *desc, int drows, double *out_xyz, int out_stride, double *out_desc,
                          int32_t *kept_idx, int32_t *out_count, int32_t *out_depth, int *n_out)
{
    return octree_grid<double>(ctx, xyz, stride, n, mem, max_point_by_node, max_size_by_node, sampling_method, seed, desc, drows, out_xyz, out_stride,
                               out_desc, kept_idx, out_count, out_depth, n_out);
}

}  // extern "C"
