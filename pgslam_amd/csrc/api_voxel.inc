// api_voxel.inc -- part of pgicp_api.cpp (one translation unit): pgicp_voxel_grid_* (VoxelGridDataPointsFilter).

template <typename T>
int voxel_grid(pgicp_ctx *c, const T *xyz, int stride, int n, int mem, const double *v, int use_centroid, const T *desc, int drows, int average,
               T *out_xyz, int out_stride, T *out_desc, int32_t *kept_idx, int32_t *out_count, int *n_out)
{
    if (!c || n < 0 || (n > 0 && !xyz) || stride < 3 || !v || (mem != PGICP_HOST && mem != PGICP_DEVICE) || !n_out || (n > 0 && !out_xyz) ||
        out_stride < 3 || (desc && (drows <= 0 || !out_desc)) || (long long)n + 2 > 0x7FFFFFFFLL)
        return fail(c, PGICP_ERR_ARG, "pgicp_voxel_grid: bad argument");
    VoxGrid<T> g;
    for (int a = 0; a < 3; a++) {
        g.v[a] = (T)v[a];
        if (!(g.v[a] > (T)0) || !std::isfinite(g.v[a])) return fail(c, PGICP_ERR_ARG, "pgicp_voxel_grid: a voxel size is not finite and > 0 in T");
    }
    *n_out = 0;
    if (n == 0) return PGICP_OK;
    HIPC(c, hipSetDevice(c->device));
    UploadUse uu(c);
    const int dr = desc ? drows : 0;
    // scratch of the sort, then (host memory) the inputs' device copies and the outputs packed: 3 values a point
    VoxScratch w;
    XFER(c, carve_buf(c, c->dpf_work, [&](Carve &cv) { w = vox_scratch(cv, n); }));
    CloudIn<T> in;
    T *d_ox = out_xyz, *d_od = out_desc;
    int32_t *d_oi = kept_idx, *d_oc = out_count;
    int os = out_stride;
    if (mem == PGICP_HOST) {
        XFER(c, carve_buf(c, c->dpf_io, [&](Carve &cv) {
            in.carve(cv, stride, n, dr);
            d_ox = cv.take<T>(3 * (size_t)n);
            d_od = cv.take<T>((size_t)dr * n, desc);
            d_oi = cv.take<int32_t>((size_t)n);
            d_oc = cv.take<int32_t>((size_t)n);
        }));
        os = 3;
    }
    XFER(c, upload_cloud<T>(c, mem, xyz, stride, n, desc, dr, in));
    VoxStat *stat;
    T lo[3], hi[3];
    XFER(c, cloud_bounds<T>(c, "pgicp_voxel_grid", in.xyz, stride, n, &stat, lo, hi));
    // rules 1-2 in T; deviation (a): a grid with a numDiv >= 2^31 or a product of divisions >= 2^62 is refused
    for (int a = 0; a < 3; a++) {
        g.minB[a] = lo[a] / g.v[a];
        const T maxB = hi[a] / g.v[a];
        const T d = ((T)1 + maxB) - g.minB[a];
        if (!(d < (T)2147483648.0)) return fail(c, PGICP_ERR_ARG, "pgicp_voxel_grid: the grid is too fine (a numDiv >= 2^31)");
        g.nd[a] = (unsigned long long)(unsigned)d;
    }
    if ((unsigned __int128)(g.nd[0] * g.nd[1]) * g.nd[2] >= ((unsigned __int128)1 << 62))
        return fail(c, PGICP_ERR_ARG, "pgicp_voxel_grid: the grid is too fine (numDivX numDivY numDivZ >= 2^62)");
    // the largest key a point can have: i_a <= numDiv_a (the rounded (1 + maxB) - minB bounds the rounded x / v - minB)
    const unsigned long long top = g.nd[0] + g.nd[1] * g.nd[0] + g.nd[2] * (g.nd[0] * g.nd[1]);
    const int bits = 64 - __builtin_clzll(top);
    {
        ProfScope ps(c, PGICP_PROF_NORMALS, n);
        launch_voxel_grid<T>(c->stream, in.xyz, stride, n, g, bits, use_centroid ? 1 : 0, in.desc, dr, average ? 1 : 0, w, d_ox, os, d_od, d_oi, d_oc, stat);
    }
    return fetch_kept<T>(c, mem, stat, out_xyz, out_stride, d_ox, out_desc, d_od, dr, {{kept_idx, d_oi}, {out_count, d_oc}}, n_out);
}
