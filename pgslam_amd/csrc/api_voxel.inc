// api_voxel.inc -- part of pgicp_api.cpp (one translation unit): pgicp_voxel_grid_* (VoxelGridDataPointsFilter).

// the order-preserving key of k_vox_bounds back to the value
template <typename T>
static T vox_unkey(unsigned long long k)
{
    if constexpr (sizeof(T) == 4) {
        const uint32_t u = (uint32_t)k, b = (u & 0x80000000u) ? (u ^ 0x80000000u) : ~u;
        float f; std::memcpy(&f, &b, 4); return f;
    } else {
        const uint64_t b = (k & 0x8000000000000000ULL) ? (k ^ 0x8000000000000000ULL) : ~k;
        double d; std::memcpy(&d, &b, 8); return d;
    }
}

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
    HIPC(c, c->dpf_stat.ensure(sizeof(VoxStat)));
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
    VoxStat *stat = c->dpf_stat.as<VoxStat>();
    VoxStat h;
    launch_voxel_bounds<T>(c->stream, in.xyz, stride, n, stat);
    XFER(c, read_back(c, &h, stat, sizeof h));
    if (h.bad) return fail(c, PGICP_ERR_ARG, "pgicp_voxel_grid: a coordinate is NaN or infinite");
    // rules 1-2 in T; deviation (a): a grid with a numDiv >= 2^31 or a product of divisions >= 2^62 is refused
    for (int a = 0; a < 3; a++) {
        const T lo = vox_unkey<T>(h.lo[a]), hi = vox_unkey<T>(h.hi[a]);
        g.minB[a] = lo / g.v[a];
        const T maxB = hi / g.v[a];
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
    int kept = 0;
    XFER(c, read_back(c, &kept, &stat->kept, sizeof kept));
    if (mem == PGICP_HOST && kept > 0) {
        RowSpread<T> late;
        XFER(c, fetch_rows3<T>(c, out_xyz, out_stride, d_ox, kept, late));
        if (desc) XFER(c, d2h(c, out_desc, d_od, sizeof(T) * (size_t)dr * kept));
        if (kept_idx) XFER(c, d2h(c, kept_idx, d_oi, sizeof(int32_t) * (size_t)kept));
        if (out_count) XFER(c, d2h(c, out_count, d_oc, sizeof(int32_t) * (size_t)kept));
        XFER(c, late.land(c));
    }
    *n_out = kept;
    return PGICP_OK;
}
