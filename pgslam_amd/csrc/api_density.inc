// api_density.inc -- part of pgicp_api.cpp (one translation unit): pgicp_surface_densities_*, pgicp_max_density_*,
// pgicp_normals_max_density_* (include/pgicp_density.h).

namespace {

// the temporary map of a normals pass: dropped when the call leaves, whichever way
template <typename T>
struct TempMap {
    pgicp_ctx *c; int id = -1;
    explicit TempMap(pgicp_ctx *c_) : c(c_) {}
    ~TempMap() { if (id >= 0) if (MapHost<T> *mh = get_map<T>(c, id)) free_map(c, *mh); }
};

template <typename T>
int surface_densities(pgicp_ctx *c, const T *xyz, int stride, int n, int mem, int knn, double max_dist, T *out_nrm, int out_stride,
                      T *out_eig, T *out_dens)
{
    if (!c || n < 0 || (n > 0 && !xyz) || stride < 3 || (out_nrm && out_stride < 3) || knn < 3 || knn > 32 || !(max_dist > 0) ||
        (mem != PGICP_HOST && mem != PGICP_DEVICE))
        return fail(c, PGICP_ERR_ARG, "pgicp_surface_densities: bad argument (3 <= knn <= 32, n >= 0, max_dist > 0)");
    if (n == 0) return PGICP_OK;
    HIPC(c, hipSetDevice(c->device));
    TempMap<T> tm(c);
    { const int st = map_create<T>(c, xyz, stride, nullptr, 0, n, mem, 0, &tm.id); if (st) return st; }   // uncentred: coordinates stay exact
    State<T> &S = state<T>(c);
    T *d_nrm = out_nrm, *d_eig = out_eig, *d_dens = out_dens;
    int ds = out_stride;
    if (mem == PGICP_HOST) {
        XFER(c, carve_buf(c, c->dpf_io, [&](Carve &cv) {
            d_nrm = cv.take<T>(3 * (size_t)n, out_nrm);
            d_eig = cv.take<T>(3 * (size_t)n, out_eig);
            d_dens = cv.take<T>((size_t)n, out_dens);
        }));
        ds = 3;
    }
    {
        ProfScope ps(c, PGICP_PROF_NORMALS, n);
        if (launch_surface_densities<T>(c->stream, S.d_maps.template as<MapDev<T>>(), map_index<T>(c, tm.id), n, knn, (T)max_dist,
                                        std::numeric_limits<T>::epsilon(), d_nrm, ds, d_eig, d_dens) != 0)
            return fail(c, PGICP_ERR_ARG, "pgicp_surface_densities: knn > 32");
    }
    RowSpread<T> late;
    if (mem == PGICP_HOST) {
        XFER(c, fetch_rows3<T>(c, out_nrm, out_stride, d_nrm, n, late));
        if (out_eig) XFER(c, d2h(c, out_eig, d_eig, sizeof(T) * 3 * (size_t)n));
        if (out_dens) XFER(c, d2h(c, out_dens, d_dens, sizeof(T) * (size_t)n));
    }
    XFER(c, late.land(c));
    HIPC(c, hipGetLastError());
    return PGICP_OK;
}

template <typename T>
int max_density_args(pgicp_ctx *c, double max_density, uint64_t seed, const char *who)
{
    if (!((T)max_density > (T)0)) return fail(c, PGICP_ERR_ARG, std::string(who) + ": maxDensity must be greater than 0");
    if (seed >= ((uint64_t)1 << 53)) return fail(c, PGICP_ERR_ARG, std::string(who) + ": the seed must be below 2^53");
    return PGICP_OK;
}

template <typename T>
int max_density(pgicp_ctx *c, const T *dens, int n, int mem, double max_density_, uint64_t seed, int32_t *kept_idx, int *n_out)
{
    if (!c || n < 0 || (n > 0 && !dens) || !n_out || (mem != PGICP_HOST && mem != PGICP_DEVICE) || (long long)n + 2 > 0x7FFFFFFFLL)
        return fail(c, PGICP_ERR_ARG, "pgicp_max_density: bad argument");
    { const int st = max_density_args<T>(c, max_density_, seed, "pgicp_max_density"); if (st) return st; }
    *n_out = 0;
    if (n == 0) return PGICP_OK;
    HIPC(c, hipSetDevice(c->device));
    UploadUse uu(c);
    DensWork<T> w;
    XFER(c, carve_buf(c, c->dpf_work, [&](Carve &cv) { w = dens_scratch<T>(cv, n, false); }));
    HIPC(c, c->dpf_stat.ensure(sizeof(DensStat)));
    const T *d_dens = dens;
    int32_t *d_idx = kept_idx;
    if (mem == PGICP_HOST) {
        XFER(c, carve_buf(c, c->dpf_io, [&](Carve &cv) { d_dens = cv.take<T>((size_t)n); d_idx = cv.take<int32_t>((size_t)n, kept_idx); }));
        XFER(c, h2d(c, (void *)d_dens, dens, sizeof(T) * (size_t)n));
    } else
        uu.touch(dens);
    launch_max_density<T>(c->stream, d_dens, n, (T)max_density_, (unsigned long long)seed, c->dpf_stat.as<DensStat>(), w.keep, w.pos, w.bsum);
    if (d_idx)
        launch_density_compact<T>(c->stream, n, w.keep, w.pos, nullptr, 0, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0,
                                  nullptr, nullptr, d_idx);
    int kept = 0;
    XFER(c, read_back(c, &kept, w.pos + n, sizeof kept));
    if (mem == PGICP_HOST && kept_idx && kept > 0) {
        XFER(c, d2h(c, kept_idx, d_idx, sizeof(int32_t) * (size_t)kept));
        HIPC(c, stream_sync(c));
    }
    *n_out = kept;
    return PGICP_OK;
}

template <typename T>
int normals_max_density(pgicp_ctx *c, const T *xyz, int stride, int n, int mem, int knn, double max_dist, double max_density_, uint64_t seed,
                        const T *desc, int drows, T *out_xyz, T *out_nrm, int out_nstride, T *out_eig, T *out_dens, T *out_desc,
                        int32_t *kept_idx, int *n_out)
{
    if (!c || n < 0 || (n > 0 && (!xyz || !out_xyz)) || stride < 3 || (out_nrm && out_nstride < 3) || knn < 3 || knn > 32 || !(max_dist > 0) ||
        (mem != PGICP_HOST && mem != PGICP_DEVICE) || !n_out || (desc && (drows <= 0 || !out_desc)) || (long long)n + 2 > 0x7FFFFFFFLL)
        return fail(c, PGICP_ERR_ARG, "pgicp_normals_max_density: bad argument (3 <= knn <= 32, n >= 0, max_dist > 0)");
    { const int st = max_density_args<T>(c, max_density_, seed, "pgicp_normals_max_density"); if (st) return st; }
    *n_out = 0;
    if (n == 0) return PGICP_OK;
    HIPC(c, hipSetDevice(c->device));
    const int dr = desc ? drows : 0;
    // work: the filter's scratch, then the normals kernel's rows in input order (normals, eigenvalues, densities)
    DensWork<T> w;
    XFER(c, carve_buf(c, c->dpf_work, [&](Carve &cv) { w = dens_scratch<T>(cv, n, true); }));
    HIPC(c, c->dpf_stat.ensure(sizeof(DensStat)));
    const bool want_nrm = out_nrm != nullptr, want_eig = out_eig != nullptr;
    CloudIn<T> in{xyz, desc};
    T *d_ox = out_xyz, *d_on = out_nrm, *d_oe = out_eig, *d_od = out_dens, *d_oc = out_desc;
    int32_t *d_oi = kept_idx;
    int ons = out_nstride;
    if (mem == PGICP_HOST) {
        // io: the cloud and its descriptors as uploaded, then the outputs (coordinates at `stride`, the rest packed)
        XFER(c, carve_buf(c, c->dpf_io, [&](Carve &cv) {
            in.carve(cv, stride, n, dr);
            d_ox = cv.take<T>((size_t)(n - 1) * stride + 3);
            d_oc = cv.take<T>((size_t)dr * n, desc);
            d_on = cv.take<T>(3 * (size_t)n, want_nrm);
            d_oe = cv.take<T>(3 * (size_t)n, want_eig);
            d_od = cv.take<T>((size_t)n, out_dens);
            d_oi = cv.take<int32_t>((size_t)n, kept_idx);
        }));
        ons = 3;
        XFER(c, upload_cloud<T>(c, mem, xyz, stride, n, desc, dr, in));
    }
    TempMap<T> tm(c);
    { const int st = map_create<T>(c, in.xyz, stride, nullptr, 0, n, PGICP_DEVICE, 0, &tm.id); if (st) return st; }
    // (after map_create, which keeps an UploadUse of its own: the compaction below reads the caller's device arrays again)
    UploadUse uu(c);
    if (mem == PGICP_DEVICE) XFER(c, upload_cloud<T>(c, mem, xyz, stride, n, desc, dr, in));
    State<T> &S = state<T>(c);
    {
        ProfScope ps(c, PGICP_PROF_NORMALS, n);
        if (launch_surface_densities<T>(c->stream, S.d_maps.template as<MapDev<T>>(), map_index<T>(c, tm.id), n, knn, (T)max_dist,
                                        std::numeric_limits<T>::epsilon(), want_nrm ? w.nrm : nullptr, 3, want_eig ? w.eig : nullptr, w.dens) != 0)
            return fail(c, PGICP_ERR_ARG, "pgicp_normals_max_density: knn > 32");
    }
    launch_max_density<T>(c->stream, (const T *)w.dens, n, (T)max_density_, (unsigned long long)seed, c->dpf_stat.as<DensStat>(), w.keep, w.pos, w.bsum);
    launch_density_compact<T>(c->stream, n, w.keep, w.pos, in.xyz, stride, in.desc, dr, (const T *)w.nrm, (const T *)w.eig, (const T *)w.dens, d_ox, d_oc,
                              d_on, ons, d_oe, d_od, d_oi);
    int kept = 0;
    XFER(c, read_back(c, &kept, w.pos + n, sizeof kept));
    if (mem == PGICP_HOST && kept > 0) {
        RowSpread<T> late;
        XFER(c, fetch_rows3<T>(c, out_xyz, stride, d_ox, kept, late, stride));
        XFER(c, fetch_rows3<T>(c, out_nrm, out_nstride, d_on, kept, late));
        if (out_eig) XFER(c, d2h(c, out_eig, d_oe, sizeof(T) * 3 * (size_t)kept));
        if (out_dens) XFER(c, d2h(c, out_dens, d_od, sizeof(T) * (size_t)kept));
        if (desc) XFER(c, d2h(c, out_desc, d_oc, sizeof(T) * (size_t)dr * kept));
        if (kept_idx) XFER(c, d2h(c, kept_idx, d_oi, sizeof(int32_t) * (size_t)kept));
        XFER(c, late.land(c));
    }
    *n_out = kept;
    return PGICP_OK;
}

}  // namespace
