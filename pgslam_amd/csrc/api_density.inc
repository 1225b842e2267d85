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

inline size_t dens_up(size_t b) { return (b + 255) & ~(size_t)255; }

// host array of 3 values a point at `stride` from a packed device array (stride 3); *after* the next stream_sync when direct
template <typename T>
int dens_fetch3(pgicp_ctx *c, T *out, int stride, const T *dev, int count, std::vector<T> &tmp)
{
    if (!out || count <= 0) return PGICP_OK;
    if (stride == 3) return d2h(c, out, dev, sizeof(T) * 3 * (size_t)count);
    tmp.resize(3 * (size_t)count);
    return d2h(c, tmp.data(), dev, sizeof(T) * 3 * (size_t)count);
}
template <typename T>
void dens_spread3(T *out, int stride, const std::vector<T> &tmp)
{
    for (size_t k = 0; k < tmp.size() / 3; k++) std::memcpy(out + k * stride, tmp.data() + 3 * k, 3 * sizeof(T));
}

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
    const size_t b3 = dens_up(sizeof(T) * 3 * (size_t)n), b1 = dens_up(sizeof(T) * (size_t)n);
    if (mem == PGICP_HOST) {
        HIPC(c, c->dens_io.ensure(2 * b3 + b1));
        char *p = (char *)c->dens_io.p;
        d_nrm = out_nrm ? (T *)p : nullptr;
        d_eig = out_eig ? (T *)(p + b3) : nullptr;
        d_dens = out_dens ? (T *)(p + 2 * b3) : nullptr;
        ds = 3;
    }
    {
        ProfScope ps(c, PGICP_PROF_NORMALS, n);
        if (launch_surface_densities<T>(c->stream, S.d_maps.template as<MapDev<T>>(), map_index<T>(c, tm.id), n, knn, (T)max_dist,
                                        std::numeric_limits<T>::epsilon(), d_nrm, ds, d_eig, d_dens) != 0)
            return fail(c, PGICP_ERR_ARG, "pgicp_surface_densities: knn > 32");
    }
    std::vector<T> tn;
    if (mem == PGICP_HOST) {
        XFER(c, dens_fetch3<T>(c, out_nrm, out_stride, d_nrm, n, tn));
        if (out_eig) XFER(c, d2h(c, out_eig, d_eig, sizeof(T) * 3 * (size_t)n));
        if (out_dens) XFER(c, d2h(c, out_dens, d_dens, sizeof(T) * (size_t)n));
    }
    HIPC(c, stream_sync(c));
    HIPC(c, hipGetLastError());
    if (!tn.empty()) dens_spread3<T>(out_nrm, out_stride, tn);
    return PGICP_OK;
}

// the scratch of the filter: keep (n + 1), pos (n + 1), the scan's block sums
struct DensWork { int *keep, *pos, *bsum; };
inline size_t dens_work_bytes(int n)
{
    return 2 * dens_up(sizeof(int) * ((size_t)n + 1)) + dens_up(sizeof(int) * ((size_t)n / kScanChunkHost + 4));
}
inline DensWork dens_work_layout(char *base, int n)
{
    DensWork w;
    const size_t bk = dens_up(sizeof(int) * ((size_t)n + 1));
    w.keep = (int *)base; w.pos = (int *)(base + bk); w.bsum = (int *)(base + 2 * bk);
    return w;
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
    const size_t b1 = dens_up(sizeof(T) * (size_t)n), bi = dens_up(sizeof(int) * (size_t)n);
    HIPC(c, c->dens_work.ensure(dens_work_bytes(n)));
    HIPC(c, c->dens_stat.ensure(sizeof(DensStat)));
    const DensWork w = dens_work_layout((char *)c->dens_work.p, n);
    const T *d_dens = dens;
    int32_t *d_idx = kept_idx;
    if (mem == PGICP_HOST) {
        HIPC(c, c->dens_io.ensure(b1 + bi));
        XFER(c, h2d(c, c->dens_io.p, dens, sizeof(T) * (size_t)n));
        d_dens = c->dens_io.as<T>();
        d_idx = kept_idx ? (int32_t *)((char *)c->dens_io.p + b1) : nullptr;
    } else
        uu.touch(dens);
    launch_max_density<T>(c->stream, d_dens, n, (T)max_density_, (unsigned long long)seed, c->dens_stat.as<DensStat>(), w.keep, w.pos, w.bsum);
    if (d_idx)
        launch_density_compact<T>(c->stream, n, w.keep, w.pos, nullptr, 0, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0,
                                  nullptr, nullptr, d_idx);
    int kept = 0;
    XFER(c, d2h(c, &kept, w.pos + n, sizeof kept));
    HIPC(c, stream_sync(c));
    HIPC(c, hipGetLastError());
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
    const size_t b_in = dens_up(sizeof(T) * ((size_t)(n - 1) * stride + 3)), b_d = dens_up(sizeof(T) * (size_t)dr * n),
                 b3 = dens_up(sizeof(T) * 3 * (size_t)n), b1 = dens_up(sizeof(T) * (size_t)n), bi = dens_up(sizeof(int) * (size_t)n);
    // work: the filter's scratch, then the normals kernel's rows in input order (normals, eigenvalues, densities)
    const size_t b_w = dens_work_bytes(n);
    HIPC(c, c->dens_work.ensure(b_w + 2 * b3 + b1));
    HIPC(c, c->dens_stat.ensure(sizeof(DensStat)));
    const DensWork w = dens_work_layout((char *)c->dens_work.p, n);
    T *t_nrm = (T *)((char *)c->dens_work.p + b_w), *t_eig = (T *)((char *)t_nrm + b3), *t_dens = (T *)((char *)t_eig + b3);
    const bool want_nrm = out_nrm != nullptr, want_eig = out_eig != nullptr;
    const T *d_xyz = xyz, *d_desc = desc;
    T *d_ox = out_xyz, *d_on = out_nrm, *d_oe = out_eig, *d_od = out_dens, *d_oc = out_desc;
    int32_t *d_oi = kept_idx;
    int ons = out_nstride;
    if (mem == PGICP_HOST) {
        // io: the cloud and its descriptors as uploaded, then the outputs (coordinates at `stride`, the rest packed)
        HIPC(c, c->dens_io.ensure(2 * b_in + 2 * b_d + 2 * b3 + b1 + bi));
        char *p = (char *)c->dens_io.p;
        XFER(c, h2d(c, p, xyz, sizeof(T) * ((size_t)(n - 1) * stride + 3)));
        d_xyz = (const T *)p; p += b_in;
        if (desc) { XFER(c, h2d(c, p, desc, sizeof(T) * (size_t)dr * n)); d_desc = (const T *)p; }
        p += b_d;
        d_ox = (T *)p; p += b_in;
        d_oc = desc ? (T *)p : nullptr; p += b_d;
        d_on = want_nrm ? (T *)p : nullptr; p += b3;
        d_oe = want_eig ? (T *)p : nullptr; p += b3;
        d_od = out_dens ? (T *)p : nullptr; p += b1;
        d_oi = kept_idx ? (int32_t *)p : nullptr;
        ons = 3;
    }
    TempMap<T> tm(c);
    { const int st = map_create<T>(c, d_xyz, stride, nullptr, 0, n, PGICP_DEVICE, 0, &tm.id); if (st) return st; }
    // (after map_create, which keeps an UploadUse of its own: the compaction below reads the caller's device arrays again)
    UploadUse uu(c);
    if (mem == PGICP_DEVICE) {
        uu.touch(xyz);
        if (desc) uu.touch(desc);
    }
    State<T> &S = state<T>(c);
    {
        ProfScope ps(c, PGICP_PROF_NORMALS, n);
        if (launch_surface_densities<T>(c->stream, S.d_maps.template as<MapDev<T>>(), map_index<T>(c, tm.id), n, knn, (T)max_dist,
                                        std::numeric_limits<T>::epsilon(), want_nrm ? t_nrm : nullptr, 3, want_eig ? t_eig : nullptr, t_dens) != 0)
            return fail(c, PGICP_ERR_ARG, "pgicp_normals_max_density: knn > 32");
    }
    launch_max_density<T>(c->stream, (const T *)t_dens, n, (T)max_density_, (unsigned long long)seed, c->dens_stat.as<DensStat>(), w.keep, w.pos, w.bsum);
    launch_density_compact<T>(c->stream, n, w.keep, w.pos, d_xyz, stride, d_desc, dr, (const T *)t_nrm, (const T *)t_eig, (const T *)t_dens, d_ox, d_oc,
                              d_on, ons, d_oe, d_od, d_oi);
    int kept = 0;
    XFER(c, d2h(c, &kept, w.pos + n, sizeof kept));
    HIPC(c, stream_sync(c));
    HIPC(c, hipGetLastError());
    if (mem == PGICP_HOST && kept > 0) {
        std::vector<T> tx, tn;
        if (stride == 3) XFER(c, d2h(c, out_xyz, d_ox, sizeof(T) * 3 * (size_t)kept));
        else { tx.resize((size_t)(kept - 1) * stride + 3); XFER(c, d2h(c, tx.data(), d_ox, sizeof(T) * tx.size())); }
        XFER(c, dens_fetch3<T>(c, out_nrm, out_nstride, d_on, kept, tn));
        if (out_eig) XFER(c, d2h(c, out_eig, d_oe, sizeof(T) * 3 * (size_t)kept));
        if (out_dens) XFER(c, d2h(c, out_dens, d_od, sizeof(T) * (size_t)kept));
        if (desc) XFER(c, d2h(c, out_desc, d_oc, sizeof(T) * (size_t)dr * kept));
        if (kept_idx) XFER(c, d2h(c, kept_idx, d_oi, sizeof(int32_t) * (size_t)kept));
        HIPC(c, stream_sync(c));
        for (int k = 0; k < kept && !tx.empty(); k++) std::memcpy(out_xyz + (size_t)k * stride, tx.data() + (size_t)k * stride, 3 * sizeof(T));
        if (!tn.empty()) dens_spread3<T>(out_nrm, out_nstride, tn);
    }
    *n_out = kept;
    return PGICP_OK;
}

}  // namespace
