// api_sensor_chain.inc -- part of pgicp_api.cpp (one translation unit): pgicp_sensor_chain_* (include/pgicp_sensor_chain.h).
// normals_max_density (api_density.inc) with a list of stages between the normals kernel and the one gather; the older entries'
// paths are not touched.

namespace {

template <typename T>
int sensor_chain(pgicp_ctx *c, const T *xyz, int stride, int n, int mem, int knn, double max_dist, int keep_normals, int keep_eig, int keep_dens,
                 int n_stages, const pgicp_chain_stage *stages, const T *desc, int drows, T *out_xyz, T *out_nrm, int out_nstride, T *out_eig,
                 T *out_dens, T *out_obs, T *out_noise, T *out_desc, int32_t *kept_idx, int *n_out)
{
    namespace sc = pgslam_amd::sensor_chain;
    const char *who = "pgicp_sensor_chain";
    if (!c || n < 0 || (n > 0 && (!xyz || !out_xyz)) || stride < 3 || (out_nrm && out_nstride < 3) || knn < 3 || knn > 32 || !(max_dist > 0) ||
        (mem != PGICP_HOST && mem != PGICP_DEVICE) || !n_out || (desc && (drows <= 0 || !out_desc)) || (long long)n + 2 > 0x7FFFFFFFLL ||
        n_stages < 0 || (n_stages > 0 && !stages))
        return fail(c, PGICP_ERR_ARG, "pgicp_sensor_chain: bad argument (3 <= knn <= 32, n >= 0, max_dist > 0)");
    if (n_stages > PGICP_CHAIN_MAX_STAGES) return fail(c, PGICP_ERR_ARG, "pgicp_sensor_chain: more than PGICP_CHAIN_MAX_STAGES stages");
    // the list: every type at most once, each stage's row there when it runs
    ChainSeg<T> P{};
    int types[PGICP_CHAIN_MAX_STAGES] = {0};
    bool seen[6] = {false, false, false, false, false, false};
    int drops = 0;
    for (int k = 0; k < n_stages; k++) {
        const pgicp_chain_stage &s = stages[k];
        if (s.type < PGICP_CHAIN_OBSERVATION_DIRECTION || s.type > PGICP_CHAIN_SIMPLE_SENSOR_NOISE)
            return fail(c, PGICP_ERR_ARG, "pgicp_sensor_chain: unknown stage type " + std::to_string(s.type));
        if (seen[s.type]) return fail(c, PGICP_ERR_ARG, "pgicp_sensor_chain: stage type " + std::to_string(s.type) + " appears twice");
        switch (s.type) {
        case PGICP_CHAIN_OBSERVATION_DIRECTION:
            for (int a = 0; a < 3; a++) P.c[a] = (T)s.p[a];
            break;
        case PGICP_CHAIN_ORIENT_NORMALS:
            if (!keep_normals) return fail(c, PGICP_ERR_ARG, "OrientNormalsDataPointsFilter: cannot find normals in descriptors (keep_normals is 0)");
            if (!seen[PGICP_CHAIN_OBSERVATION_DIRECTION])
                return fail(c, PGICP_ERR_ARG, "OrientNormalsDataPointsFilter: cannot find observation directions in descriptors (no such stage before it)");
            P.toward = s.p[0] != 0.0 ? 1 : 0;
            break;
        case PGICP_CHAIN_SHADOW:
            if (!keep_normals) return fail(c, PGICP_ERR_ARG, "ShadowDataPointsFilter: cannot find normals in descriptors (keep_normals is 0)");
            if (!sc::shadow_eps_ok(s.p[0])) return fail(c, PGICP_ERR_ARG, "ShadowDataPointsFilter: eps must be in [0, pi]");
            P.sin_eps = sc::shadow_threshold<T>((T)s.p[0]);
            drops++;
            break;
        case PGICP_CHAIN_MAX_DENSITY:
            if (!keep_dens) return fail(c, PGICP_ERR_ARG, "MaxDensityDataPointsFilter: no densities found in descriptors (keep_dens is 0)");
            if (!(s.p[1] >= 0.0 && s.p[1] < 9007199254740992.0)) return fail(c, PGICP_ERR_ARG, "pgicp_sensor_chain: the seed must be in [0, 2^53)");
            { const int st = max_density_args<T>(c, s.p[0], (uint64_t)s.p[1], who); if (st) return st; }
            P.max_density = (T)s.p[0];
            P.seed = (unsigned long long)s.p[1];
            drops++;
            break;
        default:
            if (s.p[0] != std::floor(s.p[0]) || !sc::noise_model<T>((int)s.p[0], (T)s.p[1], P.noise))
                return fail(c, PGICP_ERR_ARG, "SimpleSensorNoiseDataPointsFilter: sensorType must be 0 .. 4");
            break;
        }
        seen[s.type] = true;
        types[k] = s.type;
    }
    const bool kn = keep_normals != 0, ke = keep_eig != 0, kd = keep_dens != 0;
    const bool ko = seen[PGICP_CHAIN_OBSERVATION_DIRECTION], ks = seen[PGICP_CHAIN_SIMPLE_SENSOR_NOISE];
    if ((out_nrm && !kn) || (out_eig && !ke) || (out_dens && !kd) || (out_obs && !ko) || (out_noise && !ks))
        return fail(c, PGICP_ERR_ARG, "pgicp_sensor_chain: an output row that is not kept, or whose stage is not listed");
    *n_out = 0;
    if (n == 0) return PGICP_OK;
    HIPC(c, hipSetDevice(c->device));
    const int dr = desc ? drows : 0;
    // work: the rows at the points' input indices and the stages' scratch
    ChainRows<T> w;
    XFER(c, carve_buf(c, c->dpf_work, [&](Carve &cv) { w = chain_scratch<T>(cv, n, kn, ke, kd, ko, ks, seen[PGICP_CHAIN_MAX_DENSITY], drops); }));
    HIPC(c, c->dpf_stat.ensure(sizeof(DensStat)));
    CloudIn<T> in{xyz, desc};
    ChainOut<T> o{out_xyz, out_desc, out_nrm, out_nstride, out_eig, out_dens, out_obs, out_noise, kept_idx};
    if (mem == PGICP_HOST) {
        // io: the cloud and its descriptors as uploaded, then the outputs (coordinates at `stride`, the rest packed)
        XFER(c, carve_buf(c, c->dpf_io, [&](Carve &cv) {
            in.carve(cv, stride, n, dr);
            o.xyz = cv.take<T>((size_t)(n - 1) * stride + 3);
            o.desc = cv.take<T>((size_t)dr * n, desc);
            o.nrm = cv.take<T>(3 * (size_t)n, out_nrm);
            o.eig = cv.take<T>(3 * (size_t)n, out_eig);
            o.dens = cv.take<T>((size_t)n, out_dens);
            o.obs = cv.take<T>(3 * (size_t)n, out_obs);
            o.noise = cv.take<T>((size_t)n, out_noise);
            o.kept_idx = cv.take<int32_t>((size_t)n, kept_idx);
        }));
        o.nstride = 3;
        XFER(c, upload_cloud<T>(c, mem, xyz, stride, n, desc, dr, in));
    }
    if (!desc) o.desc = nullptr;
    TempMap<T> tm(c);
    { const int st = map_create<T>(c, in.xyz, stride, nullptr, 0, n, PGICP_DEVICE, 0, &tm.id); if (st) return st; }
    // (after map_create, which keeps an UploadUse of its own: the gather below reads the caller's device arrays again)
    UploadUse uu(c);
    if (mem == PGICP_DEVICE) XFER(c, upload_cloud<T>(c, mem, xyz, stride, n, desc, dr, in));
    State<T> &S = state<T>(c);
    {
        ProfScope ps(c, PGICP_PROF_NORMALS, n);
        if (launch_surface_densities<T>(c->stream, S.d_maps.template as<MapDev<T>>(), map_index<T>(c, tm.id), n, knn, (T)max_dist,
                                        std::numeric_limits<T>::epsilon(), w.nrm, 3, w.eig, w.dens) != 0)
            return fail(c, PGICP_ERR_ARG, "pgicp_sensor_chain: knn > 32");
    }
    const int *last_pos = nullptr;
    launch_sensor_chain<T>(c->stream, in.xyz, stride, n, in.desc, dr, n_stages, types, P, w, c->dpf_stat.as<DensStat>(), o, &last_pos);
    int kept = n;
    if (last_pos) XFER(c, read_back(c, &kept, last_pos + n, sizeof kept));
    if (mem == PGICP_HOST && kept > 0) {
        RowSpread<T> late;
        XFER(c, fetch_rows3<T>(c, out_xyz, stride, o.xyz, kept, late, stride));
        XFER(c, fetch_rows3<T>(c, out_nrm, out_nstride, o.nrm, kept, late));
        if (out_eig) XFER(c, d2h(c, out_eig, o.eig, sizeof(T) * 3 * (size_t)kept));
        if (out_dens) XFER(c, d2h(c, out_dens, o.dens, sizeof(T) * (size_t)kept));
        if (out_obs) XFER(c, d2h(c, out_obs, o.obs, sizeof(T) * 3 * (size_t)kept));
        if (out_noise) XFER(c, d2h(c, out_noise, o.noise, sizeof(T) * (size_t)kept));
        if (desc) XFER(c, d2h(c, out_desc, o.desc, sizeof(T) * (size_t)dr * kept));
        if (kept_idx) XFER(c, d2h(c, kept_idx, o.kept_idx, sizeof(int32_t) * (size_t)kept));
        XFER(c, late.land(c));
    } else if (!last_pos) {
        HIPC(c, stream_sync(c));                 // (device memory, nothing dropped: no count came back to wait for)
        HIPC(c, hipGetLastError());
    }
    *n_out = kept;
    return PGICP_OK;
}

}  // namespace

extern "C" {

int pgicp_sensor_chain_f32(pgicp_ctx *c, const float *xyz, int stride, int n, int mem, int knn, double max_dist, int keep_normals, int keep_eig,
                           int keep_dens, int n_stages, const pgicp_chain_stage *stages, const float *desc, int drows, float *out_xyz, float *out_nrm,
                           int out_nstride, float *out_eig, float *out_dens, float *out_obs, float *out_noise, float *out_desc, int32_t *kept_idx,
                           int *n_out)
{ return sensor_chain<float>(c, xyz, stride, n, mem, knn, max_dist, keep_normals, keep_eig, keep_dens, n_stages, stages, desc, drows, out_xyz, out_nrm,
                             out_nstride, out_eig, out_dens, out_obs, out_noise, out_desc, kept_idx, n_out); }
int pgicp_sensor_chain_f64(pgicp_ctx *c, const double *xyz, int stride, int n, int mem, int knn, double max_dist, int keep_normals, int keep_eig,
                           int keep_dens, int n_stages, const pgicp_chain_stage *stages, const double *desc, int drows, double *out_xyz,
                           double *out_nrm, int out_nstride, double *out_eig, double *out_dens, double *out_obs, double *out_noise, double *out_desc,
                           int32_t *kept_idx, int *n_out)
{ return sensor_chain<double>(c, xyz, stride, n, mem, knn, max_dist, keep_normals, keep_eig, keep_dens, n_stages, stages, desc, drows, out_xyz, out_nrm,
                              out_nstride, out_eig, out_dens, out_obs, out_noise, out_desc, kept_idx, n_out); }

}  // extern "C"
