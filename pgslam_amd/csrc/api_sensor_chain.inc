// api_sensor_chain.inc -- part of pgicp_api.cpp (one translation unit): pgicp_sensor_chain_* (include/pgicp_sensor_chain.h).
// normals_max_density (api_density.inc) with a list of stages between the normals kernel and the one gather; the older entries'
// paths are not touched.

namespace {

// `ext`: the call is pgicp_sensor_chain_ext_* (api_descriptor_filters.inc) -- stage types 6 .. 8 and PGICP_CHAIN_EXT_MAX_STAGES stages
// are allowed; without it the list is held to pgicp_sensor_chain.h's
template <typename T>
int sensor_chain(pgicp_ctx *c, const T *xyz, int stride, int n, int mem, int knn, double max_dist, int keep_normals, int keep_eig, int keep_dens,
                 int n_stages, const pgicp_chain_stage *stages, const T *desc, int drows, const ChainOut<T> &out, int *n_out, bool ext)
{
    namespace sc = pgslam_amd::sensor_chain;
    const char *who = "pgicp_sensor_chain";
    if (!c || n < 0 || (n > 0 && (!xyz || !out.xyz)) || stride < 3 || (out.nrm && out.nstride < 3) || knn < 3 || knn > 32 || !(max_dist > 0) ||
        (mem != PGICP_HOST && mem != PGICP_DEVICE) || !n_out || (desc && (drows <= 0 || !out.desc)) || (long long)n + 2 > 0x7FFFFFFFLL ||
        n_stages < 0 || (n_stages > 0 && !stages))
        return fail(c, PGICP_ERR_ARG, "pgicp_sensor_chain: bad argument (3 <= knn <= 32, n >= 0, max_dist > 0)");
    if (n_stages > (ext ? PGICP_CHAIN_EXT_MAX_STAGES : PGICP_CHAIN_MAX_STAGES))
        return fail(c, PGICP_ERR_ARG, ext ? "pgicp_sensor_chain_ext: more than PGICP_CHAIN_EXT_MAX_STAGES stages" : "pgicp_sensor_chain: more than PGICP_CHAIN_MAX_STAGES stages");
    // the list: every type but the cut at most once, each stage's row there when it runs
    ChainSeg<T> P{};
    ChainCut<T> cuts[PGICP_CHAIN_EXT_MAX_STAGES] = {};
    int types[PGICP_CHAIN_EXT_MAX_STAGES] = {0};
    bool seen[PGICP_CHAIN_CUT_AT_DESCRIPTOR + 1] = {};
    int drops = 0, n_cuts = 0;
    const auto flag01 = [](double v) { return v == 0.0 || v == 1.0; };
    for (int k = 0; k < n_stages; k++) {
        const pgicp_chain_stage &s = stages[k];
        if (s.type < PGICP_CHAIN_OBSERVATION_DIRECTION || s.type > (ext ? PGICP_CHAIN_CUT_AT_DESCRIPTOR : PGICP_CHAIN_SIMPLE_SENSOR_NOISE))
            return fail(c, PGICP_ERR_ARG, "pgicp_sensor_chain: unknown stage type " + std::to_string(s.type));
        if (seen[s.type] && s.type != PGICP_CHAIN_CUT_AT_DESCRIPTOR)
            return fail(c, PGICP_ERR_ARG, "pgicp_sensor_chain: stage type " + std::to_string(s.type) + " appears twice");
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
        case PGICP_CHAIN_SIMPLE_SENSOR_NOISE:
            if (s.p[0] != std::floor(s.p[0]) || !sc::noise_model<T>((int)s.p[0], (T)s.p[1], P.noise))
                return fail(c, PGICP_ERR_ARG, "SimpleSensorNoiseDataPointsFilter: sensorType must be 0 .. 4");
            break;
        case PGICP_CHAIN_INCIDENCE_ANGLE:
            if (!keep_normals) return fail(c, PGICP_ERR_ARG, "IncidenceAngleDataPointsFilter: cannot find normals in descriptors (keep_normals is 0)");
            if (!seen[PGICP_CHAIN_OBSERVATION_DIRECTION])
                return fail(c, PGICP_ERR_ARG, "IncidenceAngleDataPointsFilter: cannot find observation directions in descriptors (no such stage before it)");
            break;
        case PGICP_CHAIN_SPHERICALITY:
            if (!keep_eig) return fail(c, PGICP_ERR_ARG, "SphericalityDataPointsFilter: cannot find eigValues in descriptors (keep_eig is 0)");
            if (!flag01(s.p[0]) || !flag01(s.p[1])) return fail(c, PGICP_ERR_ARG, "SphericalityDataPointsFilter: keepUnstructureness and keepStructureness must be 0 or 1");
            P.keep_uns = (int)s.p[0];
            P.keep_str = (int)s.p[1];
            break;
        default: {
            if (++n_cuts > PGICP_CHAIN_EXT_MAX_CUTS) return fail(c, PGICP_ERR_ARG, "pgicp_sensor_chain_ext: more than PGICP_CHAIN_EXT_MAX_CUTS CutAtDescriptor stages");
            if (!flag01(s.p[1])) return fail(c, PGICP_ERR_ARG, "CutAtDescriptorThresholdDataPointsFilter: useLargerThan must be 0 or 1");
            bool there = false;
            if (s.p[0] == PGICP_CHAIN_ROW_DESC) there = desc && s.p[3] == std::floor(s.p[3]) && s.p[3] >= 0.0 && s.p[3] < (double)drows;
            else if (s.p[0] == PGICP_CHAIN_ROW_DENSITIES) there = keep_dens != 0;
            else if (s.p[0] == PGICP_CHAIN_ROW_INCIDENCE_ANGLES) there = seen[PGICP_CHAIN_INCIDENCE_ANGLE];
            else if (s.p[0] == PGICP_CHAIN_ROW_SPHERICALITY) there = seen[PGICP_CHAIN_SPHERICALITY];
            else if (s.p[0] == PGICP_CHAIN_ROW_UNSTRUCTURENESS) there = seen[PGICP_CHAIN_SPHERICALITY] && P.keep_uns;
            else if (s.p[0] == PGICP_CHAIN_ROW_STRUCTURENESS) there = seen[PGICP_CHAIN_SPHERICALITY] && P.keep_str;
            else if (s.p[0] == PGICP_CHAIN_ROW_SIMPLE_SENSOR_NOISE) there = seen[PGICP_CHAIN_SIMPLE_SENSOR_NOISE];
            if (!there) return fail(c, PGICP_ERR_ARG, "CutAtDescriptorThresholdDataPointsFilter: the descriptor row does not exist when the stage runs");
            cuts[k].row = (int)s.p[0];
            cuts[k].desc_row = cuts[k].row == PGICP_CHAIN_ROW_DESC ? (int)s.p[3] : 0;
            cuts[k].larger = (int)s.p[1];
            cuts[k].thr = (T)s.p[2];
            drops++;
            break;
        }
        }
        seen[s.type] = true;
        types[k] = s.type;
    }
    ChainHas has{};
    has.nrm = keep_normals != 0; has.eig = keep_eig != 0; has.dens = keep_dens != 0;
    has.obs = seen[PGICP_CHAIN_OBSERVATION_DIRECTION]; has.noise = seen[PGICP_CHAIN_SIMPLE_SENSOR_NOISE];
    has.inc = seen[PGICP_CHAIN_INCIDENCE_ANGLE]; has.sph = seen[PGICP_CHAIN_SPHERICALITY];
    has.uns = has.sph && P.keep_uns; has.str = has.sph && P.keep_str;
    has.max_density = seen[PGICP_CHAIN_MAX_DENSITY];
    if ((out.nrm && !has.nrm) || (out.eig && !has.eig) || (out.dens && !has.dens) || (out.obs && !has.obs) || (out.noise && !has.noise) ||
        (out.inc && !has.inc) || (out.sph && !has.sph) || (out.uns && !has.uns) || (out.str && !has.str))
        return fail(c, PGICP_ERR_ARG, "pgicp_sensor_chain: an output row that is not kept, or whose stage is not listed");
    *n_out = 0;
    if (n == 0) return PGICP_OK;
    HIPC(c, hipSetDevice(c->device));
    const int dr = desc ? drows : 0;
    // work: the rows at the points' input indices and the stages' scratch
    ChainRows<T> w;
    XFER(c, carve_buf(c, c->dpf_work, [&](Carve &cv) { w = chain_scratch<T>(cv, n, has, drops); }));
    HIPC(c, c->dpf_stat.ensure(sizeof(DensStat)));
    CloudIn<T> in{xyz, desc};
    ChainOut<T> o = out;
    if (mem == PGICP_HOST) {
        // io: the cloud and its descriptors as uploaded, then the outputs (coordinates at `stride`, the rest packed)
        XFER(c, carve_buf(c, c->dpf_io, [&](Carve &cv) {
            in.carve(cv, stride, n, dr);
            o.xyz = cv.take<T>((size_t)(n - 1) * stride + 3);
            o.desc = cv.take<T>((size_t)dr * n, desc);
            o.nrm = cv.take<T>(3 * (size_t)n, out.nrm);
            o.eig = cv.take<T>(3 * (size_t)n, out.eig);
            o.dens = cv.take<T>((size_t)n, out.dens);
            o.obs = cv.take<T>(3 * (size_t)n, out.obs);
            o.noise = cv.take<T>((size_t)n, out.noise);
            o.kept_idx = cv.take<int32_t>((size_t)n, out.kept_idx);
            if (out.inc) o.inc = cv.take<T>((size_t)n);
            if (out.sph) o.sph = cv.take<T>((size_t)n);
            if (out.uns) o.uns = cv.take<T>((size_t)n);
            if (out.str) o.str = cv.take<T>((size_t)n);
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
    launch_sensor_chain<T>(c->stream, in.xyz, stride, n, in.desc, dr, n_stages, types, P, cuts, w, c->dpf_stat.as<DensStat>(), o, &last_pos);
    int kept = n;
    if (last_pos) XFER(c, read_back(c, &kept, last_pos + n, sizeof kept));
    if (mem == PGICP_HOST && kept > 0) {
        RowSpread<T> late;
        XFER(c, fetch_rows3<T>(c, out.xyz, stride, o.xyz, kept, late, stride));
        XFER(c, fetch_rows3<T>(c, out.nrm, out.nstride, o.nrm, kept, late));
        if (out.eig) XFER(c, d2h(c, out.eig, o.eig, sizeof(T) * 3 * (size_t)kept));
        if (out.dens) XFER(c, d2h(c, out.dens, o.dens, sizeof(T) * (size_t)kept));
        if (out.obs) XFER(c, d2h(c, out.obs, o.obs, sizeof(T) * 3 * (size_t)kept));
        if (out.noise) XFER(c, d2h(c, out.noise, o.noise, sizeof(T) * (size_t)kept));
        if (desc) XFER(c, d2h(c, out.desc, o.desc, sizeof(T) * (size_t)dr * kept));
        if (out.kept_idx) XFER(c, d2h(c, out.kept_idx, o.kept_idx, sizeof(int32_t) * (size_t)kept));
        for (const auto &row : {std::make_pair(out.inc, o.inc), std::make_pair(out.sph, o.sph), std::make_pair(out.uns, o.uns), std::make_pair(out.str, o.str)})
            if (row.first) XFER(c, d2h(c, row.first, row.second, sizeof(T) * (size_t)kept));
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
{ return sensor_chain<float>(c, xyz, stride, n, mem, knn, max_dist, keep_normals, keep_eig, keep_dens, n_stages, stages, desc, drows,
                             ChainOut<float>{out_xyz, out_desc, out_nrm, out_nstride, out_eig, out_dens, out_obs, out_noise, nullptr, nullptr, nullptr, nullptr, kept_idx},
                             n_out, false); }
int pgicp_sensor_chain_f64(pgicp_ctx *c, const double *xyz, int stride, int n, int mem, int knn, double max_dist, int keep_normals, int keep_eig,
                           int keep_dens, int n_stages, const pgicp_chain_stage *stages, const double *desc, int drows, double *out_xyz,
                           double *out_nrm, int out_nstride, double *out_eig, double *out_dens, double *out_obs, double *out_noise, double *out_desc,
                           int32_t *kept_idx, int *n_out)
{ return sensor_chain<double>(c, xyz, stride, n, mem, knn, max_dist, keep_normals, keep_eig, keep_dens, n_stages, stages, desc, drows,
                              ChainOut<double>{out_xyz, out_desc, out_nrm, out_nstride, out_eig, out_dens, out_obs, out_noise, nullptr, nullptr, nullptr, nullptr, kept_idx},
                              n_out, false); }

}  // extern "C"
