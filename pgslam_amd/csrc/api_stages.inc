// api_stages.inc -- part of pgicp_api.cpp (one translation unit): stage-level entry points: matcher, partial chain, outlier weights, error statistics, transform, local-map assembly, surface normals.
// matcher-only / partial chain on one problem
// (out: the layout, the problem record and the iteration's buffer record of the one problem -- B.pair_slot / B.pair_d2 hold the pairs)
template <typename T>
int run_partial(pgicp_ctx *c, int map_id, const T *reading, int stride, int n, int mem, const double *Tmove,
                BatchLayout &L, std::vector<ProblemDev> &hp, IterBufs<T> &B)
{
    MapHost<T> *M = get_map<T>(c, map_id);
    if (!M) return fail(c, PGICP_ERR_ARG, "pgicp: unknown map id");
    const pgicp_problem pr = one_problem(map_id, reading, stride, n, mem, Tmove);
    // (the matcher alone: no outlier filter runs here, so a SurfaceNormalOutlierFilter's normals are not asked for)
    struct NoNormals { pgicp_ctx *c; double a; ~NoNormals() { c->prm.normal_max_angle = a; } } restore{c, c->prm.normal_max_angle};
    c->prm.normal_max_angle = 0.0;
    // (matching alone: the GenericDescriptor filter weighs pairs, it does not need the map's values here)
    struct NoDesc { pgicp_ctx *c; int m; ~NoDesc() { c->gd_mode = m; } } restore_gd{c, c->gd_mode};
    c->gd_mode = PGICP_DESC_FILTER_OFF;
    int st = batch_begin<T>(c, 1, &pr, [&](int, double *Tpre) { centred_pre(M, pr.T_init, Tpre); }, L, hp);
    if (st) return st;
    B = iter_bufs<T>(c, L);
    const ChainDev<T> ch = chain_of<T>(c, c->prm);
    const IterPlan pl = iter_plan(c, L, ch);
    // the matcher stage as the public matcher output / a partial chain needs it: unseeded, every queued query resolved exactly
    if (matcher_stage<T>(c, L, ch, B, pl, 1, n, 1, 0, 0, true) != 0) return fail(c, PGICP_ERR_ARG, "KDTreeMatcher.knn exceeds PGICP_MAX_KNN");
    // (pgicp_vardist.h: what the call returns is cut as an iteration's pairs are)
    if (pl.vardist) cut_pairs<T>(c, B, 1, L.max_pairs());
    return PGICP_OK;
}

template <typename T>
int match(pgicp_ctx *c, int map_id, const T *reading, int stride, int n, int mem, const double *Tm, int32_t *ids, T *dist2)
{
    VarDistCall radii(c);                        // (pgicp_arm_reading_radii: one-shot, consumed here whatever follows)
    if (!c || !reading || n <= 0 || !ids || !dist2) return fail(c, PGICP_ERR_ARG, "pgicp_match: bad argument");
    {
        const pgicp_problem one = one_problem(-1, reading, stride, n, mem, Tm);
        const int rst = radii.template check<T>(1, &one);
        if (rst) return rst;
    }
    HIPC(c, hipSetDevice(c->device));
    BatchLayout L;
    std::vector<ProblemDev> hp;
    IterBufs<T> B;
    int st = run_partial<T>(c, map_id, reading, stride, n, mem, Tm, L, hp, B);
    if (st) return st;
    const size_t np = (size_t)n * L.knn;                     // knn entries per reading point
    HIPC(c, c->tmp_a.ensure(sizeof(int) * np));
    HIPC(c, c->tmp_b.ensure(sizeof(T) * np));
    launch_unpermute<T>(c->stream, B.maps, map_index<T>(c, map_id), B.order, B.pair_slot, B.pair_d2, n, L.knn, c->tmp_a.as<int>(), c->tmp_b.as<T>());
    if (mem == PGICP_DEVICE) {
        HIPC(c, hipMemcpyAsync(ids, c->tmp_a.p, sizeof(int) * np, hipMemcpyDeviceToDevice, c->stream));
        HIPC(c, hipMemcpyAsync(dist2, c->tmp_b.p, sizeof(T) * np, hipMemcpyDeviceToDevice, c->stream));
    } else {
        XFER(c, d2h(c, ids, c->tmp_a.p, sizeof(int) * np));
        XFER(c, d2h(c, dist2, c->tmp_b.p, sizeof(T) * np));
    }
    HIPC(c, stream_sync(c));
    HIPC(c, hipGetLastError());
    return PGICP_OK;
}

// transform -> match -> trimmed outlier filter -> error elements for P (map, reading, T) problems in
// one device pass; the same lazily-exact matcher pipeline one ICP iteration uses, without the solve.
// seeds for the one problem of a partial chain, taken from another context's last align (pgicp_partial_chain_seeded)
struct SeedSpec {
    pgicp_ctx *src; int n_seg; const int32_t *src_start, *dst_start;
};

template <typename T>
int partial_chain_batch(pgicp_ctx *c, int P, const pgicp_problem *pr, double *ratio, double *residual, int *status, const SeedSpec *seed = nullptr)
{
    // (pgicp_arm_reading_radii: one-shot, consumed here whatever follows -- but a seeded probe refuses and keeps the arm)
    if (c && seed && c->vd.armed) return fail(c, PGICP_ERR_ARG, "pgicp_partial_chain_seeded: reading radii are armed (pgicp_arm_reading_radii): the seeded probe takes none");
    VarDistCall radii(c);
    if (!c || P <= 0 || !pr) return fail(c, PGICP_ERR_ARG, "pgicp_partial_chain: bad argument");
    { const int rst = radii.template check<T>(P, pr); if (rst) return rst; }
    HIPC(c, hipSetDevice(c->device));
    for (int p = 0; p < P; p++) {
        MapHost<T> *M = get_map<T>(c, pr[p].map_id);
        if (!M) return fail(c, PGICP_ERR_ARG, "pgicp_partial_chain: unknown map id");
        { const int gst = descriptor_filter_check<T>(c, M, pr[p].map_id); if (gst) return gst; }
        if (!M->has_nrm && needs_ref_normals(c->prm))
            return fail(c, PGICP_ERR_ARG, "pgicp: reference has no normals descriptor");
        if (!M->has_nrm && robust_plane_dist(c))
            return fail(c, PGICP_ERR_ARG, "RobustOutlierFilter: distanceType point2plane, and the map of problem " + std::to_string(p) + " has no normals");
    }
    BatchLayout L;
    std::vector<ProblemDev> hp;
    // Seeds (one problem): the source context's correspondences -- slot of the ICP's map per SORTED position of ITS sort -- become,
    // point by point, slots of this call's map: ICP slot -> original index in the ICP's map -> the keyframe segment it lies in ->
    // the same point's index in this map -> its slot here (slot_of).  The reading is taken in the source's order (BorrowSpec), so
    // all of it is one kernel instead of the reading sort.  Mode 2 of the matcher: seeds are read, the pass has no history.
    BorrowSpec bs;
    bool borrow = false;
    // Whether the source's state is still what it claims to be is seed_source_ok's to say (seed_source.hpp), and nobody else's.
    if (seed && seed->src) {
        pgicp_ctx *a = seed->src;
        State<T> &SA = state<T>(a);
        MapHost<T> *MB = get_map<T>(c, pr[0].map_id);
        const MapHost<T> *MA = a->last_map0 >= 0 && a->last_map0 < (int)SA.maps.size() ? &SA.maps[a->last_map0] : nullptr;
        SeedSource q;
        q.src_n = a->last_n0; q.src_elem = a->last_elem; q.src_knn = a->last_knn; q.src_map = a->last_map0; q.src_device = a->device;
        q.src_stamp = a->last_stamp0;
        q.n = pr[0].n; q.elem = (int)sizeof(T); q.device = c->device; q.n_seg = seed->n_seg; q.src_is_self = a == c;
        q.problems = P; q.knn = std::max(1, c->prm.knn); q.grid_matcher = c->prm.matcher == PGICP_MATCHER_GRID;
        q.normals_filter = c->prm.normal_max_angle > 0.0; q.desc_filter = c->gd_mode != PGICP_DESC_FILTER_OFF;
        q.map_used = MA && MA->used; q.map_stamp = MA ? MA->stamp : 0;
        if (seed_source_ok(q) && MB) {
            if (!MB->slot_of_made) { launch_slot_of<T>(c->stream, MB->pts, MB->first, MB->m, MB->slot_of); MB->slot_of_made = true; }
            bs.order_a = a->order.as<int>(); bs.slot_a = SA.slot.template as<int>(); bs.pts_a = MA->pts;
            bs.first_a = MA->first; bs.m_a = MA->m;
            bs.sg.n = seed->n_seg;
            for (int k = 0; k <= seed->n_seg; k++) bs.sg.src[k] = seed->src_start[k];
            for (int k = 0; k < seed->n_seg; k++) bs.sg.dst[k] = seed->dst_start[k];
            bs.slot_of_b = MB->slot_of; bs.m_b = MB->m;
            borrow = true;
        }
    }
    int st = batch_begin<T>(c, P, pr, [&](int p, double *Tpre) { centred_pre(get_map<T>(c, pr[p].map_id), pr[p].T_init, Tpre); }, L, hp, 1,
                            borrow ? &bs : nullptr);
    if (st) return st;
    const IterBufs<T> B = iter_bufs<T>(c, L);
    const ChainDev<T> ch = chain_of<T>(c, c->prm);
    const int mode = borrow ? (bs.capped ? 3 : 2) : 0;
    c->sel_guess_first = hints_cover_first(hp) ? 1 : 0;
    one_iteration<T>(c, L, ch, B, iter_plan(c, L, ch), false, L.total, P, mode);
    c->sel_guess_first = 0;
    launch_sum_partials(c->stream, B.partials, reduce_blocks(L.max_pairs()), kSys, B.probs, 0, c->sums.as<double>(), P);
    std::vector<double> sys((size_t)P * kSys);
    XFER(c, d2h(c, sys.data(), c->sums.p, sizeof(double) * sys.size()));
    XFER(c, batch_download(c, P, hp, 1));
    int worst = PGICP_OK;
    for (int p = 0; p < P; p++) {
        const double *s = sys.data() + (size_t)p * kSys;
        const bool ok = hp[p].n_finite != 0 && s[28] > 0.0;
        if (status) status[p] = ok ? PGICP_OK : PGICP_ERR_NO_MATCH;
        if (!ok) worst = PGICP_ERR_NO_MATCH;
        if (ratio) ratio[p] = ok ? s[27] / ((double)pr[p].n * L.knn) : 0.0;
        if (residual) residual[p] = ok ? s[29] : 0.0;
    }
    if (worst != PGICP_OK) return fail(c, worst, "no point to minimize (ConvergenceError)");
    return PGICP_OK;
}

template <typename T>
int partial_chain(pgicp_ctx *c, int map_id, const T *reading, int stride, int n, int mem, const double *Tm, double *ratio,
                  double *residual)
{
    if (!c || !reading || n <= 0) { VarDistCall radii(c); return fail(c, PGICP_ERR_ARG, "pgicp_partial_chain: bad argument"); }
    const pgicp_problem pr = one_problem(map_id, reading, stride, n, mem, Tm);
    return partial_chain_batch<T>(c, 1, &pr, ratio, residual, nullptr);
}

template <typename T>
int partial_chain_seeded(pgicp_ctx *c, int map_id, const T *reading, int stride, int n, int mem, const double *Tm, pgicp_ctx *src, int n_seg,
                         const int32_t *src_start, const int32_t *dst_start, double *ratio, double *residual)
{
    if (!c || !reading || n <= 0) return fail(c, PGICP_ERR_ARG, "pgicp_partial_chain_seeded: bad argument");
    if (src && (n_seg < 0 || (n_seg > 0 && (!src_start || !dst_start)))) return fail(c, PGICP_ERR_ARG, "pgicp_partial_chain_seeded: bad segments");
    const pgicp_problem pr = one_problem(map_id, reading, stride, n, mem, Tm);
    const SeedSpec sp{src, n_seg, src_start, dst_start};
    return partial_chain_batch<T>(c, 1, &pr, ratio, residual, nullptr, &sp);
}

template <typename T>
int outlier_weights(pgicp_ctx *c, const T *dist2, int n, int mem, T *weights, T *limit, int *n_finite)
{
    if (!c || !dist2 || n <= 0) return fail(c, PGICP_ERR_ARG, "pgicp_outlier_weights: bad argument");
    c->vt_last.clear();
    { const int vst = var_trim_check(c); if (vst) return vst; }
    if (c->rx_on) { const int xst = robust_ext_check(c, c->rx); if (xst) return xst; }
    if (robust_plane_dist(c))
        return fail(c, PGICP_ERR_ARG, "pgicp_outlier_weights: RobustOutlierFilter's distanceType is point2plane, and an array of distances has no geometry");
    HIPC(c, hipSetDevice(c->device));
    const T *d_d2 = dist2;
    T *d_w = weights;
    if (mem == PGICP_HOST) {
        HIPC(c, c->tmp_a.ensure(sizeof(T) * (size_t)n));
        HIPC(c, c->tmp_b.ensure(sizeof(T) * (size_t)n));
        XFER(c, h2d(c, c->tmp_a.p, dist2, sizeof(T) * (size_t)n));
        d_d2 = c->tmp_a.as<T>();
        d_w = weights ? c->tmp_b.as<T>() : nullptr;
    }
    HIPC(c, c->small.ensure(256));
    // RobustOutlierFilter in the chain: its weights (the median and the median absolute deviation of the finite distances
    // by the same block selection); `limit` comes back +inf -- the filter has none
    const bool robust = c->prm.robust_fct != PGICP_ROBUST_NONE;
    if (robust) HIPC(c, c->robust_dev.ensure(sizeof(T) * (size_t)n));
    // VarTrimmedDistOutlierFilter: the ratio first (k_var_trim over one problem record that spans the array), read back --
    // then the same selection and weights as TrimmedDist's at that ratio
    double ratio = c->prm.trim_ratio;
    if (c->vt_on) {
        const size_t rec = (sizeof(ProblemDev) + 63) & ~(size_t)63;
        HIPC(c, c->vt_prob.ensure(rec + 64));
        HIPC(c, c->vt_keys.ensure(2 * sizeof(T) * (size_t)n));
        ProblemDev D;
        std::memset(&D, 0, sizeof D);
        D.n = n; D.knn = 1; D.off = 0;
        const int zero = 0;
        XFER(c, h2d(c, c->vt_prob.p, &D, sizeof D));
        XFER(c, h2d(c, (char *)c->vt_prob.p + rec, &zero, sizeof zero));
        {
            ProfScope ps(c, PGICP_PROF_TRIM, n);
            launch_var_trim<T>(c->stream, c->vt_prob.as<ProblemDev>(), d_d2, (const int *)((char *)c->vt_prob.p + rec), 1, c->vt_keys.p,
                               (char *)c->vt_keys.p + sizeof(T) * (size_t)n, c->vt[0], c->vt[1], c->vt[2]);
        }
        XFER(c, d2h(c, &D, c->vt_prob.p, sizeof D));
        HIPC(c, stream_sync(c));
        HIPC(c, hipGetLastError());
        c->vt_last.assign(1, D.vt_ratio);
        if (D.vt_ratio < 0.0) {
            // (no positive finite distance: upstream's ConvergenceError; the finite count is still reported)
            if (limit) *limit = std::numeric_limits<T>::infinity();
            if (n_finite) {
                T h[2];
                launch_trim_raw<T>(c->stream, d_d2, n, (T)1, (T)1, c->small.as<T>(), nullptr);
                XFER(c, d2h(c, h, c->small.p, sizeof h));
                HIPC(c, stream_sync(c));
                *n_finite = (int)h[1];
            }
            return fail(c, PGICP_ERR_NO_MATCH, "VarTrimmedDistOutlierFilter: no outlier to filter (ConvergenceError)");
        }
        ratio = D.vt_ratio;
    }
    {
        ProfScope ps(c, PGICP_PROF_TRIM, n);
        RobustDev<T> rb = make_chain<T>(c->prm).robust;
        robust_ext_apply<T>(c, c->prm, rb);             // (one pass is iteration 1: berg's first scale; nb has no effect)
        if (robust) launch_robust_raw<T>(c->stream, d_d2, n, rb, c->robust_dev.as<T>(), c->small.as<T>(), d_w);
        else launch_trim_raw<T>(c->stream, d_d2, n, (T)ratio, (T)c->prm.quantile_scale, c->small.as<T>(), d_w);
    }
    T h[2];
    XFER(c, d2h(c, h, c->small.p, sizeof h));
    if (mem == PGICP_HOST && weights)
        XFER(c, d2h(c, weights, d_w, sizeof(T) * (size_t)n));
    HIPC(c, stream_sync(c));
    HIPC(c, hipGetLastError());
    if (limit) *limit = robust ? std::numeric_limits<T>::infinity() : h[0];
    if (n_finite) *n_finite = (int)h[1];
    if ((int)h[1] == 0) return fail(c, PGICP_ERR_NO_MATCH, "no outlier to filter (ConvergenceError)");
    return PGICP_OK;
}

template <typename T>
int error_stats(pgicp_ctx *c, int map_id, const T *reading, int stride, int n, int mem, const int32_t *ids, const T *w,
                double *ratio, double *residual, double *sys_out)
{
    if (!c || !reading || !ids || !w || n <= 0 || stride < 3) return fail(c, PGICP_ERR_ARG, "pgicp_error_stats: bad argument");
    HIPC(c, hipSetDevice(c->device));
    MapHost<T> *M = get_map<T>(c, map_id);
    if (!M || (!M->has_nrm && !is_p2point(c->prm.error_minimizer))) return fail(c, PGICP_ERR_ARG, "pgicp_error_stats: unknown map or no normals");
    State<T> &S = state<T>(c);
    const int K = std::max(1, c->prm.knn);                   // ids / w: knn entries per reading point
    const T *d_rd = reading, *d_w = w;
    const int *d_ids = ids;
    UploadUse use(c);
    if (mem == PGICP_DEVICE) use.touch(reading);
    if (mem == PGICP_HOST) {
        HIPC(c, S.staging.ensure(staged_bytes(sizeof(T), stride, n)));
        int st = to_device<T>(c, reading, stride, n, mem, S.staging, 0, &d_rd);
        if (st) return st;
        HIPC(c, c->tmp_a.ensure(sizeof(int) * (size_t)n * K));
        HIPC(c, c->tmp_b.ensure(sizeof(T) * (size_t)n * K));
        XFER(c, h2d(c, c->tmp_a.p, ids, sizeof(int) * (size_t)n * K));
        XFER(c, h2d(c, c->tmp_b.p, w, sizeof(T) * (size_t)n * K));
        d_ids = c->tmp_a.as<int>();
        d_w = c->tmp_b.as<T>();
    }
    if (!M->slot_of_made) {
        launch_slot_of<T>(c->stream, M->pts, M->first, M->m, M->slot_of);
        M->slot_of_made = true;
    }
    const int nb = (int)(((long long)n * K + kReduceSpan - 1) / kReduceSpan);
    HIPC(c, c->partials.ensure(sizeof(double) * (size_t)nb * kSys));
    HIPC(c, c->sums.ensure(sizeof(double) * kCovTerms));
    {
        ProfScope ps(c, PGICP_PROF_REDUCE, n);
        launch_error_stats<T>(c->stream, S.d_maps.template as<MapDev<T>>(), map_index<T>(c, map_id), M->slot_of, d_rd, stride, d_ids, d_w, n, K,
                              M->mean, c->partials.as<double>(), c->sums.as<double>(), is_p2point(c->prm.error_minimizer) ? 1 : 0);
    }
    double sys[kSys];
    XFER(c, d2h(c, sys, c->sums.p, sizeof sys));
    HIPC(c, stream_sync(c));
    HIPC(c, hipGetLastError());
    if (sys_out) std::memcpy(sys_out, sys, sizeof sys);
    if (!(sys[28] > 0.0)) return fail(c, PGICP_ERR_NO_MATCH, "no point to minimize (ConvergenceError)");
    if (ratio) *ratio = sys[27] / ((double)n * K);
    if (residual) *residual = sys[29];
    return PGICP_OK;
}

bool is_rigid(const double *T)
{
    // RigidTransformation::checkParameters: R^T R ~ I and det(R) ~ +1
    double err = 0.0;
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
            double s = 0.0;
            for (int k = 0; k < 3; k++) s += T[k * 4 + i] * T[k * 4 + j];
            err = std::max(err, std::fabs(s - (i == j ? 1.0 : 0.0)));
        }
    const double det = T[0] * (T[5] * T[10] - T[6] * T[9]) - T[1] * (T[4] * T[10] - T[6] * T[8]) +
                       T[2] * (T[4] * T[9] - T[5] * T[8]);
    return err < 1e-3 && std::fabs(det - 1.0) < 1e-3;
}

template <typename T>
int transform(pgicp_ctx *c, const double *T16, const T *in, int in_stride, T *out, int out_stride, int n, int rotate_only,
              int mem)
{
    if (!c || !T16 || !in || !out || n < 0 || in_stride < 3 || out_stride < 3)
        return fail(c, PGICP_ERR_ARG, "pgicp_transform: bad argument");
    if (!is_rigid(T16)) return fail(c, PGICP_ERR_NOT_RIGID, "pgicp_transform: transformation is not rigid");
    if (n == 0) return PGICP_OK;
    HIPC(c, hipSetDevice(c->device));
    State<T> &S = state<T>(c);
    UploadUse use(c);
    if (mem == PGICP_DEVICE) {
        use.touch(in);
        launch_transform<T>(c->stream, in, in_stride, out, out_stride, n, T16, rotate_only);
        HIPC(c, stream_sync(c));
        return PGICP_OK;
    }
    const size_t bi = staged_bytes(sizeof(T), in_stride, n), bo = staged_bytes(sizeof(T), out_stride, n);
    HIPC(c, S.staging.ensure(bi));
    if (in == out && in_stride == out_stride) {
        // in place: the staged copy is input and output (a thread reads and writes its own point), the caller's other
        // rows travel with it -- one upload instead of two
        const T *d_io = nullptr;
        int st0 = to_device<T>(c, in, in_stride, n, mem, S.staging, 0, &d_io);
        if (st0) return st0;
        launch_transform<T>(c->stream, d_io, in_stride, const_cast<T *>(d_io), out_stride, n, T16, rotate_only);
        XFER(c, d2h(c, out, d_io, sizeof(T) * ((size_t)(n - 1) * out_stride + 3)));
        HIPC(c, stream_sync(c));
        HIPC(c, hipGetLastError());
        return PGICP_OK;
    }
    HIPC(c, S.stage_aux.ensure(bo));
    const T *d_in = nullptr;
    int st = to_device<T>(c, in, in_stride, n, mem, S.staging, 0, &d_in);
    if (st) return st;
    // keep the caller's other rows (e.g. the homogeneous 1) when out is strided
    XFER(c, h2d(c, S.stage_aux.p, out, sizeof(T) * ((size_t)(n - 1) * out_stride + 3)));
    launch_transform<T>(c->stream, d_in, in_stride, S.stage_aux.template as<T>(), out_stride, n, T16, rotate_only);
    XFER(c, d2h(c, out, S.stage_aux.p, sizeof(T) * ((size_t)(n - 1) * out_stride + 3)));
    HIPC(c, stream_sync(c));
    HIPC(c, hipGetLastError());
    return PGICP_OK;
}

template <typename T>
int build_local_map(pgicp_ctx *c, int n_kf, const T *const *xyz, const T *const *nrm, const int *sx, const int *sn,
                    const int *counts, const double *T_ref_kf, T *out_xyz, int out_stride, T *out_nrm, int out_nstride, int mem)
{
    if (!c || n_kf <= 0 || !xyz || !counts || !T_ref_kf || !out_xyz || out_stride < 3 || (out_nrm && out_nstride < 3))
        return fail(c, PGICP_ERR_ARG, "pgicp_build_local_map: bad argument");
    HIPC(c, hipSetDevice(c->device));
    State<T> &S = state<T>(c);
    UploadUse use(c);
    long long total = 0;
    size_t stage = 0;
    for (int k = 0; k < n_kf; k++) {
        if (counts[k] <= 0 || sx[k] < 3) return fail(c, PGICP_ERR_ARG, "pgicp_build_local_map: bad keyframe");
        total += counts[k];
        if (mem == PGICP_HOST) stage += staged_bytes(sizeof(T), sx[k], counts[k]) + (nrm ? staged_bytes(sizeof(T), sn[k], counts[k]) : 0);
    }
    T *d_ox = out_xyz, *d_on = out_nrm;
    const size_t ob = sizeof(T) * ((size_t)(total - 1) * out_stride + 3);
    const size_t onb = out_nrm ? sizeof(T) * ((size_t)(total - 1) * out_nstride + 3) : 0;
    if (mem == PGICP_HOST) {
        HIPC(c, S.staging.ensure(stage));
        HIPC(c, S.stage_aux.ensure(((ob + 255) & ~(size_t)255) + onb + 256));
        d_ox = S.stage_aux.template as<T>();
        d_on = out_nrm ? (T *)((char *)S.stage_aux.p + ((ob + 255) & ~(size_t)255)) : nullptr;
        XFER(c, h2d(c, d_ox, out_xyz, ob));
        if (out_nrm) XFER(c, h2d(c, d_on, out_nrm, onb));
    }
    size_t soff = 0;
    long long off = 0;
    double I[16];
    mat4_identity(I);
    for (int k = 0; k < n_kf; k++) {
        const double *Tk = k == 0 ? I : T_ref_kf + 16 * k;     // LocalMap.hpp:214: the reference cloud is copied as is
        if (k > 0 && !is_rigid(Tk)) return fail(c, PGICP_ERR_NOT_RIGID, "pgicp_build_local_map: transformation is not rigid");
        const T *d_x = nullptr, *d_n = nullptr;
        int st = to_device<T>(c, xyz[k], sx[k], counts[k], mem, S.staging, soff, &d_x);
        if (st) return st;
        if (mem == PGICP_HOST) soff += staged_bytes(sizeof(T), sx[k], counts[k]);
        launch_transform<T>(c->stream, d_x, sx[k], d_ox + off * out_stride, out_stride, counts[k], Tk, 0);
        if (nrm && out_nrm) {
            st = to_device<T>(c, nrm[k], sn[k], counts[k], mem, S.staging, soff, &d_n);
            if (st) return st;
            if (mem == PGICP_HOST) soff += staged_bytes(sizeof(T), sn[k], counts[k]);
            launch_transform<T>(c->stream, d_n, sn[k], d_on + off * out_nstride, out_nstride, counts[k], Tk, 1);
        }
        off += counts[k];
    }
    if (mem == PGICP_HOST) {
        XFER(c, d2h(c, out_xyz, d_ox, ob));
        if (out_nrm) XFER(c, d2h(c, out_nrm, d_on, onb));
    }
    HIPC(c, stream_sync(c));
    HIPC(c, hipGetLastError());
    return PGICP_OK;
}

template <typename T>
int surface_normals(pgicp_ctx *c, const T *xyz, int stride, int n, int mem, int knn, double max_dist, T *out_nrm,
                    int out_stride, T *out_eig, int32_t *out_ids, T *out_d2)
{
    if (!c || !xyz || n <= 0 || stride < 3 || !out_nrm || out_stride < 3 || knn < 1 || knn > 32 || !(max_dist > 0))
        return fail(c, PGICP_ERR_ARG, "pgicp_surface_normals: bad argument (1 <= knn <= 32)");
    HIPC(c, hipSetDevice(c->device));
    int id = -1;
    int st = map_create<T>(c, xyz, stride, nullptr, 0, n, mem, 0, &id);       // uncentred: coordinates stay exact
    if (st) return st;
    State<T> &S = state<T>(c);
    T *d_nrm = out_nrm, *d_eig = out_eig, *d_d2 = out_d2;
    int32_t *d_ids = out_ids;
    const size_t b_nrm = sizeof(T) * ((size_t)(n - 1) * out_stride + 3), b_eig = sizeof(T) * 3 * (size_t)n,
                 b_ids = sizeof(int32_t) * (size_t)knn * n, b_d2 = sizeof(T) * (size_t)knn * n;
    auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
    if (mem == PGICP_HOST) {
        HIPC(c, S.stage_aux.ensure(up(b_nrm) + up(b_eig) + up(b_ids) + up(b_d2) + 256));
        char *base = (char *)S.stage_aux.p;
        d_nrm = (T *)base;
        d_eig = out_eig ? (T *)(base + up(b_nrm)) : nullptr;
        d_ids = out_ids ? (int32_t *)(base + up(b_nrm) + up(b_eig)) : nullptr;
        d_d2 = out_d2 ? (T *)(base + up(b_nrm) + up(b_eig) + up(b_ids)) : nullptr;
        if (out_stride > 3) XFER(c, h2d(c, d_nrm, out_nrm, b_nrm));   // keep the caller's padding
    }
    {
        ProfScope ps(c, PGICP_PROF_NORMALS, n);
        if (launch_surface_normals<T>(c->stream, S.d_maps.template as<MapDev<T>>(), map_index<T>(c, id), n, knn, (T)max_dist,
                                      std::numeric_limits<T>::epsilon(), d_nrm, out_stride, d_eig, d_ids, d_d2) != 0)
            return fail(c, PGICP_ERR_ARG, "pgicp_surface_normals: knn > 32");
    }
    if (mem == PGICP_HOST) {
        XFER(c, d2h(c, out_nrm, d_nrm, b_nrm));
        if (out_eig) XFER(c, d2h(c, out_eig, d_eig, b_eig));
        if (out_ids) XFER(c, d2h(c, out_ids, d_ids, b_ids));
        if (out_d2) XFER(c, d2h(c, out_d2, d_d2, b_d2));
    }
    HIPC(c, stream_sync(c));
    HIPC(c, hipGetLastError());
    if (MapHost<T> *mh = get_map<T>(c, id)) free_map(c, *mh);
    return PGICP_OK;
}

