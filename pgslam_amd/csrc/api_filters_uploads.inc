// api_filters_uploads.inc -- part of pgicp_api.cpp (one translation unit): input filters on the device, the batched map ABI, diagnostics of the last call, map transfer, uploads.
// the filter list of pgicp_filter_cloud*, checked, as the launcher takes it
// MaxQuantileOnAxis (pgicp_quantile.h): dim in {0, 1, 2}; ratio finite and, as T, in (0, 1)
template <typename T>
bool axis_quantile_args_ok(double dim, double ratio)
{
    const T r = (T)ratio;
    return (dim == 0.0 || dim == 1.0 || dim == 2.0) && std::isfinite(ratio) && r > (T)0 && r < (T)1;
}

// (*n_quantile: the list's MaxQuantileOnAxis entries -- the launcher wants their scratch; *n_cut: its CutAtDescriptor entries
// (pgicp_descriptor_filters.h) -- they read the descriptors, `drows` rows a point, 0: the call has none)
template <typename T>
int filter_specs(pgicp_ctx *c, int nf, const pgicp_filter *f, int drows, int *types, double *params, int *n_quantile, int *n_cut)
{
    *n_quantile = *n_cut = 0;
    for (int k = 0; k < nf; k++) {
        if (f[k].type < PGICP_FILTER_IDENTITY || f[k].type > PGICP_FILTER_CUT_AT_DESCRIPTOR) return fail(c, PGICP_ERR_ARG, "pgicp_filter_cloud: unknown filter type");
        if (f[k].type == PGICP_FILTER_CUT_AT_DESCRIPTOR) {
            if (drows <= 0) return fail(c, PGICP_ERR_ARG, "pgicp_filter_cloud: CutAtDescriptor needs descriptors (this call has none)");
            if (!(f[k].p[0] >= 0.0 && f[k].p[0] < (double)drows && f[k].p[0] == std::floor(f[k].p[0])) || (f[k].p[1] != 0.0 && f[k].p[1] != 1.0))
                return fail(c, PGICP_ERR_ARG, "pgicp_filter_cloud: CutAtDescriptor needs a row in [0, drows) and useLargerThan 0 or 1");
            ++*n_cut;
        }
        if (f[k].type == PGICP_FILTER_MAX_QUANTILE_ON_AXIS) {
            if (!axis_quantile_args_ok<T>(f[k].p[0], f[k].p[1]))
                return fail(c, PGICP_ERR_ARG, "pgicp_filter_cloud: MaxQuantileOnAxis needs dim in {0, 1, 2} and a finite ratio in (0, 1)");
            ++*n_quantile;
        }
        if (f[k].type == PGICP_FILTER_FIX_STEP && !(f[k].p[0] >= 1.0 && f[k].p[0] <= 2147483647.0))
            return fail(c, PGICP_ERR_ARG, "pgicp_filter_cloud: FixStep needs 1 <= step <= INT_MAX");
        if ((f[k].type == PGICP_FILTER_MAX_DIST || f[k].type == PGICP_FILTER_MIN_DIST) &&
            !(f[k].p[1] == 0.0 || f[k].p[1] == 1.0 || f[k].p[1] == 2.0 || f[k].p[1] == 3.0))
            return fail(c, PGICP_ERR_ARG, "pgicp_filter_cloud: Min/MaxDist p[1] must be dim + 1 in {0 (radius), 1, 2, 3}");
        if (f[k].type == PGICP_FILTER_RANDOM_SAMPLING && !(f[k].p[0] >= 0.0 && f[k].p[0] <= 1.0))
            return fail(c, PGICP_ERR_ARG, "pgicp_filter_cloud: RandomSampling needs 0 <= prob <= 1");
        if ((f[k].type == PGICP_FILTER_RANDOM_SAMPLING || f[k].type == PGICP_FILTER_MAX_POINT_COUNT) &&
            !(f[k].p[1] >= 0.0 && f[k].p[1] < 9007199254740992.0 && f[k].p[1] == std::floor(f[k].p[1])))
            return fail(c, PGICP_ERR_ARG, "pgicp_filter_cloud: the sampler's seed must be an integer in [0, 2^53)");
        if (f[k].type == PGICP_FILTER_MAX_POINT_COUNT && !(f[k].p[0] >= 1.0 && f[k].p[0] <= 2147483647.0))
            return fail(c, PGICP_ERR_ARG, "pgicp_filter_cloud: MaxPointCount needs 1 <= maxCount <= INT_MAX");
        types[k] = f[k].type;
        std::memcpy(params + 8 * k, f[k].p, sizeof f[k].p);
        if (f[k].type == PGICP_FILTER_MAX_POINT_COUNT) params[8 * k + 2] = sizeof(T) == 4 ? 1.0 : 0.0;   // prob = T(maxCount) / T(N)
        if (f[k].type == PGICP_FILTER_MAX_QUANTILE_ON_AXIS) params[8 * k + 1] = (double)(T)f[k].p[1];      // (ratio is held as T)
        if (f[k].type == PGICP_FILTER_CUT_AT_DESCRIPTOR) params[8 * k + 2] = (double)(T)f[k].p[2];         // (so is the threshold)
    }
    return PGICP_OK;
}

template <typename T>
int filter_cloud(pgicp_ctx *c, int nf, const pgicp_filter *f, const T *feat, int frows, const T *desc, int drows, int n, const double *T16,
                 int rot0, int rot1, T *out_feat, T *out_desc, int32_t *kept_idx, int *n_out, const T **dev_feat)
{
    if (!c || nf < 0 || nf > PGICP_MAX_FILTERS || (nf && !f) || !feat || frows < 3 || n <= 0 || (desc && drows <= 0) || !out_feat || !n_out ||
        (desc && !out_desc) || (rot0 >= 0 && (!desc || rot0 + 3 > drows)) || (rot1 >= 0 && (!desc || rot1 + 3 > drows)))
        return fail(c, PGICP_ERR_ARG, "pgicp_filter_cloud: bad argument");
    if (T16 && !is_rigid(T16)) return fail(c, PGICP_ERR_NOT_RIGID, "pgicp_filter_cloud: transformation is not rigid");
    int types[PGICP_MAX_FILTERS];
    double params[8 * PGICP_MAX_FILTERS];
    int n_quantile = 0, n_cut = 0;
    { const int st = filter_specs<T>(c, nf, f, desc ? drows : 0, types, params, &n_quantile, &n_cut); if (st) return st; }
    HIPC(c, hipSetDevice(c->device));
    pgicp_ctx::FilterSet &S = c->fset[c->fset_next];
    c->fset_next = (c->fset_next + 1) & 3;
    // Without a transformation (none, or the identity -- a sensor at the robot's origin) the kept points are the input's
    // own: only the features travel (the predicates look at nothing else, and the ICP wants them on the device anyway), and
    // what comes back is the list of kept indices, if anything was dropped at all -- the host copies compact themselves.  (A
    // CutAtDescriptor entry does look at the descriptors: with one they travel to the device in any case.)
    bool ident = T16 == nullptr;
    if (T16) {
        ident = true;
        for (int i = 0; i < 12; i++) ident = ident && T16[i] == (i % 5 == 0 ? 1.0 : 0.0);
    }
    const bool dev_desc = desc && !ident, in_desc = desc && (!ident || n_cut > 0);     // (which descriptors leave the pass; which enter it)
    const size_t bf = sizeof(T) * (size_t)frows * n, bd = dev_desc ? sizeof(T) * (size_t)drows * n : 0;
    HIPC(c, S.in_f.ensure(bf)); HIPC(c, S.out_f.ensure(bf));
    if (in_desc) HIPC(c, S.in_d.ensure(sizeof(T) * (size_t)drows * n));
    if (dev_desc) HIPC(c, S.out_d.ensure(bd));
    HIPC(c, S.keep.ensure(sizeof(int) * ((size_t)n + 1))); HIPC(c, S.pos.ensure(sizeof(int) * ((size_t)n + 1)));
    HIPC(c, S.bsum.ensure(sizeof(int) * scan_scratch_ints(n)));
    AqScratch aq{};
    if (n_quantile) { HIPC(c, S.qsel.ensure(axis_quantile_scratch_bytes(n, sizeof(T)))); aq = axis_quantile_scratch(S.qsel.p, n, sizeof(T)); }
    const bool want_idx = kept_idx || ident;
    if (want_idx) HIPC(c, S.idx.ensure(sizeof(int) * (size_t)n));
    XFER(c, h2d(c, S.in_f.p, feat, bf));
    if (in_desc) XFER(c, h2d(c, S.in_d.p, desc, sizeof(T) * (size_t)drows * n));
    // (without a transformation and without a caller's kept_idx the host side only has to close the gaps of the dropped points: a
    // short ascending list of them comes back with the count -- the kept indices, 4 bytes a point, are fetched only when that
    // list would not hold them)
    constexpr int kDropCap = 4096, kDropHead = 256;
    const bool want_drop = ident && !kept_idx;
    if (want_drop) HIPC(c, S.drop.ensure(sizeof(int) * kDropCap));
    launch_filter_cloud<T>(c->stream, S.in_f.as<T>(), frows, frows, in_desc ? S.in_d.as<T>() : nullptr, drows, n, nf, types, params,
                           ident ? nullptr : T16, rot0, rot1, S.keep.as<int>(), S.pos.as<int>(), S.bsum.as<int>(), S.out_f.as<T>(),
                           dev_desc ? S.out_d.as<T>() : nullptr, want_idx ? S.idx.as<int>() : nullptr, want_drop ? S.drop.as<int>() : nullptr,
                           want_drop ? std::min(kDropCap, n) : 0, n_quantile ? &aq : nullptr);
    int kept = 0;
    int drop_list[kDropCap];
    XFER(c, d2h(c, &kept, S.pos.as<int>() + n, sizeof(int)));
    if (want_drop) XFER(c, d2h(c, drop_list, S.drop.p, sizeof(int) * (size_t)std::min(kDropHead, n)));
    HIPC(c, stream_sync(c));
    HIPC(c, hipGetLastError());
    *n_out = kept;
    if (ident && want_drop && kept < n && n - kept <= std::min(kDropCap, n)) {
        const int nd = n - kept;
        if (nd > kDropHead) { XFER(c, d2h(c, drop_list + kDropHead, S.drop.as<int>() + kDropHead, sizeof(int) * (size_t)(nd - kDropHead))); HIPC(c, stream_sync(c)); }
        // the kept runs between consecutive dropped points, moved as blocks (out may alias the input: towards the front only)
        if (out_feat != feat) std::memcpy(out_feat, feat, sizeof(T) * (size_t)frows * (size_t)drop_list[0]);
        if (desc && out_desc != desc) std::memcpy(out_desc, desc, sizeof(T) * (size_t)drows * (size_t)drop_list[0]);
        int dst = drop_list[0];
        for (int k = 0; k < nd; k++) {
            const int from = drop_list[k] + 1, to = k + 1 < nd ? drop_list[k + 1] : n;
            if (to > from) {
                std::memmove(out_feat + (size_t)dst * frows, feat + (size_t)from * frows, sizeof(T) * (size_t)frows * (size_t)(to - from));
                if (desc) std::memmove(out_desc + (size_t)dst * drows, desc + (size_t)from * drows, sizeof(T) * (size_t)drows * (size_t)(to - from));
                dst += to - from;
            }
        }
    } else if (ident) {
        std::vector<int> hidx;
        const int *idx = nullptr;
        if (kept < n || kept_idx) {
            if (!want_idx) return fail(c, PGICP_ERR_HIP, "pgicp_filter_cloud: internal (kept indices not made)");
            int *dst = kept_idx;
            if (!dst) { hidx.resize((size_t)std::max(kept, 1)); dst = hidx.data(); }
            if (kept > 0) { XFER(c, d2h(c, dst, S.idx.p, sizeof(int) * (size_t)kept)); HIPC(c, stream_sync(c)); }
            idx = dst;
        }
        if (kept == n) {
            if (out_feat != feat) std::memcpy(out_feat, feat, bf);
            if (desc && out_desc != desc) std::memcpy(out_desc, desc, sizeof(T) * (size_t)drows * n);
        } else {
            // (ascending indices: compaction in place moves every point towards the front)
            for (int k = 0; k < kept; k++) {
                std::memmove(out_feat + (size_t)k * frows, feat + (size_t)idx[k] * frows, sizeof(T) * (size_t)frows);
                if (desc) std::memmove(out_desc + (size_t)k * drows, desc + (size_t)idx[k] * drows, sizeof(T) * (size_t)drows);
            }
        }
    } else if (kept > 0) {
        XFER(c, d2h(c, out_feat, S.out_f.p, sizeof(T) * (size_t)frows * kept));
        if (desc) XFER(c, d2h(c, out_desc, S.out_d.p, sizeof(T) * (size_t)drows * kept));
        if (kept_idx) XFER(c, d2h(c, kept_idx, S.idx.p, sizeof(int) * (size_t)kept));
        HIPC(c, stream_sync(c));
    }
    if (dev_feat) *dev_feat = S.out_f.as<T>();
    return PGICP_OK;
}

// pgicp_filter_cloud_dev: the same device pass for a caller that keeps the host side to itself -- no transformation, the
// caller's arrays are not written: the kept count, the device copy of the filtered features, and the ASCENDING indices of the
// dropped points (a range sensor's input filters drop a handful of a scan's points: the caller closes those gaps in its own
// arrays -- while the ICP already runs on the device copy, if it likes)
template <typename T>
int filter_cloud_dev(pgicp_ctx *c, int nf, const pgicp_filter *f, const T *feat, int frows, int n, int32_t *dropped_idx, int dropped_cap,
                     int *n_dropped, int *n_out, const T **dev_feat)
{
    if (!c || nf < 0 || nf > PGICP_MAX_FILTERS || (nf && !f) || !feat || frows < 3 || n <= 0 || !n_out || !n_dropped || dropped_cap < 0 ||
        (dropped_cap && !dropped_idx))
        return fail(c, PGICP_ERR_ARG, "pgicp_filter_cloud_dev: bad argument");
    int types[PGICP_MAX_FILTERS];
    double params[8 * PGICP_MAX_FILTERS];
    int n_quantile = 0, n_cut = 0;
    { const int st = filter_specs<T>(c, nf, f, 0, types, params, &n_quantile, &n_cut); if (st) return st; }
    HIPC(c, hipSetDevice(c->device));
    pgicp_ctx::FilterSet &S = c->fset[c->fset_next];
    c->fset_next = (c->fset_next + 1) & 3;
    const size_t bf = sizeof(T) * (size_t)frows * n;
    const int cap = std::min(dropped_cap, n);
    HIPC(c, S.in_f.ensure(bf)); HIPC(c, S.out_f.ensure(bf));
    HIPC(c, S.keep.ensure(sizeof(int) * ((size_t)n + 1))); HIPC(c, S.pos.ensure(sizeof(int) * ((size_t)n + 1)));
    HIPC(c, S.bsum.ensure(sizeof(int) * scan_scratch_ints(n)));
    AqScratch aq{};
    if (n_quantile) { HIPC(c, S.qsel.ensure(axis_quantile_scratch_bytes(n, sizeof(T)))); aq = axis_quantile_scratch(S.qsel.p, n, sizeof(T)); }
    HIPC(c, S.drop.ensure(sizeof(int) * (size_t)std::max(cap, 1)));
    XFER(c, h2d(c, S.in_f.p, feat, bf));
    launch_filter_cloud<T>(c->stream, S.in_f.as<T>(), frows, frows, nullptr, 0, n, nf, types, params, nullptr, -1, -1, S.keep.as<int>(), S.pos.as<int>(),
                           S.bsum.as<int>(), S.out_f.as<T>(), nullptr, nullptr, cap ? S.drop.as<int>() : nullptr, cap, n_quantile ? &aq : nullptr);
    // the kept count and the head of the dropped list in ONE round trip (a second one only when more than that were dropped)
    int kept = 0;
    const int head = std::min(cap, 256);
    XFER(c, d2h(c, &kept, S.pos.as<int>() + n, sizeof(int)));
    if (head) XFER(c, d2h(c, dropped_idx, S.drop.p, sizeof(int) * (size_t)head));
    HIPC(c, stream_sync(c));
    HIPC(c, hipGetLastError());
    const int nd = n - kept;
    if (nd > head && nd <= cap) { XFER(c, d2h(c, dropped_idx + head, S.drop.as<int>() + head, sizeof(int) * (size_t)(nd - head))); HIPC(c, stream_sync(c)); }
    *n_out = kept;
    *n_dropped = nd;                          // (more than dropped_cap: the list is incomplete -- the caller takes pgicp_filter_cloud)
    if (dev_feat) *dev_feat = S.out_f.as<T>();
    return PGICP_OK;
}

}  // namespace

// ---------------------------------------------------------------------------
// extern "C" surface
// ---------------------------------------------------------------------------
template <typename T>
int map_create_batch_abi(pgicp_ctx *c, int n, const T *const *xyz, const int *xs, const T *const *nrm, const int *ns,
                                const int *m, int mem, int center, int *ids)
{
    if (!c || n <= 0 || !xyz || !xs || !m || !ids || (nrm && !ns)) return fail(c, PGICP_ERR_ARG, "pgicp_map_create_batch: bad argument");
    if (n > 65535) return fail(c, PGICP_ERR_ARG, "pgicp_map_create_batch: at most 65535 clouds per call");
    std::vector<MapSrc<T>> src(n);
    for (int k = 0; k < n; k++) src[k] = MapSrc<T>{xyz[k], xs[k], nrm ? nrm[k] : nullptr, nrm ? ns[k] : 0, m[k]};
    return map_create_batch<T>(c, n, src.data(), mem, center, ids);
}
template <typename T>
int debug_last_matches(pgicp_ctx *c, int problem, int32_t *ids, T *dist2)
{
    if (!c || problem < 0 || !ids || !dist2) return PGICP_ERR_ARG;
    // (the record of `problem` sizes the copies below: an index past the last call's own problems would read a stale one)
    if (problem >= c->last_icp_P) return fail(c, PGICP_ERR_ARG, "pgicp_debug_last_matches: problem " + std::to_string(problem) + " is outside the last call's " + std::to_string(c->last_icp_P));
    HIPC(c, hipSetDevice(c->device));
    State<T> &S = state<T>(c);
    ProblemDev D;
    HIPC(c, hipMemcpy(&D, c->probs.as<ProblemDev>() + problem, sizeof D, hipMemcpyDeviceToHost));
    const size_t np = (size_t)D.n * D.knn;                   // (knn entries per point)
    HIPC(c, c->tmp_a.ensure(sizeof(int) * np));
    HIPC(c, c->tmp_b.ensure(sizeof(T) * np));
    // `order` holds positions in the batch-wide sorted arrays: point the kernel at this problem's slice
    launch_unpermute<T>(c->stream, S.d_maps.template as<MapDev<T>>(), D.map, c->order.as<int>() + D.off,
                        (c->vd.cut_live ? c->vd.slot_cut.as<int>() : S.slot.template as<int>()) + D.off * D.knn,
                        (c->vd.cut_live ? c->vd.d2_cut.as<T>() : S.d2.template as<T>()) + D.off * D.knn, D.n, D.knn, c->tmp_a.as<int>(), c->tmp_b.as<T>());     // (pgicp_vardist.h: an armed call's pairs are the cut ones)
    XFER(c, d2h(c, ids, c->tmp_a.p, sizeof(int) * np));
    XFER(c, d2h(c, dist2, c->tmp_b.p, sizeof(T) * np));
    HIPC(c, stream_sync(c));
    return PGICP_OK;
}

template <typename T>
int map_transfer_impl(pgicp_ctx *from, int id, pgicp_ctx *to, int *new_id)
{
    MapHost<T> *src = get_map<T>(from, id);
    if (!src) return -1;
    hipEvent_t ev;
    HIPC(to, hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    HIPC(to, hipEventRecord(ev, from->stream));
    HIPC(to, hipStreamWaitEvent(to->stream, ev, 0));
    HIPC(to, hipEventDestroy(ev));                 // released once the recorded work has completed
    State<T> &S = state<T>(to);
    int slot = -1;
    for (size_t i = 0; i < S.maps.size(); i++) if (!S.maps[i].used) { slot = (int)i; break; }
    if (slot < 0) { S.maps.push_back(MapHost<T>()); slot = (int)S.maps.size() - 1; }
    S.maps[slot] = *src;
    S.maps[slot].stamp = ++to->map_clock;
    *src = MapHost<T>();                           // ownership of the device block moves with the record
    ++from->map_clock;
    *new_id = slot | id_tag<T>();
    return sync_maps_table<T>(to);
}

namespace {
template <typename T>
int upload(pgicp_ctx *c, int n, const T *const *host, const int *stride, const int *npts, int mem, const T **dev_ptrs)
{
    if (!c || n <= 0 || !host || !stride || !npts || !dev_ptrs || (mem != PGICP_HOST && mem != PGICP_HOST_PINNED))
        return fail(c, PGICP_ERR_ARG, "pgicp_upload: bad argument");
    size_t total = 0;
    for (int k = 0; k < n; k++) {
        if (!host[k] || npts[k] <= 0 || stride[k] < 3) return fail(c, PGICP_ERR_ARG, "pgicp_upload: bad reading " + std::to_string(k));
        total += staged_bytes(sizeof(T), stride[k], npts[k]);
    }
    HIPC(c, hipSetDevice(c->device));
    const int set = c->up_next;                    // flipped only when the upload has been queued completely
    pgicp_ctx::UploadSet &U = c->up[set];
    std::vector<const T *> ptrs((size_t)n);
    // the set is overwritten: the calls that read its last contents must have consumed them (device-side wait), and a
    // transfer out of its pinned staging must have left it (host-side wait: two uploads ago, over long since)
    if (U.has_consumer) HIPC(c, hipStreamWaitEvent(c->copy_stream, U.consumed, 0));
    if (U.pending) HIPC(c, hipEventSynchronize(U.uploaded));
    if (total > U.dev.cap) {
        // growing means freeing (hipFree waits for the device): nothing may still read the old block
        HIPC(c, stream_sync(c));
        HIPC(c, hipStreamSynchronize(c->copy_stream));
        HIPC(c, U.dev.ensure(total));
    }
    if (mem == PGICP_HOST && total > U.pin_cap) {
        if (U.pin) HIPC(c, t_host_free(U.pin));
        U.pin = nullptr; U.pin_cap = 0;
        HIPC(c, t_host_malloc(&U.pin, total + total / 4, hipHostMallocDefault));
        U.pin_cap = total + total / 4;
    }
    size_t off = 0;
    struct Piece { char *dst; const char *src; size_t len; };
    std::vector<Piece> pieces;                     // pageable sources: what goes into the pinned staging buffer
    for (int k = 0; k < n;) {
        const size_t bytes = sizeof(T) * ((size_t)(npts[k] - 1) * stride[k] + 3), slot = staged_bytes(sizeof(T), stride[k], npts[k]);
        // pinned sources of equal size at equal spacing (scans carved out of one pinned block) go as ONE 2-D transfer:
        // a copy command per scan costs the host 10-30 us each, which a batch of 128 scans does not hide
        int run = 1;
        if (mem == PGICP_HOST_PINNED && k + 1 < n && npts[k + 1] == npts[k] && stride[k + 1] == stride[k]) {
            const ptrdiff_t pitch = (const char *)host[k + 1] - (const char *)host[k];
            if (pitch >= (ptrdiff_t)bytes) {
                run = 2;
                while (k + run < n && npts[k + run] == npts[k] && stride[k + run] == stride[k] &&
                       (const char *)host[k + run] - (const char *)host[k + run - 1] == pitch)
                    ++run;
                HIPC(c, hipMemcpy2DAsync((char *)U.dev.p + off, slot, host[k], (size_t)pitch, bytes, (size_t)run, hipMemcpyHostToDevice, c->copy_stream));
            } else
                run = 1;
        }
        if (run == 1) {
            if (mem == PGICP_HOST) {
                const size_t piece = (size_t)1 << 20;
                for (size_t b = 0; b < bytes; b += piece)
                    pieces.push_back({(char *)U.pin + off + b, (const char *)host[k] + b, std::min(piece, bytes - b)});
            } else HIPC(c, hipMemcpyAsync((char *)U.dev.p + off, host[k], bytes, hipMemcpyHostToDevice, c->copy_stream));
        }
        for (int j = 0; j < run; j++) { ptrs[k + j] = (const T *)((char *)U.dev.p + off); off += slot; }
        k += run;
    }
    if (mem == PGICP_HOST) {
        // one core copies 25-30 GB/s, and the caller's thread is the one that drives the ICP iterations: a large batch is
        // staged by a few threads side by side (the sources are the caller's again when this call returns)
        const unsigned hw = std::thread::hardware_concurrency();
        const int workers = total < ((size_t)8 << 20) ? 1 : (int)std::min<size_t>(std::min<unsigned>(hw ? hw : 1, 8u), pieces.size());
        auto stage = [&pieces, workers](int w) {
            for (size_t i = (size_t)w; i < pieces.size(); i += (size_t)workers) std::memcpy(pieces[i].dst, pieces[i].src, pieces[i].len);
        };
        std::vector<std::thread> pool;
        for (int w = 1; w < workers; w++) pool.emplace_back(stage, w);
        stage(0);
        for (auto &t : pool) t.join();
        HIPC(c, hipMemcpyAsync(U.dev.p, U.pin, total, hipMemcpyHostToDevice, c->copy_stream));
    }
    HIPC(c, hipEventRecord(U.uploaded, c->copy_stream));
    U.bytes = total;
    U.pending = true;
    U.has_consumer = false;
    c->up_next = set ^ 1;
    for (int k = 0; k < n; k++) dev_ptrs[k] = ptrs[k];
    return PGICP_OK;
}
}  // namespace


