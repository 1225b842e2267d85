// api_icp.inc -- part of pgicp_api.cpp (one translation unit): the ICP driver: batch layout and set-up, one iteration (also as a captured graph), align_batch, icp_pair.
void translation(const double *t3, double sign, double *T)
{
    mat4_identity(T);
    T[3] = sign * t3[0]; T[7] = sign * t3[1]; T[11] = sign * t3[2];
}

// one reading against one map as a problem record (`T`: its first guess; none: the identity)
static pgicp_problem one_problem(int map_id, const void *reading, int stride, int n, int mem, const double *T)
{
    pgicp_problem pr;
    std::memset(&pr, 0, sizeof pr);
    pr.map_id = map_id; pr.reading = reading; pr.stride = stride; pr.n = n; pr.mem = mem;
    mat4_identity(pr.T_init);
    if (T) std::memcpy(pr.T_init, T, sizeof pr.T_init);
    return pr;
}

// A problem's pre-transform: its first guess, centred on the map's mean (`Tref`, optional: the transform back)
template <typename T>
void centred_pre(const MapHost<T> *M, const double *T_init, double *Tpre, double *Tref = nullptr)
{
    const double mean[3] = {(double)M->mean[0], (double)M->mean[1], (double)M->mean[2]};
    double Tm_inv[16];
    translation(mean, -1.0, Tm_inv);
    if (Tref) translation(mean, +1.0, Tref);
    mat4_mul(Tm_inv, T_init, Tpre);
}

struct BatchLayout {
    int P = 0;
    int max_n = 0;
    int max_rows = 1;
    int bin_shift = 2;          // reading-sort bins are (1 << bin_shift)^3 map cells
    long long total = 0;
    int knn = 1;                // pairs per reading point (ChainDev::knn)
    bool normals = false;       // the readings' normals travel with them (a SurfaceNormalOutlierFilter is in the chain)
    int table_kinds = 0;        // bit 0: some map of the batch carries the dense cell tables, bit 1: some map the succinct one (MapDev::sw)
    double max_h = 0.0;         // largest cell edge among the batch's maps
    // Rings of cells the fast matcher walks beyond the 27-cell block before it queues a query: 3 unseeded / 1 seeded on the 9 cm
    // cells of a 1 M-pt map (measured, rounds 3 and 4); the 28 cm cells of a 100 k-pt keyframe map -- loop closing -- are
    // cheaper to walk than to queue: 5 / 2 there (round 5, tools/r5_lc_knobs.sh: +3...6 %).  The environment knobs override.
    int rings_unseeded = 3, rings_seeded = 1;
    int max_pairs() const { return (int)std::min<long long>((long long)max_n * knn, 0x7FFFFFFFLL); }
};

// Prepare a batch: stage readings, fill + upload ProblemDev, run the prologue
// transform.  `Tpre_of(p, out16)` provides each problem's pre-transform.
// `borrow` (one problem, pgicp_partial_chain_seeded): the reading is NOT sorted by this call's map -- it is taken in the order
// another context sorted the same reading in for ITS map (spatially compact there is spatially compact here: the same space, another
// grid), pre-transformed and seeded in ONE kernel (k_borrow_order) where the sort is seven launches.
struct BorrowSpec {
    const int *order_a, *slot_a; const void *pts_a; SeedSegs sg; const int *slot_of_b; int m_b;
    int first_a, m_a;           // the source map's slots: [first_a, first_a + m_a) of pts_a
    // out: the problem starts with a search cap (ProblemDev::rlimit) taken from the threshold the context's previous call of this
    // kind ended with -- matcher mode 3: seeds from outside AND the capped, lazily exact search of an ICP's later iterations
    mutable bool capped = false;
};
template <typename T, typename F>
int batch_begin(pgicp_ctx *c, int P, const pgicp_problem *pr, F Tpre_of, BatchLayout &L, std::vector<ProblemDev> &hp, int hint_kind = -1,
                const BorrowSpec *borrow = nullptr)
{
    if (P > 65535) return fail(c, PGICP_ERR_ARG, "pgicp: at most 65535 problems per batch (the problem index is a launch-grid dimension)");
    c->vt_last.clear();
    { const int vst = var_trim_check(c); if (vst) return vst; }
    if (c->rx_on) { const int xst = robust_ext_check(c, c->rx); if (xst) return xst; }
    State<T> &S = state<T>(c);
    L.P = P; L.max_n = 0; L.max_rows = 1; L.total = 0; L.table_kinds = 0;
    c->last_icp_P = P;                          // (pgicp_debug_last_matches / _reading_order: the range of their `problem`)
    c->last_n0 = -1;                            // (this call overwrites the correspondences another context might seed from)
    L.knn = std::max(1, c->prm.knn);
    L.normals = c->prm.normal_max_angle > 0.0;
    if (L.normals)
        for (int p = 0; p < P; p++)
            if (!pr[p].normals || pr[p].nstride < 3)
                return fail(c, PGICP_ERR_ARG, "SurfaceNormalOutlierFilter: the reading of problem " + std::to_string(p) + " has no normals (pgicp_problem.normals)");
    size_t stage_total = 0;
    double dens = 0.0;                         // largest reading-to-map size ratio of the batch
    for (int p = 0; p < P; p++) {
        if (pr[p].n <= 0 || !pr[p].reading || pr[p].stride < 3)
            return fail(c, PGICP_ERR_ARG, "pgicp: bad reading in problem " + std::to_string(p));
        MapHost<T> *M = get_map<T>(c, pr[p].map_id);
        if (!M) return fail(c, PGICP_ERR_ARG, "pgicp: unknown map id " + std::to_string(pr[p].map_id));
        { const int gst = descriptor_filter_check<T>(c, M, pr[p].map_id); if (gst) return gst; }
        L.max_n = std::max(L.max_n, pr[p].n);
        L.table_kinds |= M->sw ? 2 : 1;
        L.max_h = std::max(L.max_h, (double)M->g.h);
        dens = std::max(dens, (double)pr[p].n / (double)M->m);
        L.total += pr[p].n;
        if (pr[p].mem == PGICP_HOST) stage_total += staged_bytes(sizeof(T), pr[p].stride, pr[p].n) +
                                                    (L.normals ? staged_bytes(sizeof(T), pr[p].nstride, pr[p].n) : 0);
    }
    L.rings_unseeded = c->fast_rings_unseeded > 0 ? c->fast_rings_unseeded : (L.max_h >= 0.18 ? 5 : 3);
    L.rings_seeded = c->fast_rings_seeded > 0 ? c->fast_rings_seeded : (L.max_h >= 0.18 ? 2 : 1);
    if ((long long)L.max_n * L.knn > 0x7FFFFFF0LL || L.total * L.knn > 0x7FFFFFF0LL)
        return fail(c, PGICP_ERR_ARG, "pgicp: points x knn exceeds 2^31: split the batch");
    // Bins of the reading sort are blocks of map cells.  The rank pass costs O(bin population) per
    // point and map cells hold ~17 points where the data is, so a reading as dense as its map gets
    // single-cell bins and a sparse one 4x4x4-cell bins; the bin table is kept under 2^26 entries.
    L.bin_shift = std::max(0, std::min(4, (dens <= 0.25 ? 2 : (dens <= 2.0 ? 1 : 0)) + c->bin_shift_add));
    for (;; ++L.bin_shift) {
        const int s = L.bin_shift, r = (1 << s) - 1;
        L.max_rows = 1;
        for (int p = 0; p < P; p++) {
            const GridDesc<T> &g = get_map<T>(c, pr[p].map_id)->g;
            const long long rows = (long long)((g.nx + r) >> s) * ((g.ny + r) >> s) * ((g.nz + r) >> s);
            L.max_rows = (int)std::max<long long>(L.max_rows, std::min<long long>(rows, 1LL << 30));
        }
        if (s >= 2 || ((long long)L.max_rows < (1LL << 25) && (long long)L.max_rows * P <= (1LL << 26))) break;
    }
    // (the bin table is indexed with ints on the device)
    if ((long long)L.max_rows * P > 0x7FFFFFFFLL)
        return fail(c, PGICP_ERR_ARG, "pgicp: batch too large for the reading sort (problems x map blocks = " +
                                      std::to_string((long long)L.max_rows * P) + " > 2^31 - 1): split the batch");
    HIPC(c, S.rd_pre.ensure(sizeof(typename Vec4<T>::type) * (size_t)L.total));
    HIPC(c, S.rd_sorted.ensure(sizeof(T) * 3 * (size_t)L.total));
    {
        const size_t nbins = (size_t)P * L.max_rows;
        HIPC(c, c->qrow.ensure(sizeof(int) * (size_t)L.total));
        // (the sort's words; afterwards the selection's key list: one key per PAIR)
        HIPC(c, c->qtmp.ensure(std::max(sizeof(unsigned long long) * (size_t)L.total, sizeof(T) * (size_t)L.total * L.knn)));
        if (c->prm.robust_fct != PGICP_ROBUST_NONE) HIPC(c, c->robust_dev.ensure(sizeof(T) * (size_t)L.total * L.knn));
        if (c->vt_on) HIPC(c, c->vt_keys.ensure(2 * sizeof(T) * (size_t)L.total * L.knn));      // (two key lists: the sort's ping-pong)
        HIPC(c, c->order.ensure(sizeof(int) * (size_t)L.total));
        if (c->prm.sum_order == PGICP_SUM_ORDER_SCAN) HIPC(c, c->scan_pos.ensure(sizeof(int) * (size_t)L.total));
        HIPC(c, c->slow_list.ensure(sizeof(int2) * (size_t)L.total));
        HIPC(c, c->slow_lb.ensure(sizeof(T) * (size_t)L.total));
        HIPC(c, c->slow_ring.ensure(sizeof(int) * (size_t)L.total));
        HIPC(c, c->slow2.ensure(sizeof(int) * (size_t)L.total));
        HIPC(c, c->active.ensure(sizeof(int) * (size_t)P));
        HIPC(c, c->qcounts.ensure(sizeof(int) * nbins));
        HIPC(c, c->qstart.ensure(sizeof(int) * (nbins + 1)));
        HIPC(c, c->qblock.ensure(sizeof(int) * scan_scratch_ints(nbins)));
    }
    HIPC(c, S.slot.ensure(sizeof(int) * (size_t)L.total * L.knn));
    HIPC(c, S.d2.ensure(sizeof(T) * (size_t)L.total * L.knn));
    { const int vst = vardist_begin<T>(c, (size_t)L.total * L.knn); if (vst) return vst; }
    if (L.normals) {
        HIPC(c, S.nrm_pre.ensure(sizeof(typename Vec4<T>::type) * (size_t)L.total));
        HIPC(c, S.nrm_sorted.ensure(sizeof(T) * 3 * (size_t)L.total));
    }
    HIPC(c, S.none_r.ensure(sizeof(T) * (size_t)L.total));
    // (the problem records and the readings' source descriptors share one buffer: one upload -- batch_begin)
    const size_t src_off = (sizeof(ProblemDev) * (size_t)P + 63) & ~(size_t)63;
    HIPC(c, c->probs.ensure(src_off + sizeof(SrcDesc) * (size_t)P));
    HIPC(c, c->partials.ensure(sizeof(double) * (size_t)P * reduce_blocks(L.max_pairs()) * kCovTerms));
    HIPC(c, c->sums.ensure(sizeof(double) * (size_t)P * kCovTerms));
    HIPC(c, c->small.ensure(256));
    HIPC(c, c->sel_tables.ensure(trim_select_table_bytes(P)));
    HIPC(c, c->queue.ensure(knn_queue_bytes(P, L.max_n, sizeof(T))));
    if (stage_total) HIPC(c, S.staging.ensure(stage_total));

    hp.assign(P, ProblemDev());
    std::vector<SrcDesc> &hs = c->h_src;        // context members: they outlive the async uploads below
    hs.assign(P, SrcDesc());
    size_t soff = 0;
    long long off = 0;
    int up_mask = 0;
    for (int p = 0; p < P; p++) {
        const T *d_rd = nullptr;
        if (pr[p].mem == PGICP_DEVICE && (c->up[0].pending || c->up[1].pending)) up_mask |= upload_wait(c, pr[p].reading);
        int st = to_device<T>(c, (const T *)pr[p].reading, pr[p].stride, pr[p].n, pr[p].mem, S.staging, soff, &d_rd);
        if (st) return st;
        if (pr[p].mem == PGICP_HOST) soff += staged_bytes(sizeof(T), pr[p].stride, pr[p].n);
        hs[p].ptr = d_rd; hs[p].stride = pr[p].stride; hs[p].nptr = nullptr; hs[p].nstride = 0;
        if (L.normals) {
            const T *d_nr = nullptr;
            if (pr[p].mem == PGICP_DEVICE && (c->up[0].pending || c->up[1].pending)) up_mask |= upload_wait(c, pr[p].normals);
            st = to_device<T>(c, (const T *)pr[p].normals, pr[p].nstride, pr[p].n, pr[p].mem, S.staging, soff, &d_nr);
            if (st) return st;
            if (pr[p].mem == PGICP_HOST) soff += staged_bytes(sizeof(T), pr[p].nstride, pr[p].n);
            hs[p].nptr = d_nr; hs[p].nstride = pr[p].nstride;
        }
        ProblemDev &D = hp[p];
        std::memset(&D, 0, sizeof D);
        D.map = map_index<T>(c, pr[p].map_id); D.n = pr[p].n; D.off = off; D.knn = L.knn;
        off += pr[p].n;
        if (hint_kind >= 0 && c->sel_hints_on && (int)c->sel_hints[hint_kind].size() == P) std::memcpy(D.qhint, c->sel_hints[hint_kind][(size_t)p].q, sizeof D.qhint);
        if (borrow && D.qhint[0][0] > 0.0) {
            // (what sel_store would have left: the quantile, the threshold the pairs are kept with, what the search must be exact up to)
            const ChainDev<T> chh = chain_of<T>(c, c->prm);
            const double q = D.qhint[1][0] > 0.0 ? D.qhint[1][0] : D.qhint[0][0];
            D.limit = std::min(q * (double)chh.trim_scale, (double)chh.outlier_max_d2);
            // (PGICP_PROBE_CAP_SCALE: the previous probe's threshold times this -- the cap is 1.21 x that; a probe's threshold moves more
            //  from scan to scan than an ICP's from iteration to iteration, and a cap below the new threshold sends every query beyond
            //  it through the queue's paths)
            static const double cap_scale = [] { const char *e = std::getenv("PGICP_PROBE_CAP_SCALE"); const double v = e && *e ? std::atof(e) : 3.0; return v > 0.0 ? v : 3.0; }();      // (measured 1 / 1.5 / 2.5 / 4: profiles/r06_experiments/probe_seeds.txt)
            D.rlimit = std::max(q, D.limit) * cap_scale;
            borrow->capped = true;
        }
        Tpre_of(p, D.Tpre);
        mat4_identity(D.T_iter); mat4_identity(D.T_prev); mat4_identity(D.dT);
        for (int i = 0; i < 12; i++) { D.Tcur[i] = D.T_iter[i]; D.Tcur_f[i] = (float)D.T_iter[i]; }
        checker_init(D.chk);
    }
    // One upload and one kernel set a batch up (round 6; three copies and three memsets before: six launches a call, twelve per
    // scan of the facade, which is bound by its launches at sensor size): the problem records and the source descriptors
    // travel as ONE pinned block into ONE buffer; k_batch_setup writes the identity list of active problems and clears the
    // small counters, the selection tables and the reading sort's bin counts.
    { const int pst = pinned_ensure(c, &c->h_up, &c->h_up_cap, src_off + sizeof(SrcDesc) * (size_t)P); if (pst) return pst; }
    std::memcpy(c->h_up, hp.data(), sizeof(ProblemDev) * (size_t)P);
    std::memcpy(c->h_up + src_off, hs.data(), sizeof(SrcDesc) * (size_t)P);
    HIPC(c, hipMemcpyAsync(c->probs.p, c->h_up, src_off + sizeof(SrcDesc) * (size_t)P, hipMemcpyHostToDevice, c->stream));
    const SrcDesc *src_dev = (const SrcDesc *)((const char *)c->probs.p + src_off);
    std::vector<int> &ident = c->h_ident;
    ident.resize(P);
    std::iota(ident.begin(), ident.end(), 0);
    const bool grid_matcher = c->prm.matcher == PGICP_MATCHER_GRID;
    launch_batch_setup(c->stream, c->active.as<int>(), P, c->small.as<int>(), 64, c->sel_tables.as<int>(), (long long)(trim_select_table_bytes(P) / sizeof(int)),
                       c->qcounts.as<int>(), (long long)P * L.max_rows,
                       grid_matcher ? (int *)c->queue.p : nullptr, grid_matcher ? (long long)knn_queue_counter_words(P) : 0);
    c->counters_clean = 1;
    c->seg_clean = grid_matcher ? 1 : 0;       // (the matcher's segmented queue counters start clean: no memset launch before the first pass)
    {
        ProfScope ps(c, PGICP_PROF_PRETRANSFORM, L.total, P);
        // pre-transform + ordering of each reading by (block of map cells, cell, index), once per scan: waves stay spatially
        // coherent for every iteration
        if (borrow && P == 1 && !L.normals)
            launch_borrow_order<T>(c->stream, c->probs.as<ProblemDev>(), src_dev, borrow->order_a, borrow->slot_a, (const typename Vec4<T>::type *)borrow->pts_a,
                                   borrow->first_a, borrow->m_a, pr[0].n, borrow->sg, borrow->slot_of_b, borrow->m_b, S.rd_sorted.template as<T>(), c->order.as<int>(), S.slot.template as<int>());
        else
        launch_query_sort<T>(c->stream, c->probs.as<ProblemDev>(), src_dev, S.d_maps.template as<MapDev<T>>(),
                             S.rd_pre.template as<typename Vec4<T>::type>(), S.rd_sorted.template as<T>(), c->qrow.as<int>(), c->qtmp.as<unsigned long long>(),
                             c->order.as<int>(), c->qcounts.as<int>(), c->qblock.as<int>(), c->qstart.as<int>(),
                             P, L.max_n, L.max_rows, L.bin_shift, L.normals ? S.nrm_pre.template as<typename Vec4<T>::type>() : nullptr,
                             L.normals ? S.nrm_sorted.template as<T>() : nullptr);
        if (c->prm.sum_order == PGICP_SUM_ORDER_SCAN)
            launch_invert_order(c->stream, c->probs.as<ProblemDev>(), c->order.as<int>(), c->scan_pos.as<int>(), P, L.max_n);
        upload_consumed(c, up_mask);                 // its first kernel is the only one that reads the readings where they lie
        c->up_seen = 0;
    }
    // (no synchronisation here: hp is the caller's, hs / ident are context members, and every caller ends with
    // a stream synchronisation before it returns -- a wait at this point idles the GPU for ~25 us per scan)
    if (const char *e = std::getenv("PGICP_TRACE_ORIG")) {     // diagnostics build: narrate one query of problem 0
        HIPC(c, stream_sync(c));
        std::vector<int> ord(hp[0].n);
        (void)hipMemcpy(ord.data(), c->order.as<int>(), sizeof(int) * ord.size(), hipMemcpyDeviceToHost);
        const int want = std::atoi(e);
        for (int j = 0; j < (int)ord.size(); j++) if (ord[j] == want) { (void)knn_trace_set(j); break; }
    }
    return PGICP_OK;
}

// rings the fast pass of a capped, seeded probe walks before it queues a query (PGICP_PROBE_RINGS; 0: as an unseeded pass)
static int probe_rings(const BatchLayout &L)
{
    static const int v = [] { const char *e = std::getenv("PGICP_PROBE_RINGS"); return e && *e ? std::atoi(e) : 0; }();
    return v > 0 ? v : L.rings_unseeded;
}

// Every device and pinned address the launches of an iteration name, and nothing else.  enqueue_iteration and its stages take their
// addresses from this record only and one_iteration mixes the whole record into the key of a captured iteration: a buffer enters the
// iteration by entering this record, so the key cannot fall behind the launches.  Plain data, zeroed with memset before it is filled
// (padding hashes the same); built behind batch_begin, and again wherever a buffer it names may have been re-`ensure`d.
// The seeding invariant (DESIGN.md, KDTreeVarDistMatcher): `slot` / `d2` / `none_r` are the matcher's own -- they seed its next pass
// and are never written by the cut.  Everything behind the matcher reads `pair_slot` / `pair_d2`: the cut arrays when radii are armed.
template <typename T>
struct IterBufs {
    ProblemDev *probs; const MapDev<T> *maps; const T *rd, *rd_nrm; T *none_r;
    int *slot; T *d2;                                   // the matcher's own
    const int *pair_slot; const T *pair_d2;             // what the consumers read
    int *active, *small, *qcount;                       // qcount: the queue counters (small + 16)
    int2 *slow_list; T *slow_lb; int *slow_ring, *slow2; void *queue;
    int *sel_tables; void *qtmp; double *partials; T *robust_dev;
    void *vt_keys_a, *vt_keys_b;                        // VarTrimmed: the sort's two key lists
    const int *order; const T *radii; const long long *radii_off; int *slot_cut; T *d2_cut;     // armed radii: the cut (order: the tail's too)
    int *h_flag, *stamp_dev;
};
template <typename T>
IterBufs<T> iter_bufs(pgicp_ctx *c, const BatchLayout &L)
{
    State<T> &S = state<T>(c);
    IterBufs<T> B;
    std::memset(&B, 0, sizeof B);
    B.probs = c->probs.as<ProblemDev>(); B.maps = S.d_maps.template as<MapDev<T>>(); B.rd = S.rd_sorted.template as<T>();
    if (L.normals) B.rd_nrm = S.nrm_sorted.template as<T>();
    B.none_r = S.none_r.template as<T>(); B.slot = S.slot.template as<int>(); B.d2 = S.d2.template as<T>();
    B.pair_slot = B.slot; B.pair_d2 = B.d2;
    B.active = c->active.as<int>(); B.small = c->small.as<int>(); B.qcount = B.small + 16;
    B.slow_list = c->slow_list.as<int2>(); B.slow_lb = c->slow_lb.as<T>(); B.slow_ring = c->slow_ring.as<int>(); B.slow2 = c->slow2.as<int>();
    B.queue = c->queue.p; B.sel_tables = c->sel_tables.as<int>(); B.qtmp = c->qtmp.p; B.partials = c->partials.as<double>();
    if (c->prm.robust_fct != PGICP_ROBUST_NONE) B.robust_dev = c->robust_dev.as<T>();
    if (c->vt_on) { B.vt_keys_a = c->vt_keys.p; B.vt_keys_b = (char *)c->vt_keys.p + sizeof(T) * (size_t)L.total * L.knn; }
    B.order = c->order.as<int>();
    if (c->vd.on) {
        B.radii = c->vd.vals.template as<T>(); B.radii_off = c->vd.off_dev.as<long long>();
        B.pair_slot = B.slot_cut = c->vd.slot_cut.as<int>(); B.pair_d2 = B.d2_cut = c->vd.d2_cut.as<T>();
    }
    B.h_flag = c->h_flag; B.stamp_dev = c->stamp_dev;
    return B;
}

// The host-side switches of an iteration, computed once a call; the whole record is part of a captured iteration's key.
struct IterPlan {
    int topk, grid;     // KDTreeMatcher.knn > 1: the top-K matcher finds every pair exactly (no queue, no lazy resolution); the grid matcher (else brute force)
    int vardist;        // KDTreeVarDistMatcher's radii armed (pgicp_vardist.h): the cut behind the matcher
    int robust, gd_soft;        // RobustOutlierFilter; GenericDescriptorOutlierFilter, soft mode
    int exact_all;      // this iteration must resolve every pair exactly
    int n_pairs;        // pairs a problem has at most: what everything behind the matcher is launched over
    int fold_solve;     // one problem: the solve kernel also does the bookkeeping of k_compact_active (one launch less per iteration)
    int robust_phase;   // what the robust scale of THIS iteration takes (RobustPhase; robust_phase_of): the one switch that differs
                        // from iteration to iteration of a call
};
// The launches the robust scale of an iteration needs (pgicp_robust.h).  `it`: the iteration (1, 2, ...) the active problems share -- they
// iterate in lockstep -- or 0: the problems' iterations differ (the residual pass behind a batch of ICPs: each is at its own
// iterations + 1 >= 2: k_reopen reopens only problems whose status is OK, and such a problem has been through at least one solve,
// which counts its iteration -- so none of them is at berg's first iteration, the one that reads the median) and the launches are
// those that any of them may need.  The device decides the rest (k_robust_finish).
template <typename T>
int robust_phase_of(const RobustDev<T> &rb, int it)
{
    if (rb.fct == 0 || rb.est == 0 || (rb.est == 1 && rb.nb == 0)) return kRobustLegacy;
    const bool estimate = rb.nb == 0 || (it > 0 ? it <= rb.nb : rb.nb >= 2);
    if (rb.est == 1) return estimate ? kRobustMad : kRobustHold;
    return it == 1 ? kRobustMedian : kRobustHold;       // (berg: the recurrence of the later iterations reads no distance)
}
template <typename T>
IterPlan iter_plan(const pgicp_ctx *c, const BatchLayout &L, const ChainDev<T> &ch)
{
    IterPlan pl;
    std::memset(&pl, 0, sizeof pl);
    const bool robust = ch.robust.fct != 0, vardist = c->vd.on;
    pl.topk = L.knn > 1; pl.grid = c->prm.matcher == PGICP_MATCHER_GRID; pl.vardist = vardist; pl.robust = robust;
    // RobustOutlierFilter: nothing is trimmed -- the threshold the lazy path resolves queued queries up to is +inf;
    // VarTrimmedDistOutlierFilter: its ratio is chosen over every distance; armed radii: the cut needs every pair under maxDist
    pl.exact_all = robust || ch.var_trim || vardist;
    pl.gd_soft = ch.gd_mode == PGICP_DESC_FILTER_SOFT;
    pl.n_pairs = pl.topk ? L.max_pairs() : L.max_n; pl.fold_solve = L.P == 1 && !pl.topk;
    pl.robust_phase = robust_phase_of(ch.robust, 1);        // (a single pass is iteration 1; align_batch sets it per iteration)
    return pl;
}

// KDTreeVarDistMatcher's cut, behind a matcher pass that resolved every pair of the active problems exactly
template <typename T>
void cut_pairs(pgicp_ctx *c, const IterBufs<T> &B, int nA, int n_pairs)
{
    launch_vardist_cut<T>(c->stream, B.probs, B.active, nA, n_pairs, B.slot, B.d2, B.order, B.radii, B.radii_off, B.slot_cut, B.d2_cut);
}

// the queue a fast pass left: the medium pass (`med`), then the wave-per-query pass
template <typename T>
void resolve_queue(pgicp_ctx *c, const ChainDev<T> &ch, const IterBufs<T> &B, bool med, int use_seed, int exact_all)
{
    if (med) launch_knn_med<T>(c->stream, B.probs, B.maps, B.rd, B.slot, B.d2, ch, B.qcount, B.slow_list, B.slow_lb, B.slow_ring, B.slow2,
                               c->med_rings, (use_seed == 1 || use_seed == 3) ? 1 : 0, B.none_r);
    launch_knn_slow<T>(c->stream, B.probs, B.maps, B.rd, B.slot, B.d2, ch, B.qcount, B.slow_list, B.slow_lb, B.slow2, exact_all, B.none_r);
}

// The matcher stage: the top-K launch, or the fast pass, the first selection, the opens, the medium and slow resolution and the
// re-selection.  `stage`: see enqueue_iteration.  Returns launch_knn_topk's status (0 otherwise).
// `partial` (run_partial: the matcher's public output, no outlier filter behind it): the fast pass clears the queue counters itself
// and leaves them for pgicp_debug_counters, every queued query is resolved exactly at once (no medium pass), nothing is selected.
// use_seed: 0 no correspondences to start from, 1 the previous iteration's (with its threshold as search cap and its proven-empty
// radii), 2 seeds from outside (pgicp_partial_chain_seeded): candidates only, no history, 3 the same with a search cap from
// the threshold of the context's previous call (BorrowSpec::capped)
template <typename T>
int matcher_stage(pgicp_ctx *c, const BatchLayout &L, const ChainDev<T> &ch, const IterBufs<T> &B, const IterPlan &pl, int nA,
                  long long units, long long problems, int use_seed, int stage, bool partial = false)
{
    if (pl.topk) {
        ProfScope ps(c, PGICP_PROF_KNN_GRID, units, problems);
        return launch_knn_topk<T>(c->stream, B.probs, B.maps, B.rd, B.slot, B.d2, ch, nA, L.max_n, B.active);
    }
    if (stage != 2) {
        ProfScope ps(c, pl.grid ? PGICP_PROF_KNN_GRID : PGICP_PROF_KNN_BRUTE, units, problems);
        if (!partial && use_seed != 1 && pl.grid) ps.also(PGICP_PROF_KNN_GRID_UNSEEDED);
        launch_knn<T>(c->stream, pl.grid ? PGICP_MATCHER_GRID : PGICP_MATCHER_BRUTE, B.probs, B.maps, B.rd, B.slot, B.d2, ch, nA, L.max_n, use_seed,
                      B.qcount, B.slow_list, B.slow_lb, B.slow_ring, use_seed == 1 ? L.rings_seeded : use_seed == 3 ? probe_rings(L) : L.rings_unseeded,
                      B.active, B.none_r, L.P, B.queue, (partial || !c->seg_clean) ? 1 : 0, L.table_kinds);
        c->counters_clean = 0;                 // (partial, pgicp_debug_counters: this pass's queue counters, not the copy batch_begin cleared)
        if (partial) {
            c->seg_clean = 0;
            if (pl.grid) resolve_queue<T>(c, ch, B, false, use_seed, 1);
            return 0;
        }
    }
    if (stage == 1) return 0;
    {
        ProfScope ps(c, PGICP_PROF_TRIM, units, problems);
        // (with the grid matcher this selection also clears the matcher's segmented queue counters for the next iteration; under
        //  VarTrimmed that -- and far_mode -- is all it is for: k_robust_open and the second == 2 selection overwrite its threshold.
        //  A cheaper counter clear would spare one selection an iteration there; the TrimmedDist path is left as it is)
        // (every selection but a run's first starts from the last one's result, ProblemDev::qraw; a run's first from the previous
        //  call's, ::qhint, if there is one)
        launch_trim_select<T>(c->stream, B.probs, B.d2, ch, nA, L.max_n, 0, B.active, B.sel_tables, B.qtmp, pl.grid ? (int *)B.queue : nullptr,
                              pl.exact_all ? 0 : (use_seed == 1 || c->sel_guess_first));
        c->seg_clean = pl.grid ? 1 : 0;
    }
    if (pl.exact_all) launch_robust_open(c->stream, B.probs, B.active, nA);
    // GenericDescriptorOutlierFilter, soft mode: its maximum covers every pair with a neighbour -- the same, and (no Robust /
    // VarTrimmed filter to set it) the second selection below must then restore the iteration's threshold
    if (pl.gd_soft && !pl.exact_all && pl.grid) launch_gd_open(c->stream, B.probs, B.active, nA);
    if (!pl.grid) return 0;
    // lazy resolution: only queued queries whose lower bound is within the threshold just selected (an upper bound of the final
    // one) are searched exactly; then the threshold is re-selected if anything changed.  Kept pairs / threshold / n_finite stay exact.
    {
        ProfScope ps(c, PGICP_PROF_KNN_SLOW, units, problems);
        resolve_queue<T>(c, ch, B, true, use_seed, 0);
        static const bool each_pass = std::getenv("PGICP_PHASE_EACH_PASS") != nullptr;     // diagnostics builds only
        if (each_pass) {
            unsigned long long ph[48];
            (void)stream_sync(c);
            (void)knn_xcc_report(use_seed, 1);
            if (knn_phase_read(ph, 1) == 0)
                std::fprintf(stderr, "    pass (seeded %d): wave-per-query kernel entries=%llu, longest wave %llu, longest entry %llu cycles; per entry: walk %.0f\n",
                             use_seed, ph[46], ph[44], ph[45], (double)ph[36] / (double)std::max<unsigned long long>(1ULL, ph[46]));
        }
    }
    ProfScope ps(c, PGICP_PROF_TRIM, 0, 0);
    if (!pl.exact_all) launch_trim_select<T>(c->stream, B.probs, B.d2, ch, nA, L.max_n, 1, B.active, B.sel_tables, B.qtmp, nullptr, 1);
    return 0;
}

// Everything behind the matcher, for both matchers: the armed-radii cut, the VarTrimmed ratio and selection, the robust scale, the
// soft descriptor maximum, the reduce and the solve.  Every pair is exact here.
// One ProfScope is one counted entry of profile(): the top-K path has ONE PGICP_PROF_TRIM scope round the parts before the reduce (its
// only selection is among them, with the iteration's units); the grid path one for each part that runs, without units.
template <typename T>
void pairs_stage(pgicp_ctx *c, const BatchLayout &L, const ChainDev<T> &ch, const IterBufs<T> &B, const IterPlan &pl, int nA,
                 long long units, long long problems, int use_seed, bool with_solve)
{
    auto select = [&](int second, int guess) {
        launch_trim_select<T>(c->stream, B.probs, B.pair_d2, ch, nA, pl.n_pairs, second, B.active, B.sel_tables, B.qtmp, nullptr, guess);
    };
    auto part = [&](bool on, auto body) {
        if (!on) return;
        if (pl.topk) { body(); return; }
        ProfScope ps(c, PGICP_PROF_TRIM, 0, 0);
        body();
    };
    {
        std::optional<ProfScope> all;
        if (pl.topk) all.emplace(c, PGICP_PROF_TRIM, units, problems);
        part(pl.vardist, [&] {
            cut_pairs<T>(c, B, nA, pl.n_pairs);
            // the grid path, no Robust or VarTrimmed filter to do it below: the quantile filter's selection over the cut distances (a
            // first selection without a guess, as RobustOutlierFilter's own), and the search cap lifted again for the next matcher
            // pass: a threshold over cut distances says nothing about the search
            if (!pl.topk && !pl.robust && !ch.var_trim) { select(0, 0); launch_vardist_reset(c->stream, B.probs, B.active, nA); }
        });
        part(ch.var_trim, [&] {                 // the ratio of this iteration, then the selection at that ratio
            launch_var_trim<T>(c->stream, B.probs, B.pair_d2, B.active, nA, B.vt_keys_a, B.vt_keys_b, ch.vt_min, ch.vt_max, ch.vt_lambda);
            select(2, 0);
        });
        part(pl.topk && !ch.var_trim, [&] { select(0, use_seed); });     // (top-K: the iteration's one selection, over the knn * N distances)
        // the scale of this iteration from the distances: median, absolute deviations, their median
        // (with pgicp_robust.h's scale settings every selection is an entry of its own, and so is the finish: an iteration that holds
        //  the scale shows in the profile as the one that spares them)
        auto scale = [&](int piece) { launch_robust_scale<T>(c->stream, B.probs, B.pair_d2, B.robust_dev, ch, nA, pl.n_pairs, B.active, B.sel_tables, B.qtmp, pl.robust_phase, piece); };
        part(pl.robust && pl.robust_phase == kRobustLegacy, [&] { scale(-1); });
        part(pl.robust && (pl.robust_phase == kRobustMad || pl.robust_phase == kRobustMedian), [&] { scale(0); });
        part(pl.robust && pl.robust_phase == kRobustMad, [&] { scale(1); });
        part(pl.robust && pl.robust_phase != kRobustLegacy, [&] { scale(2); });
        part(pl.gd_soft, [&] { launch_gd_max<T>(c->stream, B.probs, B.maps, B.pair_slot, nA, pl.n_pairs, B.active); });      // the soft maximum of this iteration
    }
    {
        ProfScope ps(c, PGICP_PROF_REDUCE, units, problems);
        launch_reduce<T>(c->stream, B.probs, B.maps, B.rd, B.rd_nrm, B.pair_slot, B.pair_d2, B.partials, nA, pl.n_pairs, B.active, ch);
    }
    if (!with_solve) return;
    ProfScope ps(c, PGICP_PROF_SOLVE, units, problems);
    const bool fold = pl.fold_solve;
    launch_solve<T>(c->stream, B.probs, B.partials, ch, B.small, nA, pl.n_pairs, B.active, fold ? B.h_flag : nullptr, fold ? B.stamp_dev : nullptr,
                    fold ? B.qcount : nullptr);
    if (!fold) launch_compact_active(c->stream, B.probs, L.P, B.active, B.h_flag, B.stamp_dev, B.qcount);
}

// One iteration of the problems still iterating: `active` lists them first (k_compact_active), act_probs of them.
// `stage`: 0 the whole iteration; 1 only its matcher pass (fast kernel + queue compaction); 2 everything but that pass -- the
// driver of a single problem enqueues the NEXT iteration's matcher pass before it knows whether there is a next iteration
// (align_batch: every kernel leaves at once for a problem that is done), so that the device does not wait for the host's
// look at the convergence flag: a round trip per iteration, and at one problem per launch the matcher pass is all latency.
template <typename T>
void enqueue_iteration(pgicp_ctx *c, const BatchLayout &L, const ChainDev<T> &ch, const IterBufs<T> &B, const IterPlan &pl, bool with_solve,
                       long long act_units, long long act_probs, int use_seed, int stage = 0)
{
    (void)matcher_stage<T>(c, L, ch, B, pl, (int)act_probs, act_units, act_probs, use_seed, stage);
    if (stage != 1) pairs_stage<T>(c, L, ch, B, pl, (int)act_probs, act_units, act_probs, use_seed, with_solve);
}

// One ICP iteration.  For a batch of a few problems (a streamed scan, a SLAM front end) -- a chain of ten small launches --
// the sequence can be captured once per shape into a hipGraph and replayed (PGICP_GRAPH_MAX_P = largest such batch).
// Everything a kernel argument depends on is in the key; a context keeps the eight graphs used last.  OFF by default:
// built, parity-green (74 GPU tests with it on) and measured on ROCm 7.2 / MI355X -- 4 725 replays in a 1 500-scan SLAM
// run, 860-990 scans/s with and without, streaming 1 066 vs 1 103: hipGraphLaunch of ten kernel nodes costs the host and
// the GPU what ten launches cost there, and the workloads are not bound by launching (GPU 52 % busy in the SLAM run; the
// rest is host logic between ICP calls).
template <typename T>
void one_iteration(pgicp_ctx *c, const BatchLayout &L, const ChainDev<T> &ch, const IterBufs<T> &B, const IterPlan &pl, bool with_solve,
                   long long act_units, long long act_probs, int use_seed, int stage = 0)
{
    if (stage == 1) { enqueue_iteration<T>(c, L, ch, B, pl, with_solve, act_units, act_probs, use_seed, 1); return; }     // (the matcher pass ahead of its iteration)
    const bool want_graph = stage == 0 && L.P <= c->graph_max_problems && !c->prof_on && c->graph_failures < 3;
    bool done = false;
    if (want_graph) {
        // FNV-1a over the argument values: shapes, chain parameters, the plan's switches, and the record of every address the launches name
        unsigned long long key = 1469598103934665603ULL;
        auto mix = [&key](const void *p, size_t n) { const unsigned char *b = (const unsigned char *)p; for (size_t i = 0; i < n; i++) { key ^= b[i]; key *= 1099511628211ULL; } };
        // (sel_guess_first decides the `guess` argument of the iteration's first selection launch: the hinted and the
        //  unhinted first iteration are different graphs)
        const int shape[14] = {(int)sizeof(T), L.P, (int)act_probs, L.max_n, use_seed, with_solve ? 1 : 0, c->med_rings, L.rings_seeded,
                               L.rings_unseeded, c->prm.matcher, c->seg_clean, c->sel_guess_first, c->sel_hints_on, L.table_kinds};
        mix(shape, sizeof shape);
        mix(&ch, sizeof ch);
        mix(&pl, sizeof pl);
        mix(&B, sizeof B);
        pgicp_ctx::IterGraph *g = nullptr;
        for (auto &e : c->iter_graphs) if (e.exec && e.key == key) { g = &e; break; }
        if (!g) {
            hipGraph_t graph = nullptr;
            hipGraphExec_t exec = nullptr;
            bool ok = hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal) == hipSuccess;
            if (ok) {
                enqueue_iteration<T>(c, L, ch, B, pl, with_solve, act_units, act_probs, use_seed);
                ok = hipStreamEndCapture(c->stream, &graph) == hipSuccess && graph != nullptr;
            }
            if (ok) ok = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0) == hipSuccess;
            if (graph) (void)hipGraphDestroy(graph);
            if (ok) {
                if (c->iter_graphs.size() < 8) { c->iter_graphs.push_back(pgicp_ctx::IterGraph()); g = &c->iter_graphs.back(); }
                else {
                    g = &c->iter_graphs[0];
                    for (auto &e : c->iter_graphs) if (e.used < g->used) g = &e;
                    if (g->exec) (void)hipGraphExecDestroy(g->exec);
                }
                g->key = key; g->exec = exec;
                c->graph_captures++;
            } else {
                (void)hipGetLastError();
                c->graph_failures++;
            }
        }
        if (g) {
            g->used = ++c->graph_clock;
            if (hipGraphLaunch(g->exec, c->stream) == hipSuccess) { done = true; c->graph_launches++; }
            else { (void)hipGetLastError(); c->graph_failures++; }
        }
    }
    if (!done) enqueue_iteration<T>(c, L, ch, B, pl, with_solve, act_units, act_probs, use_seed, stage);
    c->counters_clean = with_solve ? 1 : 0;      // k_compact_active clears the matcher's queue counters
    c->seg_clean = pl.grid ? 1 : 0;    // (a replayed graph did not pass through enqueue_iteration)
    if (with_solve) ++c->flag_stamp;
}

// every problem of the batch carries a hint for the first selection of its first pass
static bool hints_cover_first(const std::vector<ProblemDev> &hp)
{
    for (const ProblemDev &D : hp) if (!(D.qhint[0][0] > 0.0)) return false;
    return !hp.empty();
}
// The end of a batched call: the problem records into pinned memory, the wait for the stream, the records into `hp`.  `behind`: what
// the call still enqueues between the copy and the wait (align_batch's residual pass overwrites what the stats report).  Then
// what this call's selections found becomes the next call's hints of its kind (problem by problem; a call with another number of
// problems starts over), and pgicp_last_var_trim_ratio's answers the tuned ratio of every problem's last iteration (the chain has no
// VarTrimmed filter: none).
template <typename F = int (*)()>
int batch_download(pgicp_ctx *c, int P, std::vector<ProblemDev> &hp, int hint_kind, F behind = [] { return (int)PGICP_OK; })
{
    { const int pst = pinned_ensure(c, &c->h_down, &c->h_down_cap, sizeof(ProblemDev) * (size_t)P); if (pst) return pst; }
    HIPC(c, hipMemcpyAsync(c->h_down, c->probs.p, sizeof(ProblemDev) * P, hipMemcpyDeviceToHost, c->stream));
    XFER(c, behind());
    HIPC(c, stream_sync(c));
    HIPC(c, hipGetLastError());
    std::memcpy(hp.data(), c->h_down, sizeof(ProblemDev) * (size_t)P);
    std::vector<pgicp_ctx::SelHint> &H = c->sel_hints[hint_kind];
    H.resize(hp.size());
    for (size_t p = 0; p < hp.size(); p++) std::memcpy(H[p].q, hp[p].qrec, sizeof H[p].q);
    c->vt_last.clear();
    if (c->vt_on) for (const ProblemDev &D : hp) c->vt_last.push_back(D.vt_ratio);
    return PGICP_OK;
}

// number of finished problems after the iteration just enqueued (its k_compact_active carries c->flag_stamp)
// (`behind`: iterations enqueued AFTER the one waited for -- a single problem's look-ahead iteration; the flag may then already
//  carry a later stamp: "done" is sticky, a later look is as good)
static int wait_iteration_flag(pgicp_ctx *c, int behind = 0)
{
    const int want = c->flag_stamp - behind;
    const auto t0 = std::chrono::steady_clock::now();
    for (int spin = 0;; ++spin) {
        if ((int)(__atomic_load_n(&c->h_flag[1], __ATOMIC_ACQUIRE) - want) >= 0 &&
            (int)(__atomic_load_n(&c->h_flag[1], __ATOMIC_ACQUIRE) - c->flag_stamp) <= 0) return __atomic_load_n(&c->h_flag[0], __ATOMIC_RELAXED);
        if ((spin & 63) == 63) {
            const auto us = std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count();
            if (us > c->poll_us) break;
            std::this_thread::yield();
        }
    }
    if (stream_sync(c) != hipSuccess) { fail(c, PGICP_ERR_HIP, "pgicp: stream synchronisation failed"); return -1; }
    if (__atomic_load_n(&c->h_flag[1], __ATOMIC_ACQUIRE) != c->flag_stamp) {
        // a launch failed somewhere: the device's stamp and the host's are out of step.  Take the device's, so that the
        // context's NEXT call can work again instead of timing out for ever.
        int dev_stamp = 0;
        if (hipMemcpy(&dev_stamp, c->stamp_dev, sizeof(int), hipMemcpyDeviceToHost) == hipSuccess) c->flag_stamp = dev_stamp;
        fail(c, PGICP_ERR_HIP, "pgicp: iteration flag not written");
        return -1;
    }
    return __atomic_load_n(&c->h_flag[0], __ATOMIC_RELAXED);
}

// `residual` / `res_ratio` / `res_status` (optional, P entries each): after the ICP, LoopCloser::ComputeResidualError's chain
// on the result (LoopCloser.hpp:343-365) -- see pgicp_align_residual_batch_*.
template <typename T>
int align_batch(pgicp_ctx *c, int P, const pgicp_problem *pr, double *T_out, pgicp_stats *stats, double *residual = nullptr,
                double *res_ratio = nullptr, int *res_status = nullptr)
{
    const bool noisy = noise_take(c);            // (pgicp_arm_reading_noise: one-shot, consumed here whatever follows)
    VarDistCall radii(c);                        // (pgicp_arm_reading_radii: the same)
    if (!c || P <= 0 || !pr || !T_out) return fail(c, PGICP_ERR_ARG, "pgicp_align_batch: bad argument");
    if (noisy) { const int nst = noise_check<T>(c, P, pr); if (nst) return nst; }
    { const int rst = radii.template check<T>(P, pr); if (rst) return rst; }
    HIPC(c, hipSetDevice(c->device));
    State<T> &S = state<T>(c);
    const pgicp_params &prm = c->prm;
    std::vector<std::vector<double>> Tref(P, std::vector<double>(16));
    BatchLayout L;
    std::vector<ProblemDev> hp;
    for (int p = 0; p < P; p++) {
        MapHost<T> *M = get_map<T>(c, pr[p].map_id);
        if (!M) return fail(c, PGICP_ERR_ARG, "pgicp_align: unknown map id");
        if (!M->has_nrm && needs_ref_normals(prm))
            return fail(c, PGICP_ERR_ARG, "pgicp_align: reference has no normals descriptor");
        if (!M->has_nrm && robust_plane_dist(c))
            return fail(c, PGICP_ERR_ARG, "RobustOutlierFilter: distanceType point2plane, and the map of problem " + std::to_string(p) + " has no normals");
    }
    static const bool host_timing = std::getenv("PGICP_HOST_TIMING") != nullptr;      // diagnostics
    const auto ht0 = std::chrono::steady_clock::now();
    int st = batch_begin<T>(c, P, pr, [&](int p, double *Tpre) { centred_pre(get_map<T>(c, pr[p].map_id), pr[p].T_init, Tpre, Tref[p].data()); }, L, hp, 0);
    if (st) return st;
    const IterBufs<T> B = iter_bufs<T>(c, L);
    const bool hint_first = hints_cover_first(hp);
    long long total_m = 0;                       // (profile only) reference points over the batch's problems
    if (c->prof_on) for (int p = 0; p < P; p++) total_m += get_map<T>(c, pr[p].map_id)->m;
    const auto ht1 = std::chrono::steady_clock::now();
    const ChainDev<T> ch = chain_of<T>(c, prm);
    const IterPlan pl = iter_plan(c, L, ch);
    // (the plan of iteration `at`, 1-based: the robust scale's launches are the one switch that moves with the iteration)
    auto plan_at = [&](int at) { IterPlan q = pl; q.robust_phase = robust_phase_of(ch.robust, at); return q; };
    const int every = std::max(1, prm.check_every);
    // active-problem accounting for the profile: exact when check_every == 1 and all
    // readings have the same size (the benchmark's case), an upper bound otherwise
    int n_done = 0;
    // One problem: the next iteration's matcher pass is enqueued BEHIND this iteration, before the host has seen the convergence
    // flag (enqueue_iteration's `stage`): when the problem turns out done the pass's kernels leave at once (three empty launches
    // before the covariance pass), otherwise the device went straight on instead of idling through the host's round trip.
    // PGICP_SPECULATE=0: off.  (Batches: the gap is ~1 % of an iteration there, and the active list changes under the pass.)
    static const int spec_knob = [] { const char *e = std::getenv("PGICP_SPECULATE"); return e && *e ? std::atoi(e) : -1; }();
    // (unset / 1: the next iteration's matcher pass runs ahead; 2: the whole next iteration -- a converged run then pays ten empty launches,
    //  measured no better than 0 on 10 k-pt scans and worse on 100 k-pt ones: profiles/r06_experiments/facade_knobs.txt; 0: off)
    const bool spec_ok = P == 1 && L.knn == 1 && every == 1 && prm.matcher == PGICP_MATCHER_GRID && c->graph_max_problems == 0;
    const int ahead_mode = !spec_ok ? 0 : spec_knob >= 0 ? std::min(spec_knob, 2) : 1;
    bool ahead = false;                          // this iteration (mode 2) / its matcher pass (mode 1) is on the stream already
    size_t ahead_events = 0;                     // profile events of what was enqueued ahead start here
    for (int it = 0; it < prm.max_iters; it++) {
        const long long act_p = P - n_done;
        c->prof_next_m = total_m * act_p / P;
        if (!(ahead && ahead_mode == 2)) {
            c->sel_guess_first = it == 0 && hint_first ? 1 : 0;
            one_iteration<T>(c, L, ch, B, plan_at(it + 1), true, L.total * act_p / P, act_p, it > 0 ? 1 : 0, ahead ? 2 : 0);
            c->sel_guess_first = 0;
        }
        ahead = false;
        if (ahead_mode && it + 1 < prm.max_iters) {
            if (c->prof_on) { std::lock_guard<std::mutex> lock(c->prof_m); ahead_events = c->prof_events.size(); }
            one_iteration<T>(c, L, ch, B, plan_at(it + 2), true, L.total, 1, 1, ahead_mode == 1 ? 1 : 0);
            ahead = true;
        }
        if ((it + 1) % every == 0 || it + 1 == prm.max_iters) {
            // k_compact_active stores {problems done, stamp} straight into pinned host memory: polling it spares
            // the copy and the wake-up of a blocking wait (30-40 us of idle GPU per iteration of a single scan)
            int got = wait_iteration_flag(c, ahead && ahead_mode == 2 ? 1 : 0);
            if (got < 0) return PGICP_ERR_HIP;
            n_done = got;
            if (n_done >= P) {
                if (ahead) {
                    // what was enqueued ahead found its problem done: not part of the profile
                    c->counters_clean = 1;
                    if (c->prof_on) {
                        std::lock_guard<std::mutex> lock(c->prof_m);
                        for (size_t e = std::min(ahead_events, c->prof_events.size()); e < c->prof_events.size(); e++) { c->prof_events[e].kid = -1; c->prof_events[e].kid2 = -1; }
                    }
                }
                break;
            }
        }
    }
    const auto ht2 = std::chrono::steady_clock::now();
    std::vector<char> nres;                   // {S, nb} of every problem (2 P doubles), then the P counts: one copy
    if (noisy) {
        // getOverlap()'s sensor-noise branch over the last error elements (pgicp_noise.h): here, between the last iteration and
        // the residual pass, which overwrites the correspondences and the threshold.  {S, nb} per problem, then the counts.
        pgicp_ctx::Noise &N = c->noise;
        const size_t cnt_off = sizeof(double) * 2 * (size_t)P;
        HIPC(c, N.out.ensure(cnt_off + sizeof(int) * (size_t)P));
        HIPC(c, N.dist.ensure(sizeof(T) * (size_t)L.total * L.knn));
        HIPC(c, hipMemsetAsync((char *)N.out.p + cnt_off, 0, sizeof(int) * (size_t)P, c->stream));
        launch_noise_overlap<T>(c->stream, B.probs, B.maps, B.rd, B.rd_nrm, B.pair_slot, B.pair_d2, B.order, N.vals.template as<T>(),
                                N.off_dev.as<long long>(), N.dist.template as<T>(), B.partials, N.out.as<double>(),
                                (int *)((char *)N.out.p + cnt_off), P, L.max_pairs(), ch);
        nres.resize(cnt_off + sizeof(int) * (size_t)P);
        XFER(c, d2h(c, nres.data(), N.out.p, nres.size()));
    }
    const bool with_cov = prm.error_minimizer != PGICP_MINIMIZER_POINT_TO_POINT;      // (PointToPoint: the base class's zeros; its WithCov form: the same Censi estimate)
    if (with_cov) {
        ProfScope ps(c, PGICP_PROF_COV, L.total, P);
        launch_cov<T>(c->stream, B.probs, B.maps, B.rd, B.rd_nrm, B.pair_slot, B.pair_d2, B.partials, c->sums.as<double>(), P, L.max_pairs(), ch);
    } else HIPC(c, hipMemsetAsync(c->sums.p, 0, sizeof(double) * (size_t)P * kCovTerms, c->stream));
    std::vector<double> cs((size_t)P * kCovTerms), rsys;
    st = batch_download(c, P, hp, 0, [&]() -> int {
        XFER(c, d2h(c, cs.data(), c->sums.p, sizeof(double) * cs.size()));
        if (!residual && !res_ratio && !res_status) return PGICP_OK;
        // The residual check of the result: one more pass of the chain WITHOUT a solve, with the final transform (it is in
        // ProblemDev::Tcur) -- transform, match, outlier weights, error elements.  The pass is SEEDED with the last
        // iteration's correspondences, which the final increment (below the convergence thresholds) hardly moves: as a
        // separate, unseeded chain it cost a fifth of a loop-closure batch.  Seeds are candidates only: the matches are exact.
        launch_reopen(c->stream, B.probs, P);
        XFER(c, h2d(c, B.active, c->h_ident.data(), sizeof(int) * P));
        c->prof_next_m = total_m;
        one_iteration<T>(c, L, ch, B, plan_at(0), false, L.total, P, 1);
        HIPC(c, c->sums2.ensure(sizeof(double) * (size_t)P * kSys));
        launch_sum_partials(c->stream, B.partials, reduce_blocks(L.max_pairs()), kSys, B.probs, 0, c->sums2.as<double>(), P);
        rsys.resize((size_t)P * kSys);
        XFER(c, d2h(c, rsys.data(), c->sums2.p, sizeof(double) * rsys.size()));
        return PGICP_OK;
    });
    if (st) return st;
    if (noisy) {
        pgicp_ctx::Noise &N = c->noise;
        N.last_P = P;
        N.last_overlap.assign(P, 0.0); N.last_nb.assign(P, 0); N.last_ok.assign(P, 0);
        for (int p = 0; p < P; p++) {
            // (a problem without noise, or one that failed, wrote no partials: its sums are not looked at)
            if (N.off[p] < 0 || hp[p].status != PGICP_ST_OK) continue;
            double kept;
            int cnt;
            std::memcpy(&kept, nres.data() + sizeof(double) * (2 * (size_t)p + 1), sizeof kept);
            std::memcpy(&cnt, nres.data() + sizeof(double) * 2 * (size_t)P + sizeof(int) * (size_t)p, sizeof cnt);
            const int nb = (int)kept;                     // (a count of pairs, exact in a double)
            if (nb <= 0) continue;
            N.last_ok[p] = 1;
            N.last_nb[p] = nb;
            N.last_overlap[p] = (double)((T)cnt / (T)nb);
        }
    }
    for (int p = 0; p < P && !rsys.empty(); p++) {
        const double *rs = rsys.data() + (size_t)p * kSys;
        const bool ok = hp[p].status == PGICP_ST_OK && rs[28] > 0.0;
        if (res_status) res_status[p] = ok ? PGICP_OK : PGICP_ERR_NO_MATCH;
        if (res_ratio) res_ratio[p] = ok ? rs[27] / ((double)pr[p].n * L.knn) : 0.0;
        if (residual) residual[p] = ok ? rs[29] : std::numeric_limits<double>::infinity();
    }
    // (pgicp_partial_chain_seeded may read problem 0's correspondences: knn slots per point, of the map that carries this stamp)
    c->last_n0 = pr[0].n; c->last_map0 = map_index<T>(c, pr[0].map_id); c->last_elem = (int)sizeof(T); c->last_knn = L.knn;
    c->last_stamp0 = c->last_map0 >= 0 ? S.maps[c->last_map0].stamp : 0;
    if (host_timing) {
        const auto ht3 = std::chrono::steady_clock::now();
        auto ms = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
        std::fprintf(stderr, "align_batch P=%d: begin %.2f ms, iterations %.2f ms, tail %.2f ms\n", P, ms(ht0, ht1), ms(ht1, ht2), ms(ht2, ht3));
    }
    int worst = PGICP_OK;
    for (int p = 0; p < P; p++) {
        const ProblemDev &D = hp[p];
        double *To = T_out + 16 * p;
        pgicp_stats s;
        std::memset(&s, 0, sizeof s);
        s.status = D.status;
        s.iterations = D.iters; s.converged = D.converged; s.max_iter_reached = D.max_iter_reached;
        s.status = D.status == PGICP_ST_BOUND ? PGICP_ERR_BOUND : D.status;
        s.overlap = D.sys[27] / ((double)D.n * L.knn); s.residual = D.sys[29]; s.trim_limit = D.limit;
        s.n_kept = D.n_kept; s.n_finite = D.n_finite;
        if (D.status == PGICP_ST_OK) {
            double t1[16];
            mat4_mul(D.T_iter, D.Tpre, t1);
            mat4_mul(Tref[p].data(), t1, To);
            double H[36], G[36], Hi[36];
            sys_to_full(cs.data() + (size_t)p * kCovTerms, H);
            sys_to_full(cs.data() + (size_t)p * kCovTerms + 21, G);
            if (!with_cov) { /* zeros */ }
            else if (inverse6(H, Hi)) sandwich6(Hi, G, prm.sensor_std_dev * prm.sensor_std_dev, s.cov);
            else
                for (int i = 0; i < 6; i++) s.cov[i * 6 + i] = std::numeric_limits<double>::max();
        } else {
            mat4_identity(To);
            if (worst == PGICP_OK) worst = s.status;
        }
        if (stats) stats[p] = s;
    }
    if (worst != PGICP_OK)
        return fail(c, worst, worst == PGICP_ERR_NO_MATCH ? "ICP: no point to minimize (ConvergenceError)"
                           : worst == PGICP_ERR_BOUND ? "ICP: BoundTransformationChecker: limit exceeded (ConvergenceError)"
                                                      : "ICP: NaN in transformation checker (ConvergenceError)");
    return PGICP_OK;
}

template <typename T>
int icp_pair(pgicp_ctx *c, const T *reading, int rd_stride, int n, const T *ref_xyz, int ref_stride, const T *ref_nrm,
             int nrm_stride, int m, int mem, const double *T_init, double *T_out, pgicp_stats *stats)
{
    int id = -1;
    int st = map_create<T>(c, ref_xyz, ref_stride, ref_nrm, nrm_stride, m, mem, 1, &id);
    if (st) { (void)noise_take(c); VarDistCall radii(c); return st; }
    const pgicp_problem pr = one_problem(id, reading, rd_stride, n, mem, T_init);
    st = align_batch<T>(c, 1, &pr, T_out, stats);
    (void)stream_sync(c);
    if (MapHost<T> *mh = get_map<T>(c, id)) free_map(c, *mh);
    return st;
}

