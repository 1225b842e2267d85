// api_context.inc -- part of pgicp_api.cpp (one translation unit): context, allocation accounting, error / transfer helpers (bounce buffer), profile.
namespace {

// ---- allocation accounting (pgicp_debug_alloc_stats): hipMalloc / hipFree / hipHostMalloc are the calls of this library whose
// cost depends on the HOST (1 ms on some boxes, 45 ms on others; hipFree waits for the whole device) -- counted and timed, so
// that a slow pass of a caller can be told apart from a slow GPU
struct AllocStats { std::atomic<long long> n[4], ns[4]; };
AllocStats g_alloc;
struct AllocTimer {
    int k; std::chrono::steady_clock::time_point t0;
    explicit AllocTimer(int kind) : k(kind), t0(std::chrono::steady_clock::now()) {}
    ~AllocTimer() { g_alloc.n[k]++; g_alloc.ns[k] += std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t0).count(); }
};
inline hipError_t t_malloc(void **p, size_t bytes) { AllocTimer t(0); return hipMalloc(p, bytes); }
inline hipError_t t_free(void *p) { AllocTimer t(1); return hipFree(p); }
inline hipError_t t_host_malloc(void **p, size_t bytes, unsigned flags) { AllocTimer t(2); return hipHostMalloc(p, bytes, flags); }
inline hipError_t t_host_free(void *p) { AllocTimer t(3); return hipHostFree(p); }

struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
    hipError_t ensure(size_t bytes)
    {
        if (bytes <= cap) return hipSuccess;
        if (p) { hipError_t e = t_free(p); p = nullptr; cap = 0; if (e != hipSuccess) return e; }
        size_t want = bytes + bytes / 4 + 256;
        hipError_t e = t_malloc(&p, want);
        if (e == hipSuccess) cap = want;
        return e;
    }
    void release() { if (p) (void)t_free(p); p = nullptr; cap = 0; }
    template <typename U> U *as() const { return (U *)p; }
};

// the one device allocation of a (batch of) map(s); freed here only when nobody released it properly (an error path)
struct SharedBlock {
    char *p = nullptr;
    size_t bytes = 0;
    ~SharedBlock() { if (p) (void)t_free(p); }
};

template <typename T>
struct MapHost {
    bool used = false;
    unsigned long long stamp = 0;   // pgicp_ctx::map_clock when this context created or adopted the map (seed_source.hpp)
    int m = 0;
    T mean[3] = {0, 0, 0};
    bool has_nrm = false;
    typename Vec4<T>::type *pts = nullptr;
    typename Vec4<T>::type *nrm = nullptr;
    int *cell_start = nullptr;
    int *cell_start_f = nullptr;
    uint4 *sw = nullptr;            // MapDev::sw / ostart: the succinct table (then cell_start / cell_start_f are null)
    int *ostart = nullptr;
    int kx = 1;
    int *slot_of = nullptr;
    bool slot_of_made = false;      // (filled on first use: error_stats)
    int *sc_count = nullptr;
    int *near = nullptr;
    int *sc_dist = nullptr;
    int *sc_wit = nullptr;
    float *sc_ext = nullptr;
    unsigned *occ = nullptr;
    float *ptsf = nullptr;          // MapDev::ptsf (double maps)
    // (ABI 6, added) GenericDescriptorOutlierFilter: the map's values in slot order (pgicp_map_set_values; MapDev::val), their own
    // allocation -- dropped with the record -- and whether one of them is negative (soft mode refuses the map then)
    std::shared_ptr<SharedBlock> vblock;
    T *val = nullptr;
    bool val_neg = false;
    int first = 0;                  // MapDev::first
    // the one device allocation holding all of the above -- shared by the maps of one batched build and
    // returned to the pool (or freed) by whoever drops the last reference
    std::shared_ptr<SharedBlock> block;
    GridDesc<T> g{};
};

template <typename T>
struct State {
    std::vector<MapHost<T>> maps;
    DevBuf d_maps;                  // MapDev<T>[capacity]
    int d_maps_cap = 0;
    DevBuf rd_pre, rd_sorted, slot, d2, none_r, staging, stage_aux, nrm_pre, nrm_sorted;
};

struct ProfEvent {
    hipEvent_t a, b;
    int kid;
    int kid2 = -1;          // a second account the launch also goes to (-1: none)
    long long units;
    long long problems;
    long long map_points;
};

}  // namespace

struct pgicp_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    std::string err;
    pgicp_params prm{};
    State<float> f32;
    State<double> f64;
    DevBuf probs, src, partials, sums, sums2, small, stats, bdesc, tmp_a, tmp_b, tmp_c, tmp_d, tmp_e, tmp_f, tmp_r, tmp_w, tmp_p, tmp_n;
    // what problem 0 of the last ALIGN call was (pgicp_partial_chain_seeded reads another context's correspondences): its reading's
    // size, the slot of its map in the context's table, the cloud type, the knn it ran with, that map's stamp; -1: none
    int last_n0 = -1, last_map0 = -1, last_elem = 0, last_knn = 0;
    unsigned long long last_stamp0 = 0;
    // moves with every map create, destroy, transfer in and transfer out (either cloud type); a map keeps the value it was
    // registered with (MapHost::stamp) -- table entries are reused, stamps are not
    unsigned long long map_clock = 0;
    DevBuf scan_pos;                // PGICP_SUM_ORDER_SCAN: the inverse of `order` (sorted position of every reading point)
    DevBuf qrow, qtmp, order, qcounts, qblock, qstart, qcursor, slow_list, slow_lb, slow_ring, slow2, active, sel_tables, queue;
    // host-input pipeline (pgicp_upload_*): a copy stream and two upload sets used alternately
    struct UploadSet {
        DevBuf dev;                     // device copies of the readings of one upload
        void *pin = nullptr;            // pinned staging for pageable sources
        size_t pin_cap = 0;
        size_t bytes = 0;               // bytes of `dev` in use
        hipEvent_t uploaded = nullptr;  // recorded on the copy stream after the last transfer of the upload
        hipEvent_t consumed = nullptr;  // recorded on the compute stream after the last kernel that reads the set
        bool pending = false, has_consumer = false;
    } up[2];
    hipStream_t copy_stream = nullptr;
    // pgicp_filter_cloud: four sets of device buffers used in turn (the filtered features of a call stay valid, as a device
    // reading, for the next three calls: a localizer that pre-processes scan k + 1 while scan k aligns, and now and then a
    // scan that was not pre-processed ahead, has three calls between making a reading and aligning it)
    struct FilterSet { DevBuf in_f, in_d, keep, pos, bsum, out_f, out_d, idx, drop, qsel; } fset[4];     // (qsel: a MaxQuantileOnAxis entry's scratch)
    // pgicp_sampling_surface_normal_*, pgicp_voxel_grid_* and include/pgicp_density.h share three buffers: the scratch of the call
    // running, the device copies of its host inputs / outputs, its counters.  The calls of a context are serialised on its stream
    // and none hands a pointer into these back, so every call carves them anew and they hold the largest call's need.
    DevBuf dpf_work, dpf_io, dpf_stat;
    DevBuf robust_dev;              // RobustOutlierFilter: the pairs' absolute deviations from the median (the second selection's input)
    DevBuf gd_stage;                // pgicp_map_set_values: host values packed for the copy, and the kernel's two flags
    // (ABI 6, added) VarTrimmedDistOutlierFilter (pgicp_set_var_trim): on, {minRatio, maxRatio, lambda}; the sort's two key
    // lists (one key per pair each); the tuned ratio of every problem's last iteration in the last align / partial-chain /
    // outlier-weights call (empty: that call did not run the filter)
    int vt_on = 0;
    double vt[3] = {0.0, 0.0, 0.0};
    DevBuf vt_keys, vt_prob;
    std::vector<double> vt_last;
    // RobustOutlierFilter's distanceType, berg and nbIterationForScale (pgicp_robust.h, pgicp_set_robust_ext): on, the setting
    int rx_on = 0;
    pgicp_robust_ext rx = {0, 0, 0};
    // (ABI 6, added) GenericDescriptorOutlierFilter (pgicp_set_descriptor_filter): PGICP_DESC_FILTER_*, the hard modes' threshold
    int gd_mode = 0;
    double gd_thr = 0.0;
    // Sensor-noise getOverlap() (include/pgicp_noise.h).  pgicp_arm_reading_noise copies the readings' noise rows into `vals`
    // (packed, one problem after the other; off[p]: where problem p's start, -1: it has none) and the next ICP call consumes
    // them (api_noise.inc); every buffer here is allocated by an arm call or an armed ICP call only.  last_*: what
    // pgicp_last_noise_overlap answers with -- last_P < 0: the last ICP call was not armed.
    // (ArmedRows: one value per reading point, armed for the next call -- what the noise rows and KDTreeVarDistMatcher's radii share)
    struct ArmedRows {
        bool armed = false, bad = false;    // bad: a value was refused (noise: negative or not finite; radii: negative or a NaN)
        int elem = 0;                       // sizeof(T) of the armed values
        std::vector<long long> off;
        std::vector<int> n;
        DevBuf vals, off_dev;               // off_dev: `off` on the device, then the staging kernel's flag
    };
    struct Noise : ArmedRows {
        DevBuf dist, out;                   // dist: sqrt(d2) per pair (-1: not kept); out: {S, nb} per problem, then the counts
        int last_P = -1;
        std::vector<double> last_overlap;
        std::vector<int> last_nb;
        std::vector<char> last_ok;
    } noise;
    // KDTreeVarDistMatcher's radii (include/pgicp_vardist.h, api_vardist.inc).  pgicp_arm_reading_radii copies the rows as the noise
    // rows are copied; the next matching call consumes them: `on` while that call runs -- its iterations cut the matcher's pairs
    // into slot_cut / d2_cut (laid out as State::slot / ::d2) and everything downstream reads those (IterBufs::pair_slot / ::pair_d2);
    // cut_live: the last call that matched was such a call (pgicp_debug_last_matches reads the cut pairs then).  Every buffer here
    // is allocated by an arm call or an armed call only.
    struct VarDist : ArmedRows {
        bool on = false, cut_live = false;
        DevBuf slot_cut, d2_cut;
    } vd;
    int last_icp_P = 0;             // problems of the last ICP call: the last-call diagnostics check their `problem` against it
    int fset_next = 0;
    int up_next = 0;
    int up_seen = 0;            // upload sets whose device pointers the running call was handed (see UploadUse)
    int *h_pinned = nullptr;        // pinned scratch for small D2H polls (64 ints)
    // pinned bounce buffers for the problem records of a batch (4.6 KB each: a Checker history rides in them): a megabyte
    // copied between device and PAGEABLE host memory takes the runtime's slow path -- 10-13 ms per step at 256-320
    // problems, none at 128 or 384 -- so the records travel through pinned memory in both directions
    char *h_up = nullptr, *h_down = nullptr;
    size_t h_up_cap = 0, h_down_cap = 0;
    // Bounce buffer (pinned): host memory the CALLER owns never reaches hipMemcpy*.  The runtime pins a pageable range of more
    // than ~128 KB on the fly (a userptr buffer object); when the caller later frees that memory (munmap, or a trimmed heap)
    // the MMU notifier makes the kernel driver EVICT every queue of the process for 25-40 ms.  Measured in round 5 (NOTES_r05,
    // profiles/r05_stall_diagnosis.txt): 10-100 such pauses in the first second of a process -- until glibc's dynamic mmap
    // threshold stops handing out mmap()ed chunks of a cloud's size -- made slam_100k's ICP phase 0.6 s on one box and 3.0 s on
    // another.  h2d() / d2h() below: memcpy through this buffer; copy-outs are completed by stream_sync().
    struct Bounce {
        char *p = nullptr;
        size_t cap = 0, off = 0;
        struct Out { void *dst; const char *src; size_t bytes; };
        std::vector<Out> outs;
        bool direct_out_pending = false;    // a small device -> host copy went straight to a caller's / a local buffer (see fail())
    } bounce;
    int *h_flag = nullptr;          // coherent pinned pair {problems done, stamp} the last kernel of an iteration writes
    int flag_stamp = 0;             // iterations enqueued so far == the value the last one's k_compact_active will store
    int *stamp_dev = nullptr;       // the same count on the device (k_compact_active advances it)
    // captured iterations (small batches): the launch sequence of one ICP iteration as an executable graph, keyed by
    // everything its kernel arguments depend on
    struct IterGraph { unsigned long long key = 0; hipGraphExec_t exec = nullptr; unsigned long long used = 0; };
    std::vector<IterGraph> iter_graphs;
    unsigned long long graph_clock = 0;
    int graph_max_problems = 0;     // batches of at most this many problems replay captured iterations (0: never -- the default:
                                    // measured on ROCm 7.2 / MI355X, replaying costs what the ten launches cost; PGICP_GRAPH_MAX_P)
    int graph_failures = 0;
    long long graph_captures = 0, graph_launches = 0;
    std::vector<SrcDesc> h_src;     // host copies of per-batch descriptors (uploaded asynchronously)
    std::vector<int> h_ident;
    int counters_clean = 0;         // the matcher's queue counters were zeroed by the last kernel of the previous iteration
    int seg_clean = 0;              // the matcher's SEGMENTED queue counters were zeroed by the previous iteration's first selection
    int poll_us = 400;              // how long the host polls h_flag before it blocks on the stream instead
    // selection hints (ProblemDev::qhint): what the previous call of the same kind found, per problem index -- [0] pgicp_align*,
    // [1] pgicp_partial_chain*; dropped when the chain changes.  sel_guess_first: the enqueued iteration's FIRST selection may take
    // the band path although the matcher is unseeded (every problem carries a hint for it).
    struct SelHint { double q[2][4]; };
    std::vector<SelHint> sel_hints[2];
    int sel_guess_first = 0;
    int sel_hints_on = 1;           // PGICP_SEL_HINTS=0 turns them off (A/B)
    int fast_rings_seeded = 0, fast_rings_unseeded = 0;      // 0: by the maps' cell size (BatchLayout::rings_*); PGICP_FAST_RINGS_* set them
    double cell_scale = 1.0;     // experiment knob PGICP_CELL_SCALE: the automatic grid cell times this
    int grid_kx = 4;                // x refinement of the table the matcher narrows ranges with (MapDev::cell_start_f)
    int table_mode = 0;             // the cell tables a map is built with: 0 / 1 dense (the default), 2 succinct (MapDev::sw);
                                    // PGICP_TABLES=dense|succinct, read when the context is made
    double near_frac = 0.2;         // MapDev::near looks this fraction of maxDist far (at most kNearReach cells)
    int bin_shift_add = 0;          // experiment knob PGICP_BIN_SHIFT_ADD: coarser (+) or finer (-) bins of the reading sort
    int med_rings = 4;              // rings a queued query may walk per lane before the wave-cooperative path takes it   // rings walked in the fast kernel before a query is queued
    bool prof_on = false;
    std::mutex prof_m;              // prof_events and the sums below: pgicp_profile_process collects from another thread
    std::vector<ProfEvent> prof_events;
    long long prof_launches[PGICP_PROF_COUNT] = {0};
    double prof_ms[PGICP_PROF_COUNT] = {0};
    long long prof_units[PGICP_PROF_COUNT] = {0};
    long long prof_problems[PGICP_PROF_COUNT] = {0};
    long long prof_map_points[PGICP_PROF_COUNT] = {0};      // reference points of the active problems of those launches
    long long prof_next_m = 0;                               // what the next matcher launch is charged with
};

namespace {

template <typename T> State<T> &state(pgicp_ctx *c);
template <> State<float> &state<float>(pgicp_ctx *c) { return c->f32; }
template <> State<double> &state<double>(pgicp_ctx *c) { return c->f64; }

// public map ids carry the precision in bit 30 so f32 and f64 maps never alias
template <typename T> constexpr int id_tag();
template <> constexpr int id_tag<float>() { return 0; }
template <> constexpr int id_tag<double>() { return 0x40000000; }

template <typename T>
int map_index(pgicp_ctx *c, int id)
{
    State<T> &S = state<T>(c);
    if (id < 0 || (id & 0x40000000) != id_tag<T>()) return -1;
    const int idx = id & 0x3FFFFFFF;
    if (idx >= (int)S.maps.size() || !S.maps[idx].used) return -1;
    return idx;
}

template <typename T>
MapHost<T> *get_map(pgicp_ctx *c, int id)
{
    const int idx = map_index<T>(c, id);
    return idx < 0 ? nullptr : &state<T>(c).maps[idx];
}

// Every failing exit of every entry point passes through here (directly, or through HIPC / XFER).  A device -> host copy may
// still be queued at that point: a bounce copy-out whose destination is a local of the failing call or a caller's buffer
// (pgicp_ctx::Bounce::outs), or a small direct hipMemcpyAsync into one.  Let the stream run dry so that nothing writes into
// memory that goes out of scope with the return, and DROP the queued copy-outs -- the call has failed, its outputs are void --
// so that no later stream_sync() (the next call's, bounce_take's wrap-around, pgicp_ctx_destroy) replays them.
int fail(pgicp_ctx *c, int code, const std::string &msg)
{
    if (c) {
        c->err = msg;
        if (!c->bounce.outs.empty() || c->bounce.direct_out_pending) {
            if (c->stream) (void)hipStreamSynchronize(c->stream);
            c->bounce.outs.clear();
            c->bounce.off = 0;
            c->bounce.direct_out_pending = false;
        }
    }
    return code;
}

#define HIPC(ctx, call)                                                                                  \
    do {                                                                                                 \
        hipError_t e_ = (call);                                                                          \
        if (e_ != hipSuccess)                                                                            \
            return fail(ctx, PGICP_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(e_));          \
    } while (0)

// process-wide view of the profile (pgicp_profile_process): totals of the contexts already destroyed plus, at the time
// of the call, of the live ones -- for callers that do not hold the contexts themselves (the C++ facade's ICP objects)
struct ProcessProfile {
    std::mutex m;
    std::vector<pgicp_ctx *> live;
    long long launches[PGICP_PROF_COUNT] = {0}, units[PGICP_PROF_COUNT] = {0}, problems[PGICP_PROF_COUNT] = {0}, map_points[PGICP_PROF_COUNT] = {0};
    double ms[PGICP_PROF_COUNT] = {0};
};
ProcessProfile &process_profile() { static ProcessProfile *p = new ProcessProfile(); return *p; }

struct ProfScope {
    pgicp_ctx *c;
    int kid;
    ProfEvent ev{};
    bool on;
    ProfScope(pgicp_ctx *c_, int kid_, long long units, long long problems = 1) : c(c_), kid(kid_), on(c_->prof_on)
    {
        if (!on) return;
        ev.kid = kid;
        ev.units = units;
        ev.problems = problems;
        ev.map_points = (kid_ == PGICP_PROF_KNN_GRID || kid_ == PGICP_PROF_KNN_BRUTE) ? c_->prof_next_m : 0;
        if (hipEventCreate(&ev.a) != hipSuccess || hipEventCreate(&ev.b) != hipSuccess) { on = false; return; }
        (void)hipEventRecord(ev.a, c->stream);
    }
    void also(int kid2) { ev.kid2 = kid2; }
    ~ProfScope();
};

// (with c->prof_m held) waits for the stream and folds the finished event pairs into the sums
void prof_collect_locked(pgicp_ctx *c)
{
    if (c->prof_events.empty()) return;
    (void)hipStreamSynchronize(c->stream);
    // diagnostics (PGICP_STALL_LOG=<ms>): scopes and gaps between consecutive scopes of this context longer than that
    static const double stall_ms = std::getenv("PGICP_STALL_LOG") ? std::atof(std::getenv("PGICP_STALL_LOG")) : 0.0;
    const ProfEvent *prev = nullptr;
    for (auto &e : c->prof_events) {
        float ms = 0.f;
        if (stall_ms > 0.0 && prev) {
            float gap = 0.f;
            if (hipEventElapsedTime(&gap, prev->b, e.a) == hipSuccess && gap > stall_ms)
                std::fprintf(stderr, "pgicp stall: %.2f ms between scope %d and scope %d (context %p)\n", gap, prev->kid, e.kid, (void *)c);
        }
        prev = &e;
        if (hipEventElapsedTime(&ms, e.a, e.b) == hipSuccess) {
            if (stall_ms > 0.0 && ms > stall_ms) std::fprintf(stderr, "pgicp stall: scope %d took %.2f ms (context %p)\n", e.kid, ms, (void *)c);
            for (int kid : {e.kid, e.kid2}) {
                if (kid < 0) continue;
                c->prof_launches[kid] += 1;
                c->prof_ms[kid] += ms;
                c->prof_units[kid] += e.units;
                c->prof_problems[kid] += e.problems;
                c->prof_map_points[kid] += e.map_points;
            }
        }
    }
    for (auto &e : c->prof_events) { (void)hipEventDestroy(e.a); (void)hipEventDestroy(e.b); }
    c->prof_events.clear();
}
void prof_collect(pgicp_ctx *c)
{
    std::lock_guard<std::mutex> lock(c->prof_m);
    prof_collect_locked(c);
}
ProfScope::~ProfScope()
{
    if (!on) return;
    (void)hipEventRecord(ev.b, c->stream);
    std::lock_guard<std::mutex> lock(c->prof_m);
    c->prof_events.push_back(ev);
    // a context that profiles from its creation (PGICP_PROFILE_ALL: the facade's ICP objects) is never asked for its
    // numbers between calls: fold the events in now and then, or a long run holds hundreds of thousands of live events
    if (c->prof_events.size() >= 4096) prof_collect_locked(c);
}

static inline bool is_p2point(int m) { return m == PGICP_MINIMIZER_POINT_TO_POINT || m == PGICP_MINIMIZER_POINT_TO_POINT_WITH_COV; }
// the chain reads the reference's normals: every minimiser but the plain point-to-point one (its WithCov form estimates the
// covariance from them), and a SurfaceNormalOutlierFilter
static inline bool needs_ref_normals(const pgicp_params &p) { return p.error_minimizer != PGICP_MINIMIZER_POINT_TO_POINT || p.normal_max_angle > 0.0; }

template <typename T>
ChainDev<T> make_chain(const pgicp_params &p)
{
    ChainDev<T> ch;
    ch.max_dist = (T)p.max_dist;
    ch.max_dist2 = ch.max_dist * ch.max_dist;
    ch.trim_ratio = (T)p.trim_ratio;
    ch.trim_scale = (T)p.quantile_scale;
    {
        const T md = (T)p.outlier_max_dist;
        ch.outlier_max_d2 = (p.outlier_max_dist > 0.0 && std::isfinite(p.outlier_max_dist)) ? md * md : std::numeric_limits<T>::infinity();
    }
    ch.max_iters = p.max_iters;
    ch.smooth = p.smooth_length;
    ch.min_rot = p.min_diff_rot;
    ch.min_trans = p.min_diff_trans;
    ch.rank_rel_tol = 6.0 * (double)std::numeric_limits<T>::epsilon();
    ch.knn = std::max(1, p.knn);
    ch.minimizer = is_p2point(p.error_minimizer) ? 1 : 0;
    ch.robust.fct = p.robust_fct; ch.robust.mad = p.robust_scale == PGICP_ROBUST_SCALE_MAD ? 1 : 0;
    ch.robust.k = (T)p.robust_tuning; ch.robust.k2 = ch.robust.k * ch.robust.k;
    ch.robust.cut = (p.robust_approx > 0.0 && std::isfinite(p.robust_approx)) ? 1 : 0;
    { const T a = (T)p.robust_approx; ch.robust.a2 = a * a; }
    ch.robust.dist = 0; ch.robust.est = ch.robust.mad; ch.robust.nb = 0; ch.robust.target = (T)0;      // (pgicp_robust.h's settings: robust_ext_apply)
    ch.force4dof = p.error_minimizer == PGICP_MINIMIZER_POINT_TO_PLANE_4DOF ? 1 : 0;
    ch.bound_rot = (p.bound_max_rot > 0.0 && std::isfinite(p.bound_max_rot)) ? p.bound_max_rot : 0.0;
    ch.bound_trans = (p.bound_max_trans > 0.0 && std::isfinite(p.bound_max_trans)) ? p.bound_max_trans : 0.0;
    ch.use_normals = p.normal_max_angle > 0.0 ? 1 : 0;
    ch.normal_cos = std::cos((T)p.normal_max_angle);          // in T, as the filter evaluates `cos(maxAngle)`
    ch.scan_pos = nullptr;                                     // (set by chain_of: it names a buffer of the context)
    ch.var_trim = 0; ch.vt_min = ch.vt_max = ch.vt_lambda = 0.0;   // (set by chain_of: a setting of the context)
    ch.gd_mode = PGICP_DESC_FILTER_OFF; ch.gd_thr = (T)0;            // (the same)
    return ch;
}

// pgicp_set_robust_ext's setting laid over the robust filter of pgicp_params (pgicp_robust.h).  berg: the tuning is the target
// scale and the weight function runs with tuning 1.  Off, or {point2point, -1, 0}: `rb` stays what make_chain made it.
template <typename T>
void robust_ext_apply(const pgicp_ctx *c, const pgicp_params &p, RobustDev<T> &rb)
{
    if (!c->rx_on || rb.fct == 0) return;
    rb.dist = c->rx.distance_type == PGICP_ROBUST_DIST_POINT2PLANE ? 1 : 0;
    if (c->rx.scale_estimator >= 0) rb.est = c->rx.scale_estimator;
    rb.mad = rb.est == 1 ? 1 : 0;
    rb.nb = c->rx.nb_iteration_for_scale;
    if (rb.est == 2) { rb.target = (T)p.robust_tuning; rb.k = (T)1; rb.k2 = (T)1; }
}
// the setting against the robust filter of pgicp_params: checked by the setter and again by every call that runs the chain (the two
// settings are made separately, as VarTrimmedDist's)
int robust_ext_check(pgicp_ctx *c, const pgicp_robust_ext &x)
{
    const bool asks = x.distance_type != PGICP_ROBUST_DIST_POINT2POINT || x.scale_estimator == PGICP_ROBUST_SCALE_BERG || x.nb_iteration_for_scale != 0;
    if (asks && c->prm.robust_fct == PGICP_ROBUST_NONE)
        return fail(c, PGICP_ERR_ARG, "RobustOutlierFilter: distanceType point2plane, scaleEstimator berg and nbIterationForScale need a robustFct (pgicp_params.robust_fct is none)");
    return PGICP_OK;
}
static inline bool robust_plane_dist(const pgicp_ctx *c)
{
    return c->rx_on && c->prm.robust_fct != PGICP_ROBUST_NONE && c->rx.distance_type == PGICP_ROBUST_DIST_POINT2PLANE;
}

// the chain of a call that has sorted its readings (begin_batch): with PGICP_SUM_ORDER_SCAN the reduce kernels are handed the
// inverse of that sort (pgicp_ctx::scan_pos, filled by begin_batch)
template <typename T>
ChainDev<T> chain_of(pgicp_ctx *c, const pgicp_params &p)
{
    ChainDev<T> ch = make_chain<T>(p);
    ch.scan_pos = p.sum_order == PGICP_SUM_ORDER_SCAN ? c->scan_pos.as<int>() : nullptr;
    ch.var_trim = c->vt_on;
    ch.vt_min = c->vt[0]; ch.vt_max = c->vt[1]; ch.vt_lambda = c->vt[2];
    ch.gd_mode = c->gd_mode; ch.gd_thr = (T)c->gd_thr;              // (the threshold in T, as the comparison is)
    robust_ext_apply<T>(c, p, ch.robust);
    return ch;
}

// VarTrimmedDistOutlierFilter takes the chain's quantile slot: no RobustOutlierFilter, no MedianDist factor beside it
// (checked at every call that runs the chain: the two settings are made separately)
int var_trim_check(pgicp_ctx *c)
{
    if (!c->vt_on) return PGICP_OK;
    if (c->prm.robust_fct != PGICP_ROBUST_NONE)
        return fail(c, PGICP_ERR_ARG, "VarTrimmedDistOutlierFilter: no RobustOutlierFilter beside it (one quantile / robust filter per chain)");
    if (c->prm.quantile_scale != 1.0)
        return fail(c, PGICP_ERR_ARG, "VarTrimmedDistOutlierFilter: quantile_scale must be 1 (no MedianDistOutlierFilter beside it)");
    return PGICP_OK;
}

double key_to_double(unsigned long long k)
{
    long long i = (k & 0x8000000000000000ULL) ? (long long)(k ^ 0x8000000000000000ULL) : (long long)~k;
    double d;
    std::memcpy(&d, &i, sizeof d);
    return d;
}

// A device pointer handed out by pgicp_upload_*: the context stream waits (on the device) for that upload.
// Returns the bit mask of upload sets the pointer belongs to.
int upload_wait(pgicp_ctx *c, const void *p)
{
    int mask = 0;
    for (int s = 0; s < 2; s++) {
        pgicp_ctx::UploadSet &U = c->up[s];
        if (!U.pending || !U.dev.p) continue;
        const char *q = (const char *)p;
        if (q >= (const char *)U.dev.p && q < (const char *)U.dev.p + U.bytes) {
            (void)hipStreamWaitEvent(c->stream, U.uploaded, 0);
            mask |= 1 << s;
        }
    }
    return mask;
}
// ... and after the last kernel that reads them has been queued, the sets may be overwritten once it has run
void upload_consumed(pgicp_ctx *c, int mask)
{
    for (int s = 0; s < 2; s++)
        if (mask & (1 << s)) { (void)hipEventRecord(c->up[s].consumed, c->stream); c->up[s].has_consumer = true; }
}

// ---- transfers between the device and host memory the caller owns (see pgicp_ctx::Bounce) ----
constexpr size_t kDirectCopyBytes = 64 << 10;        // below this the runtime stages the copy itself (it pins from ~128 KB on)
static void bounce_drain(pgicp_ctx *c)               // the stream is idle: finish the copy-outs, the whole buffer is free again
{
    for (auto &o : c->bounce.outs) std::memcpy(o.dst, o.src, o.bytes);
    c->bounce.outs.clear();
    c->bounce.off = 0;
    c->bounce.direct_out_pending = false;
}
static hipError_t stream_sync(pgicp_ctx *c)
{
    const hipError_t e = hipStreamSynchronize(c->stream);
    bounce_drain(c);
    return e;
}
static int bounce_take(pgicp_ctx *c, size_t bytes, char **out)
{
    pgicp_ctx::Bounce &B = c->bounce;
    const size_t need = (bytes + 255) & ~(size_t)255;
    if (B.off + need > B.cap) {
        HIPC(c, stream_sync(c));                     // wrap around: what is in flight lands first
        if (need > B.cap) {
            if (B.p) (void)t_host_free(B.p);
            B.p = nullptr; B.cap = 0;
            const size_t want = need + need / 4 + (1u << 20);
            HIPC(c, t_host_malloc((void **)&B.p, want, hipHostMallocDefault));
            B.cap = want;
        }
    }
    *out = B.p + B.off;
    B.off += need;
    return PGICP_OK;
}
// host -> device on the context's stream; `src` may be reused as soon as the call returns
static int h2d(pgicp_ctx *c, void *dst_dev, const void *src_host, size_t bytes)
{
    if (bytes == 0) return PGICP_OK;
    if (bytes < kDirectCopyBytes) { HIPC(c, hipMemcpyAsync(dst_dev, src_host, bytes, hipMemcpyHostToDevice, c->stream)); return PGICP_OK; }
    char *b = nullptr;
    { const int st = bounce_take(c, bytes, &b); if (st) return st; }
    std::memcpy(b, src_host, bytes);
    HIPC(c, hipMemcpyAsync(dst_dev, b, bytes, hipMemcpyHostToDevice, c->stream));
    return PGICP_OK;
}
// device -> host on the context's stream; `dst` holds the data after the next stream_sync(c)
static int d2h(pgicp_ctx *c, void *dst_host, const void *src_dev, size_t bytes)
{
    if (bytes == 0) return PGICP_OK;
    // (small copies too go through the pinned buffer: hipMemcpyAsync into PAGEABLE host memory -- a caller's variable, a local
    //  vector -- does not return before the copy has happened, i.e. before every kernel queued ahead of it has run; two small
    //  results read back one after the other were two round trips: 18 us each in the facade's input stage and in its overlap probe;
    //  PGICP_D2H_DIRECT=1 restores the direct copy for an A/B)
    static const bool direct_small = [] { const char *e = std::getenv("PGICP_D2H_DIRECT"); return e && *e == '1'; }();
    if (direct_small && bytes < kDirectCopyBytes) {
        c->bounce.direct_out_pending = true;
        HIPC(c, hipMemcpyAsync(dst_host, src_dev, bytes, hipMemcpyDeviceToHost, c->stream));
        return PGICP_OK;
    }
    char *b = nullptr;
    { const int st = bounce_take(c, bytes, &b); if (st) return st; }
    HIPC(c, hipMemcpyAsync(b, src_dev, bytes, hipMemcpyDeviceToHost, c->stream));
    c->bounce.outs.push_back({dst_host, b, bytes});
    return PGICP_OK;
}
#define XFER(ctx, call) do { const int st_ = (call); if (st_) return st_; } while (0)

// Every entry point that may be handed a device pointer of pgicp_upload_* declares one of these: to_device() makes the
// compute stream wait for the upload (on the device) and notes the set; when the call returns -- its kernels queued, most
// calls synchronised -- the set is marked consumed, so that the next upload into it waits for them.
struct UploadUse {
    pgicp_ctx *c;
    explicit UploadUse(pgicp_ctx *c_) : c(c_) { if (c) c->up_seen = 0; }
    ~UploadUse() { if (c && c->up_seen) { upload_consumed(c, c->up_seen); c->up_seen = 0; } }
    void touch(const void *p) { if (c && p && (c->up[0].pending || c->up[1].pending)) c->up_seen |= upload_wait(c, p); }
};

// Bring a strided point buffer onto the device if it is host memory.
// Returns the device pointer to use (either the caller's or the staging copy).
template <typename T>
int to_device(pgicp_ctx *c, const T *p, int stride, int n, int mem, DevBuf &stage, size_t stage_off_bytes, const T **out)
{
    if (mem == PGICP_DEVICE) {
        if (c->up[0].pending || c->up[1].pending) c->up_seen |= upload_wait(c, p);
        *out = p;
        return PGICP_OK;
    }
    const size_t bytes = sizeof(T) * ((size_t)(n - 1) * stride + 3);
    XFER(c, h2d(c, (char *)stage.p + stage_off_bytes, p, bytes));
    *out = (const T *)((char *)stage.p + stage_off_bytes);
    return PGICP_OK;
}

// ---- staging of the cloud-in, cloud-out filters (pgicp_ctx::dpf_*) ----
// Size `buf` for a layout and point the layout into it: `layout(Carve &)` names every array once and is run twice.
template <class Layout>
int carve_buf(pgicp_ctx *c, DevBuf &buf, Layout &&layout)
{
    Carve measure;
    layout(measure);
    HIPC(c, buf.ensure(measure.used));
    Carve cv(buf.p);
    layout(cv);
    return PGICP_OK;
}

// The cloud a filter reads: strided coordinates and optional descriptor rows.  carve() names their device copies in the I/O
// buffer (host memory); upload_cloud() fills those, or -- device memory -- points at the caller's arrays and makes the stream
// wait for an upload they may belong to (the caller holds an UploadUse).
template <typename T>
struct CloudIn {
    const T *xyz, *desc;
    void carve(Carve &cv, int stride, int n, int drows) { xyz = cv.take<T>((size_t)(n - 1) * stride + 3); desc = cv.take<T>((size_t)drows * n, drows > 0); }
};
template <typename T>
int upload_cloud(pgicp_ctx *c, int mem, const T *xyz, int stride, int n, const T *desc, int drows, CloudIn<T> &in)
{
    if (mem == PGICP_DEVICE) {
        for (const T *p : {xyz, desc})
            if (p && (c->up[0].pending || c->up[1].pending)) c->up_seen |= upload_wait(c, p);
        in.xyz = xyz; in.desc = desc;
        return PGICP_OK;
    }
    XFER(c, h2d(c, (void *)in.xyz, xyz, sizeof(T) * ((size_t)(n - 1) * stride + 3)));
    if (desc) XFER(c, h2d(c, (void *)in.desc, desc, sizeof(T) * (size_t)drows * n));
    return PGICP_OK;
}

// A call's counters back on the host: one round trip, after which everything queued so far has run.
static int read_back(pgicp_ctx *c, void *host, const void *dev, size_t bytes)
{
    XFER(c, d2h(c, host, dev, bytes));
    HIPC(c, stream_sync(c));
    HIPC(c, hipGetLastError());
    return PGICP_OK;
}

// Rows of 3 values a point from a device array at `dev_stride` to a host array at `stride`.  Packed on both sides it is one d2h;
// otherwise the rows travel into a temporary, and land() -- the sync that completes every fetch queued before it -- spreads them.
template <typename T>
struct RowSpread {
    struct Job { T *out; int stride, dev_stride, count; std::vector<T> tmp; };
    std::vector<Job> jobs;
    int land(pgicp_ctx *c)
    {
        HIPC(c, stream_sync(c));
        for (const Job &j : jobs)
            for (int k = 0; k < j.count; k++) std::memcpy(j.out + (size_t)k * j.stride, j.tmp.data() + (size_t)k * j.dev_stride, 3 * sizeof(T));
        jobs.clear();
        return PGICP_OK;
    }
};
template <typename T>
int fetch_rows3(pgicp_ctx *c, T *out, int stride, const T *dev, int count, RowSpread<T> &late, int dev_stride = 3)
{
    if (!out || count <= 0) return PGICP_OK;
    const size_t vals = (size_t)(count - 1) * dev_stride + 3;
    if (stride == 3 && dev_stride == 3) return d2h(c, out, dev, sizeof(T) * vals);
    late.jobs.push_back({out, stride, dev_stride, count, std::vector<T>(vals)});
    return d2h(c, late.jobs.back().tmp.data(), dev, sizeof(T) * vals);
}

// ---- the two ends VoxelGrid and OctreeGrid share ----
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
// The bounds step: dpf_stat holds the call's VoxStat (*stat; launch_voxel_bounds zeroes its counters), one round trip brings each
// axis's min and max back, in T.  A coordinate that is not finite fails the call of `who` (pgicp_<name>).
template <typename T>
int cloud_bounds(pgicp_ctx *c, const char *who, const T *d_xyz, int stride, int n, VoxStat **stat, T lo[3], T hi[3])
{
    HIPC(c, c->dpf_stat.ensure(sizeof(VoxStat)));
    *stat = c->dpf_stat.as<VoxStat>();
    VoxStat h;
    launch_voxel_bounds<T>(c->stream, d_xyz, stride, n, *stat);
    XFER(c, read_back(c, &h, *stat, sizeof h));
    if (h.bad) return fail(c, PGICP_ERR_ARG, std::string(who) + ": a coordinate is NaN or infinite");
    for (int a = 0; a < 3; a++) { lo[a] = vox_unkey<T>(h.lo[a]); hi[a] = vox_unkey<T>(h.hi[a]); }
    return PGICP_OK;
}
// The tail: the kept count back, then -- host memory -- the packed device outputs into the caller's arrays: the coordinates, `dr`
// descriptor rows, and each (host, device) pair of int32_t arrays whose host side is not null
template <typename T>
int fetch_kept(pgicp_ctx *c, int mem, const VoxStat *stat, T *out_xyz, int out_stride, const T *d_ox, T *out_desc, const T *d_od, int dr,
               std::initializer_list<std::pair<int32_t *, const int32_t *>> ints, int *n_out)
{
    int kept = 0;
    XFER(c, read_back(c, &kept, &stat->kept, sizeof kept));
    if (mem == PGICP_HOST && kept > 0) {
        RowSpread<T> late;
        XFER(c, fetch_rows3<T>(c, out_xyz, out_stride, d_ox, kept, late));
        if (dr) XFER(c, d2h(c, out_desc, d_od, sizeof(T) * (size_t)dr * kept));
        for (const auto &io : ints)
            if (io.first) XFER(c, d2h(c, io.first, io.second, sizeof(int32_t) * (size_t)kept));
        XFER(c, late.land(c));
    }
    *n_out = kept;
    return PGICP_OK;
}

static int pinned_ensure(pgicp_ctx *c, char **buf, size_t *cap, size_t bytes)
{
    if (bytes <= *cap) return PGICP_OK;
    HIPC(c, stream_sync(c));                 // a transfer out of / into the old buffer may still be queued
    if (*buf) (void)t_host_free(*buf);
    *buf = nullptr; *cap = 0;
    HIPC(c, t_host_malloc((void **)buf, bytes + bytes / 4 + 4096, hipHostMallocDefault));
    *cap = bytes + bytes / 4 + 4096;
    return PGICP_OK;
}

size_t staged_bytes(size_t elt, int stride, int n)
{
    size_t b = elt * ((size_t)(n - 1) * stride + 3);
    return (b + 255) & ~(size_t)255;
}

