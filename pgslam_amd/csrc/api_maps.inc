// api_maps.inc -- part of pgicp_api.cpp (one translation unit): maps: the device table, the block pool, the batched index build.
template <typename T>
int sync_maps_table(pgicp_ctx *c)
{
    State<T> &S = state<T>(c);
    const int n = (int)S.maps.size();
    if (n == 0) return PGICP_OK;
    if (n > S.d_maps_cap) {
        HIPC(c, stream_sync(c));
        HIPC(c, S.d_maps.ensure(sizeof(MapDev<T>) * (size_t)(n + 16)));
        S.d_maps_cap = n + 16;
    }
    std::vector<MapDev<T>> h(n);
    for (int i = 0; i < n; i++) {
        const MapHost<T> &m = S.maps[i];
        h[i].pts = m.pts; h[i].nrm = m.nrm; h[i].ptsf = m.ptsf; h[i].cell_start = m.cell_start; h[i].g = m.g; h[i].m = m.used ? m.m : 0;
        h[i].cell_start_f = m.cell_start_f; h[i].kx = m.kx; h[i].sw = m.sw; h[i].ostart = m.ostart;
        h[i].sc_count = m.sc_count;
        h[i].slot_of = m.slot_of;
        h[i].val = m.val;
        h[i].near = m.near;
        h[i].sc_dist = m.sc_dist;
        h[i].sc_wit = m.sc_wit;
        h[i].sc_ext = m.sc_ext;
        h[i].occ = m.occ;
        h[i].first = m.first;
        h[i].nsx = (m.g.nx + 7) >> 3; h[i].nsy = (m.g.ny + 7) >> 3; h[i].nsz = (m.g.nz + 7) >> 3;
    }
    XFER(c, h2d(c, S.d_maps.p, h.data(), sizeof(MapDev<T>) * n));
    HIPC(c, stream_sync(c));   // h goes out of scope
    return PGICP_OK;
}

// Freed map blocks are kept for reuse (hipFree waits for the whole device, and loop closing / the streaming mapper create
// and destroy an index per candidate pair / per keyframe).  The pool belongs to the DEVICE, not to a context: in the
// streaming mapper a builder context allocates every block and the serving context -- which received the map through
// pgicp_map_transfer -- releases it; with per-context pools the blocks piled up where nobody allocates.  A pooled block
// carries an event recorded on the releasing context's stream; whoever takes it makes its own stream wait for that event,
// so work still queued on the old owner's stream is ordered before the new contents.
// A batch of 128 loop-closure maps is ONE block of 3-4 GB: with a 2 GiB pool it was never recycled, every batch paid a
// hipMalloc and a (device-synchronising) hipFree of that size -- 1 ms on some hosts, 45 ms on others, which made the
// loop-closing workload run at 4 700 or at 1 700 pairs/s depending on the box.  The pool may hold an eighth of the
// device's memory (36 GB of an MI355X's 288), and a block is allocated an eighth larger than asked for, so that the
// slightly larger batch that follows fits the block of the one before.
constexpr size_t kPoolLimitFallback = (size_t)8 << 30;
struct PooledBlock { char *p; hipEvent_t released; };
struct DevicePool {
    std::mutex m;
    std::multimap<size_t, PooledBlock> blocks;
    size_t bytes = 0;
    size_t limit = 0;               // set on first use: total device memory / 8
    int contexts = 0;
};
// one pool per device, made on first use (never destroyed: contexts may outlive static destruction order)
DevicePool &pool_of(int device)
{
    static std::mutex m;
    static std::vector<DevicePool *> pools;
    std::lock_guard<std::mutex> lock(m);
    if ((size_t)device >= pools.size()) pools.resize((size_t)device + 1, nullptr);
    if (!pools[device]) pools[device] = new DevicePool();
    return *pools[device];
}

int block_alloc(pgicp_ctx *c, size_t bytes, char **out, size_t *got)
{
    DevicePool &dp = pool_of(c->device);
    {
        std::lock_guard<std::mutex> lock(dp.m);
        auto it = dp.blocks.lower_bound(bytes);
        if (it != dp.blocks.end() && it->first <= bytes + bytes / 2 + (1u << 20)) {
            *out = it->second.p; *got = it->first;
            const hipEvent_t ev = it->second.released;
            dp.bytes -= it->first;
            dp.blocks.erase(it);
            if (ev) {
                (void)hipStreamWaitEvent(c->stream, ev, 0);
                (void)hipEventDestroy(ev);             // released once the recorded work has completed
            }
            return PGICP_OK;
        }
    }
    const size_t padded = bytes + bytes / 8;
    if (t_malloc((void **)out, padded) == hipSuccess) { *got = padded; return PGICP_OK; }
    (void)hipGetLastError();
    HIPC(c, t_malloc((void **)out, bytes));
    *got = bytes;
    return PGICP_OK;
}

void block_release(pgicp_ctx *c, char *p, size_t bytes)
{
    if (!p) return;
    if (c) {
        DevicePool &dp = pool_of(c->device);
        std::lock_guard<std::mutex> lock(dp.m);
        if (dp.limit == 0) {
            size_t free_b = 0, total_b = 0;
            dp.limit = hipMemGetInfo(&free_b, &total_b) == hipSuccess && total_b ? total_b / 8 : kPoolLimitFallback;
        }
        if (dp.bytes + bytes <= dp.limit) {
            PooledBlock b{p, nullptr};
            if (hipEventCreateWithFlags(&b.released, hipEventDisableTiming) == hipSuccess) (void)hipEventRecord(b.released, c->stream);
            else b.released = nullptr;
            dp.blocks.emplace(bytes, b);
            dp.bytes += bytes;
            return;
        }
    }
    (void)t_free(p);
}

// Work on the context stream that uses the map is ordered before whatever reuses the block (block_release records an
// event there); work queued on OTHER streams must have been waited for by the caller.
template <typename T>
void free_map(pgicp_ctx *c, MapHost<T> &m)
{
    if (m.block && m.block.use_count() == 1 && m.block->p) {
        block_release(c, m.block->p, m.block->bytes);
        m.block->p = nullptr;
    }
    m = MapHost<T>();
    if (c) ++c->map_clock;          // (pgicp_ctx_destroy frees its maps with no context: the block goes straight back to the device)
}

// one reference cloud of a batched map creation
template <typename T>
struct MapSrc {
    const T *xyz; int xyz_stride; const T *nrm; int nrm_stride; int m;
};

// Builds n maps with ONE host round trip: all centroid/bbox kernels first, one copy back of the
// statistics, then every grid build back to back on the context stream.  Each map's arrays live in a
// single device allocation.
template <typename T>
int map_create_batch(pgicp_ctx *c, int n, const MapSrc<T> *src, int mem, int center, int *map_ids)
{
    if (!c || n <= 0 || !src || !map_ids) return fail(c, PGICP_ERR_ARG, "pgicp_map_create: bad argument");
    for (int k = 0; k < n; k++)
        if (!src[k].xyz || src[k].m <= 0 || src[k].xyz_stride < 3 || (src[k].nrm && src[k].nrm_stride < 3))
            return fail(c, PGICP_ERR_ARG, "pgicp_map_create: bad argument");
    HIPC(c, hipSetDevice(c->device));
    State<T> &S = state<T>(c);
    UploadUse use(c);
    using V4 = typename Vec4<T>::type;
    // ---- phase 1: inputs on the device, centroid + bbox of every cloud ----
    std::vector<const T *> d_xyz(n), d_nrm(n, nullptr);
    if (mem == PGICP_HOST) {
        size_t tot = 0;
        for (int k = 0; k < n; k++)
            tot += staged_bytes(sizeof(T), src[k].xyz_stride, src[k].m) + (src[k].nrm ? staged_bytes(sizeof(T), src[k].nrm_stride, src[k].m) : 0);
        HIPC(c, S.staging.ensure(tot));
    }
    size_t soff = 0;
    for (int k = 0; k < n; k++) {
        if (mem == PGICP_DEVICE && (c->up[0].pending || c->up[1].pending)) {       // clouds handed out by pgicp_upload_*
            (void)upload_wait(c, src[k].xyz);                                       // (this call ends with a stream synchronisation:
            if (src[k].nrm) (void)upload_wait(c, src[k].nrm);                       //  nothing of it reads them afterwards)
        }
        int st = to_device<T>(c, src[k].xyz, src[k].xyz_stride, src[k].m, mem, S.staging, soff, &d_xyz[k]);
        if (st) return st;
        if (mem == PGICP_HOST) soff += staged_bytes(sizeof(T), src[k].xyz_stride, src[k].m);
        if (src[k].nrm) {
            st = to_device<T>(c, src[k].nrm, src[k].nrm_stride, src[k].m, mem, S.staging, soff, &d_nrm[k]);
            if (st) return st;
            if (mem == PGICP_HOST) soff += staged_bytes(sizeof(T), src[k].nrm_stride, src[k].m);
        }
    }
    std::vector<unsigned long long> h_stats((size_t)9 * n);
    for (int k = 0; k < n; k++) {
        unsigned long long *s = h_stats.data() + 9 * k;
        s[0] = s[1] = s[2] = 0; s[3] = s[4] = s[5] = ~0ULL; s[6] = s[7] = s[8] = 0;
    }
    std::vector<BuildDesc<T>> descs(n);
    int max_m = 0;
    for (int k = 0; k < n; k++) {
        BuildDesc<T> &d = descs[k];
        std::memset(&d, 0, sizeof d);
        d.xyz = d_xyz[k]; d.nrm = d_nrm[k]; d.xstride = src[k].xyz_stride; d.nstride = src[k].nrm_stride; d.m = src[k].m;
        max_m = std::max(max_m, src[k].m);
    }
    HIPC(c, c->stats.ensure(sizeof(unsigned long long) * 9 * (size_t)n));
    HIPC(c, c->bdesc.ensure(sizeof(BuildDesc<T>) * (size_t)n));
    XFER(c, h2d(c, c->stats.p, h_stats.data(), sizeof(unsigned long long) * 9 * n));
    XFER(c, h2d(c, c->bdesc.p, descs.data(), sizeof(BuildDesc<T>) * n));
    {
        ProfScope ps(c, PGICP_PROF_GRID_BUILD, max_m, n);
        launch_centroid_bbox_batch<T>(c->stream, c->bdesc.as<BuildDesc<T>>(), n, max_m, c->stats.as<unsigned long long>());
    }
    XFER(c, d2h(c, h_stats.data(), c->stats.p, sizeof(unsigned long long) * 9 * n));
    HIPC(c, stream_sync(c));

    // ---- phase 2: grids; every cloud gets its slice of ONE allocation and ONE set of build launches ----
    std::vector<MapHost<T>> Ms(n);
    long long tot_m = 0, tot_c = 0, tot_s = 0, tot_f = 0, tot_o = 0, tot_b = 0, tot_w = 0;
    // The succinct table (MapDev::sw) is an OPTION (PGICP_TABLES=succinct), the dense tables the default for every map:
    // measured in round 6 (profiles/r06_experiments/succinct_tables.txt) the succinct table makes a 100 k-pt map's tables 1.1 MB
    // instead of 14 MB and the batched build 0.9 ms shorter per 512 maps, but the fast matcher pays a third dependent load and
    // ~290 more instructions: +7 % per launch in loop closing (its traffic -13 %: the launches' bytes are results and points,
    // not tables), -6 % headline, -5 % streaming.  It is what a map too sparse for dense tables would be built with.
    const bool succ = c->table_mode == 2;
    int max_cells = 0, max_nsc = 0, max_bins = 0, max_blocks = 0;
    const int kx = std::max(1, std::min(8, c->grid_kx));
    bool any_nrm = false;
    for (int k = 0; k < n; k++) {
        MapHost<T> &M = Ms[k];
        const int m = src[k].m;
        const unsigned long long *st = h_stats.data() + 9 * k;
        M.used = true; M.m = m; M.has_nrm = src[k].nrm != nullptr;
        any_nrm = any_nrm || M.has_nrm;
        double lo[3], hi[3];
        for (int a = 0; a < 3; a++) {
            // the centroid is an order-independent fixed-point sum (2^-24 units in an int64): sum |v| 2^24 must stay
            // below 2^63 -- e.g. a million points at ECEF / UTM-scale coordinates would wrap silently.  Refused, not wrong.
            // An uncentred map (mean 0, as pgicp_surface_normals builds its cloud) never reads the sum: no limit there.
            const double vmax = std::max(std::fabs((double)key_to_double(st[3 + a])), std::fabs((double)key_to_double(st[6 + a])));
            if (center && vmax * (double)m >= 5.0e11)
                return fail(c, PGICP_ERR_ARG, "pgicp_map_create: |coordinate| x points = " + std::to_string(vmax * (double)m) +
                                              " overflows the centroid's fixed-point sum (limit 5e11): express the cloud in a local frame first");
            const double mean_d = ((double)(long long)st[a] / 16777216.0) / (double)m;
            M.mean[a] = center ? (T)mean_d : (T)0;
            // rounding is monotone: min/max of fl(x - mean) are fl(min - mean), fl(max - mean)
            lo[a] = (double)((T)key_to_double(st[3 + a]) - M.mean[a]);
            hi[a] = (double)((T)key_to_double(st[6 + a]) - M.mean[a]);
            if (!(lo[a] <= hi[a]) || !std::isfinite(lo[a]) || !std::isfinite(hi[a]))
                return fail(c, PGICP_ERR_ARG, "pgicp_map_create: non-finite coordinates");
        }
        const double ex = hi[0] - lo[0], ey = hi[1] - lo[1], ez = hi[2] - lo[2];
        double h = c->prm.grid_cell;
        if (!(h > 0)) {
            // Range-scan clouds sit on surfaces (and, ring by ring, on curves): cells sized for ~2
            // points per cell of the projected bounding-box area end up holding ~15-20 points where
            // the data actually is (measured on the Velodyne-shaped benchmark map).
            const double area = ex * ey + ey * ez + ex * ez;
            h = std::sqrt(2.0 * std::max(area, 1e-12) / (double)m);
            const double diag = std::sqrt(ex * ex + ey * ey + ez * ez);
            h *= c->cell_scale;
            if (!(h > diag * 1e-4)) h = std::max(diag * 1e-4, 1e-6);
        }
        for (;;) {   // bound the dense cell table
            const double nx = std::floor(ex / h) + 1, ny = std::floor(ey / h) + 1, nz = std::floor(ez / h) + 1;
            if (nx <= 65535 && ny <= 65535 && nz <= 65535 && nx * ny * nz <= 67108864.0) break;
            h *= 1.26;
        }
        GridDesc<T> &g = M.g;
        g.h = (T)h; g.inv_h = (T)1 / g.h; g.margin = (T)0.02 * g.h;
        g.ox = (T)lo[0]; g.oy = (T)lo[1]; g.oz = (T)lo[2];
        g.nx = (int)std::floor(ex / (double)g.h) + 1; g.ny = (int)std::floor(ey / (double)g.h) + 1;
        g.nz = (int)std::floor(ez / (double)g.h) + 1;
        BuildDesc<T> &d = descs[k];
        d.g = g;
        for (int a = 0; a < 3; a++) d.mean[a] = M.mean[a];
        d.ncells = g.nx * g.ny * g.nz;
        d.nsc = ((g.nx + 7) >> 3) * ((g.ny + 7) >> 3) * ((g.nz + 7) >> 3);
        d.pbase = tot_m; d.cbase = tot_c; d.sbase = tot_s; d.fbase = tot_f; d.obase = tot_o; d.bbase = tot_b; d.wbase = tot_w;
        d.kx = kx; d.ncells_f = d.ncells * kx;
        d.nbins = (d.ncells_f >> 9) + 1;                 // bins of the build's counting sort: 512 fine cells (kMapBinShift), sentinel included
        M.kx = kx;
        // a first candidate farther than a fraction of maxDist prunes little: do not look for one beyond that
        const double reach_len = std::isfinite(c->prm.max_dist) ? c->near_frac * c->prm.max_dist : 1e30;
        d.near_reach = (int)std::min((double)kNearReach, std::max(2.0, std::ceil(reach_len / (double)g.h)));
        tot_m += m; tot_c += (long long)d.ncells + 1; tot_s += d.nsc;
        tot_f += ((long long)d.ncells_f + 1 + 3) & ~3LL;     // (every cloud's fine table starts on a 16-byte boundary: k_mfill stores four entries at a time)
        tot_o += (long long)(d.ncells >> 5) + 2;         // (a range test reads one word past the last cell's)
        tot_b += d.nbins;
        tot_w += (long long)(d.ncells_f >> 6) + 2;       // (the sentinel cell's group, and one to spare)
        max_cells = std::max(max_cells, d.ncells);
        max_bins = std::max(max_bins, d.nbins);
        max_nsc = std::max(max_nsc, d.nsc);
        max_blocks = std::max(max_blocks, ((g.nx + 1) >> 1) * ((g.ny + 1) >> 1) * ((g.nz + 1) >> 1));
    }
    if (tot_m > 0x7FFFFFF0LL || tot_c > 0x7FFFFFF0LL) {
        // the concatenated index space must fit an int: an oversized batch is built in two halves (each may split again)
        if (n == 1) return fail(c, PGICP_ERR_ARG, "pgicp_map_create: cloud too large");
        const int half = n / 2;
        const int st1 = map_create_batch<T>(c, half, src, mem, center, map_ids);
        if (st1) return st1;
        return map_create_batch<T>(c, n - half, src + half, mem, center, map_ids + half);
    }
    const size_t n_scratch = (size_t)std::max(tot_b + 2, tot_c);
    HIPC(c, c->tmp_a.ensure(sizeof(int) * (size_t)tot_m));                               // fine-cell keys: by point, then by slot
    HIPC(c, c->tmp_b.ensure(sizeof(int) * n_scratch));                                   // bin counts, then sweep scratch
    HIPC(c, c->tmp_c.ensure(sizeof(int) * scan_scratch_ints((size_t)std::max(tot_b + 1, succ ? tot_m + 1 : 0LL))));  // the scans' block sums
    if (succ) {                                                                           // first-of-cell flags, and their ranks
        HIPC(c, c->tmp_f.ensure(sizeof(int) * (size_t)(tot_m + 1)));
        HIPC(c, c->tmp_r.ensure(sizeof(int) * (size_t)(tot_m + 1)));
    }
    HIPC(c, c->tmp_d.ensure(sizeof(int) * n_scratch));                                   // bin starts, then sweep scratch
    HIPC(c, c->tmp_e.ensure(sizeof(int) * (size_t)tot_m));                               // arrival positions
    HIPC(c, c->tmp_w.ensure(sizeof(unsigned long long) * (size_t)tot_m));                // (fine cell, index) words of the cell sort
    HIPC(c, c->tmp_p.ensure(sizeof(V4) * 2 * (size_t)tot_m));                            // the records in cloud order: (point, normal) pairs
    auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
    // (succinct: no dense tables -- b_cs keeps one entry so that the layout below stays one expression)
    const size_t b_pts = up(sizeof(V4) * (size_t)tot_m), b_nrm = any_nrm ? up(2 * sizeof(V4) * (size_t)tot_m) : 0, b_cs = up(sizeof(int) * (size_t)(succ ? 1 : tot_c)),
                 b_slot = up(sizeof(int) * (size_t)tot_m), b_sc = up(sizeof(int) * (size_t)tot_s), b_near = up(sizeof(int) * (size_t)tot_c),
                 b_csf = (kx > 1 && !succ) ? up(sizeof(int) * (size_t)tot_f) : 0, b_occ = up(sizeof(unsigned) * (size_t)tot_o),
                 b_ext = up(sizeof(float) * 6 * (size_t)tot_s), b_ptsf = sizeof(T) == 8 ? up(sizeof(float) * 4 * (size_t)tot_m + 64) : 0,
                 b_sw = succ ? up(sizeof(uint4) * (size_t)tot_w) : 0, b_ost = succ ? up(sizeof(int) * (size_t)(tot_m + 2)) : 0;
    auto blk = std::make_shared<SharedBlock>();
    { const int ast = block_alloc(c, b_pts + b_nrm + b_cs + b_slot + 3 * b_sc + b_near + b_csf + b_occ + b_ext + b_ptsf + b_sw + b_ost, &blk->p, &blk->bytes); if (ast) return ast; }
    char *base = blk->p;
    V4 *g_pts = (V4 *)base, *g_nrm = any_nrm ? (V4 *)(base + b_pts) : nullptr;
    int *g_cs = (int *)(base + b_pts + b_nrm), *g_slot = (int *)(base + b_pts + b_nrm + b_cs),
        *g_sc = (int *)(base + b_pts + b_nrm + b_cs + b_slot), *g_near = (int *)(base + b_pts + b_nrm + b_cs + b_slot + b_sc),
        *g_scd = (int *)(base + b_pts + b_nrm + b_cs + b_slot + b_sc + b_near),
        *g_wit = (int *)(base + b_pts + b_nrm + b_cs + b_slot + 2 * b_sc + b_near),
        *g_csf = kx > 1 ? (int *)(base + b_pts + b_nrm + b_cs + b_slot + 3 * b_sc + b_near) : g_cs;
    unsigned *g_occ = (unsigned *)(base + b_pts + b_nrm + b_cs + b_slot + 3 * b_sc + b_near + b_csf);
    float *g_ext = (float *)(base + b_pts + b_nrm + b_cs + b_slot + 3 * b_sc + b_near + b_csf + b_occ);
    float *g_ptsf = b_ptsf ? (float *)(base + b_pts + b_nrm + b_cs + b_slot + 3 * b_sc + b_near + b_csf + b_occ + b_ext) : nullptr;   // (16-byte records: blocks are 256-byte aligned)
    uint4 *g_sw = succ ? (uint4 *)(base + b_pts + b_nrm + b_cs + b_slot + 3 * b_sc + b_near + b_csf + b_occ + b_ext + b_ptsf) : nullptr;
    int *g_ost = succ ? (int *)(base + b_pts + b_nrm + b_cs + b_slot + 3 * b_sc + b_near + b_csf + b_occ + b_ext + b_ptsf + b_sw) : nullptr;
    for (int k = 0; k < n; k++) {
        MapHost<T> &M = Ms[k];
        const BuildDesc<T> &d = descs[k];
        M.block = blk;
        M.pts = g_pts;                               // shared by the batch; this map's points start at slot `first`
        M.nrm = M.has_nrm ? g_nrm : nullptr;
        M.first = (int)d.pbase;
        M.cell_start = succ ? nullptr : g_cs + d.cbase;
        M.cell_start_f = succ ? nullptr : g_csf + d.fbase;
        M.sw = succ ? g_sw + d.wbase : nullptr;
        M.ostart = g_ost;
        M.slot_of = g_slot + d.pbase;
        M.sc_count = g_sc + d.sbase;
        M.near = g_near + d.cbase;
        M.sc_dist = g_scd + d.sbase;
        M.sc_wit = g_wit + d.sbase;
        M.sc_ext = g_ext + 6 * d.sbase;
        M.occ = g_occ + d.obase;
        M.ptsf = g_ptsf;                             // (indexed by slot, like pts)
    }
    XFER(c, h2d(c, c->bdesc.p, descs.data(), sizeof(BuildDesc<T>) * n));
    {
        ProfScope ps(c, PGICP_PROF_GRID_BUILD, tot_m, n);
        launch_grid_build_batch<T>(c->stream, c->bdesc.as<BuildDesc<T>>(), n, tot_m, tot_b, tot_s, max_m, max_cells, max_bins, max_nsc, max_blocks, kx == 4 ? 1 : 0, c->tmp_a.as<int>(),
                                   c->tmp_b.as<int>(), c->tmp_c.as<int>(), g_cs, g_csf, c->tmp_d.as<int>(), c->tmp_e.as<int>(), c->tmp_w.as<unsigned long long>(), c->tmp_p.as<V4>(), c->tmp_n.as<V4>(), g_pts, g_nrm,
                                   g_slot, g_sc, g_near, g_scd, g_wit, g_occ, tot_o, g_ext, g_ptsf, g_sw, g_ost, succ ? c->tmp_f.as<int>() : nullptr, succ ? c->tmp_r.as<int>() : nullptr);
    }
    HIPC(c, stream_sync(c));          // `descs` (host) feeds an async copy
    HIPC(c, hipGetLastError());
    // ---- phase 3: register ----
    for (int k = 0; k < n; k++) {
        int id = -1;
        for (size_t i = 0; i < S.maps.size(); i++) if (!S.maps[i].used) { id = (int)i; break; }
        if (id < 0) { S.maps.push_back(MapHost<T>()); id = (int)S.maps.size() - 1; }
        S.maps[id] = Ms[k];
        S.maps[id].stamp = ++c->map_clock;
        map_ids[k] = id | id_tag<T>();
    }
    return sync_maps_table<T>(c);
}

template <typename T>
int map_create(pgicp_ctx *c, const T *xyz, int xyz_stride, const T *nrm, int nrm_stride, int m, int mem, int center,
               int *map_id)
{
    if (!map_id) return fail(c, PGICP_ERR_ARG, "pgicp_map_create: bad argument");
    MapSrc<T> s{xyz, xyz_stride, nrm, nrm_stride, m};
    return map_create_batch<T>(c, 1, &s, mem, center, map_id);
}


// pgicp_map_set_values: values[i * stride] of every map point i, into the map's slot order (its own allocation)
template <typename T>
int map_set_values(pgicp_ctx *c, int map_id, const T *values, int stride, int mem)
{
    if (!c) return PGICP_ERR_ARG;
    MapHost<T> *M = get_map<T>(c, map_id);
    if (!M) return fail(c, PGICP_ERR_ARG, "pgicp_map_set_values: unknown map id");
    HIPC(c, hipSetDevice(c->device));
    if (!values) {
        HIPC(c, stream_sync(c));                  // (work queued on the stream may still read the old values)
        M->vblock.reset(); M->val = nullptr; M->val_neg = false;
        return sync_maps_table<T>(c);
    }
    if (stride < 1 || (mem != PGICP_HOST && mem != PGICP_DEVICE)) return fail(c, PGICP_ERR_ARG, "pgicp_map_set_values: bad argument");
    const int m = M->m;
    const size_t vbytes = sizeof(T) * (size_t)m;
    const T *d_src = values;
    int d_stride = stride;
    std::vector<T> packed;
    HIPC(c, c->gd_stage.ensure(64 + (mem == PGICP_HOST ? vbytes : 0)));
    if (mem == PGICP_HOST) {
        packed.resize((size_t)m);
        for (int i = 0; i < m; i++) packed[(size_t)i] = values[(size_t)i * stride];
        XFER(c, h2d(c, (char *)c->gd_stage.p + 64, packed.data(), vbytes));
        d_src = (const T *)((char *)c->gd_stage.p + 64);
        d_stride = 1;
    }
    auto blk = std::make_shared<SharedBlock>();
    HIPC(c, t_malloc((void **)&blk->p, vbytes));
    blk->bytes = vbytes;
    HIPC(c, hipMemsetAsync(c->gd_stage.p, 0, 2 * sizeof(int), c->stream));
    launch_map_values<T>(c->stream, M->pts, M->first, m, d_src, d_stride, (T *)blk->p, c->gd_stage.as<int>());
    int flags[2] = {0, 0};
    XFER(c, d2h(c, flags, c->gd_stage.p, sizeof flags));
    HIPC(c, stream_sync(c));
    HIPC(c, hipGetLastError());
    if (flags[0]) return fail(c, PGICP_ERR_ARG, "pgicp_map_set_values: a value is not finite (GenericDescriptorOutlierFilter)");
    // (the old values, if any, go now: nothing queued reads them any more -- the stream has run dry)
    M->vblock = blk;
    M->val = (T *)blk->p;
    M->val_neg = flags[1] != 0;
    return sync_maps_table<T>(c);
}

// every map of a call that runs the GenericDescriptor filter must carry values (non-negative ones in soft mode)
template <typename T>
int descriptor_filter_check(pgicp_ctx *c, const MapHost<T> *M, int map_id)
{
    if (c->gd_mode == PGICP_DESC_FILTER_OFF) return PGICP_OK;
    if (!M->val)
        return fail(c, PGICP_ERR_ARG, "GenericDescriptorOutlierFilter: map " + std::to_string(map_id) + " has no values (pgicp_map_set_values)");
    if (c->gd_mode == PGICP_DESC_FILTER_SOFT && M->val_neg)
        return fail(c, PGICP_ERR_ARG, "GenericDescriptorOutlierFilter: soft mode needs values >= 0 (map " + std::to_string(map_id) + " holds a negative one)");
    return PGICP_OK;
}
