// k_normals.inc -- part of kernels.hip (one translation unit, included inside namespace pgicp): surface normals (k nearest neighbours in the cloud + 3x3 eigen-decomposition).

// ---------------------------------------------------------------------------
// SurfaceNormalDataPointsFilter ([EXT] libpointmatcher; SURVEY.md section 8(f) rank 2): per point
// of a cloud its knn nearest neighbours IN the cloud, the scatter matrix of those neighbours and the
// eigenvector of its smallest eigenvalue.  The cloud is indexed like any map; lane i owns the point
// in slot i, so a wave is 64 points of one run of cells and shares its neighbourhood in L1.
// The K-entry candidate list lives in registers (every loop over it is unrolled, no dynamic index);
// K - knn dummy entries with distance -1 sit at its front and are never displaced, so the last entry
// is always the current knn-th best: the pruning bound.  Order = lexicographic (d2, original index),
// the order the oracle's k-d tree produces.
// ---------------------------------------------------------------------------
template <typename T, int K>
struct TopK {
    T d[K];
    int idx[K];
    int slot[K];
};

template <typename T, int K>
__device__ __forceinline__ void topk_offer(TopK<T, K> &L, T d, int idx, int slot)
{
    if (!(d < L.d[K - 1] || (d == L.d[K - 1] && idx < L.idx[K - 1]))) return;
    L.d[K - 1] = d; L.idx[K - 1] = idx; L.slot[K - 1] = slot;
#pragma unroll
    for (int p = K - 1; p > 0; --p) {
        const bool sw = L.d[p] < L.d[p - 1] || (L.d[p] == L.d[p - 1] && L.idx[p] < L.idx[p - 1]);
        const T td = L.d[p]; const int ti = L.idx[p], ts = L.slot[p];
        L.d[p] = sw ? L.d[p - 1] : td;       L.idx[p] = sw ? L.idx[p - 1] : ti;       L.slot[p] = sw ? L.slot[p - 1] : ts;
        L.d[p - 1] = sw ? td : L.d[p - 1];   L.idx[p - 1] = sw ? ti : L.idx[p - 1];   L.slot[p - 1] = sw ? ts : L.slot[p - 1];
    }
}

template <typename T, int K>
__device__ __forceinline__ void topk_row(const MapDev<T> &M, int row_base, int xa, int xb, T ux, T lb2, T qx, T qy, T qz,
                                         TopK<T, K> &L)
{
    const T bound = L.d[K - 1];
    if (bound < Bits<T>::inf()) {
        const T rad = sqrt(fmax(bound - lb2, (T)0)) + M.g.margin;
        xa = max(xa, clamp_cell<T>(ux - rad, M.g.inv_h, M.g.nx));
        xb = min(xb, clamp_cell<T>(ux + rad, M.g.inv_h, M.g.nx));
        if (xa > xb) return;
    }
    const int a = tab_coarse_any<T>(M, row_base + xa), b = tab_coarse_any<T>(M, row_base + xb + 1);
    for (int s = a; s < b; ++s) {
        const auto v = load_rec<T>(M.pts, s);
        const T dx = qx - v.x, dy = qy - v.y, dz = qz - v.z;
        topk_offer<T, K>(L, (dx * dx + dy * dy) + dz * dz, Bits<T>::unpack_idx(v.w), s);
    }
}

// exact K nearest map points of (qx, qy, qz) by expanding Chebyshev rings of cells (every entry of L starts at the bound
// maxDist^2: anything beyond is useless)
template <typename T, int K>
__device__ __forceinline__ void topk_walk(const MapDev<T> &M, T qx, T qy, T qz, T max_dist, TopK<T, K> &L)
{
    const GridDesc<T> g = M.g;
    const T ux = qx - g.ox, uy = qy - g.oy, uz = qz - g.oz;
    const int c0x = clamp_cell<T>(ux, g.inv_h, g.nx), c0y = clamp_cell<T>(uy, g.inv_h, g.ny), c0z = clamp_cell<T>(uz, g.inv_h, g.nz);
    for (int r = 0;; ++r) {
        const int z0 = max(c0z - r, 0), z1 = min(c0z + r, g.nz - 1);
        const int y0 = max(c0y - r, 0), y1 = min(c0y + r, g.ny - 1);
        const int xa = max(c0x - r, 0), xb = min(c0x + r, g.nx - 1);
        for (int z = z0; z <= z1; ++z) {
            const T lz = fmax(slab_dist(uz, z, g.h) - g.margin, (T)0);
            const bool zo = (z - c0z == r) || (c0z - z == r);
            for (int y = y0; y <= y1; ++y) {
                const T ly = fmax(slab_dist(uy, y, g.h) - g.margin, (T)0);
                const T lb2 = ly * ly + lz * lz;
                if (lb2 > L.d[K - 1]) continue;
                const int row = g.nx * (y + g.ny * z);
                if (zo || (y - c0y == r) || (c0y - y == r)) {
                    topk_row<T, K>(M, row, xa, xb, ux, lb2, qx, qy, qz, L);
                } else {                         // inner row of the shell: only its two end cells are new
                    if (c0x - r >= 0) topk_row<T, K>(M, row, c0x - r, c0x - r, ux, lb2, qx, qy, qz, L);
                    if (c0x + r <= g.nx - 1 && r > 0) topk_row<T, K>(M, row, c0x + r, c0x + r, ux, lb2, qx, qy, qz, L);
                }
            }
        }
        T gr = ring_guarantee<T>(g, ux, uy, uz, c0x, c0y, c0z, r);
        if (!(gr < Bits<T>::inf())) break;                         // grid exhausted
        gr = gr - g.margin;
        if (gr > (T)0 && (L.d[K - 1] < gr * gr || gr > max_dist)) break;
    }
}

// cyclic Jacobi on a symmetric 3x3 in double -- the same sequence of operations as the oracle's jacobi3
__device__ __forceinline__ void jacobi3(double a[3][3], double v[3][3])
{
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) v[i][j] = i == j ? 1.0 : 0.0;
    for (int sweep = 0; sweep < 16; sweep++) {
        const double off = a[0][1] * a[0][1] + a[0][2] * a[0][2] + a[1][2] * a[1][2];
        if (off == 0.0) break;
#pragma unroll
        for (int p = 0; p < 2; p++)
#pragma unroll
            for (int q = p + 1; q < 3; q++) {
                if (a[p][q] == 0.0) continue;
                const double theta = (a[q][q] - a[p][p]) / (2.0 * a[p][q]);
                const double tt = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                const double c = 1.0 / sqrt(tt * tt + 1.0), s = tt * c;
#pragma unroll
                for (int r = 0; r < 3; r++) {
                    const double arp = a[r][p], arq = a[r][q];
                    a[r][p] = c * arp - s * arq; a[r][q] = s * arp + c * arq;
                }
#pragma unroll
                for (int r = 0; r < 3; r++) {
                    const double apr = a[p][r], aqr = a[q][r];
                    a[p][r] = c * apr - s * aqr; a[q][r] = s * apr + c * aqr;
                }
#pragma unroll
                for (int r = 0; r < 3; r++) {
                    const double vrp = v[r][p], vrq = v[r][q];
                    v[r][p] = c * vrp - s * vrq; v[r][q] = s * vrp + c * vrq;
                }
            }
    }
}

// DENS (pgicp_density.h): the `densities` row as an epilogue -- the neighbours, their count and their mean are at hand, so the
// largest squared distance to the mean rides in the scatter loop and no id table leaves the kernel; out_nrm may then be null.
// The statement is the oracle's orc_densities, in T.  DENS = false is the kernel as it was.
// EXT (pgicp_normals_ext.h): the rows the kernel used to drop, as a second epilogue -- the three eigenvector columns in
// ascending-eigenvalue order, the point's distance to its neighbours' mean, the neighbour ids as values of T -- and, for the
// smoothing pass (k_smooth_normals), the raw normal, the point's index and its neighbours' SLOTS, all in slot order, the table
// transposed ([neighbour][slot]) so that the wave writes and later reads it coalesced.  EXT = false takes no argument for it
// (an empty structure) and is the kernel as it was.
struct NormalsNoExt {};
template <typename T, int K, bool DENS = false, bool EXT = false>
__global__ __launch_bounds__(128) void k_surface_normals(const MapDev<T> *__restrict__ maps, int map, int knn, T max_dist,
                                                          T eps_rank, T *__restrict__ out_nrm, int out_stride,
                                                          T *__restrict__ out_eig, int *__restrict__ out_ids,
                                                          T *__restrict__ out_d2, T *__restrict__ out_dens = nullptr,
                                                          typename std::conditional<EXT, NormalsExtOut<T>, NormalsNoExt>::type x = {})
{
    const MapDev<T> M = maps[map];
    const int s0 = blockIdx.x * blockDim.x + threadIdx.x;
    if (s0 >= M.m) return;
    const auto me = load_rec<T>(M.pts, M.first + s0);
    const T qx = me.x, qy = me.y, qz = me.z;
    const int self = Bits<T>::unpack_idx(me.w);
    const T md2 = max_dist * max_dist;
    TopK<T, K> L;
#pragma unroll
    for (int j = 0; j < K; j++) {
        const bool real = j >= K - knn;
        L.d[j] = real ? md2 : (T)-1;              // anything beyond maxDist is useless
        L.idx[j] = real ? 0x7FFFFFFF : -1;
        L.slot[j] = -1;
    }
    topk_walk<T, K>(M, qx, qy, qz, max_dist, L);
    // ---- scatter matrix of the neighbours, in list order (the oracle's order), in T ----
    int cnt = 0;
    T sx = 0, sy = 0, sz = 0;
#pragma unroll
    for (int j = 0; j < K; j++)
        if (j >= K - knn && L.slot[j] >= 0) {
            const auto v = load_rec<T>(M.pts, L.slot[j]);
            sx += v.x; sy += v.y; sz += v.z; cnt++;
        }
    T c00 = 0, c01 = 0, c02 = 0, c11 = 0, c12 = 0, c22 = 0;
    T r2 = 0;                                                        // DENS: the largest squared distance to the mean, by strict >
    T mean_dist = 0;                                                 // EXT: |point - mean|
    if (cnt > 0) {
        const T mx = sx / (T)cnt, my = sy / (T)cnt, mz = sz / (T)cnt;
        if constexpr (EXT) {
            const T dx = qx - mx, dy = qy - my, dz = qz - mz;
            mean_dist = sqrt_rn_t((dx * dx + dy * dy) + dz * dz);
        }
#pragma unroll
        for (int j = 0; j < K; j++)
            if (j >= K - knn && L.slot[j] >= 0) {
                const auto v = load_rec<T>(M.pts, L.slot[j]);
                const T dx = v.x - mx, dy = v.y - my, dz = v.z - mz;
                c00 += dx * dx; c01 += dx * dy; c02 += dx * dz; c11 += dy * dy; c12 += dy * dz; c22 += dz * dz;
                if constexpr (DENS) { const T q = (dx * dx + dy * dy) + dz * dz; if (q > r2) r2 = q; }
            }
    }
    if constexpr (DENS) {
        if (out_dens) {
            const T r = sqrt_rn_t(r2);
            out_dens[self] = (T)cnt / ((T)((4.0 / 3.0) * 3.14159265358979323846) * ((r * r) * r));
        }
    }
    double A[3][3] = {{(double)c00, (double)c01, (double)c02}, {(double)c01, (double)c11, (double)c12}, {(double)c02, (double)c12, (double)c22}};
    double V[3][3];
    jacobi3(A, V);
    const double e0 = A[0][0], e1 = A[1][1], e2 = A[2][2];
    int lo = 0, hi = 0;
    double elo = e0, ehi = e0;
    if (e1 < elo) { lo = 1; elo = e1; }
    if (e2 < elo) { lo = 2; elo = e2; }
    if (e1 > ehi) { hi = 1; ehi = e1; }
    if (e2 > ehi) { hi = 2; ehi = e2; }
    const int mid = 3 - lo - hi;
    const double emid = lo == hi ? e0 : (mid == 0 ? e0 : (mid == 1 ? e1 : e2));
    const bool degenerate = lo == hi || !(ehi > 0.0) || !(emid > 3.0 * (double)eps_rank * ehi);
    T nx = 0, ny = 1, nz = 0, w0 = 0, w1 = 0, w2 = 1;              // libpointmatcher's defaults for a rank < 2 scatter
    if (!degenerate) {
        nx = (T)(lo == 0 ? V[0][0] : (lo == 1 ? V[0][1] : V[0][2]));
        ny = (T)(lo == 0 ? V[1][0] : (lo == 1 ? V[1][1] : V[1][2]));
        nz = (T)(lo == 0 ? V[2][0] : (lo == 1 ? V[2][1] : V[2][2]));
        w0 = (T)elo; w1 = (T)emid; w2 = (T)ehi;
    }
    if (!DENS || out_nrm) {
        T *o = out_nrm + (long long)self * out_stride;
        o[0] = nx; o[1] = ny; o[2] = nz;
    }
    if (out_eig) { out_eig[3LL * self] = w0; out_eig[3LL * self + 1] = w1; out_eig[3LL * self + 2] = w2; }
    if (out_ids || out_d2) {
#pragma unroll
        for (int j = 0; j < K; j++)
            if (j >= K - knn) {
                const int jj = j - (K - knn);
                const bool ok = L.slot[j] >= 0;
                if (out_ids) out_ids[(long long)self * knn + jj] = ok ? L.idx[j] : -1;
                if (out_d2) out_d2[(long long)self * knn + jj] = ok ? L.d[j] : Bits<T>::inf();
            }
    }
    if constexpr (EXT) {
        if (x.eigvec) {
            // columns lo, mid, hi of V; a rank < 2 scatter: libpointmatcher's defaults (eigenvalues (1,0,0), eigenvectors I) in the
            // same ascending, first-minimum order.  The first column is the normal written above, bit for bit
            T *o = x.eigvec + 9LL * self;
            T m0 = 0, m1 = 0, m2 = 1, h0 = 1, h1 = 0, h2 = 0;
            if (!degenerate) {
                m0 = (T)(mid == 0 ? V[0][0] : (mid == 1 ? V[0][1] : V[0][2]));
                m1 = (T)(mid == 0 ? V[1][0] : (mid == 1 ? V[1][1] : V[1][2]));
                m2 = (T)(mid == 0 ? V[2][0] : (mid == 1 ? V[2][1] : V[2][2]));
                h0 = (T)(hi == 0 ? V[0][0] : (hi == 1 ? V[0][1] : V[0][2]));
                h1 = (T)(hi == 0 ? V[1][0] : (hi == 1 ? V[1][1] : V[1][2]));
                h2 = (T)(hi == 0 ? V[2][0] : (hi == 1 ? V[2][1] : V[2][2]));
            }
            o[0] = nx; o[1] = ny; o[2] = nz; o[3] = m0; o[4] = m1; o[5] = m2; o[6] = h0; o[7] = h1; o[8] = h2;
        }
        if (x.mean_dist) x.mean_dist[self] = mean_dist;
        if (x.raw) {
            x.raw[3LL * s0] = nx; x.raw[3LL * s0 + 1] = ny; x.raw[3LL * s0 + 2] = nz;
            x.self[s0] = self;
        }
        if (x.matched || x.raw) {
#pragma unroll
            for (int j = 0; j < K; j++)
                if (j >= K - knn) {
                    const int jj = j - (K - knn);
                    const bool ok = L.slot[j] >= 0;
                    if (x.matched) x.matched[(long long)self * knn + jj] = ok ? (T)L.idx[j] : (T)-1;
                    if (x.raw) x.nb[(long long)jj * M.m + s0] = ok ? L.slot[j] - M.first : -1;
                }
        }
    }
}

// smoothNormals (pgicp_normals_ext.h): one lane per row of the table.  Row i names its neighbours by position in `nrm` (entry j at
// nb[i * rs + j * cs], -1 = none); the result goes to row out_of[i] of `out` (out_of null: row i).  After k_surface_normals<..,
// EXT> the rows are slots: a wave's 64 points are neighbours in space, so their lists name mostly one another and the gather stays
// in cache.  The arithmetic is the statement's: list order, sums in T, no contraction, a correctly rounded root and division.  An
// id outside [-1, n) is never followed; it raises *bad (bad null: the table is the kernel's own).
template <typename T>
__global__ __launch_bounds__(128) void k_smooth_normals(const T *__restrict__ nrm, int ns, const int *__restrict__ nb, long long rs,
                                                         long long cs, int knn, int n, const int *__restrict__ out_of,
                                                         T *__restrict__ out, int os, int *__restrict__ bad)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const T *r = nrm + (long long)i * ns;
    const T rx = r[0], ry = r[1], rz = r[2];
    T ax = 0, ay = 0, az = 0;
    bool wrong = false;
    for (int j = 0; j < knn; j++) {
        const int id = nb[(long long)i * rs + (long long)j * cs];
        if (id < 0 || id >= n) { wrong = wrong || id != -1; continue; }
        const T *p = nrm + (long long)id * ns;
        const T px = p[0], py = p[1], pz = p[2];
        const T d = (rx * px + ry * py) + rz * pz;
        if (d > (T)0) { ax += px; ay += py; az += pz; }
        else { ax -= px; ay -= py; az -= pz; }
    }
    if (wrong && bad) atomicOr(bad, 1);
    const T len = sqrt_rn_t((ax * ax + ay * ay) + az * az);
    const bool ok = len > (T)0 && len < Bits<T>::inf();
    T *o = out + (long long)(out_of ? out_of[i] : i) * os;
    o[0] = ok ? ax / len : rx; o[1] = ok ? ay / len : ry; o[2] = ok ? az / len : rz;
}

// KDTreeMatcher.knn > 1 (SURVEY.md A.3): the knn nearest map points of every reading point, in (distance, index) order,
// pairs laid out [point][neighbour] as libpointmatcher's knn x N matrices are; -1 / +inf where fewer lie within maxDist.
// One query per lane, no lazy resolution: every later stage sees all knn * N pairs.
template <typename T, int K>
__global__ __launch_bounds__(128) void k_knn_topk(const ProblemDev *__restrict__ probs, const MapDev<T> *__restrict__ maps,
                                                   const T *__restrict__ rd, int *__restrict__ slot_out, T *__restrict__ d2_out,
                                                   ChainDev<T> ch, const int *__restrict__ active)
{
    const ProblemDev &P = probs[active[blockIdx.y]];
    if (P.done) return;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P.n) return;
    const MapDev<T> M = maps[P.map];
    const T *q = rd + 3 * (P.off + i);
    T qx, qy, qz;
    apply_T<T>(tcur_of<T>(P), q[0], q[1], q[2], qx, qy, qz);
    const int knn = P.knn;
    TopK<T, K> L;
#pragma unroll
    for (int j = 0; j < K; j++) {
        const bool real = j >= K - knn;
        L.d[j] = real ? ch.max_dist2 : (T)-1;
        L.idx[j] = real ? 0x7FFFFFFF : -1;
        L.slot[j] = -1;
    }
    topk_walk<T, K>(M, qx, qy, qz, ch.max_dist, L);
    const long long base = pairs_off(P) + (long long)i * knn;
#pragma unroll
    for (int j = 0; j < K; j++)
        if (j >= K - knn) {
            const int jj = j - (K - knn);
            const bool ok = L.slot[j] >= 0;
            slot_out[base + jj] = ok ? L.slot[j] : -1;
            d2_out[base + jj] = ok ? L.d[j] : Bits<T>::inf();
        }
}

// Brute force (parity path): a block owns 256 queries; the map streams through
// LDS in tiles, every lane reads the same LDS address (broadcast, conflict free).
constexpr int kBruteTile = 1024;

template <typename T>
__global__ __launch_bounds__(kKnnBlock) void k_knn_brute(const ProblemDev *__restrict__ probs,
                                                          const MapDev<T> *__restrict__ maps, const T *__restrict__ rd_pre,
                                                          int *__restrict__ slot_out, T *__restrict__ d2_out,
                                                          ChainDev<T> ch, const int *__restrict__ active)
{
    using V4 = typename Vec4<T>::type;
    __shared__ V4 tile[kBruteTile];
    const ProblemDev &P = probs[active[blockIdx.y]];
    if (P.done) return;
    if (blockIdx.x * kKnnBlock >= P.n) return;
    const MapDev<T> M = maps[P.map];
    const int i = blockIdx.x * kKnnBlock + threadIdx.x;
    const bool live = i < P.n;
    T qx = 0, qy = 0, qz = 0;
    if (live) {
        const T *q = rd_pre + 3 * (P.off + i);
        apply_T<T>(tcur_of<T>(P), q[0], q[1], q[2], qx, qy, qz);
    }
    Best<T> best;
    best.d2 = ch.max_dist2; best.idx = 0x7FFFFFFF; best.slot = -1;
    for (int base = 0; base < M.m; base += kBruteTile) {
        const int cnt = min(kBruteTile, M.m - base);
        for (int k = threadIdx.x; k < cnt; k += kKnnBlock) tile[k] = M.pts[M.first + base + k];
        __syncthreads();
        for (int k = 0; k < cnt; ++k) {
            const V4 v = tile[k];
            const T dx = qx - v.x, dy = qy - v.y, dz = qz - v.z;
            const T d = (dx * dx + dy * dy) + dz * dz;
            const int idx = Bits<T>::unpack_idx(v.w);
            if (d < best.d2 || (d == best.d2 && idx < best.idx)) { best.d2 = d; best.idx = idx; best.slot = M.first + base + k; }
        }
        __syncthreads();
    }
    if (live) {
        if (best.slot < 0) best.d2 = Bits<T>::inf();
        slot_out[P.off + i] = best.slot;
        d2_out[P.off + i] = best.d2;
    }
}
