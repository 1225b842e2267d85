// k_sensor_chain.inc -- part of kernels.hip (one translation unit, included inside namespace pgicp): the stages of
// pgicp_sensor_chain_* (include/pgicp_sensor_chain.h) and pgicp_sensor_chain_ext_* (include/pgicp_descriptor_filters.h) behind the
// normals kernel.
//
// The head's rows (normals, eigenvalues, densities) stay where k_surface_normals wrote them, at the points' INPUT indices, and so do
// the rows the stages make (observation directions, noise).  What moves is a list of survivors: idx[r] = the input index of the
// r-th survivor (null: the identity, nothing dropped yet) and its length, which lives on the device (cnt; null: n) -- no count
// comes back to the host between stages.  The stage list is cut behind each dropping stage into segments:
//   1. k_chain_segment: one thread a survivor runs the segment's elementwise stages in list order on registers (the per-point
//      statements are sensor_chain_host.hpp's and descriptor_filters_host.hpp's, shared with the host filters) and ends with the dropping stage's part: Shadow's
//      or CutAtDescriptor's keep flag, or the survivor's density gathered into a contiguous row for MaxDensity.  Ranks past the
//      count get flag 0 / NaN;
//   2. MaxDensity over that row: k_md_max and k_md_count of k_density.inc (a NaN is no maximum and equals nothing, so the padding is
//      inert), then k_chain_md_keep = k_md_keep with n read from the device; with nothing dropped ahead of it launch_max_density
//      itself runs.  The draw's index is the rank, as the statement says;
//   3. launch_exclusive_scan ranks the flags (pos[n] = the new count), k_chain_index composes the survivor list;
//   4. k_chain_gather, once: every row of the survivors to its rank -- the only pass that moves rows.
// Integer atomics only (DensStat); the arithmetic contract of kernels.hip holds.

namespace sc = pgslam_amd::sensor_chain;
namespace df = pgslam_amd::descriptor_filters;

template <typename T>
__global__ __launch_bounds__(256) void k_chain_segment(const T *__restrict__ xyz, int stride, int n, const int *__restrict__ cnt,
                                                       const int *__restrict__ idx, ChainSeg<T> S, ChainRows<T> w, const T *__restrict__ desc,
                                                       int drows, int *__restrict__ keep, T *__restrict__ dens_rank)
{
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    const int m = cnt ? *cnt : n;
    if (r >= m) {
        if (keep) keep[r] = 0;
        if (dens_rank) dens_rank[r] = Bits<T>::val((typename Bits<T>::U)~(typename Bits<T>::U)0);      // a NaN
        return;
    }
    const long long i = idx ? idx[r] : r;
    const T *p = xyz + i * stride;
    const T x[3] = {p[0], p[1], p[2]};
    T nv[3] = {0, 0, 0}, ov[3] = {0, 0, 0};
    bool have_n = false, have_o = false;
#pragma unroll 1
    for (int k = 0; k < S.n_ops; k++) {
        const int op = S.op[k];
        if (op == PGICP_CHAIN_OBSERVATION_DIRECTION) {
            sc::observation_direction<T>(S.c, x, ov);
            w.obs[3 * i] = ov[0]; w.obs[3 * i + 1] = ov[1]; w.obs[3 * i + 2] = ov[2];
            have_o = true;
        } else if (op == PGICP_CHAIN_SIMPLE_SENSOR_NOISE) {
            w.noise[i] = sc::noise_value<T>(S.noise, x);
        } else if (op == PGICP_CHAIN_ORIENT_NORMALS || op == PGICP_CHAIN_INCIDENCE_ANGLE) {
            if (!have_n) { nv[0] = w.nrm[3 * i]; nv[1] = w.nrm[3 * i + 1]; nv[2] = w.nrm[3 * i + 2]; have_n = true; }
            if (!have_o) { ov[0] = w.obs[3 * i]; ov[1] = w.obs[3 * i + 1]; ov[2] = w.obs[3 * i + 2]; have_o = true; }
            if (op == PGICP_CHAIN_INCIDENCE_ANGLE) w.inc[i] = df::incidence_angle<T>(nv, ov);
            else if (sc::orient_flips<T>(nv, ov, S.toward != 0)) {
                nv[0] = -nv[0]; nv[1] = -nv[1]; nv[2] = -nv[2];
                w.nrm[3 * i] = nv[0]; w.nrm[3 * i + 1] = nv[1]; w.nrm[3 * i + 2] = nv[2];
            }
        } else if (op == PGICP_CHAIN_SPHERICALITY) {
            const T e[3] = {w.eig[3 * i], w.eig[3 * i + 1], w.eig[3 * i + 2]};
            T sph, uns, str;
            df::sphericality<T>(e, sph, uns, str);
            w.sph[i] = sph;
            if (S.keep_uns) w.uns[i] = uns;
            if (S.keep_str) w.str[i] = str;
        } else if (op == PGICP_CHAIN_SHADOW) {
            if (!have_n) { nv[0] = w.nrm[3 * i]; nv[1] = w.nrm[3 * i + 1]; nv[2] = w.nrm[3 * i + 2]; have_n = true; }
            keep[r] = sc::shadow_keep<T>(nv, x, S.sin_eps) ? 1 : 0;
        } else if (op == PGICP_CHAIN_CUT_AT_DESCRIPTOR) {
            // (a row made earlier in this segment was written by this thread through the same pointer: it reads its own value)
            const int row = S.cut.row;
            const T v = row == PGICP_CHAIN_ROW_DESC ? desc[i * drows + S.cut.desc_row]
                      : row == PGICP_CHAIN_ROW_DENSITIES ? w.dens[i]
                      : row == PGICP_CHAIN_ROW_INCIDENCE_ANGLES ? w.inc[i]
                      : row == PGICP_CHAIN_ROW_SPHERICALITY ? w.sph[i]
                      : row == PGICP_CHAIN_ROW_UNSTRUCTURENESS ? w.uns[i]
                      : row == PGICP_CHAIN_ROW_STRUCTURENESS ? w.str[i] : w.noise[i];
            keep[r] = df::cut_keep<T>(v, S.cut.thr, S.cut.larger != 0) ? 1 : 0;
        } else if (op == PGICP_CHAIN_MAX_DENSITY) {
            dens_rank[r] = w.dens[i];
        }
    }
}

// k_md_keep (k_density.inc) over the first *cnt entries of a row of n: the same rule, the count read on the device
template <typename T>
__global__ __launch_bounds__(256) void k_chain_md_keep(const T *__restrict__ dens, int n, const int *__restrict__ cnt, T max_density,
                                                       unsigned long long seed, const DensStat *__restrict__ stat, int *__restrict__ keep)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int m = *cnt;
    if (i >= m) { keep[i] = 0; return; }
    const T d = dens[i];
    int k = 1;
    if (d > max_density) {
        float accept = (float)(max_density / d);
        if (d == md_last<T>(*stat)) accept = accept * (float)(1 - stat->saturated / m);       // INTEGER division, as upstream writes it
        k = (double)(seeded_mix(seed, i) >> 11) / 9007199254740992.0 < (double)accept ? 1 : 0;
    }
    keep[i] = k;
}

// the survivor list behind a dropping stage: idx_new[pos[r]] = the input index of survivor r
__global__ __launch_bounds__(256) void k_chain_index(int n, const int *__restrict__ keep, const int *__restrict__ pos,
                                                     const int *__restrict__ idx_old, int *__restrict__ idx_new)
{
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n || !keep[r]) return;
    idx_new[pos[r]] = idx_old ? idx_old[r] : r;
}

// every row of the survivors to its rank (any output may be null; a row that was not made is not asked for)
template <typename T>
__global__ __launch_bounds__(256) void k_chain_gather(int n, const int *__restrict__ cnt, const int *__restrict__ idx, const T *__restrict__ xyz,
                                                      int stride, const T *__restrict__ desc, int drows, ChainRows<T> w, ChainOut<T> o)
{
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n || r >= (cnt ? *cnt : n)) return;
    const long long i = idx ? idx[r] : r, q = r;
    { const T *p = xyz + i * stride; T *d = o.xyz + q * stride; d[0] = p[0]; d[1] = p[1]; d[2] = p[2]; }
    if (o.desc) for (int k = 0; k < drows; k++) o.desc[q * drows + k] = desc[i * drows + k];
    if (o.nrm) { T *d = o.nrm + q * o.nstride; d[0] = w.nrm[3 * i]; d[1] = w.nrm[3 * i + 1]; d[2] = w.nrm[3 * i + 2]; }
    if (o.eig) { o.eig[3 * q] = w.eig[3 * i]; o.eig[3 * q + 1] = w.eig[3 * i + 1]; o.eig[3 * q + 2] = w.eig[3 * i + 2]; }
    if (o.dens) o.dens[q] = w.dens[i];
    if (o.obs) { o.obs[3 * q] = w.obs[3 * i]; o.obs[3 * q + 1] = w.obs[3 * i + 1]; o.obs[3 * q + 2] = w.obs[3 * i + 2]; }
    if (o.noise) o.noise[q] = w.noise[i];
    if (o.inc) o.inc[q] = w.inc[i];
    if (o.sph) o.sph[q] = w.sph[i];
    if (o.uns) o.uns[q] = w.uns[i];
    if (o.str) o.str[q] = w.str[i];
    if (o.kept_idx) o.kept_idx[q] = (int)i;
}

// The stages of a validated list (api_sensor_chain.inc) over the head's rows.  *last_pos: null when nothing drops (n survive), else
// the scan whose entry [n] is the number kept.
template <typename T>
void launch_sensor_chain(hipStream_t st, const T *xyz, int stride, int n, const T *desc, int drows, int n_stages, const int *types,
                         const ChainSeg<T> &params, const ChainCut<T> *cuts, const ChainRows<T> &w, DensStat *stat, const ChainOut<T> &out,
                         const int **last_pos)
{
    const dim3 grid(cdiv(n, 256)), block(256);
    const int *cnt = nullptr, *idx = nullptr;
    int drop = 0;
    ChainSeg<T> S = params;
    S.n_ops = 0;
    for (int k = 0; k < n_stages; k++) {
        S.op[S.n_ops++] = types[k];
        const bool md = types[k] == PGICP_CHAIN_MAX_DENSITY, cut = types[k] == PGICP_CHAIN_CUT_AT_DESCRIPTOR;
        const bool flag = types[k] == PGICP_CHAIN_SHADOW || cut;            // the segment kernel itself writes the keep flags
        if (!flag && !md && k + 1 < n_stages) continue;
        if (cut) S.cut = cuts[k];
        int *keep = flag || md ? w.keep[drop] : nullptr, *pos = flag || md ? w.pos[drop] : nullptr;
        hipLaunchKernelGGL(k_chain_segment<T>, grid, block, 0, st, xyz, stride, n, cnt, idx, S, w, desc, drows, flag ? keep : (int *)nullptr,
                           md ? w.dens_rank : (T *)nullptr);
        S.n_ops = 0;
        if (!flag && !md) break;
        if (flag) launch_exclusive_scan(st, keep, n, pos, w.bsum);
        else if (!cnt) launch_max_density<T>(st, (const T *)w.dens_rank, n, S.max_density, S.seed, stat, keep, pos, w.bsum);
        else {
            (void)hipMemsetAsync(stat, 0, sizeof(DensStat), st);
            hipLaunchKernelGGL(k_md_max<T>, dim3(cdiv(n, 256 * kMdItems)), block, 0, st, (const T *)w.dens_rank, n, stat);
            hipLaunchKernelGGL(k_md_count<T>, grid, block, 0, st, (const T *)w.dens_rank, n, stat);
            hipLaunchKernelGGL(k_chain_md_keep<T>, grid, block, 0, st, (const T *)w.dens_rank, n, cnt, S.max_density, S.seed, (const DensStat *)stat, keep);
            launch_exclusive_scan(st, keep, n, pos, w.bsum);
        }
        hipLaunchKernelGGL(k_chain_index, grid, block, 0, st, n, (const int *)keep, (const int *)pos, idx, w.idx[drop]);
        idx = w.idx[drop];
        cnt = pos + n;
        drop++;
    }
    hipLaunchKernelGGL(k_chain_gather<T>, grid, block, 0, st, n, cnt, idx, xyz, stride, desc, drows, w, out);
    *last_pos = cnt ? cnt - n : nullptr;
}

#define INSTANTIATE_SENSOR_CHAIN(T)                                                                                                    \
    template void launch_sensor_chain<T>(hipStream_t, const T *, int, int, const T *, int, int, const int *, const ChainSeg<T> &,     \
                                         const ChainCut<T> *, const ChainRows<T> &, DensStat *, const ChainOut<T> &, const int **);
INSTANTIATE_SENSOR_CHAIN(float)
INSTANTIATE_SENSOR_CHAIN(double)
#undef INSTANTIATE_SENSOR_CHAIN
