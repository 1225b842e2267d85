// api_normalspace.inc -- part of pgicp_api.cpp (one translation unit): pgicp_normal_space_sampling_* (include/
// pgicp_normalspace.h).  The grid and the draw between the two kernels are include/pgslam_amd/normalspace_host.hpp, which the C++
// drop-in's host form shares.

namespace {

namespace nsp = pgslam_amd::normalspace;

template <typename T>
int normal_space_sampling(pgicp_ctx *c, const T *xyz, int stride, const T *nrm, int nstride, int n, int mem, int nb_sample, double epsilon,
                          unsigned long long seed, const T *desc, int drows, T *out_xyz, T *out_nrm, int out_nstride, T *out_desc, int32_t *kept_idx,
                          int32_t *bucket_out, int *n_out)
{
    nsp::Grid grid;
    if (!c || n < 0 || (n > 0 && (!xyz || !nrm)) || stride < 3 || nstride < 3 || (out_nrm && out_nstride < 3) || nb_sample < 1 ||
        (mem != PGICP_HOST && mem != PGICP_DEVICE) || !n_out || (desc && (drows <= 0 || !out_desc)) || (long long)n + 2 > 0x7FFFFFFFLL ||
        seed >= (1ULL << 53) || !nsp::make_grid(epsilon, grid))
        return fail(c, PGICP_ERR_ARG,
                    "pgicp_normal_space_sampling: bad argument (n >= 0, nb_sample >= 1, epsilon finite, > 0, <= pi and at most 65536 buckets, "
                    "seed < 2^53, strides >= 3, out_desc with desc)");
    *n_out = 0;
    if (n == 0) return PGICP_OK;
    HIPC(c, hipSetDevice(c->device));
    UploadUse uu(c);
    const int dr = desc ? drows : 0;
    const bool noop = nb_sample >= n;
    const int m = noop ? n : nb_sample;
    NsScratch w;
    XFER(c, carve_buf(c, c->dpf_work, [&](Carve &cv) { w = ns_scratch(cv, n, m, grid.nbBucket); }));
    CloudIn<T> in;
    const T *d_nrm = nrm;
    T *d_ox = out_xyz, *d_on = out_nrm, *d_od = out_desc;
    int32_t *d_oi = kept_idx, *d_ob = bucket_out;
    int ons = out_nstride;
    if (mem == PGICP_HOST) {
        // io: the cloud, its normals and descriptors as uploaded, then the outputs (coordinates at `stride`, the rest packed)
        XFER(c, carve_buf(c, c->dpf_io, [&](Carve &cv) {
            in.carve(cv, stride, n, dr);
            d_nrm = cv.take<T>((size_t)(n - 1) * nstride + 3);
            d_ox = cv.take<T>((size_t)(m - 1) * stride + 3, out_xyz);
            d_on = cv.take<T>(3 * (size_t)m, out_nrm);
            d_od = cv.take<T>((size_t)dr * m, desc);
            d_oi = cv.take<int32_t>((size_t)m, kept_idx);
            d_ob = cv.take<int32_t>((size_t)m, bucket_out);
        }));
        ons = 3;
        XFER(c, h2d(c, (void *)d_nrm, nrm, sizeof(T) * ((size_t)(n - 1) * nstride + 3)));
    } else
        uu.touch(nrm);
    XFER(c, upload_cloud<T>(c, mem, xyz, stride, n, desc, dr, in));
    const int *d_pos = nullptr;
    const unsigned long long *d_skey = nullptr;
    const int *d_sidx = nullptr;
    if (!noop) {
        NsGrid g;
        g.epsilon = epsilon; g.n_phi = grid.nPhi; g.n_theta = grid.nTheta; g.nb_bucket = grid.nbBucket;
        const int cur = launch_ns_sort<T>(c->stream, d_nrm, nstride, n, g, seed, w);
        std::vector<int32_t> counts((size_t)grid.nbBucket + 1);
        XFER(c, read_back(c, counts.data(), w.counts, sizeof(int32_t) * counts.size()));      // the one sync: the counts and the flag
        if (counts[(size_t)grid.nbBucket]) return fail(c, PGICP_ERR_ARG, "pgicp_normal_space_sampling: a normal component is NaN or infinite");
        std::vector<int32_t> start((size_t)grid.nbBucket + 1, 0), pb, pr;
        for (int b = 0; b < grid.nbBucket; b++) {
            if (counts[(size_t)b] < 0) return fail(c, PGICP_ERR_HIP, "pgicp_normal_space_sampling: internal error: a negative count");
            start[(size_t)b + 1] = start[(size_t)b] + counts[(size_t)b];
        }
        if (start[(size_t)grid.nbBucket] != n) return fail(c, PGICP_ERR_HIP, "pgicp_normal_space_sampling: internal error: the counts do not sum to n");
        nsp::draw(counts.data(), grid.nbBucket, m, seed, pb, pr);
        for (int j = 0; j < m; j++) pr[(size_t)j] += start[(size_t)pb[(size_t)j]];            // the position in the sorted order
        XFER(c, h2d(c, w.pos, pr.data(), sizeof(int32_t) * (size_t)m));
        d_pos = w.pos; d_skey = w.sort.key[cur]; d_sidx = w.sort.idx[cur];
    }
    launch_gather_rows<T>(c->stream, d_pos, d_skey, d_sidx, m, n, in.xyz, stride, d_nrm, nstride, in.desc, dr, d_ox, stride, d_on, ons, d_od, d_oi, d_ob);
    if (mem == PGICP_HOST) {
        RowSpread<T> late;
        XFER(c, fetch_rows3<T>(c, out_xyz, stride, d_ox, m, late, stride));
        XFER(c, fetch_rows3<T>(c, out_nrm, out_nstride, d_on, m, late));
        if (desc) XFER(c, d2h(c, out_desc, d_od, sizeof(T) * (size_t)dr * m));
        if (kept_idx) XFER(c, d2h(c, kept_idx, d_oi, sizeof(int32_t) * (size_t)m));
        if (bucket_out) XFER(c, d2h(c, bucket_out, d_ob, sizeof(int32_t) * (size_t)m));
        XFER(c, late.land(c));
    } else
        HIPC(c, stream_sync(c));
    HIPC(c, hipGetLastError());
    *n_out = m;
    return PGICP_OK;
}

}  // namespace

extern "C" {

int pgicp_normal_space_sampling_f32(pgicp_ctx *ctx, const float *xyz, int stride, const float *nrm, int nstride, int n, int mem, int nb_sample,
                                    double epsilon, unsigned long long seed, const float *desc, int drows, float *out_xyz, float *out_nrm,
                                    int out_nstride, float *out_desc, int32_t *kept_idx, int32_t *bucket_out, int *n_out)
{
    return normal_space_sampling<float>(ctx, xyz, stride, nrm, nstride, n, mem, nb_sample, epsilon, seed, desc, drows, out_xyz, out_nrm, out_nstride,
                                        out_desc, kept_idx, bucket_out, n_out);
}
int pgicp_normal_space_sampling_f64(pgicp_ctx *ctx, const double *xyz, int stride, const double *nrm, int nstride, int n, int mem, int nb_sample,
                                    double epsilon, unsigned long long seed, const double *desc, int drows, double *out_xyz, double *out_nrm,
                                    int out_nstride, double *out_desc, int32_t *kept_idx, int32_t *bucket_out, int *n_out)
{
    return normal_space_sampling<double>(ctx, xyz, stride, nrm, nstride, n, mem, nb_sample, epsilon, seed, desc, drows, out_xyz, out_nrm, out_nstride,
                                         out_desc, kept_idx, bucket_out, n_out);
}

}  // extern "C"
