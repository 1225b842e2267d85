// api_descriptor_filters.inc -- part of pgicp_api.cpp (one translation unit): pgicp_sensor_chain_ext_*
// (include/pgicp_descriptor_filters.h).  The call is api_sensor_chain.inc's sensor_chain with the longer list allowed; the entry
// of pgicp_filter_cloud_* that the header also declares is checked in api_filters_uploads.inc (filter_specs).

namespace {

template <typename T>
int sensor_chain_ext(pgicp_ctx *c, const T *xyz, int stride, int n, int mem, int knn, double max_dist, int keep_normals, int keep_eig, int keep_dens,
                     int n_stages, const pgicp_chain_stage *stages, const T *desc, int drows, const pgicp_chain_out *out, int *n_out)
{
    if (!c) return PGICP_ERR_ARG;
    if (!out) return fail(c, PGICP_ERR_ARG, "pgicp_sensor_chain_ext: out is null");
    const ChainOut<T> o{(T *)out->xyz, (T *)out->desc, (T *)out->nrm, out->nstride, (T *)out->eig, (T *)out->dens, (T *)out->obs, (T *)out->noise,
                        (T *)out->incidence, (T *)out->sphericality, (T *)out->unstructureness, (T *)out->structureness, out->kept_idx};
    return sensor_chain<T>(c, xyz, stride, n, mem, knn, max_dist, keep_normals, keep_eig, keep_dens, n_stages, stages, desc, drows, o, n_out, true);
}

}  // namespace

extern "C" {

int pgicp_sensor_chain_ext_f32(pgicp_ctx *c, const float *xyz, int stride, int n, int mem, int knn, double max_dist, int keep_normals, int keep_eig,
                               int keep_dens, int n_stages, const pgicp_chain_stage *stages, const float *desc, int drows, const pgicp_chain_out *out,
                               int *n_out)
{ return sensor_chain_ext<float>(c, xyz, stride, n, mem, knn, max_dist, keep_normals, keep_eig, keep_dens, n_stages, stages, desc, drows, out, n_out); }
int pgicp_sensor_chain_ext_f64(pgicp_ctx *c, const double *xyz, int stride, int n, int mem, int knn, double max_dist, int keep_normals, int keep_eig,
                               int keep_dens, int n_stages, const pgicp_chain_stage *stages, const double *desc, int drows, const pgicp_chain_out *out,
                               int *n_out)
{ return sensor_chain_ext<double>(c, xyz, stride, n, mem, knn, max_dist, keep_normals, keep_eig, keep_dens, n_stages, stages, desc, drows, out, n_out); }

}  // extern "C"
