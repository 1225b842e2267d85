// api_robust.inc -- part of pgicp_api.cpp (one translation unit): pgicp_set_robust_ext / pgicp_get_robust_ext (pgicp_robust.h).  The
// setting itself is laid over the chain by robust_ext_apply and checked against pgicp_params by robust_ext_check (api_context.inc).
extern "C" {

int pgicp_set_robust_ext(pgicp_ctx *c, const pgicp_robust_ext *x)
{
    if (!c) return PGICP_ERR_ARG;
    if (!x) { c->rx_on = 0; c->rx = pgicp_robust_ext{0, 0, 0}; return PGICP_OK; }
    if (x->distance_type != PGICP_ROBUST_DIST_POINT2POINT && x->distance_type != PGICP_ROBUST_DIST_POINT2PLANE)
        return fail(c, PGICP_ERR_ARG, "RobustOutlierFilter: unknown distanceType " + std::to_string(x->distance_type));
    if (x->scale_estimator < -1 || x->scale_estimator > PGICP_ROBUST_SCALE_BERG)
        return fail(c, PGICP_ERR_ARG, "RobustOutlierFilter: unknown scaleEstimator " + std::to_string(x->scale_estimator));
    if (x->nb_iteration_for_scale < 0) return fail(c, PGICP_ERR_ARG, "RobustOutlierFilter: nbIterationForScale must be >= 0");
    { const int st = robust_ext_check(c, *x); if (st) return st; }
    // (a robust chain's selections take no guess from earlier calls -- iter_plan's exact_all -- so the hints need no clearing here)
    c->rx_on = 1;
    c->rx = *x;
    return PGICP_OK;
}

int pgicp_get_robust_ext(const pgicp_ctx *c, int *on, pgicp_robust_ext *x)
{
    if (!c) return PGICP_ERR_ARG;
    if (on) *on = c->rx_on;
    if (x) *x = c->rx;
    return PGICP_OK;
}

}  // extern "C"
