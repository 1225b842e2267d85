// The product's checker_check (pgslam_amd/csrc/icp_math.hpp: what k_solve_update runs per problem), compiled for the host
// and exported for ctypes: tests/test_checkers_ref_host.py walks it past its 16-entry history, which no device run is
// needed for; and small_angles / det_atan2, which the covariance kernel runs.  Built with -ffp-contract=off (the arithmetic contract: no FMA is formed).
#include "icp_math.hpp"

extern "C" {

int pgicp_host_checker_size() { return (int)sizeof(pgicp::Checker); }
int pgicp_host_checker_hist() { return pgicp::kHist; }
void pgicp_host_checker_init(void *c) { pgicp::checker_init(*(pgicp::Checker *)c); }
int pgicp_host_checker_check(void *c, const double *T, int max_iters, double min_rot, double min_trans, int smooth,
                             double bound_rot, double bound_trans)
{
    return pgicp::checker_check(*(pgicp::Checker *)c, T, max_iters, min_rot, min_trans, smooth, bound_rot, bound_trans);
}

// the covariance's small-angle parameters and the arctangent under them (tests/test_small_angles_host.py)
double pgicp_host_atan2(double y, double x) { return pgicp::det_atan2(y, x); }
void pgicp_host_small_angles(const double *dT, double *abg) { pgicp::small_angles(dT, abg[0], abg[1], abg[2]); }


}
