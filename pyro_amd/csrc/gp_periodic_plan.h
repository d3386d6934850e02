// gp_periodic_plan.h -- host-side launch arithmetic of the periodic covariance kernels (gp_periodic.hip).  The tile
// geometry and the split rule are gp_kernel_plan.h's; here is what differs: LDS holds 1 / p_k and 1 / l_k^2, the
// backward's LDS has per-feature accumulators for the period beside the lengthscale's, and the scalar record carries
// the period's entries (gpp_record_doubles, the record size that gpk_launch_plan and gpk_call_plan are called with).
// Plain C++ with no HIP in it (tools/probes/gp_periodic_plan_check.cpp runs it under the address / undefined-behaviour
// sanitizers).
#pragma once
#include "gp_kernel_plan.h"

namespace pa {

constexpr int GPP_SCALARS = 2;        // per-workgroup scalar partials: variance, scalar lengthscale

inline bool gpp_shape_ok(int64_t N, int64_t M, int64_t D, int n_ls, int n_p) {
  return gpk_shape_ok(0, N, M, D, n_ls) && (n_p == 1 || n_p == D);
}

// a workgroup's scalar record: {variance, scalar lengthscale, lengthscale_k [D], period_k [D]}
GPK_HD inline int gpp_record_doubles(int D) { return GPP_SCALARS + 2 * D; }
// forward: the two staged tiles, then 1 / p [D] and 1 / l^2 [D] in float64
inline size_t gpp_fwd_lds_bytes(int D, size_t elem) { return gpk_lds_head_bytes(D, elem) + (size_t)2 * D * sizeof(double); }
// backward: the same, then the float64 row accumulators [TILE, D] and the per-wave lengthscale and period sums [2, 4, D]
inline size_t gpp_bwd_lds_bytes(int D, size_t elem) {
  return gpp_fwd_lds_bytes(D, elem) + ((size_t)GPK_TILE * D + (size_t)2 * GPK_WAVES * D) * sizeof(double);
}

}  // namespace pa
