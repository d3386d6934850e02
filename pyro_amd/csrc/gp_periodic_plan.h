// gp_periodic_plan.h -- host-side launch arithmetic of the periodic covariance kernels (gp_periodic.hip).  The tile
// geometry and the split rule are gp_kernel_plan.h's; here is what differs: LDS holds 1 / p_k and 1 / l_k^2, the
// backward's LDS has per-feature accumulators for the period beside the lengthscale's, and the scalar record carries
// the period's entries.  Plain C++ with no HIP in it (tools/probes/gp_periodic_plan_check.cpp runs it under the
// address / undefined-behaviour sanitizers).
#pragma once
#include "gp_kernel_plan.h"

namespace pa {

constexpr int GPP_SCALARS = 2;        // per-workgroup scalar partials: variance, scalar lengthscale
constexpr int GPP_WAVES = GPK_THREADS / 64;

inline bool gpp_shape_ok(int64_t N, int64_t M, int64_t D, int n_ls, int n_p) {
  return gpk_shape_ok(0, N, M, D, n_ls) && (n_p == 1 || n_p == D);
}

// a workgroup's scalar record: {variance, scalar lengthscale, lengthscale_k [D], period_k [D]}
GPK_HD inline int gpp_record_doubles(int D) { return GPP_SCALARS + 2 * D; }
// forward: the two staged tiles, then 1 / p [D] and 1 / l^2 [D] in float64
inline size_t gpp_fwd_lds_bytes(int D, size_t elem) { return gpk_lds_head_bytes(D, elem) + (size_t)2 * D * sizeof(double); }
// backward: the same, then the float64 row accumulators [TILE, D] and the per-wave lengthscale and period sums [2, 4, D]
inline size_t gpp_bwd_lds_bytes(int D, size_t elem) {
  return gpp_fwd_lds_bytes(D, elem) + ((size_t)GPK_TILE * D + (size_t)2 * GPP_WAVES * D) * sizeof(double);
}

// gp_kernel_plan.h's launch and call plans with this kernel's scalar record
inline GpkLaunchPlan gpp_launch_plan(int64_t rows, int64_t cols, int D, bool row_records, int cus, int forced_splits) {
  GpkLaunchPlan pl = gpk_launch_plan(rows, cols, D, row_records, cus, forced_splits);
  pl.scalar_doubles = (size_t)pl.workgroups * (size_t)gpp_record_doubles(D);
  pl.bytes = (pl.row_doubles + pl.scalar_doubles) * sizeof(double);
  return pl;
}

inline GpkCallPlan gpp_call_plan(int64_t N, int64_t M, int D, bool z_null, bool want_gx, bool want_gz, int cus,
                                 int forced_splits) {
  GpkCallPlan cp;
  cp.run_z = want_gz && !z_null;
  cp.run_x = want_gx || !cp.run_z;
  cp.x = gpp_launch_plan(N, z_null ? N : M, D, want_gx, cus, forced_splits);
  cp.z = gpp_launch_plan(M, N, D, true, cus, forced_splits);
  if (!cp.run_x) cp.x.bytes = 0, cp.x.row_doubles = 0, cp.x.scalar_doubles = 0;
  if (!cp.run_z) cp.z.bytes = 0, cp.z.row_doubles = 0, cp.z.scalar_doubles = 0;
  cp.z_offset_doubles = cp.x.bytes / sizeof(double);
  cp.bytes = cp.x.bytes + cp.z.bytes;
  return cp;
}

}  // namespace pa
