// gp_wrap_plan.h -- host-side launch arithmetic of the wrapped covariance kernels (gp_wrap.hip), where it differs from
// gp_kernel_plan.h: the row record of a workgroup is [TILE rows, D + 1] (the last column is the gradient of the row's
// vertical scale), and the 64 + 64 scales of a tile are staged in LDS between the two point tiles and the float64 words.
// The tile, the split rule and the scalar record are gp_kernel_plan.h's.  Plain C++ with no HIP in it
// (tools/probes/gp_wrap_plan_check.cpp runs it under the address / undefined-behaviour sanitizers).
#pragma once
#include "gp_kernel_plan.h"

namespace pa {

constexpr int GPW_MAX_COEF = 8;           // coefficients of the output polynomial
constexpr int GPW_COSINE = 6;             // PA_GP_COSINE; 0 .. 4 are the families of gp_kernel_plan.h
constexpr int GPW_Q_IDENTITY = 0, GPW_Q_EXP = 1, GPW_Q_POLY = 2;

inline bool gpw_family_ok(int family) { return (family >= 0 && family < GPK_FAMILIES) || family == GPW_COSINE; }
// what gp_wrap.hip instantiates: the plain stationary families without a transform are gp_kernel.hip's
inline bool gpw_variant_ok(int family, int q, bool scaled) {
  return gpw_family_ok(family) && q >= GPW_Q_IDENTITY && q <= GPW_Q_POLY &&
         (family == GPW_COSINE || q != GPW_Q_IDENTITY || scaled);
}

// what is outside the caps: over 8 coefficients, and <f64, polynomial, scaled>, whose backward does not fit the registers
inline bool gpw_supported(size_t elem, int q, int n_coef, bool scaled) {
  if (q != GPW_Q_POLY) return true;
  return n_coef >= 1 && n_coef <= GPW_MAX_COEF && !(elem == 8 && scaled);
}

GPK_HD inline int gpw_row_width(int D) { return D + 1; }
// the two staged tiles and the scales of their rows [2, TILE], in bytes up to the next multiple of 8
GPK_HD inline size_t gpw_lds_head_bytes(int D, size_t elem) {
  return ((gpk_tile_elems(D) + (size_t)2 * GPK_TILE) * elem + 7) / 8 * 8;
}
inline size_t gpw_fwd_lds_bytes(int D, size_t elem) { return gpw_lds_head_bytes(D, elem) + (size_t)D * sizeof(double); }
// backward: 1 / lengthscale [D], the row accumulators [TILE, D + 1] and the per-wave lengthscale sums [4, D]
inline size_t gpw_bwd_lds_bytes(int D, size_t elem) {
  return gpw_lds_head_bytes(D, elem) +
         ((size_t)D + (size_t)GPK_TILE * gpw_row_width(D) + (size_t)GPK_WAVES * D) * sizeof(double);
}

// gp_kernel_plan.h's launch plan with the row records widened to D + 1 columns
inline GpkLaunchPlan gpw_widen(GpkLaunchPlan pl) {
  if (pl.bytes == 0) return pl;                       // (a launch that does not run)
  pl.row_doubles = pl.row_records ? (size_t)pl.splits * (size_t)pl.rows * (size_t)gpw_row_width(pl.D) : 0;
  pl.bytes = (pl.row_doubles + pl.scalar_doubles) * sizeof(double);
  return pl;
}

// One call of pa_gp_wrap_bwd.  ``rows_x``: gx or the gradient of x's scale is wanted; ``rows_z`` likewise for a z of its
// own.  The launches and their order are gpk_call_plan's.
inline GpkCallPlan gpw_call_plan(int64_t N, int64_t M, int D, bool z_null, bool rows_x, bool rows_z, int cus,
                                 int forced_splits) {
  GpkCallPlan cp = gpk_call_plan(N, M, D, gpk_record_doubles(D), z_null, rows_x, rows_z, cus, forced_splits);
  cp.x = gpw_widen(cp.x), cp.z = gpw_widen(cp.z);
  cp.z_offset_doubles = cp.x.bytes / sizeof(double);
  cp.bytes = cp.x.bytes + cp.z.bytes;
  return cp;
}

}  // namespace pa
