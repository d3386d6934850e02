// gp_compose_plan.h -- host-side arithmetic of the composite covariance kernels (gp_compose.hip): what a descriptor
// may hold, the LDS layout, the scalar record and the workspace.  The tile geometry and the split rule are
// gp_kernel_plan.h's, with the width U of the staged union of columns in the place of D.  Plain C++ with no HIP in it.
//
// Caps.  6 terms, 3 factors per term, 8 factors in all, U <= 64 (pa_gp_compose_spec).  The sum of the factors' D_f is
// capped at GPX_MAX_SUM_D = 256: that is what keeps the descriptor, which travels in the kernel arguments with one
// byte per column, under 1 KiB (592 bytes).  LDS would allow more: at U = 64 in float64 the backward holds 99328
// bytes of tiles and row accumulators and 80 bytes per unit of sum D_f, 119808 + 768 bytes at the cap, under the
// 160 KiB of a gfx950 workgroup (gpx_supported checks it all the same).
#pragma once
#include "../../include/pyro_amd.h"
#include "gp_kernel_plan.h"

namespace pa {

constexpr int GPX_MAX_TERMS = PA_GP_COMPOSE_MAX_TERMS;
constexpr int GPX_MAX_TERM_FACTORS = PA_GP_COMPOSE_MAX_TERM_FACTORS;
constexpr int GPX_MAX_FACTORS = PA_GP_COMPOSE_MAX_FACTORS;
constexpr int GPX_MAX_SUM_D = PA_GP_COMPOSE_MAX_SUM_D;
constexpr int GPX_SCALARS = 3;        // per factor and workgroup: variance, scale_mixture, scalar lengthscale
constexpr size_t GPX_MAX_LDS_BYTES = 160 * 1024;
static_assert(sizeof(pa_gp_compose_spec) <= 1024, "the descriptor travels by value in the kernel arguments");

// the descriptor is well formed: counts within the caps, factors laid out one after the other in ``cols``, every
// column inside the staged tile.  (Pointers are checked where they are used.)
inline bool gpx_spec_ok(const pa_gp_compose_spec& s) {
  if (s.n_terms < 1 || s.n_terms > GPX_MAX_TERMS || s.n_factors < 1 || s.n_factors > GPX_MAX_FACTORS) return false;
  if (s.U < 1 || s.U > GPK_MAX_D || s.sum_d < 1 || s.sum_d > GPX_MAX_SUM_D) return false;
  int factors = 0;
  for (int t = 0; t < s.n_terms; ++t) {
    if (s.term_count[t] < 1 || s.term_count[t] > GPX_MAX_TERM_FACTORS) return false;
    factors += s.term_count[t];
  }
  if (factors != s.n_factors) return false;
  int col0 = 0;
  for (int f = 0; f < s.n_factors; ++f) {
    const pa_gp_factor& fa = s.factor[f];
    if (fa.kind > PA_GP_PERIODIC || fa.D < 1 || fa.D > GPK_MAX_D || fa.col0 != col0) return false;
    if (fa.n_ls != 1 && fa.n_ls != fa.D) return false;
    const bool aux_ok = fa.kind == PA_GP_PERIODIC ? (fa.n_aux == 1 || fa.n_aux == fa.D)
                                                  : fa.n_aux == (fa.kind == PA_GP_RATIONAL_QUADRATIC ? 1 : 0);
    if (!aux_ok) return false;
    col0 += fa.D;
    if (col0 > s.sum_d) return false;
    for (int k = 0; k < fa.D; ++k)
      if (s.cols[fa.col0 + k] >= s.U) return false;
  }
  return col0 == s.sum_d;
}

// LDS.  Forward: the two staged tiles [64, U | 1], then per factor and feature two float64 words: 1 / l_k (and an
// unused word), or 1 / p_k and 1 / l_k^2.  Backward: then the row accumulators [64, U], the per-wave lengthscale and
// period sums [2, 4, sum_d] and the per-wave scalar sums [4, 3 * factors].
inline size_t gpx_fwd_lds_bytes(int U, int sum_d, size_t elem) {
  return gpk_lds_head_bytes(U, elem) + (size_t)2 * sum_d * sizeof(double);
}
inline size_t gpx_bwd_lds_bytes(int U, int sum_d, size_t elem) {
  return gpx_fwd_lds_bytes(U, sum_d, elem) +
         ((size_t)GPK_TILE * U + (size_t)2 * GPK_WAVES * sum_d + (size_t)GPK_WAVES * GPX_SCALARS * GPX_MAX_FACTORS) *
             sizeof(double);
}
inline bool gpx_supported(const pa_gp_compose_spec& s, size_t elem) {
  return gpx_spec_ok(s) && gpx_bwd_lds_bytes(s.U, s.sum_d, elem) <= GPX_MAX_LDS_BYTES;
}

// a workgroup's scalar record, factor by factor: {variance, scale_mixture, scalar lengthscale, lengthscale_k [D_f],
// period_k [D_f]} at gpx_record_base(f, col0_f)
GPK_HD inline int gpx_record_base(int f, int col0) { return GPX_SCALARS * f + 2 * col0; }
GPK_HD inline int gpx_record_doubles(int n_factors, int sum_d) { return GPX_SCALARS * n_factors + 2 * sum_d; }

}  // namespace pa
