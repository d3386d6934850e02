// glm_family_plan.h -- host-side launch arithmetic of the family GLM kernels (glm_family.hip): tile counts, grid,
// trips of the tile loop, record and workspace sizes.  Plain C++ with no HIP in it, so that the same code is
// compiled into a stand-alone host program and run under the address / undefined-behaviour sanitizers
// (tools/probes/glm_family_plan_check.cpp).
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace pa {

constexpr int GLMF_WAVES = 4;          // waves per workgroup, one 32-row tile each
constexpr int GLMF_FAMILIES = 4;
constexpr int64_t GLMF_MAX_N = int64_t(1) << 40;
constexpr int64_t GLMF_MAX_P = int64_t(1) << 20;

// floats in one workgroup's partial record: the raw MFMA accumulator tiles of gw, then three 32-particle rows per
// particle tile {S0, gb, S1}, then {sum of the rows' lgamma terms, number of unmasked rows} padded to 32
constexpr int glmf_record_floats(int DT, int PT) { return PT * DT * 1024 + 3 * PT * 32 + 32; }

// aux columns of a family (PA_GLM_NORMAL .. PA_GLM_BINOMIAL_LOGITS), -1 for an unknown one
inline int glmf_aux_columns(int family) {
  switch (family) {
    case 0: return 1;
    case 1: return 2;
    case 2: return 0;
    case 3: return 0;
    default: return -1;
  }
}

struct GlmFamilyPlan {
  int DT, PT, npass, nblocks, rec;
  int64_t ntiles, iters;
  size_t lds_bytes, workspace_bytes;
};

inline bool glmf_shape_ok(int family, int64_t N, int64_t D, int64_t P) {
  return glmf_aux_columns(family) >= 0 && N >= 0 && N < GLMF_MAX_N && D >= 1 && D <= 128 && P >= 1 &&
         P < GLMF_MAX_P;
}

// PT: two particle tiles per wave where one feature tile leaves the registers for it.  (Every family fits: see
// the resource table in the README entry.)  ``cus``: compute units of the device; ``max_blocks`` > 0 caps grid.x.
inline GlmFamilyPlan glmf_plan(int64_t N, int64_t D, int64_t P, int cus, int max_blocks) {
  GlmFamilyPlan pl;
  pl.DT = D <= 32 ? 1 : (D <= 64 ? 2 : 4);
  pl.PT = (pl.DT == 1 && P > 32) ? 2 : 1;
  pl.npass = (int)((P + 32 * pl.PT - 1) / (32 * pl.PT));
  pl.ntiles = (N + 31) / 32;
  int64_t want = (pl.ntiles + GLMF_WAVES - 1) / GLMF_WAVES;
  // workgroups in flight per CU: 2 (8 waves), or 1 with four feature tiles (the kernel's launch bounds: its
  // accumulators take the AGPRs of a whole SIMD lane budget) -- the grid is one resident wave of workgroups
  const int per_cu = pl.DT == 4 ? 1 : 2;
  int64_t cap = (int64_t)(cus > 0 ? cus : 1) * per_cu / pl.npass;
  if (cap < 1) cap = 1;
  if (max_blocks > 0 && cap > max_blocks) cap = max_blocks;
  pl.nblocks = (int)(want < cap ? (want < 1 ? 1 : want) : cap);
  pl.iters = (pl.ntiles + (int64_t)pl.nblocks * GLMF_WAVES - 1) / ((int64_t)pl.nblocks * GLMF_WAVES);
  if (pl.iters < 1) pl.iters = 1;
  pl.rec = glmf_record_floats(pl.DT, pl.PT);
  pl.lds_bytes = (size_t)GLMF_WAVES * 32 * (32 * pl.DT + 3) * sizeof(float);
  pl.workspace_bytes = (size_t)pl.nblocks * (size_t)pl.npass * (size_t)pl.rec * sizeof(float);
  return pl;
}

}  // namespace pa
