// gp_cond_plan.h -- host-side launch arithmetic of the streamed sparse-GP conditional marginals (gp_cond.hip): tiles of
// the forward, block pairs / chunks / splits of the two backward launches, record counts, LDS and workspace bytes.  Plain
// C++ with no HIP in it, as gp_sgpr_plan.h is, whose tile constants and split rule it shares.
#pragma once
#include "gp_sgpr_plan.h"

namespace pa {

constexpr int GPC_MAX_J = GPS_MAX_Q + 1;              // P_0 = Luu^-1 and one projection per latent output
constexpr size_t GPC_MAX_LDS = 160 * 1024;            // one workgroup's LDS on gfx950

inline bool gpc_shape_ok(int family, int64_t N, int64_t M, int64_t D, int64_t Q, int n_ls, size_t elem) {
  return gps_shape_ok(family, N, M, D, Q, n_ls, elem);
}

// ---- forward: one workgroup per tile of GPS_TN points; Kuf[:, tile] [M rounded up to 32, 32] in LDS, the waves' partial
// s [waves, J, 32] in float64 beside it.  No records.
struct GpcFwdPlan {
  int D, Q, J, row_blocks;
  int64_t workgroups;
  size_t lds_bytes;
};

inline size_t gpc_fwd_lds_bytes(int64_t M, int D, int Q, size_t elem) {
  const size_t s = gps_lds_stride(D), rows = (size_t)gps_div_up(M, GPS_SUB) * GPS_SUB;
  const size_t f64 = (size_t)D + (size_t)(GPS_THREADS / 64) * (Q + 1) * GPS_TN;
  return f64 * sizeof(double) + (rows * GPS_KS + GPS_TN * s) * elem;
}

inline GpcFwdPlan gpc_fwd_plan(int64_t N, int64_t M, int D, int Q, size_t elem) {
  GpcFwdPlan p;
  p.D = D, p.Q = Q, p.J = Q + 1;
  p.row_blocks = (int)gps_div_up(M, GPS_SUB);
  p.workgroups = gps_div_up(N, GPS_TN);
  p.lds_bytes = gpc_fwd_lds_bytes(M, D, Q, elem);
  return p;
}

// ---- backward, launch one: workgroup (j, block pair I <= J', split) leaves one record [rec_dim, rec_dim] of
// Aw_j = Kuf diag(g_s[:, j]) Kuf^T, and for j = 0 on the diagonal one record [rec_dim, Q] of ga = Kuf g_loc.
// Launch two: workgroup (chunk of GPS_BWD_ROWS inducing rows, split), records as gp_sgpr's backward.  One workspace:
// the records of launch one, then those of launch two.
struct GpcBwdPlan {
  int D, Q, J;
  // launch one
  int tm, blocks, pairs, rec_dim, splits1;
  int64_t steps, per_split1, workgroups1;
  size_t a_doubles, b_doubles, lds1_bytes;
  // launch two
  int chunks, splits2;
  int64_t per_split2, workgroups2;
  bool want_gx, want_gxu;
  size_t row_doubles, scalar_doubles, gx_doubles, lds2_bytes;
  size_t bytes;
};

inline size_t gpc_gram_lds_bytes(int D, int Q, size_t elem) {
  const size_t tm = gps_tm(elem), s = gps_lds_stride(D);
  return (size_t)D * sizeof(double) + (2 * tm * s + GPS_TN * s + 2 * tm * GPS_KS + (size_t)GPS_TN * Q) * elem;
}

inline size_t gpc_chain_lds_bytes(int64_t M, int D, int Q, size_t elem) {
  const size_t s = gps_lds_stride(D), rows = (size_t)(M > GPS_BWD_ROWS ? M : GPS_BWD_ROWS) + 1;
  const size_t f64 = (size_t)D + (size_t)GPS_BWD_ROWS * D + (size_t)(GPS_THREADS / 64) * D;
  return f64 * sizeof(double) + (rows * GPS_KS + GPS_TN * s + (size_t)GPS_TN * (2 * Q + 1)) * elem;
}

inline GpcBwdPlan gpc_bwd_plan(int64_t N, int64_t M, int D, int Q, size_t elem, bool want_gx, bool want_gxu, int cus,
                               int forced_splits) {
  GpcBwdPlan p;
  p.D = D, p.Q = Q, p.J = Q + 1, p.want_gx = want_gx, p.want_gxu = want_gxu;
  p.steps = gps_div_up(N, GPS_TN);
  p.tm = gps_tm(elem);
  p.blocks = (int)gps_div_up(M, p.tm);
  p.pairs = p.blocks * (p.blocks + 1) / 2;
  p.rec_dim = (int)(M < p.tm ? M : p.tm);
  gps_split(p.steps, (int64_t)p.pairs * p.J, cus, forced_splits, &p.per_split1, &p.splits1);
  p.workgroups1 = (int64_t)p.J * p.pairs * p.splits1;
  p.a_doubles = (size_t)p.J * p.pairs * p.splits1 * p.rec_dim * p.rec_dim;
  p.b_doubles = (size_t)p.blocks * p.splits1 * p.rec_dim * Q;
  p.lds1_bytes = gpc_gram_lds_bytes(D, Q, elem);
  p.chunks = (int)gps_div_up(M, GPS_BWD_ROWS);
  gps_split(p.steps, p.chunks, cus, forced_splits, &p.per_split2, &p.splits2);
  p.workgroups2 = (int64_t)p.chunks * p.splits2;
  p.row_doubles = want_gxu ? (size_t)p.splits2 * M * D : 0;
  p.scalar_doubles = (size_t)p.workgroups2 * (GPS_SCALARS + D);
  p.gx_doubles = want_gx ? (size_t)p.chunks * (size_t)N * D : 0;
  p.lds2_bytes = gpc_chain_lds_bytes(M, D, Q, elem);
  p.bytes = (p.a_doubles + p.b_doubles + p.row_doubles + p.scalar_doubles + p.gx_doubles) * sizeof(double);
  return p;
}

}  // namespace pa
