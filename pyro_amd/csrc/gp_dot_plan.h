// gp_dot_plan.h -- host-side launch arithmetic of the dot-product covariance kernels (gp_dot.hip): the padded inner
// dimension of the matrix instructions, LDS layouts, the flush length, record counts and workspace bytes.  The 64 x 64
// tile and the split rule are gp_kernel_plan.h's.  Plain C++ with no HIP in it (tools/probes/gp_dot_plan_check.cpp runs
// it under the address / undefined-behaviour sanitizers).
#pragma once
#include "gp_kernel_plan.h"

namespace pa {

constexpr int GPD_THREADS = GPK_THREADS;      // 4 waves, a 32 x 32 block of the 64 x 64 tile each
constexpr int GPD_SUB = 32;
constexpr int GPD_WT = GPD_SUB + 1;           // row stride of a wave's transposition buffer
constexpr int GPD_MAX_DEGREE = 16;
constexpr int GPD_SCALARS = 2;                // per-workgroup scalar partials: variance, bias
// columns after which the backward's working-precision accumulators of gX are added to float64 and cleared: no sum in
// the tensor's dtype is longer (a multiple of the tile)
constexpr int GPD_FLUSH = 1024;

inline bool gpd_shape_ok(int64_t N, int64_t M, int64_t D, int degree) {
  return gpk_shape_ok(0, N, M, D, 1) && degree >= 1 && degree <= GPD_MAX_DEGREE;
}

// the inner dimension as the matrix instructions walk it: 2 features per v_mfma_f32_32x32x2_f32, 4 per
// v_mfma_f64_16x16x4_f64; the staged rows carry zeros in [D, stride)
GPK_HD inline int gpd_padded_d(int D, size_t elem) { return elem == 4 ? (D + 1) / 2 * 2 : (D + 3) / 4 * 4; }
// the tree's odd row stride, over the padded width
GPK_HD inline int gpd_lds_stride(int D, size_t elem) { return gpk_lds_stride(gpd_padded_d(D, elem)); }
// the two staged tiles, in bytes
GPK_HD inline size_t gpd_fwd_lds_bytes(int D, size_t elem) { return (size_t)2 * GPK_TILE * gpd_lds_stride(D, elem) * elem; }
// backward: the tiles, one [32, 33] transposition buffer per wave, then (8-byte aligned) the float64 rows [TILE, D]
GPK_HD inline size_t gpd_bwd_acc_offset(int D, size_t elem) {
  return (gpd_fwd_lds_bytes(D, elem) + (size_t)GPK_WAVES * GPD_SUB * GPD_WT * elem + 7) / 8 * 8;
}
inline size_t gpd_bwd_lds_bytes(int D, size_t elem) { return gpd_bwd_acc_offset(D, elem) + (size_t)GPK_TILE * D * sizeof(double); }

// ONE backward launch.  Workgroup (row block, split) walks its column tiles.  rows_part: gX of the row block,
// one record [TILE rows, D] in slot ``split``.  cols_part: W^T X of every column it meets, one record [cols, D] per
// HALF row block (a wave's 32 rows): gZ, or with z = x the second role of gX.  One scalar record per workgroup.
struct GpdPlan {
  GpkLaunchPlan grid;      // row blocks, column tiles, splits (gp_kernel_plan.h)
  bool rows_part, cols_part, sym;
  int64_t half_blocks;
  size_t row_doubles, col_doubles, scalar_doubles, bytes;      // float64 words, in this order
};

inline GpdPlan gpd_plan(int64_t N, int64_t M, int D, bool z_null, bool want_gx, bool want_gz, int cus, int forced_splits) {
  GpdPlan p;
  p.sym = z_null;
  p.rows_part = want_gx;
  p.cols_part = z_null ? want_gx : want_gz;
  p.grid = gpk_launch_plan(N, z_null ? N : M, D, GPD_SCALARS, p.rows_part, cus, forced_splits);
  p.half_blocks = (N + GPD_SUB - 1) / GPD_SUB;
  p.row_doubles = p.grid.row_doubles;
  p.col_doubles = p.cols_part ? (size_t)p.half_blocks * (size_t)p.grid.cols * (size_t)D : 0;
  p.scalar_doubles = (size_t)p.grid.workgroups * GPD_SCALARS;
  p.bytes = (p.row_doubles + p.col_doubles + p.scalar_doubles) * sizeof(double);
  return p;
}

}  // namespace pa
