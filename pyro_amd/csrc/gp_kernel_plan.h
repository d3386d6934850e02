// gp_kernel_plan.h -- host-side launch arithmetic of the stationary covariance kernels (gp_kernel.hip): tiles, column
// splits, record counts, LDS and workspace bytes.  Plain C++ with no HIP in it, so that the same code is compiled into
// a stand-alone host program and run under the address / undefined-behaviour sanitizers
// (tools/probes/gp_kernel_plan_check.cpp).
#pragma once
#include <stddef.h>
#include <stdint.h>

// the sizes that the kernels work out again on the device
#ifdef __HIPCC__
#define GPK_HD __host__ __device__
#else
#define GPK_HD
#endif

namespace pa {

constexpr int GPK_TILE = 64;          // rows and columns of a workgroup's tile
constexpr int GPK_THREADS = 256;      // 16 x 16 lanes, a 4 x 4 register tile of outputs each
constexpr int GPK_MAX_D = 64;
constexpr int GPK_FAMILIES = 5;       // PA_GP_RBF .. PA_GP_MATERN52
constexpr int GPK_SCALARS = 3;        // per-workgroup scalar partials: variance, scale_mixture, scalar lengthscale
constexpr int64_t GPK_MAX_POINTS = int64_t(1) << 36;
constexpr int64_t GPK_MAX_WORKGROUPS = (int64_t(1) << 31) - 1;

inline bool gpk_shape_ok(int family, int64_t N, int64_t M, int64_t D, int n_ls) {
  return family >= 0 && family < GPK_FAMILIES && N >= 0 && M >= 0 && N < GPK_MAX_POINTS && M < GPK_MAX_POINTS &&
         D >= 1 && D <= GPK_MAX_D && (n_ls == 1 || n_ls == D);
}

inline int64_t gpk_tiles(int64_t n) { return (n + GPK_TILE - 1) / GPK_TILE; }
// row stride of a staged tile, in elements: odd, so that the 16 columns a wave reads fall into 16 banks
GPK_HD inline int gpk_lds_stride(int D) { return D | 1; }
// the two staged tiles, in elements; float64 words follow them at the next multiple of 8 bytes
GPK_HD inline size_t gpk_tile_elems(int D) { return (size_t)2 * GPK_TILE * gpk_lds_stride(D); }
GPK_HD inline size_t gpk_lds_head_bytes(int D, size_t elem) { return (gpk_tile_elems(D) * elem + 7) / 8 * 8; }
// forward: the tiles and 1 / lengthscale [D] in float64
inline size_t gpk_fwd_lds_bytes(int D, size_t elem) { return gpk_lds_head_bytes(D, elem) + (size_t)D * sizeof(double); }
// backward: the same, then the float64 row accumulators [TILE, D] and the per-wave lengthscale sums [4, D]
inline size_t gpk_bwd_lds_bytes(int D, size_t elem) {
  return gpk_lds_head_bytes(D, elem) + ((size_t)D + (size_t)GPK_TILE * D + (size_t)(GPK_THREADS / 64) * D) * sizeof(double);
}

// One backward launch: ``rows`` points get a gradient, ``cols`` points are walked.  Workgroup (row block, split) takes
// column tiles [split * tiles_per_split, (split + 1) * tiles_per_split) and leaves one row record [TILE rows, D] in
// slot ``split`` and one scalar record.
struct GpkLaunchPlan {
  int64_t rows, cols, row_blocks, col_tiles, tiles_per_split, workgroups;
  int splits, D;
  bool row_records;
  size_t row_doubles, scalar_doubles, bytes;      // float64 words: [splits, rows, D] then [workgroups, SCALARS + D]
};

inline GpkLaunchPlan gpk_launch_plan(int64_t rows, int64_t cols, int D, bool row_records, int cus, int forced_splits) {
  GpkLaunchPlan pl;
  pl.rows = rows, pl.cols = cols, pl.D = D, pl.row_records = row_records;
  pl.row_blocks = gpk_tiles(rows);
  pl.col_tiles = gpk_tiles(cols);
  // fill the device: two workgroups per compute unit, from column splits where the row blocks alone are too few
  const int64_t blocks = pl.row_blocks > 0 ? pl.row_blocks : 1;
  int64_t want = forced_splits > 0 ? forced_splits : ((int64_t)2 * (cus > 0 ? cus : 1) + blocks - 1) / blocks;
  if (want > pl.col_tiles) want = pl.col_tiles;
  if (want < 1) want = 1;
  pl.tiles_per_split = (pl.col_tiles + want - 1) / want;
  if (pl.tiles_per_split < 1) pl.tiles_per_split = 1;
  int64_t splits = (pl.col_tiles + pl.tiles_per_split - 1) / pl.tiles_per_split;      // none of them is empty
  if (splits < 1) splits = 1;
  pl.splits = (int)splits;
  pl.workgroups = pl.row_blocks * pl.splits;
  pl.row_doubles = row_records ? (size_t)pl.splits * (size_t)rows * (size_t)D : 0;
  pl.scalar_doubles = (size_t)pl.workgroups * (size_t)(GPK_SCALARS + D);
  pl.bytes = (pl.row_doubles + pl.scalar_doubles) * sizeof(double);
  return pl;
}

// One call of pa_gp_kernel_bwd: the launch that gives x its gradient (and the reduced gradients), and, with a z of
// its own that wants a gradient, a second launch of the same kernel with the roles exchanged.  The reduced gradients
// come from the first launch that runs.
struct GpkCallPlan {
  bool run_x, run_z;
  GpkLaunchPlan x, z;
  size_t z_offset_doubles, bytes;
};

inline GpkCallPlan gpk_call_plan(int64_t N, int64_t M, int D, bool z_null, bool want_gx, bool want_gz, int cus,
                                 int forced_splits) {
  GpkCallPlan cp;
  cp.run_z = want_gz && !z_null;
  cp.run_x = want_gx || !cp.run_z;
  cp.x = gpk_launch_plan(N, z_null ? N : M, D, want_gx, cus, forced_splits);
  cp.z = gpk_launch_plan(M, N, D, true, cus, forced_splits);
  if (!cp.run_x) cp.x.bytes = 0, cp.x.row_doubles = 0, cp.x.scalar_doubles = 0;
  if (!cp.run_z) cp.z.bytes = 0, cp.z.row_doubles = 0, cp.z.scalar_doubles = 0;
  cp.z_offset_doubles = cp.x.bytes / sizeof(double);
  cp.bytes = cp.x.bytes + cp.z.bytes;
  return cp;
}

}  // namespace pa
