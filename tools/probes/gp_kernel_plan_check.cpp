// gp_kernel_plan_check.cpp -- the host-side launch arithmetic of the stationary covariance kernels
// (csrc/gp_kernel_plan.h: tiles, column splits, record and workspace sizes behind pa_gp_kernel_bwd_workspace /
// pa_gp_kernel_bwd) as a stand-alone host program, for the sanitizers:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       -I pyro_amd/csrc tools/probes/gp_kernel_plan_check.cpp -o gp_kernel_plan_check && ./gp_kernel_plan_check
//
// Over a grid of (N, M, D, element size, forced splits, compute units, wanted gradients) it checks the plan's
// invariants -- at least one split, no empty split, every row and every column tile taken exactly once -- and walks a
// workspace of exactly the planned size the way the kernel and the finalize address it: every workgroup's row record
// and scalar record, of both launches.  An off-by-one in the record or workspace arithmetic is an out-of-bounds
// access here, on the host.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "gp_kernel_plan.h"

static int failures = 0;
#define CHECK(c, ...)                    \
  do {                                   \
    if (!(c)) {                          \
      std::printf("FAIL %s: ", #c);      \
      std::printf(__VA_ARGS__);          \
      std::printf("\n");                 \
      ++failures;                        \
    }                                    \
  } while (0)

// one launch: the kernel's writes into its part of the workspace, then the finalize's reads
static void walk_launch(const pa::GpkLaunchPlan& pl, double* ws, size_t ws_doubles, bool scalars) {
  const int D = pl.D;
  CHECK(pl.splits >= 1 && pl.tiles_per_split >= 1, "splits=%d tiles_per_split=%lld", pl.splits, (long long)pl.tiles_per_split);
  CHECK(pl.row_blocks * pa::GPK_TILE >= pl.rows && (pl.row_blocks - 1) * pa::GPK_TILE < (pl.rows > 0 ? pl.rows : 1),
        "row_blocks=%lld rows=%lld", (long long)pl.row_blocks, (long long)pl.rows);
  CHECK(pl.workgroups == pl.row_blocks * pl.splits && pl.workgroups <= pa::GPK_MAX_WORKGROUPS, "workgroups");
  CHECK((pl.row_doubles + pl.scalar_doubles) * sizeof(double) == pl.bytes && pl.bytes / sizeof(double) <= ws_doubles,
        "bytes=%zu", pl.bytes);
  // every column tile belongs to exactly one split and no split is empty
  std::vector<int> col_seen((size_t)pl.col_tiles, 0);
  for (int s = 0; s < pl.splits; ++s) {
    int64_t end = (int64_t)(s + 1) * pl.tiles_per_split;
    if (end > pl.col_tiles) end = pl.col_tiles;
    CHECK(pl.col_tiles == 0 || (int64_t)s * pl.tiles_per_split < end, "split %d of %d is empty", s, pl.splits);
    for (int64_t ct = (int64_t)s * pl.tiles_per_split; ct < end; ++ct) col_seen[(size_t)ct] += 1;
  }
  for (int64_t ct = 0; ct < pl.col_tiles; ++ct) CHECK(col_seen[(size_t)ct] == 1, "column tile %lld taken %d times", (long long)ct, col_seen[(size_t)ct]);
  double* row_rec = ws;
  double* sc_rec = ws + pl.row_doubles;
  std::vector<int> row_seen((size_t)pl.rows, 0);
  for (int64_t wg = 0; wg < pl.workgroups; ++wg) {
    const int64_t rb = wg / pl.splits;
    const int split = (int)(wg - rb * pl.splits);
    const int64_t i0 = rb * pa::GPK_TILE;
    const int64_t rows_here = pl.rows - i0 < pa::GPK_TILE ? pl.rows - i0 : pa::GPK_TILE;
    CHECK(rows_here >= 1, "workgroup %lld has no rows", (long long)wg);
    if (pl.row_records) {
      double* rec = row_rec + ((int64_t)split * pl.rows + i0) * D;
      for (int64_t e = 0; e < rows_here * D; ++e) rec[e] = 1.0;
      if (split == 0)
        for (int64_t r = 0; r < rows_here; ++r) row_seen[(size_t)(i0 + r)] += 1;
    }
    if (scalars) {
      double* sc = sc_rec + wg * (pa::GPK_SCALARS + D);
      for (int k = 0; k < pa::GPK_SCALARS + D; ++k) sc[k] = 2.0;
    }
  }
  double sum = 0.0;
  if (pl.row_records) {
    for (int64_t r = 0; r < pl.rows; ++r) CHECK(row_seen[(size_t)r] == 1, "row %lld taken %d times", (long long)r, row_seen[(size_t)r]);
    const int64_t total = pl.rows * D;
    for (int64_t e = 0; e < total; ++e)
      for (int sp = 0; sp < pl.splits; ++sp) sum += row_rec[(int64_t)sp * total + e];
    CHECK(sum == (double)total * pl.splits, "row records: %.1f", sum);
  }
  if (scalars) {
    sum = 0.0;
    for (int slot = 0; slot < pa::GPK_SCALARS + D; ++slot)
      for (int64_t w = 0; w < pl.workgroups; ++w) sum += sc_rec[w * (pa::GPK_SCALARS + D) + slot];
    CHECK(sum == 2.0 * (double)pl.workgroups * (pa::GPK_SCALARS + D), "scalar records: %.1f", sum);
  }
}

static void check_call(int64_t N, int64_t M, int D, size_t elem, bool z_null, bool want_gx, bool want_gz, int cus,
                       int forced, bool walk) {
  if (z_null && N != M) return;
  if (!pa::gpk_shape_ok(0, N, M, D, 1) || N == 0 || M == 0) return;
  const pa::GpkCallPlan cp = pa::gpk_call_plan(N, M, D, z_null, want_gx, want_gz, cus, forced);
  CHECK(cp.run_x || cp.run_z, "nothing runs");
  CHECK(cp.run_z == (want_gz && !z_null), "run_z");
  CHECK(cp.bytes == cp.x.bytes + cp.z.bytes && cp.z_offset_doubles * sizeof(double) == cp.x.bytes, "offsets");
  CHECK(cp.bytes % sizeof(double) == 0, "alignment");
  // LDS of the launches fits a compute unit's 160 KiB
  CHECK(pa::gpk_fwd_lds_bytes(D, elem) <= 160 * 1024 && pa::gpk_bwd_lds_bytes(D, elem) <= 160 * 1024, "LDS");
  CHECK(pa::gpk_lds_stride(D) >= D && (pa::gpk_lds_stride(D) & 1) == 1, "stride");
  if (forced > 0) {
    const int64_t tiles = pa::gpk_tiles(z_null ? N : M);
    CHECK(!cp.run_x || (cp.x.splits <= forced && cp.x.splits <= tiles), "forced splits %d -> %d", forced, cp.x.splits);
    CHECK(!cp.run_x || forced < tiles || cp.x.splits == tiles, "more splits than column tiles: one tile each");
  }
  if (!walk) return;
  std::vector<double> ws(cp.bytes / sizeof(double));
  if (cp.run_x) walk_launch(cp.x, ws.data(), ws.size(), true);
  if (cp.run_z) walk_launch(cp.z, ws.data() + cp.z_offset_doubles, ws.size() - cp.z_offset_doubles, !cp.run_x);
  // few rows against many columns still fill the device
  if (forced == 0 && cus >= 8 && cp.run_x && cp.x.col_tiles >= 2 * cus) CHECK(cp.x.workgroups >= cus, "device not filled");
}

int main() {
  const int64_t Ns[] = {0, 1, 2, 63, 64, 65, 130, 300, 5000, 100000};
  const int Ds[] = {1, 2, 3, 5, 8, 17, 63, 64};
  const int forced_list[] = {0, 1, 2, 7, 1000};
  const int cus_list[] = {256, 1, 0};
  long calls = 0;
  for (int64_t N : Ns)
    for (int64_t M : Ns)
      for (int D : Ds)
        for (int forced : forced_list)
          for (int cus : cus_list)
            for (int flags = 0; flags < 8; ++flags) {
              const bool z_null = flags & 4, want_gx = flags & 1, want_gz = flags & 2;
              const bool walk = (double)N * M <= 2e7 && (N <= 5000 || D <= 8);
              check_call(N, M, D, D & 1 ? 4 : 8, z_null, want_gx, want_gz, cus, forced, walk);
              ++calls;
            }
  // the limits of the entry points
  CHECK(!pa::gpk_shape_ok(0, 10, 10, 65, 1) && !pa::gpk_shape_ok(0, 10, 10, 0, 1) && !pa::gpk_shape_ok(0, -1, 10, 3, 1),
        "D / N limits");
  CHECK(!pa::gpk_shape_ok(5, 10, 10, 3, 1) && !pa::gpk_shape_ok(-1, 10, 10, 3, 1) && !pa::gpk_shape_ok(0, 10, 10, 3, 2) &&
            pa::gpk_shape_ok(4, 10, 10, 3, 3),
        "family / lengthscale limits");
  CHECK(!pa::gpk_shape_ok(0, pa::GPK_MAX_POINTS, 1, 3, 1), "size limit");
  check_call(1000000, 32, 8, 4, false, true, true, 256, 0, true);       // Xu [32, D] against X [1e6, D]
  {
    const pa::GpkCallPlan cp = pa::gpk_call_plan(1000000, 32, 8, false, true, true, 256, 0);
    CHECK(cp.z.row_blocks == 1 && cp.z.splits >= 256, "32 rows against 1e6 columns run on %d workgroups", cp.z.splits);
  }
  check_call(pa::GPK_MAX_POINTS - 1, 64, 64, 8, false, true, true, 256, 0, false);
  std::printf("%ld calls, %d failures\n", calls, failures);
  return failures ? 1 : 0;
}
