// gp_dot_plan_check.cpp -- the host-side launch arithmetic of the dot-product covariance kernels (csrc/gp_dot_plan.h
// over csrc/gp_kernel_plan.h: the padded inner dimension, LDS layouts, record counts and workspace sizes behind
// pa_gp_dot_bwd_workspace / pa_gp_dot_bwd) as a stand-alone host program, for the sanitizers:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       -I pyro_amd/csrc tools/probes/gp_dot_plan_check.cpp -o gp_dot_plan_check && ./gp_dot_plan_check
//
// Over a grid of (N, M, D, element size, forced splits, compute units, wanted gradients) it walks a workspace of exactly
// the planned size the way the backward kernel and the finalize address it -- a row record per (row block, split), a
// cols record per half row block and column tile, a scalar record per workgroup -- and a byte array of exactly the
// planned LDS size the way the kernels carve and read it.  An off-by-one is an out-of-bounds access here, on the host.
#include <cstdio>
#include <vector>

#include "gp_dot_plan.h"

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

// the kernels' carving of dynamic LDS: two tiles [64, stride]; (backward) four [32, 33] buffers, then the float64 rows
// [64, D]; and the furthest element a matrix-instruction operand reads in a staged tile
static void walk_lds(int D, size_t elem, bool backward) {
  const size_t bytes = backward ? pa::gpd_bwd_lds_bytes(D, elem) : pa::gpd_fwd_lds_bytes(D, elem);
  CHECK(bytes <= 160 * 1024, "LDS of %zu bytes at D=%d", bytes, D);
  std::vector<unsigned char> lds(bytes, 0);
  const int stride = pa::gpd_lds_stride(D, elem), kp = pa::gpd_padded_d(D, elem), step = elem == 4 ? 2 : 4;
  CHECK(kp >= D && kp % step == 0 && kp - D < step && stride >= kp && stride % 2 == 1, "D=%d kp=%d stride=%d", D, kp, stride);
  size_t at = 0;
  for (size_t e = 0; e < (size_t)2 * pa::GPK_TILE * stride * elem; ++e) lds[at++] += 1;
  // operand reads of s = x z^T: row 63, inner index kp - 1
  CHECK(((size_t)pa::GPK_TILE * stride + (size_t)(pa::GPK_TILE - 1) * stride + kp) * elem <= at, "operand read past the tiles");
  if (backward) {
    for (size_t e = 0; e < (size_t)pa::GPK_WAVES * pa::GPD_SUB * pa::GPD_WT * elem; ++e) lds[at++] += 1;
    const size_t off = pa::gpd_bwd_acc_offset(D, elem);
    CHECK(off % 8 == 0 && off >= at && off - at < 8, "accumulators at %zu after %zu", off, at);
    for (size_t e = 0; e < (size_t)pa::GPK_TILE * D * sizeof(double); ++e) lds[off + e] += 1;
    at = off + (size_t)pa::GPK_TILE * D * sizeof(double);
  }
  CHECK(at == bytes, "LDS ends at %zu of %zu", at, bytes);
  for (size_t e = 0; e < bytes; ++e)
    if (lds[e] > 1) CHECK(false, "LDS byte %zu written %d times", e, (int)lds[e]);
}

static void check_call(int64_t N, int64_t M, int D, bool z_null, bool want_gx, bool want_gz, int cus, int forced, bool walk) {
  if (z_null && N != M) return;
  if (!pa::gpd_shape_ok(N, M, D, 1) || N == 0 || M == 0) return;
  const pa::GpdPlan pl = pa::gpd_plan(N, M, D, z_null, want_gx, want_gz, cus, forced);
  const pa::GpkLaunchPlan& g = pl.grid;
  const pa::GpkLaunchPlan base = pa::gpk_launch_plan(N, M, D, pa::GPD_SCALARS, want_gx, cus, forced);      // the split rule is the tree's
  CHECK(g.splits == base.splits && g.workgroups == base.workgroups && g.tiles_per_split == base.tiles_per_split, "split rule");
  CHECK(g.splits >= 1 && g.workgroups == g.row_blocks * g.splits && g.workgroups <= pa::GPK_MAX_WORKGROUPS, "grid");
  CHECK(pl.rows_part == want_gx && pl.cols_part == (z_null ? want_gx : want_gz) && pl.sym == z_null, "parts");
  CHECK(pl.half_blocks * pa::GPD_SUB >= N && (pl.half_blocks - 1) * pa::GPD_SUB < N && 2 * g.row_blocks >= pl.half_blocks,
        "half_blocks=%lld", (long long)pl.half_blocks);
  CHECK((pl.row_doubles + pl.col_doubles + pl.scalar_doubles) * sizeof(double) == pl.bytes, "bytes=%zu", pl.bytes);
  if (!walk) return;
  std::vector<double> ws(pl.bytes / sizeof(double), 0.0);
  double* row_rec = ws.data();
  double* col_rec = row_rec + pl.row_doubles;
  double* sc_rec = col_rec + pl.col_doubles;
  for (int64_t wg = 0; wg < g.workgroups; ++wg) {
    const int64_t rb = wg / g.splits, r0 = rb * pa::GPK_TILE;
    const int split = (int)(wg - rb * g.splits);
    const int64_t rows_here = g.rows - r0 < pa::GPK_TILE ? g.rows - r0 : pa::GPK_TILE;
    CHECK(rows_here >= 1, "workgroup %lld has no rows", (long long)wg);
    int64_t ct_end = (int64_t)(split + 1) * g.tiles_per_split;
    if (ct_end > g.col_tiles) ct_end = g.col_tiles;
    CHECK((int64_t)split * g.tiles_per_split < ct_end, "workgroup %lld has no tiles", (long long)wg);
    if (pl.rows_part) {
      double* r = row_rec + ((int64_t)split * g.rows + r0) * D;
      for (int64_t e = 0; e < rows_here * D; ++e) r[e] += 1.0;
    }
    if (pl.cols_part)
      for (int wr = 0; wr < 2; ++wr) {
        const int64_t hb = 2 * rb + wr;
        if (hb >= pl.half_blocks) continue;
        double* rec = col_rec + hb * g.cols * D;
        for (int64_t c = (int64_t)split * g.tiles_per_split * pa::GPK_TILE; c < ct_end * pa::GPK_TILE && c < g.cols; ++c)
          for (int d = 0; d < D; ++d) rec[c * D + d] += 1.0;
      }
    sc_rec[wg * pa::GPD_SCALARS] += 1.0, sc_rec[wg * pa::GPD_SCALARS + 1] += 1.0;
  }
  double sum = 0.0;      // the finalize's reads: every entry was written exactly once
  for (size_t e = 0; e < ws.size(); ++e) {
    sum += ws[e];
    if (ws[e] != 1.0) CHECK(false, "word %zu written %.0f times", e, ws[e]);
  }
  CHECK(sum == (double)ws.size(), "records: %.1f of %zu", sum, ws.size());
}

int main() {
  const int64_t Ns[] = {0, 1, 2, 31, 32, 33, 63, 64, 65, 130, 300, 5000, 100000};
  const int Ds[] = {1, 2, 3, 5, 7, 8, 17, 33, 63, 64};
  const int forced_list[] = {0, 1, 2, 7, 1000};
  const int cus_list[] = {256, 1, 0};
  long calls = 0;
  for (int D = 1; D <= pa::GPK_MAX_D; ++D)
    for (size_t elem : {sizeof(float), sizeof(double)}) walk_lds(D, elem, false), walk_lds(D, elem, true), calls += 2;
  for (int64_t N : Ns)
    for (int64_t M : Ns)
      for (int D : Ds)
        for (int forced : forced_list)
          for (int cus : cus_list)
            for (int flags = 0; flags < 8; ++flags) {
              const bool walk = (double)N * M <= 2e7 && (double)(N / 32 + 1) * M * D <= 4e6;
              check_call(N, M, D, flags & 4, flags & 1, flags & 2, cus, forced, walk);
              ++calls;
            }
  CHECK(!pa::gpd_shape_ok(10, 10, 65, 1) && !pa::gpd_shape_ok(10, 10, 0, 1) && !pa::gpd_shape_ok(-1, 10, 3, 1) &&
            !pa::gpd_shape_ok(10, 10, 3, 0) && !pa::gpd_shape_ok(10, 10, 3, 17) && pa::gpd_shape_ok(10, 10, 64, 16),
        "D / N / degree limits");
  CHECK(pa::GPD_FLUSH % pa::GPK_TILE == 0, "the flush length is whole tiles");
  check_call(512, 100000, 8, false, true, true, 256, 0, false);        // Xu [512, D] against X [1e5, D]
  check_call(pa::GPK_MAX_POINTS - 1, 64, 64, false, true, false, 256, 0, false);
  std::printf("%ld calls, %d failures\n", calls, failures);
  return failures ? 1 : 0;
}
