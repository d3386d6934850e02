// gp_periodic_plan_check.cpp -- the host-side launch arithmetic of the periodic covariance kernels
// (csrc/gp_periodic_plan.h over csrc/gp_kernel_plan.h: LDS layout, scalar records with the period's entries, workspace
// sizes behind pa_gp_periodic_bwd_workspace / pa_gp_periodic_bwd) as a stand-alone host program, for the sanitizers:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       -I pyro_amd/csrc tools/probes/gp_periodic_plan_check.cpp -o gp_periodic_plan_check && ./gp_periodic_plan_check
//
// Over a grid of (N, M, D, element size, forced splits, compute units, wanted gradients) it walks a workspace of
// exactly the planned size the way the backward kernel and the finalize address it -- every workgroup's row record and
// scalar record {variance, scalar lengthscale, lengthscale_k, period_k}, of both launches -- and a byte array of exactly
// the planned LDS size the way the kernels carve it.  The tile and split invariants themselves are
// gp_kernel_plan_check.cpp's.  An off-by-one in the record, workspace or LDS arithmetic is an out-of-bounds access
// here, on the host.
#include <cstdio>
#include <vector>

#include "gp_periodic_plan.h"

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

// the kernels' carving of dynamic LDS: tiles, 1 / p [D], 1 / l^2 [D], then (backward) rows [64, D], lengthscale and
// period sums [4, D] each; every byte is written exactly once
static void walk_lds(int D, size_t elem, bool backward) {
  const size_t bytes = backward ? pa::gpp_bwd_lds_bytes(D, elem) : pa::gpp_fwd_lds_bytes(D, elem);
  CHECK(bytes <= 160 * 1024, "LDS of %zu bytes at D=%d", bytes, D);
  std::vector<unsigned char> lds(bytes, 0);
  const int stride = pa::gpk_lds_stride(D);
  for (size_t e = 0; e < (size_t)2 * pa::GPK_TILE * stride * elem; ++e) lds[e] += 1;
  const size_t head = pa::gpk_lds_head_bytes(D, elem);
  CHECK(head % 8 == 0 && head >= (size_t)2 * pa::GPK_TILE * stride * elem, "head=%zu", head);
  const size_t doubles = (size_t)2 * D + (backward ? (size_t)(pa::GPK_TILE + 2 * pa::GPK_WAVES) * D : 0);
  for (size_t e = 0; e < doubles * sizeof(double); ++e) lds[head + e] += 1;
  CHECK(head + doubles * sizeof(double) == bytes, "LDS ends at %zu of %zu", head + doubles * sizeof(double), bytes);
  for (size_t e = 0; e < bytes; ++e)
    if (lds[e] > 1) CHECK(false, "LDS byte %zu written %d times", e, (int)lds[e]);
}

// one launch: the kernel's writes into its part of the workspace, then the finalize's reads
static void walk_launch(const pa::GpkLaunchPlan& pl, double* ws, size_t ws_doubles, bool scalars) {
  const int D = pl.D, rec = pa::gpp_record_doubles(D);
  CHECK(pl.splits >= 1 && pl.workgroups == pl.row_blocks * pl.splits && pl.workgroups <= pa::GPK_MAX_WORKGROUPS, "grid");
  CHECK(pl.scalar_doubles == (size_t)pl.workgroups * rec, "scalar_doubles=%zu", pl.scalar_doubles);
  CHECK((pl.row_doubles + pl.scalar_doubles) * sizeof(double) == pl.bytes && pl.bytes / sizeof(double) <= ws_doubles,
        "bytes=%zu", pl.bytes);
  double* row_rec = ws;
  double* sc_rec = ws + pl.row_doubles;
  for (int64_t wg = 0; wg < pl.workgroups; ++wg) {
    const int64_t rb = wg / pl.splits, i0 = rb * pa::GPK_TILE;
    const int split = (int)(wg - rb * pl.splits);
    const int64_t rows_here = pl.rows - i0 < pa::GPK_TILE ? pl.rows - i0 : pa::GPK_TILE;
    CHECK(rows_here >= 1, "workgroup %lld has no rows", (long long)wg);
    if (pl.row_records) {
      double* r = row_rec + ((int64_t)split * pl.rows + i0) * D;
      for (int64_t e = 0; e < rows_here * D; ++e) r[e] += 1.0;
    }
    if (scalars) {
      double* sc = sc_rec + wg * rec;
      sc[0] += 2.0, sc[1] += 2.0;
      for (int k = 0; k < D; ++k) sc[pa::GPP_SCALARS + k] += 2.0, sc[pa::GPP_SCALARS + D + k] += 2.0;
    }
  }
  double sum = 0.0;
  if (pl.row_records) {
    const int64_t total = pl.rows * D;
    for (int64_t e = 0; e < total; ++e)
      for (int sp = 0; sp < pl.splits; ++sp) sum += row_rec[(int64_t)sp * total + e];
    CHECK(sum == (double)total * pl.splits, "row records: %.1f", sum);      // every entry written exactly once
  }
  if (scalars) {
    sum = 0.0;
    for (int slot = 0; slot < rec; ++slot)
      for (int64_t w = 0; w < pl.workgroups; ++w) sum += sc_rec[w * rec + slot];
    CHECK(sum == 2.0 * (double)pl.workgroups * rec, "scalar records: %.1f", sum);
  }
}

static void check_call(int64_t N, int64_t M, int D, bool z_null, bool want_gx, bool want_gz, int cus, int forced, bool walk) {
  if (z_null && N != M) return;
  if (!pa::gpp_shape_ok(N, M, D, 1, D) || N == 0 || M == 0) return;
  const pa::GpkCallPlan cp = pa::gpk_call_plan(N, M, D, pa::gpp_record_doubles(D), z_null, want_gx, want_gz, cus, forced);
  CHECK(cp.run_x || cp.run_z, "nothing runs");
  CHECK(cp.run_z == (want_gz && !z_null), "run_z");
  CHECK(cp.bytes == cp.x.bytes + cp.z.bytes && cp.z_offset_doubles * sizeof(double) == cp.x.bytes, "offsets");
  // the split rule is gp_kernel_plan.h's: same grid, larger scalar records
  const pa::GpkCallPlan base = pa::gpk_call_plan(N, M, D, pa::gpk_record_doubles(D), z_null, want_gx, want_gz, cus, forced);
  CHECK(cp.x.splits == base.x.splits && cp.z.splits == base.z.splits && cp.x.workgroups == base.x.workgroups, "split rule");
  if (!walk) return;
  std::vector<double> ws(cp.bytes / sizeof(double), 0.0);
  if (cp.run_x) walk_launch(cp.x, ws.data(), ws.size(), true);
  if (cp.run_z) walk_launch(cp.z, ws.data() + cp.z_offset_doubles, ws.size() - cp.z_offset_doubles, !cp.run_x);
}

int main() {
  const int64_t Ns[] = {0, 1, 2, 63, 64, 65, 130, 300, 5000, 100000};
  const int Ds[] = {1, 2, 3, 5, 8, 17, 63, 64};
  const int forced_list[] = {0, 1, 2, 7, 1000};
  const int cus_list[] = {256, 1, 0};
  long calls = 0;
  for (int D : Ds)
    for (size_t elem : {sizeof(float), sizeof(double)}) walk_lds(D, elem, false), walk_lds(D, elem, true), calls += 2;
  for (int64_t N : Ns)
    for (int64_t M : Ns)
      for (int D : Ds)
        for (int forced : forced_list)
          for (int cus : cus_list)
            for (int flags = 0; flags < 8; ++flags) {
              const bool walk = (double)N * M <= 2e7 && (N <= 5000 || D <= 8);
              check_call(N, M, D, flags & 4, flags & 1, flags & 2, cus, forced, walk);
              ++calls;
            }
  CHECK(!pa::gpp_shape_ok(10, 10, 65, 1, 1) && !pa::gpp_shape_ok(10, 10, 0, 1, 1) && !pa::gpp_shape_ok(-1, 10, 3, 1, 1),
        "D / N limits");
  CHECK(!pa::gpp_shape_ok(10, 10, 3, 2, 1) && !pa::gpp_shape_ok(10, 10, 3, 1, 2) && pa::gpp_shape_ok(10, 10, 3, 3, 1) &&
            pa::gpp_shape_ok(10, 10, 3, 1, 3) && pa::gpp_shape_ok(10, 10, 3, 3, 3),
        "lengthscale / period limits");
  check_call(512, 100000, 8, false, true, true, 256, 0, true);        // Xu [512, D] against X [1e5, D]
  check_call(pa::GPK_MAX_POINTS - 1, 64, 64, false, true, true, 256, 0, false);
  std::printf("%ld calls, %d failures\n", calls, failures);
  return failures ? 1 : 0;
}
