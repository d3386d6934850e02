// gp_wrap_plan_check.cpp -- the host-side launch arithmetic of the wrapped covariance kernels (csrc/gp_wrap_plan.h: the
// row records widened to D + 1 columns, the LDS layout with the staged scales, the caps behind pa_gp_wrap_bwd_workspace /
// pa_gp_wrap_bwd) as a stand-alone host program, for the sanitizers:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       -I pyro_amd/csrc tools/probes/gp_wrap_plan_check.cpp -o gp_wrap_plan_check && ./gp_wrap_plan_check
//
// Over a grid of (N, M, D, forced splits, compute units, wanted sides) it walks a workspace of exactly the planned size
// the way the kernel, gp_copy_row_record and the finalize address it -- every workgroup's row record [rows, D + 1] and
// scalar record, of both launches -- and the LDS of a workgroup the way the backward kernel lays it out.  An off-by-one
// in the record, workspace or LDS arithmetic is an out-of-bounds access here, on the host.  The splits themselves are
// gp_kernel_plan.h's (tools/probes/gp_kernel_plan_check.cpp).
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "gp_wrap_plan.h"

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
  const int D = pl.D, W = pa::gpw_row_width(D), rec_doubles = pa::gpk_record_doubles(D);
  CHECK((pl.row_doubles + pl.scalar_doubles) * sizeof(double) == pl.bytes && pl.bytes / sizeof(double) <= ws_doubles,
        "bytes=%zu", pl.bytes);
  CHECK(pl.row_doubles == (pl.row_records ? (size_t)pl.splits * pl.rows * W : 0), "row_doubles=%zu", pl.row_doubles);
  double* row_rec = ws;
  double* sc_rec = ws + pl.row_doubles;
  for (int64_t wg = 0; wg < pl.workgroups; ++wg) {
    const int64_t rb = wg / pl.splits;
    const int split = (int)(wg - rb * pl.splits);
    const int64_t i0 = rb * pa::GPK_TILE;
    const int64_t rows_here = pl.rows - i0 < pa::GPK_TILE ? pl.rows - i0 : pa::GPK_TILE;
    if (pl.row_records) {
      double* rec = row_rec + ((int64_t)split * pl.rows + i0) * W;
      for (int64_t e = 0; e < rows_here * W; ++e) rec[e] += 1.0;
    }
    if (scalars)
      for (int k = 0; k < rec_doubles; ++k) sc_rec[wg * rec_doubles + k] += 2.0;
  }
  double sum = 0.0;
  if (pl.row_records) {
    const int64_t total = pl.rows * W;
    for (int64_t e = 0; e < total; ++e)
      for (int sp = 0; sp < pl.splits; ++sp) sum += row_rec[(int64_t)sp * total + e];
    CHECK(sum == (double)total * pl.splits, "row records: %.1f", sum);      // every entry written exactly once
  }
  if (scalars) {
    sum = 0.0;
    for (int64_t w = 0; w < pl.workgroups * rec_doubles; ++w) sum += sc_rec[w];
    CHECK(sum == 2.0 * (double)pl.workgroups * rec_doubles, "scalar records: %.1f", sum);
  }
}

// the backward kernel's LDS: two point tiles, the scales [2, TILE], then 1 / l [D], acc [TILE, D + 1], ls_acc [4, D]
static void walk_lds(int D, size_t elem) {
  const size_t bytes = pa::gpw_bwd_lds_bytes(D, elem), head = pa::gpw_lds_head_bytes(D, elem);
  CHECK(bytes <= 160 * 1024 && pa::gpw_fwd_lds_bytes(D, elem) <= bytes && head % 8 == 0, "LDS of D=%d: %zu bytes", D, bytes);
  std::vector<unsigned char> lds(bytes, 0);
  const int stride = pa::gpk_lds_stride(D);
  const size_t scales_end = ((size_t)2 * pa::GPK_TILE * stride + 2 * pa::GPK_TILE) * elem;
  CHECK(scales_end <= head, "the scales end at %zu, the float64 words begin at %zu", scales_end, head);
  for (size_t e = 0; e < scales_end; ++e) lds[e] += 1;
  double* words = reinterpret_cast<double*>(lds.data() + head);
  const size_t n = (size_t)D + (size_t)pa::GPK_TILE * pa::gpw_row_width(D) + (size_t)pa::GPK_WAVES * D;
  for (size_t e = 0; e < n; ++e) words[e] = 1.0;
  // the last entries that the kernel addresses: the scale column of row 63, and wave 3's lengthscale sum of feature D - 1
  double* acc = words + D;
  acc[63 * pa::gpw_row_width(D) + D] = 2.0;
  (acc + pa::GPK_TILE * pa::gpw_row_width(D))[3 * D + D - 1] = 2.0;
}

static void check_call(int64_t N, int64_t M, int D, bool z_null, bool rows_x, bool rows_z, int cus, int forced) {
  if ((z_null && N != M) || !pa::gpk_shape_ok(0, N, M, D, 1) || N == 0 || M == 0) return;
  const pa::GpkCallPlan cp = pa::gpw_call_plan(N, M, D, z_null, rows_x, rows_z, cus, forced);
  const pa::GpkCallPlan base = pa::gpk_call_plan(N, M, D, pa::gpk_record_doubles(D), z_null, rows_x, rows_z, cus, forced);
  CHECK(cp.run_x == base.run_x && cp.run_z == base.run_z && cp.x.splits == base.x.splits && cp.z.splits == base.z.splits,
        "the launches are gp_kernel_plan.h's");
  CHECK(cp.bytes == cp.x.bytes + cp.z.bytes && cp.z_offset_doubles * sizeof(double) == cp.x.bytes && cp.bytes >= base.bytes,
        "offsets");
  CHECK(!cp.run_x || cp.x.row_records == rows_x, "x's row records");
  std::vector<double> ws(cp.bytes / sizeof(double), 0.0);
  if (cp.run_x) walk_launch(cp.x, ws.data(), ws.size(), true);
  if (cp.run_z) walk_launch(cp.z, ws.data() + cp.z_offset_doubles, ws.size() - cp.z_offset_doubles, !cp.run_x);
}

int main() {
  const int64_t Ns[] = {0, 1, 2, 63, 64, 65, 130, 300, 5000};
  const int Ds[] = {1, 2, 3, 5, 8, 17, 63, 64};
  const int forced_list[] = {0, 1, 2, 7, 1000};
  const int cus_list[] = {256, 1, 0};
  long calls = 0;
  for (int64_t N : Ns)
    for (int64_t M : Ns)
      for (int D : Ds)
        for (int forced : forced_list)
          for (int cus : cus_list)
            for (int flags = 0; flags < 8; ++flags, ++calls)
              if ((double)N * M <= 2e6 || D <= 8) check_call(N, M, D, flags & 4, flags & 1, flags & 2, cus, forced);
  for (int D = 1; D <= pa::GPK_MAX_D; ++D) walk_lds(D, 4), walk_lds(D, 8);
  // the variants and the caps of the entry points
  CHECK(pa::gpw_variant_ok(pa::GPW_COSINE, pa::GPW_Q_IDENTITY, false) && !pa::gpw_variant_ok(0, pa::GPW_Q_IDENTITY, false) &&
            pa::gpw_variant_ok(0, pa::GPW_Q_IDENTITY, true) && pa::gpw_variant_ok(4, pa::GPW_Q_EXP, false) &&
            !pa::gpw_variant_ok(5, pa::GPW_Q_EXP, false) && !pa::gpw_variant_ok(0, 3, true),
        "variants");
  CHECK(pa::gpw_supported(4, pa::GPW_Q_POLY, 8, true) && !pa::gpw_supported(4, pa::GPW_Q_POLY, 9, false) &&
            !pa::gpw_supported(4, pa::GPW_Q_POLY, 0, false) && !pa::gpw_supported(8, pa::GPW_Q_POLY, 4, true) &&
            pa::gpw_supported(8, pa::GPW_Q_POLY, 4, false) && pa::gpw_supported(8, pa::GPW_Q_EXP, 0, true),
        "caps");
  std::printf("%ld calls, %d failures\n", calls, failures);
  return failures ? 1 : 0;
}
