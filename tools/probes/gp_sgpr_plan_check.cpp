// gp_sgpr_plan_check.cpp -- the host-side launch arithmetic of the streamed sparse-GP statistics
// (csrc/gp_sgpr_plan.h, behind pa_gp_sgpr_workspace / pa_gp_sgpr_fwd / pa_gp_sgpr_bwd) as a stand-alone host program,
// for the sanitizers:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       -I pyro_amd/csrc tools/probes/gp_sgpr_plan_check.cpp -o gp_sgpr_plan_check && ./gp_sgpr_plan_check
//
// Over a grid of (N, M, D, Q, element size, forced splits, compute units, wanted gradients) it checks the plans'
// invariants -- at least one split, no empty split, every step of N taken exactly once, LDS within 160 KiB -- and walks
// a workspace of exactly the planned size the way the kernels and the finalizes address it.  An off-by-one in the
// record arithmetic is an out-of-bounds access here, on the host.  N = 2^36 - 1 is planned (not allocated) to show
// that nothing overflows.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "gp_sgpr_plan.h"

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

static void check_splits(int64_t steps, int64_t per, int splits, int forced) {
  CHECK(splits >= 1 && per >= 1, "splits=%d per=%lld", splits, (long long)per);
  CHECK((int64_t)splits * per >= steps && (int64_t)(splits - 1) * per < (steps > 0 ? steps : 1),
        "an empty split or a step left out: steps=%lld per=%lld splits=%d", (long long)steps, (long long)per, splits);
  if (forced > 0) CHECK(splits <= forced, "splits=%d over forced=%d", splits, forced);
}

static void walk(int64_t N, int64_t M, int D, int Q, size_t elem, int cus, int forced, bool gx, bool gxu) {
  const pa::GpsFwdPlan f = pa::gps_fwd_plan(N, M, D, Q, elem, cus, forced);
  check_splits(f.steps, f.steps_per_split, f.splits, forced);
  CHECK(f.lds_bytes <= 160 * 1024 && f.workgroups == (int64_t)f.pairs * f.splits, "forward LDS=%zu", f.lds_bytes);
  CHECK((f.a_doubles + f.b_doubles) * sizeof(double) == f.bytes, "forward bytes");
  const pa::GpsBwdPlan b = pa::gps_bwd_plan(N, M, D, Q, elem, gx, gxu, cus, forced);
  check_splits(b.steps, b.steps_per_split, b.splits, forced);
  CHECK(b.lds_bytes <= 160 * 1024 && b.workgroups == (int64_t)b.chunks * b.splits, "backward LDS=%zu", b.lds_bytes);
  CHECK((b.s_doubles + b.row_doubles + b.scalar_doubles + b.gx_doubles) * sizeof(double) == b.bytes, "backward bytes");
  if (N > (1 << 16)) return;      // (planned only)
  {  // forward: every workgroup's record entries, then the finalize's reads
    std::vector<double> ws(f.bytes / sizeof(double), 0.0);
    double *a_rec = ws.data(), *b_rec = a_rec + f.a_doubles;
    const int rd = f.rec_dim;
    for (int pair = 0; pair < f.pairs; ++pair)
      for (int sp = 0; sp < f.splits; ++sp) {
        int I = 0, rem = pair;
        while (rem >= f.blocks - I) rem -= f.blocks - I, ++I;
        const int J = I + rem;
        CHECK(J < f.blocks, "pair %d -> (%d, %d)", pair, I, J);
        double* rec = a_rec + ((int64_t)pair * f.splits + sp) * rd * rd;
        for (int li = 0; li < f.tm; ++li)
          for (int lj = 0; lj < f.tm; ++lj)
            if (li < rd && lj < rd) rec[li * rd + lj] += 1.0;
        if (I == J)
          for (int li = 0; li < rd; ++li)
            for (int q = 0; q < Q; ++q) b_rec[((int64_t)I * f.splits + sp) * rd * Q + li * Q + q] += 1.0;
      }
    for (int64_t i = 0; i < M; ++i)
      for (int64_t j = i; j < M; ++j) {
        const int I = (int)(i / f.tm), J = (int)(j / f.tm), pair = I * f.blocks - I * (I - 1) / 2 + (J - I);
        double s = 0.0;
        for (int sp = 0; sp < f.splits; ++sp)
          s += a_rec[((int64_t)pair * f.splits + sp) * rd * rd + (i - I * f.tm) * rd + (j - J * f.tm)];
        CHECK(s == (double)f.splits, "A record (%lld, %lld) written %g times", (long long)i, (long long)j, s);
      }
    for (size_t e = 0; e < f.b_doubles; ++e) CHECK(b_rec[e] == 1.0, "b record %zu", e);
  }
  {  // backward
    std::vector<double> ws(b.bytes / sizeof(double), 0.0);
    double *row = ws.data() + b.s_doubles, *sc = row + b.row_doubles, *gxr = sc + b.scalar_doubles;
    for (int c = 0; c < b.chunks; ++c)
      for (int sp = 0; sp < b.splits; ++sp) {
        const int64_t c0 = (int64_t)c * pa::GPS_BWD_ROWS, rows = M - c0 < pa::GPS_BWD_ROWS ? M - c0 : pa::GPS_BWD_ROWS;
        CHECK(rows >= 1, "an empty chunk");
        if (gxu)
          for (int64_t e = 0; e < rows * D; ++e) row[((int64_t)sp * M + c0) * D + e] += 1.0;
        for (int k = 0; k < pa::GPS_SCALARS + D; ++k) sc[((int64_t)c * b.splits + sp) * (pa::GPS_SCALARS + D) + k] += 1.0;
        if (gx) {
          int64_t end = (int64_t)(sp + 1) * b.steps_per_split;
          if (end > b.steps) end = b.steps;
          for (int64_t n = (int64_t)sp * b.steps_per_split * pa::GPS_TN; n < end * pa::GPS_TN && n < N; ++n)
            for (int k = 0; k < D; ++k) gxr[((int64_t)c * N + n) * D + k] += 1.0;
        }
      }
    for (size_t e = b.s_doubles; e < ws.size(); ++e) CHECK(ws[e] == 1.0, "backward record word %zu written %g times", e, ws[e]);
  }
}

int main() {
  const int64_t Ns[] = {1, 31, 32, 33, 101, 4133, 65536, 1000000, (int64_t(1) << 36) - 1};
  const int Ms[] = {1, 63, 64, 65, 127, 128, 129, 256, 257, 511, 512};
  const int Ds[] = {1, 3, 8, 64}, Qs[] = {1, 3, 16}, forced[] = {0, 1, 3, 1000}, cus[] = {0, 1, 256};
  long cases = 0;
  for (int64_t N : Ns)
    for (int M : Ms)
      for (size_t elem : {size_t(4), size_t(8)}) {
        if (M > pa::gps_max_m(elem)) {
          CHECK(!pa::gps_shape_ok(0, N, M, 8, 1, 1, elem), "M=%d accepted", M);
          continue;
        }
        for (int D : Ds)
          for (int Q : Qs) {
            if (N == 65536 && (D != 8 || Q != 3)) continue;      // (one large allocation is enough)
            for (int f : forced)
              for (int cu : cus) {
                CHECK(pa::gps_shape_ok(0, N, M, D, Q, 1, elem), "shape refused");
                walk(N, M, D, Q, elem, cu, f, (cases & 1) != 0, (cases & 2) != 0);
                ++cases;
              }
          }
      }
  CHECK(!pa::gps_shape_ok(0, 8, 8, 65, 1, 1, 4) && !pa::gps_shape_ok(0, 8, 8, 8, 17, 1, 4) &&
            !pa::gps_shape_ok(0, int64_t(1) << 36, 8, 8, 1, 1, 4) && !pa::gps_shape_ok(5, 8, 8, 8, 1, 1, 4),
        "a shape outside the limits was accepted");
  std::printf("%ld cases, %d failures\n", cases, failures);
  return failures ? 1 : 0;
}
