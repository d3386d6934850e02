// glm_family_plan_check.cpp -- the host-side launch arithmetic of the family GLM kernels (csrc/glm_family_plan.h: the
// shape checks, grid, trips of the tile loop, record and workspace sizes behind pa_glm_family_workspace /
// pa_glm_family_fwd_bwd) as a stand-alone host program, for the sanitizers:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       -I pyro_amd/csrc tools/probes/glm_family_plan_check.cpp -o glm_family_plan_check && ./glm_family_plan_check
//
// Over the shapes of tests/glm_family_cases.py (and the limits) it checks the plan's invariants and walks a workspace
// of exactly the planned size the way the kernel and the finalize address it: every record's accumulator tiles, its
// three scalar rows per particle tile and its two fp64 words, for every (pass, workgroup) -- an off-by-one in the
// record or workspace arithmetic is an out-of-bounds access here, on the host.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "glm_family_plan.h"

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

static void check_shape(int family, int64_t N, int64_t D, int64_t P, int cus, int max_blocks, bool walk) {
  if (!pa::glmf_shape_ok(family, N, D, P)) return;
  const pa::GlmFamilyPlan pl = pa::glmf_plan(N, D, P, cus, max_blocks);
  const long long n = (long long)N, d = (long long)D, p = (long long)P;
  CHECK(pl.DT * 32 >= D && (pl.DT == 1 || (pl.DT / 2) * 32 < D), "DT=%d D=%lld", pl.DT, d);
  CHECK(pl.PT == 1 || pl.DT == 1, "PT=%d DT=%d", pl.PT, pl.DT);
  CHECK((int64_t)pl.npass * 32 * pl.PT >= P && (int64_t)(pl.npass - 1) * 32 * pl.PT < P, "npass=%d P=%lld", pl.npass, p);
  CHECK(pl.npass <= 65535, "grid.y %d", pl.npass);
  CHECK(pl.nblocks >= 1 && (max_blocks == 0 || pl.nblocks <= max_blocks), "nblocks=%d cap=%d", pl.nblocks, max_blocks);
  CHECK(pl.ntiles * 32 >= N && (pl.ntiles - 1) * 32 < N, "ntiles=%lld N=%lld", (long long)pl.ntiles, n);
  // every tile is visited: wave (blk, wv) takes tiles blk * WAVES + wv + it * nblocks * WAVES, it < iters
  CHECK(pl.iters >= 1 && pl.iters * pl.nblocks * pa::GLMF_WAVES >= pl.ntiles, "iters=%lld", (long long)pl.iters);
  CHECK((pl.iters - 1) * pl.nblocks * pa::GLMF_WAVES < (pl.ntiles > 0 ? pl.ntiles : 1), "one trip too many");
  // the largest flat element offset a lane forms fits int64 with room to spare
  CHECK((pl.iters * pl.nblocks * pa::GLMF_WAVES + 1) * 32 * D < (int64_t(1) << 62), "offset overflow");
  CHECK(pl.rec == pa::glmf_record_floats(pl.DT, pl.PT) && pl.rec % 32 == 0, "rec=%d", pl.rec);
  // the epilogue's LDS use fits the tiles' LDS; the dynamic allocation fits the CU
  const size_t epi = (size_t)pl.PT * pl.DT * 1024 + 3 * pl.PT * 64 + 4 * pa::GLMF_WAVES;
  CHECK(epi * sizeof(float) <= pl.lds_bytes, "epilogue %zu floats, LDS %zu bytes", epi, pl.lds_bytes);
  CHECK(pl.lds_bytes <= 160 * 1024, "LDS %zu", pl.lds_bytes);
  CHECK(pl.workspace_bytes == (size_t)pl.nblocks * pl.npass * pl.rec * sizeof(float), "workspace");
  if (!walk) return;
  std::vector<float> ws(pl.workspace_bytes / sizeof(float));
  const int gwf = pl.PT * pl.DT * 1024;
  for (int pass = 0; pass < pl.npass; ++pass)
    for (int blk = 0; blk < pl.nblocks; ++blk) {
      float* rec = ws.data() + ((int64_t)pass * pl.nblocks + blk) * pl.rec;      // the kernel's record
      for (int i = 0; i < gwf; ++i) rec[i] = 1.0f;
      for (int i = 0; i < 3 * pl.PT * 32; ++i) rec[gwf + i] = 2.0f;
      double ex[2] = {3.0, 4.0};
      std::memcpy(rec + gwf + 3 * pl.PT * 32, ex, sizeof(ex));
      CHECK(((gwf + 3 * pl.PT * 32) * sizeof(float)) % 8 == 0 && ((size_t)pl.rec * sizeof(float)) % 8 == 0, "fp64 slot");
    }
  // the finalize's reads: output (p, d) and the particle's scalars
  double sum = 0.0;
  for (int64_t pp = 0; pp < P; ++pp) {
    const int plx = (int)(pp % (32 * pl.PT)), pt = plx >> 5, i = plx & 31, pass = (int)(pp / (32 * pl.PT));
    const int hh = (i >> 2) & 1, reg = (i & 3) + 4 * (i >> 3);
    for (int blk = 0; blk < pl.nblocks; ++blk) {
      const float* r = ws.data() + ((int64_t)pass * pl.nblocks + blk) * pl.rec;
      for (int dd = 0; dd < D; ++dd) sum += r[((pt * pl.DT + (dd >> 5)) * 16 + reg) * 64 + (dd & 31) + 32 * hh];
      for (int which = 0; which < 3; ++which) sum += r[gwf + (3 * pt + which) * 32 + i];
      double ex[2];
      std::memcpy(ex, ws.data() + (int64_t)blk * pl.rec + gwf + 3 * pl.PT * 32, sizeof(ex));
      sum += ex[0] + ex[1];
    }
  }
  const double want = (double)P * pl.nblocks * ((double)D + 3 * 2.0 + 7.0);
  CHECK(sum == want, "walk sum %.1f want %.1f (N=%lld D=%lld P=%lld)", sum, want, n, d, p);
}

int main() {
  const int64_t Ns[] = {0, 1, 31, 32, 33, 127, 128, 129, 300, 1000, 1100, 1000000};
  const int64_t Ds[] = {1, 3, 4, 5, 31, 32, 33, 64, 127, 128};
  const int64_t Ps[] = {1, 3, 31, 32, 33, 64, 65, 1000};
  const int caps[] = {0, 1, 2};
  const int cus_list[] = {256, 1, 0};
  long shapes = 0;
  for (int family = 0; family < pa::GLMF_FAMILIES; ++family)
    for (int64_t N : Ns)
      for (int64_t D : Ds)
        for (int64_t P : Ps)
          for (int cap : caps)
            for (int cus : cus_list) {
              check_shape(family, N, D, P, cus, cap, family == 0 || (N <= 1100 && P <= 65));
              ++shapes;
            }
  // the limits of the entry points: refused before any arithmetic, or planned without overflow
  CHECK(!pa::glmf_shape_ok(0, 10, 129, 4) && !pa::glmf_shape_ok(0, 10, 0, 4) && !pa::glmf_shape_ok(0, -1, 8, 4),
        "D / N limits");
  CHECK(!pa::glmf_shape_ok(4, 10, 8, 4) && !pa::glmf_shape_ok(-1, 10, 8, 4) && !pa::glmf_shape_ok(0, 10, 8, 0),
        "family / P limits");
  CHECK(!pa::glmf_shape_ok(0, pa::GLMF_MAX_N, 8, 4) && !pa::glmf_shape_ok(0, 10, 8, pa::GLMF_MAX_P), "size limits");
  CHECK(pa::glmf_aux_columns(0) == 1 && pa::glmf_aux_columns(1) == 2 && pa::glmf_aux_columns(2) == 0 &&
            pa::glmf_aux_columns(3) == 0 && pa::glmf_aux_columns(4) == -1,
        "aux columns");
  check_shape(1, pa::GLMF_MAX_N - 1, 128, pa::GLMF_MAX_P - 1, 256, 0, false);
  check_shape(3, pa::GLMF_MAX_N - 1, 1, 1, 256, 1, false);
  check_shape(2, pa::GLMF_MAX_N - 1, 32, 33, 1 << 20, 0, false);
  std::printf("%ld shapes, %d failures\n", shapes, failures);
  return failures ? 1 : 0;
}
