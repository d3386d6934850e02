// gp_sgpr_plan.h -- host-side launch arithmetic of the streamed sparse-GP statistics (gp_sgpr.hip): block pairs, splits
// of N, record counts, LDS and workspace bytes.  Plain C++ with no HIP in it, so that the same code is compiled into a
// stand-alone host program and run under the address / undefined-behaviour sanitizers
// (tools/probes/gp_sgpr_plan_check.cpp).
#pragma once
#include <stddef.h>
#include <stdint.h>

#ifdef __HIPCC__
#define GPS_HD __host__ __device__
#else
#define GPS_HD
#endif

namespace pa {

constexpr int GPS_THREADS = 256;      // four waves
constexpr int GPS_SUB = 32;           // one matrix-core block: 32 x 32 outputs
constexpr int GPS_TN = 32;            // points of N staged per step (T_N)
constexpr int GPS_KS = GPS_TN + 1;    // row stride of a staged Kuf tile: odd, so 32 rows fall into 32 banks
constexpr int GPS_FLUSH = 4096;       // points an accumulator runs before it is added to its float64 record (F)
constexpr int GPS_MAX_D = 64;
constexpr int GPS_MAX_Q = 16;
constexpr int GPS_BWD_ROWS = 128;     // inducing rows whose gradient one backward workgroup accumulates
constexpr int GPS_SCALARS = 3;        // per-workgroup scalar partials: variance, scale_mixture, scalar lengthscale
constexpr int GPS_FAMILIES = 5;
constexpr int64_t GPS_MAX_POINTS = int64_t(1) << 36;
constexpr int64_t GPS_MAX_WORKGROUPS = (int64_t(1) << 31) - 1;

// rows of a forward block of A (T_M) and the largest M, by element size
GPS_HD inline int gps_tm(size_t elem) { return elem == 4 ? 128 : 64; }
GPS_HD inline int gps_max_m(size_t elem) { return elem == 4 ? 512 : 256; }
GPS_HD inline int gps_lds_stride(int D) { return D | 1; }

inline bool gps_shape_ok(int family, int64_t N, int64_t M, int64_t D, int64_t Q, int n_ls, size_t elem) {
  return family >= 0 && family < GPS_FAMILIES && N >= 0 && N < GPS_MAX_POINTS && M >= 0 && M <= gps_max_m(elem) &&
         D >= 1 && D <= GPS_MAX_D && Q >= 1 && Q <= GPS_MAX_Q && (n_ls == 1 || n_ls == D);
}

inline int64_t gps_div_up(int64_t a, int64_t b) { return (a + b - 1) / b; }

// splits of ``steps`` steps of T_N points so that ``units`` x splits workgroups are two per compute unit; none is empty
inline void gps_split(int64_t steps, int64_t units, int cus, int forced, int64_t* per_split, int* splits) {
  int64_t want = forced > 0 ? forced : gps_div_up((int64_t)2 * (cus > 0 ? cus : 1), units > 0 ? units : 1);
  if (want > steps) want = steps;
  if (want < 1) want = 1;
  int64_t per = gps_div_up(steps, want);
  if (per < 1) per = 1;
  int64_t s = gps_div_up(steps, per);
  *per_split = per, *splits = (int)(s < 1 ? 1 : s);
}

// ---- forward: workgroup (block pair I <= J, split) leaves one record [rec_dim, rec_dim] of A, and on the diagonal
// (I = J) one record [rec_dim, Q] of b
struct GpsFwdPlan {
  int tm, blocks, pairs, rec_dim, splits, D, Q;
  int64_t steps, steps_per_split, workgroups;
  size_t a_doubles, b_doubles, bytes, lds_bytes;
};

inline size_t gps_fwd_lds_bytes(int D, int Q, size_t elem) {
  const size_t tm = gps_tm(elem), s = gps_lds_stride(D);
  return (size_t)D * sizeof(double) + (2 * tm * s + GPS_TN * s + 2 * tm * GPS_KS + (size_t)GPS_TN * Q) * elem;
}

inline GpsFwdPlan gps_fwd_plan(int64_t N, int64_t M, int D, int Q, size_t elem, int cus, int forced_splits) {
  GpsFwdPlan p;
  p.tm = gps_tm(elem), p.D = D, p.Q = Q;
  p.blocks = (int)gps_div_up(M, p.tm);
  p.pairs = p.blocks * (p.blocks + 1) / 2;
  p.rec_dim = (int)(M < p.tm ? M : p.tm);
  p.steps = gps_div_up(N, GPS_TN);
  gps_split(p.steps, p.pairs, cus, forced_splits, &p.steps_per_split, &p.splits);
  p.workgroups = (int64_t)p.pairs * p.splits;
  p.a_doubles = (size_t)p.pairs * p.splits * p.rec_dim * p.rec_dim;
  p.b_doubles = (size_t)p.blocks * p.splits * p.rec_dim * Q;
  p.bytes = (p.a_doubles + p.b_doubles) * sizeof(double);
  p.lds_bytes = gps_fwd_lds_bytes(D, Q, elem);
  return p;
}

// ---- backward: workgroup (chunk of GPS_BWD_ROWS inducing rows, split) walks its steps of N with ALL of Kuf[:, step]
// in LDS, and leaves one record [rows of the chunk, D] and one scalar record.  The workspace: S = gA + gA^T [M, M] in
// the tensor's dtype (rounded up to 8 bytes), the row records [splits, M, D], the scalar records
// [workgroups, SCALARS + D], and with want_gx the per-chunk partial gradients of x [chunks, N, D]
struct GpsBwdPlan {
  int chunks, splits, D, Q;
  int64_t steps, steps_per_split, workgroups;
  bool want_gx, want_gxu;
  size_t s_doubles, row_doubles, scalar_doubles, gx_doubles, bytes, lds_bytes;
};

inline size_t gps_bwd_lds_bytes(int64_t M, int D, int Q, size_t elem) {
  const size_t s = gps_lds_stride(D), rows = (size_t)(M > GPS_BWD_ROWS ? M : GPS_BWD_ROWS) + 1;
  const size_t f64 = (size_t)D + (size_t)GPS_BWD_ROWS * D + (size_t)(GPS_THREADS / 64) * D;
  return f64 * sizeof(double) + (rows * GPS_KS + GPS_TN * s + (size_t)GPS_TN * Q) * elem;
}

inline GpsBwdPlan gps_bwd_plan(int64_t N, int64_t M, int D, int Q, size_t elem, bool want_gx, bool want_gxu, int cus,
                               int forced_splits) {
  GpsBwdPlan p;
  p.D = D, p.Q = Q, p.want_gx = want_gx, p.want_gxu = want_gxu;
  p.chunks = (int)gps_div_up(M, GPS_BWD_ROWS);
  p.steps = gps_div_up(N, GPS_TN);
  gps_split(p.steps, p.chunks, cus, forced_splits, &p.steps_per_split, &p.splits);
  p.workgroups = (int64_t)p.chunks * p.splits;
  p.s_doubles = ((size_t)M * M * elem + 7) / 8;
  p.row_doubles = want_gxu ? (size_t)p.splits * M * D : 0;
  p.scalar_doubles = (size_t)p.workgroups * (GPS_SCALARS + D);
  p.gx_doubles = want_gx ? (size_t)p.chunks * (size_t)N * D : 0;
  p.bytes = (p.s_doubles + p.row_doubles + p.scalar_doubles + p.gx_doubles) * sizeof(double);
  p.lds_bytes = gps_bwd_lds_bytes(M, D, Q, elem);
  return p;
}

}  // namespace pa
