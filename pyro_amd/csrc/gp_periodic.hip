// gp_periodic.hip -- the periodic covariance matrix of a Gaussian-process model and its gradient, by DIRECT
// DIFFERENCES with an exact range reduction: with theta_ijk = pi (x_ik - z_jk) / p_k and s = sin(theta),
//   K[i, j] = variance * exp(-2 sum_k s_ijk^2 / l_k^2),
// lengthscale and period of 1 or D elements each, f32 and f64, D <= 64.  The forward is ONE launch that writes K once;
// the backward is one pass over the incoming gradient G per side that wants a gradient, plus a fixed-order finalize.
// No float atomics: bit-reproducible from call to call.
//
// Reference path replaced: pyro/contrib/gp/kernels/periodic.py forms X.unsqueeze(1) - Z.unsqueeze(0), a [N, M, D]
// tensor, and makes four more element-wise passes of that size, which autograd keeps alive.  Nothing of size
// N x M x D exists here: a pair's D angles live in registers, one at a time.
//
// Per pair and feature.  x and z are staged in LDS UNSCALED (gp_tile.h), beside 1 / p_k and 1 / l_k^2 in float64.
//   d = (double)x - (double)z          float32 inputs are exact in float64
//   u = d * (1 / p)                    the angle in half-turns, theta = pi u
//   t = u - rint(u)                    in [-1/2, 1/2], EXACT once u is formed (Sterbenz)
//   s = sinpi(t), c = cospi(t)         of the gradient pass in the tensor's dtype: the cast of t to float32 keeps a
//                                      RELATIVE error, so nearby points keep relative accuracy in s; s^2 and
//                                      sin(2 theta) = 2 s c have period 1 in u.  The s of the exponent: gpp_sinpi_reduced
// The exponent sum_k s^2 / l_k^2 is accumulated in float64 for both dtypes and the exponential taken through the hi / lo
// split (gp_exp_of): exp magnifies a relative error of its argument by the argument.
//
// Two cheaper forms were rejected and are not built.  (1) Per-point features, sin and cos of pi x / p combined by the
// angle-difference identity, would take the transcendentals out of the pair loop, but their absolute error in s does not
// shrink with s: at l = 1e-3 the exponent 2 s^2 / l^2 magnifies an error of 1e-16 in s by 1e6 s, orders of magnitude
// over the float64 bound the tests derive, and in float32 the gradients of nearby points lose their relative accuracy.
// (2) The expansion s^2 = (1 - cos 2 theta) / 2 with cos 2 theta = cos a cos b + sin a sin b turns the exponent into a
// [N, 2D] x [2D, M] product that matrix instructions could take, but it cancels at nearby points by eps sum_k 1 / l_k^2,
// the failure the README documents for the Euclidean expansion of the stationary kernel.  So this kernel is VALU work.
//
// Tiles, splits, records: gp_kernel.hip's (64 x 64 tiles, 256 threads, 4 x 4 per lane, odd LDS row stride, column
// splits that fill the device; gp_kernel_plan.h), with gp_periodic_plan.h for what differs.  The frame itself is
// gp_tile.h's, the launch and the two-sided backward driver gp_host.h's, gp_exp_of gp_families.h's.
//
// Backward.  Nothing of the forward is kept: K is recomputed from the inputs (a model adds noise to its diagonal in
// place).  With W = G K, a tile first forms the exponent (gpp_sinpi_reduced per pair and feature), then W, then walks the
// features once more with ONE sincospi per pair and feature and no other transcendental:
//   gx_ik = -(2 pi / (p_k l_k^2)) sum_j W_ij sin(2 theta_ijk)       gz: the same launch with the roles exchanged
//   g_l_k = (4 / l_k^3) sum_ij W_ij s_ijk^2                         g_p_k = (2 / (p_k l_k^2)) sum_ij W_ij theta_ijk sin(2 theta_ijk)
//   g_variance = sum_ij G_ij K_ij / variance
// (theta in g_p is the angle itself, pi u, not its reduced value.)  A scalar lengthscale takes sum_k s^2 = l^2 * exponent
// and needs no per-feature pass; a scalar period sums its per-feature records in the finalize.  Per tile and feature a
// thread sums over its 4 columns, the 16 lanes of a row add theirs on DPP and lane tx = 0 adds the result to the row's
// float64 accumulator in LDS; the lengthscale's and the period's sums go wave by wave to per-wave float64 accumulators
// (one writer per entry).  A workgroup leaves one row record [64, D] in slot ``split`` and one scalar record
// {variance, scalar lengthscale, lengthscale_k, period_k}; the finalize kernel adds records in a fixed order in
// float64, applies the factors above and rounds once.  With z = x (null) one launch gives x both roles: the weight of
// the row gradient is (G_ij + G_ji) K_ij, G is read twice.
//
// gfx950 cross-compile (hipcc -O3, -Rpass-analysis=kernel-resource-usage): no instantiation uses scratch; LDS is
// dynamic; the register table is in the README entry "Gaussian processes".
#include "gp_families.h"
#include "gp_host.h"
#include "gp_periodic_dev.h"
#include "gp_periodic_plan.h"

namespace pa {

// 1 / p_k and 1 / l_k^2 in float64
template <typename T>
__device__ __forceinline__ void gpp_stage_parameters(const T* __restrict__ ls, int n_ls, const T* __restrict__ period,
                                                     int n_p, int D, double* inv_p, double* inv_l2) {
  for (int k = threadIdx.x; k < D; k += GPK_THREADS) {
    const double l = (double)ls[n_ls == 1 ? 0 : k];
    inv_p[k] = 1.0 / (double)period[n_p == 1 ? 0 : k];
    inv_l2[k] = 1.0 / (l * l);
  }
}

// sum_k s^2 / l_k^2 of the thread's 4 x 4 entries, in float64 for both dtypes
template <typename T>
__device__ __forceinline__ void gpp_exponent_tile(const T* xs, const T* zs, const double* inv_p, const double* inv_l2,
                                                  int D, int stride, int ty, int tx, double (&acc)[4][4]) {
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[r][c] = 0.0;
  for (int k = 0; k < D; ++k) {
    const double ip = inv_p[k], il2 = inv_l2[k];
    double xv[4], zv[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) xv[r] = (double)xs[(4 * ty + r) * stride + k];
#pragma unroll
    for (int c = 0; c < 4; ++c) zv[c] = (double)zs[(4 * tx + c) * stride + k];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const double u = (xv[r] - zv[c]) * ip;
        const double s = gpp_sinpi_reduced<T>(u - rint(u));
        acc[r][c] = fma(s * s, il2, acc[r][c]);
      }
  }
}

// ---- forward ---------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(GPK_THREADS) void gp_periodic_fwd_kernel(const T* __restrict__ x, const T* __restrict__ z,
                                                                      const T* __restrict__ ls, int n_ls,
                                                                      const T* __restrict__ period, int n_p,
                                                                      const T* __restrict__ variance, T* __restrict__ K,
                                                                      int64_t N, int64_t M, int D, int64_t col_tiles) {
  extern __shared__ __attribute__((aligned(16))) unsigned char gp_lds[];
  const int stride = gpk_lds_stride(D);
  T* xs = reinterpret_cast<T*>(gp_lds);
  T* zs = xs + GPK_TILE * stride;
  double* inv_p = reinterpret_cast<double*>(gp_lds + gpk_lds_head_bytes(D, sizeof(T)));      // [D]
  double* inv_l2 = inv_p + D;                                                                  // [D]
  const int64_t rt = (int64_t)blockIdx.x / col_tiles, ct = (int64_t)blockIdx.x - rt * col_tiles;
  const int64_t i0 = rt * GPK_TILE, j0 = ct * GPK_TILE;
  gp_stage(x, i0, N, D, stride, xs);
  gp_stage(z, j0, M, D, stride, zs);
  gpp_stage_parameters(ls, n_ls, period, n_p, D, inv_p, inv_l2);
  __syncthreads();
  const int ty = threadIdx.x >> 4, tx = threadIdx.x & 15;
  double e[4][4];
  gpp_exponent_tile(xs, zs, inv_p, inv_l2, D, stride, ty, tx, e);
  const T var = variance[0];
  const int64_t j = j0 + 4 * tx;
  const bool vec = (M & 3) == 0 && j + 3 < M && (uintptr_t)K % sizeof(Vec4<T>) == 0;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int64_t i = i0 + 4 * ty + r;
    if (i >= N) continue;
    Vec4<T> out;
#pragma unroll
    for (int c = 0; c < 4; ++c) out.v[c] = var * gp_exp_of<T>(-2.0 * e[r][c]);
    T* dst = K + i * M + j;
    if (vec) {
      *reinterpret_cast<Vec4<T>*>(dst) = out;
    } else {
#pragma unroll
      for (int c = 0; c < 4; ++c)
        if (j + c < M) dst[c] = out.v[c];
    }
  }
}

// ---- backward ----------------------------------------------------------------------------------------------------------
template <typename T>
struct GppBwdArgs {
  const T *xr, *xc;            // the points that get a gradient [R, D], the points that are walked [C, D]
  const T* G;                  // G(i, j) = G[i * g_sr + j * g_sc], one of the strides is 1
  int64_t g_sr, g_sc;
  const T *ls, *period;
  int n_ls, n_p, D, splits;
  int want_rows, want_ls, want_period, want_scalars;
  int64_t R, C, tiles_per_split, col_tiles;
  double *row_rec, *sc_rec;    // [splits, R, D], [workgroups, GPP_SCALARS + 2 D]
};

// SYM: z = x, the row gradient's weight is (G_ij + G_ji) K_ij
template <typename T, bool SYM>
__global__ __launch_bounds__(GPK_THREADS) void gp_periodic_bwd_kernel(const GppBwdArgs<T> a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char gp_lds[];
  __shared__ double red[GPK_WAVES];
  const int D = a.D, stride = gpk_lds_stride(D);
  T* xs = reinterpret_cast<T*>(gp_lds);
  T* zs = xs + GPK_TILE * stride;
  double* inv_p = reinterpret_cast<double*>(gp_lds + gpk_lds_head_bytes(D, sizeof(T)));      // [D]
  double* inv_l2 = inv_p + D;                                                                  // [D]
  double* acc = inv_l2 + D;                                                                    // [64, D]
  double* ls_acc = acc + GPK_TILE * D;                                                         // [4, D]
  double* p_acc = ls_acc + GPK_WAVES * D;                                                      // [4, D]
  const int tid = threadIdx.x, ty = tid >> 4, tx = tid & 15, lane = tid & 63, wave = tid >> 6;
  const int64_t rb = (int64_t)blockIdx.x / a.splits;
  const int split = (int)((int64_t)blockIdx.x - rb * a.splits);
  const int64_t i0 = rb * GPK_TILE;
  gp_stage(a.xr, i0, a.R, D, stride, xs);
  gpp_stage_parameters(a.ls, a.n_ls, a.period, a.n_p, D, inv_p, inv_l2);
  for (int e = tid; e < (GPK_TILE + 2 * GPK_WAVES) * D; e += GPK_THREADS) acc[e] = 0.0;
  const bool ard = a.want_ls && a.n_ls != 1, per_feature = a.want_rows || ard || a.want_period;
  double s_var = 0.0, s_ls = 0.0;
  int64_t ct_end = (int64_t)(split + 1) * a.tiles_per_split;
  if (ct_end > a.col_tiles) ct_end = a.col_tiles;
  for (int64_t ct = (int64_t)split * a.tiles_per_split; ct < ct_end; ++ct) {
    const int64_t j0 = ct * GPK_TILE;
    __syncthreads();                               // the previous tile's reads of zs are over
    gp_stage(a.xc, j0, a.C, D, stride, zs);
    __syncthreads();
    T ws[4][4], wr[SYM ? 4 : 1][4];                // W / variance, and its symmetric twin for the rows
    T t_var = T(0), t_ls = T(0);
    {
      double e[4][4];
      gpp_exponent_tile(xs, zs, inv_p, inv_l2, D, stride, ty, tx, e);
      T g[4][4], gt[SYM ? 4 : 1][4];
      gp_load_g(a, a.g_sr, a.g_sc, i0, j0, ty, tx, g);
      if constexpr (SYM) gp_load_g(a, a.g_sc, a.g_sr, i0, j0, ty, tx, gt);      // G(j, i)
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const T f = gp_exp_of<T>(-2.0 * e[r][c]);
          ws[r][c] = g[r][c] * f;                  // zero outside [R, C]: padded entries weigh nothing
          if constexpr (SYM) wr[r][c] = (g[r][c] + gt[r][c]) * f;
          t_var += ws[r][c];
          t_ls += ws[r][c] * (T)e[r][c];
        }
    }
    s_var += (double)t_var, s_ls += (double)t_ls;
    if (!per_feature) continue;
    for (int k = 0; k < D; ++k) {
      const double ip = inv_p[k];
      double xv[4], zv[4];
      T p[4], ql = T(0), qp = T(0);
#pragma unroll
      for (int r = 0; r < 4; ++r) xv[r] = (double)xs[(4 * ty + r) * stride + k];
#pragma unroll
      for (int c = 0; c < 4; ++c) zv[c] = (double)zs[(4 * tx + c) * stride + k];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        p[r] = T(0);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const double u = (xv[r] - zv[c]) * ip;
          T s, co;
          gpp_sincospi((T)(u - rint(u)), s, co);
          const T s2t = T(2) * s * co;             // sin(2 theta)
          const T w = ws[r][c], wrow = SYM ? wr[SYM ? r : 0][c] : w;
          p[r] += wrow * s2t;
          ql += w * s * s;
          qp += w * s2t * (T)(3.14159265358979323846 * u);
        }
      }
      if (a.want_rows) {
#pragma unroll
        for (int r = 0; r < 4; ++r) gp_row_add(p[r], acc, (4 * ty + r) * D + k, tx);
      }
      if (ard) gp_wave_add(ql, ls_acc, wave * D + k, lane);
      if (a.want_period) gp_wave_add(qp, p_acc, wave * D + k, lane);
    }
  }
  __syncthreads();
  if (a.want_rows) gp_copy_row_record(acc, a.row_rec, split, a.R, i0, D);
  if (a.want_scalars) {
    double* sc = a.sc_rec + (int64_t)blockIdx.x * gpp_record_doubles(D);
    const double v0 = block_sum_f64_waves(s_var, red, GPK_WAVES);
    const double v1 = block_sum_f64_waves(s_ls, red, GPK_WAVES);
    if (tid == 0) sc[0] = v0, sc[1] = v1;
    for (int k = tid; k < D; k += GPK_THREADS) {
      sc[GPP_SCALARS + k] = gp_fold_waves(ls_acc, k, D);
      sc[GPP_SCALARS + D + k] = gp_fold_waves(p_acc, k, D);
    }
  }
}

// records -> gradients, float64 sums in a fixed order.  Blocks [0, row_fin_blocks): g_rows[i, k] = -(2 pi variance /
// (p_k l_k^2)) sum_split rec[split, i, k].  Then one block per reduced output: lengthscale (n_ls of them), period
// (n_p), variance.
template <typename T>
struct GppFinArgs {
  const double *row_rec, *sc_rec;
  const T *ls, *period, *variance;
  int n_ls, n_p, D, splits;
  int64_t R, workgroups, row_fin_blocks;
  T *g_rows, *g_ls, *g_period, *g_var;
};

template <typename T>
__global__ __launch_bounds__(GPK_THREADS) void gp_periodic_fin_kernel(const GppFinArgs<T> a) {
  __shared__ double red[GPK_WAVES];
  const double var = (double)a.variance[0];
  const auto l_of = [&](int k) { return (double)a.ls[a.n_ls == 1 ? 0 : k]; };
  const auto p_of = [&](int k) { return (double)a.period[a.n_p == 1 ? 0 : k]; };
  if ((int64_t)blockIdx.x < a.row_fin_blocks) {
    const int64_t e = (int64_t)blockIdx.x * GPK_THREADS + threadIdx.x, total = a.R * a.D;
    if (e >= total) return;
    const int k = (int)(e % a.D);
    const double s = gp_sum_splits(a.row_rec, a.splits, total, e);
    a.g_rows[e] = (T)(-2.0 * 3.14159265358979323846 * var / (p_of(k) * l_of(k) * l_of(k)) * s);
    return;
  }
  const int which = (int)((int64_t)blockIdx.x - a.row_fin_blocks);      // lengthscale, then period, then variance
  const int rec = gpp_record_doubles(a.D);
  T* out;
  double s = 0.0;
  if (which < a.n_ls) {
    out = a.g_ls ? a.g_ls + which : nullptr;
    if (out == nullptr) return;                   // (uniform over the block)
    const int slot = a.n_ls == 1 ? 1 : GPP_SCALARS + which;
    const double l = l_of(which);
    for (int64_t w = threadIdx.x; w < a.workgroups; w += GPK_THREADS) s += a.sc_rec[w * rec + slot];
    s *= a.n_ls == 1 ? 4.0 * var / l : 4.0 * var / (l * l * l);
  } else if (which < a.n_ls + a.n_p) {
    const int first = which - a.n_ls;
    out = a.g_period ? a.g_period + first : nullptr;
    if (out == nullptr) return;
    const int last = a.n_p == 1 ? a.D : first + 1;      // a scalar period takes the sum over the features as well
    for (int64_t w = threadIdx.x; w < a.workgroups; w += GPK_THREADS)
      for (int k = first; k < last; ++k)
        s += 2.0 * var / (p_of(k) * l_of(k) * l_of(k)) * a.sc_rec[w * rec + GPP_SCALARS + a.D + k];
  } else {
    out = a.g_var;
    if (out == nullptr) return;
    for (int64_t w = threadIdx.x; w < a.workgroups; w += GPK_THREADS) s += a.sc_rec[w * rec];
  }
  s = block_sum_f64_waves(s, red, GPK_WAVES);
  if (threadIdx.x == 0) *out = (T)s;
}

// ---- launchers -----------------------------------------------------------------------------------------------------
template <typename T>
static int gpp_fwd_launch(const void* x, const void* z, const void* ls, int n_ls, const void* period, int n_p,
                          const void* variance, void* K, int64_t N, int64_t M, int D, hipStream_t st) {
  const int64_t col_tiles = gpk_tiles(M), tiles = gpk_tiles(N) * col_tiles;
  PA_REQUIRE(tiles <= GPK_MAX_WORKGROUPS, "pa_gp_periodic_fwd: %lld tiles over the grid limit", (long long)tiles);
  return gp_launch("gp_periodic_fwd_kernel", gp_periodic_fwd_kernel<T>, tiles, GPK_THREADS, gpp_fwd_lds_bytes(D, sizeof(T)), st,
                   (const T*)x, (const T*)(z ? z : x), (const T*)ls, n_ls, (const T*)period, n_p, (const T*)variance, (T*)K,
                   N, M, D, col_tiles);
}

template <typename T>
struct GppParams {
  const T *ls, *period, *variance;
  int n_ls, n_p;
  T *g_ls, *g_period, *g_var;
};

template <typename T>
static int gpp_bwd_side(const GpkLaunchPlan& pl, const T* xr, const T* xc, const T* G, int64_t g_sr, int64_t g_sc, bool sym,
                        const GppParams<T>& pr, bool scalars, double* ws, T* g_rows, hipStream_t st) {
  PA_REQUIRE(pl.workgroups <= GPK_MAX_WORKGROUPS, "pa_gp_periodic_bwd: %lld workgroups over the grid limit",
             (long long)pl.workgroups);
  GppBwdArgs<T> a;
  a.xr = xr, a.xc = xc, a.G = G, a.g_sr = g_sr, a.g_sc = g_sc;
  a.ls = pr.ls, a.period = pr.period, a.n_ls = pr.n_ls, a.n_p = pr.n_p, a.D = pl.D, a.splits = pl.splits;
  a.want_rows = pl.row_records ? 1 : 0, a.want_scalars = scalars ? 1 : 0;
  a.want_ls = scalars && pr.g_ls ? 1 : 0, a.want_period = scalars && pr.g_period ? 1 : 0;
  a.R = pl.rows, a.C = pl.cols, a.tiles_per_split = pl.tiles_per_split, a.col_tiles = pl.col_tiles;
  a.row_rec = ws, a.sc_rec = ws + pl.row_doubles;
  int rc = gp_launch("gp_periodic_bwd_kernel", sym ? gp_periodic_bwd_kernel<T, true> : gp_periodic_bwd_kernel<T, false>,
                     pl.workgroups, GPK_THREADS, gpp_bwd_lds_bytes(pl.D, sizeof(T)), st, a);
  if (rc != PA_OK) return rc;
  GppFinArgs<T> f;
  f.row_rec = a.row_rec, f.sc_rec = a.sc_rec, f.ls = pr.ls, f.period = pr.period, f.variance = pr.variance;
  f.n_ls = pr.n_ls, f.n_p = pr.n_p, f.D = pl.D, f.splits = pl.splits, f.R = pl.rows, f.workgroups = pl.workgroups;
  f.row_fin_blocks = pl.row_records ? (pl.rows * pl.D + GPK_THREADS - 1) / GPK_THREADS : 0;
  f.g_rows = g_rows, f.g_ls = pr.g_ls, f.g_period = pr.g_period, f.g_var = pr.g_var;
  const int64_t blocks = f.row_fin_blocks + (scalars ? pr.n_ls + pr.n_p + 1 : 0);
  if (blocks == 0) return PA_OK;
  PA_REQUIRE(blocks <= GPK_MAX_WORKGROUPS, "pa_gp_periodic_bwd: finalize grid of %lld blocks", (long long)blocks);
  return gp_launch("gp_periodic_fin_kernel", gp_periodic_fin_kernel<T>, blocks, GPK_THREADS, 0, st, f);
}

template <typename T>
static int gpp_bwd_launch(const GpkCallPlan& cp, const void* x, const void* z, const GppParams<T>& pr, const void* G,
                          int64_t M, void* gx, void* gz, void* workspace, hipStream_t st) {
  return gp_bwd_two_sided<T>(cp, x, z, M, gx, gz, pr.g_ls || pr.g_period || pr.g_var, workspace,
                             [&](const GpkLaunchPlan& pl, const T* xr, const T* xc, int64_t g_sr, int64_t g_sc, bool sym,
                                 bool scalars, double* ws, T* g_rows) {
                               return gpp_bwd_side<T>(pl, xr, xc, (const T*)G, g_sr, g_sc, sym, pr, scalars, ws, g_rows, st);
                             });
}

static int gpp_check(const char* who, int dtype, const void* x, const void* z, const void* ls, int n_ls, const void* period,
                     int n_p, const void* variance, int64_t N, int64_t M, int64_t D) {
  PA_REQUIRE(dtype == PA_F32 || dtype == PA_F64, "%s: dtype %d", who, dtype);
  if (!(D >= 1 && D <= GPK_MAX_D))
    return fail(PA_ERR_UNSUPPORTED, "%s: D=%lld outside [1, %d]", who, (long long)D, GPK_MAX_D);
  PA_REQUIRE(gpp_shape_ok(N, M, D, n_ls, n_p), "%s: N=%lld M=%lld D=%lld n_ls=%d n_period=%d", who, (long long)N,
             (long long)M, (long long)D, n_ls, n_p);
  PA_REQUIRE(z != nullptr || N == M, "%s: z = x needs M = N, got N=%lld M=%lld", who, (long long)N, (long long)M);
  PA_REQUIRE(ls != nullptr && period != nullptr && variance != nullptr && (N == 0 || x != nullptr), "%s: null input", who);
  return PA_OK;
}

}  // namespace pa

extern "C" {

int pa_gp_periodic_fwd(int dtype, const void* x, const void* z, const void* lengthscale, int n_ls, const void* period,
                       int n_period, const void* variance, void* K, int64_t N, int64_t M, int64_t D, pa_stream_t stream) {
  int rc = pa::gpp_check("pa_gp_periodic_fwd", dtype, x, z, lengthscale, n_ls, period, n_period, variance, N, M, D);
  if (rc != PA_OK) return rc;
  if (N == 0 || M == 0) return PA_OK;
  PA_REQUIRE(K != nullptr, "pa_gp_periodic_fwd: null output");
  hipStream_t st = pa::as_stream(stream);
  if (dtype == PA_F32)
    return pa::gpp_fwd_launch<float>(x, z, lengthscale, n_ls, period, n_period, variance, K, N, M, (int)D, st);
  return pa::gpp_fwd_launch<double>(x, z, lengthscale, n_ls, period, n_period, variance, K, N, M, (int)D, st);
}

size_t pa_gp_periodic_bwd_workspace(int64_t N, int64_t M, int64_t D, int z_null, int want_gx, int want_gz,
                                    int forced_splits) {
  if (!pa::gpp_shape_ok(N, M, D, 1, 1) || N == 0 || M == 0) return 0;
  return pa::gpk_call_plan(N, M, (int)D, pa::gpp_record_doubles((int)D), z_null != 0, want_gx != 0, want_gz != 0,
                           pa::cu_count(), forced_splits)
      .bytes;
}

int pa_gp_periodic_bwd(int dtype, const void* x, const void* z, const void* lengthscale, int n_ls, const void* period,
                       int n_period, const void* variance, const void* G, int64_t N, int64_t M, int64_t D, void* gx,
                       void* gz, void* g_lengthscale, void* g_period, void* g_variance, int forced_splits,
                       void* workspace, size_t workspace_bytes, pa_stream_t stream) {
  int rc = pa::gpp_check("pa_gp_periodic_bwd", dtype, x, z, lengthscale, n_ls, period, n_period, variance, N, M, D);
  if (rc != PA_OK) return rc;
  bool launch;
  rc = pa::gp_bwd_preamble("pa_gp_periodic_bwd", z, gz, forced_splits, gx || gz || g_lengthscale || g_period || g_variance,
                           N, M, G, &launch);
  if (rc != PA_OK || !launch) return rc;
  const pa::GpkCallPlan cp = pa::gpk_call_plan(N, M, (int)D, pa::gpp_record_doubles((int)D), z == nullptr, gx != nullptr,
                                               gz != nullptr, pa::cu_count(), forced_splits);
  rc = pa::gp_workspace_check("pa_gp_periodic_bwd", workspace, workspace_bytes, cp.bytes);
  if (rc != PA_OK) return rc;
  hipStream_t st = pa::as_stream(stream);
  if (dtype == PA_F32) {
    const pa::GppParams<float> pr = {(const float*)lengthscale, (const float*)period, (const float*)variance, n_ls,
                                     n_period,                  (float*)g_lengthscale, (float*)g_period, (float*)g_variance};
    return pa::gpp_bwd_launch<float>(cp, x, z, pr, G, M, gx, gz, workspace, st);
  }
  const pa::GppParams<double> pr = {(const double*)lengthscale, (const double*)period, (const double*)variance, n_ls,
                                    n_period,                   (double*)g_lengthscale, (double*)g_period, (double*)g_variance};
  return pa::gpp_bwd_launch<double>(cp, x, z, pr, G, M, gx, gz, workspace, st);
}

}  // extern "C"
