// gp_compose.hip -- a whole sum of products of covariance kernels in ONE launch:
//   K[i, j] = bias + sum_t coef_t prod_{f in term t} v_f phi_f(x_i, z_j),
// phi_f one of the five stationary families (gp_families.h) or the periodic kernel (gp_periodic_dev.h), each on its own
// columns of the inputs, f32 and f64.  Up to 6 terms, 3 factors per term, 8 factors in all, a union of U <= 64 columns
// (gp_compose_plan.h).  The forward writes K once; the backward is one pass over the incoming gradient G per side that
// wants a gradient, from which EVERY factor's parameter gradients and the input gradient come, plus a fixed-order
// finalize.  No float atomics: bit-reproducible from call to call.
//
// Path replaced: Sum.forward / Product.forward evaluate every leaf in a launch of its own and combine the [N, M]
// matrices with torch operators; for A * B + C that is three launches and two element-wise passes forward, two [N, M]
// factors kept alive by autograd, and three backward launches that each read an [N, M] gradient of their own.
//
// The descriptor (pa_gp_compose_spec, 592 bytes) travels BY VALUE in the kernel arguments: kinds, sizes, one byte per
// column, coefficients, and the device pointers of the parameters, which the kernels read themselves.  Nothing is
// copied to the device per call.  The factor kind is a switch that is uniform over the workgroup, a scalar branch:
// one instantiation per dtype.
//
// Staging.  The host slices the union of the factors' columns once; the 64-row tiles of x and z, U wide, are staged
// once (gp_tile.h, odd row stride) and every factor reads its own columns of the same tile through its column list.
// Beside the tiles, per factor and feature in float64: 1 / l_k, or 1 / p_k and 1 / l_k^2.
//
// Per-factor arithmetic is the leaf kernels': differences first, unscaled, in float64; r2 or the periodic exponent
// accumulated in float64 for both dtypes; the exponential through the hi / lo split (gp_exp_of); u - rint(u) and
// gpp_sinpi_reduced for the periodic exponent; the sqrt(r2 + 1e-12) guard inside the evaluators.
//
// Forward.  64 x 64 tiles, 256 threads, 4 x 4 entries per lane.  Term by term: the running product of the term's
// factors starts at coef_t, each factor multiplies v_f phi_f in, the term is added to the entry's sum.
//
// Backward.  Grid: row blocks x column splits (gpk_launch_plan).  Registers decide the shape of the tile loop: all
// factors' values at once do not fit, so a tile is walked TERM BY TERM.  Of a term with more than one factor, pass 1
// forms the (at most 3 x 16) values v_f phi_f in the tensor's dtype.  Pass 2 takes the factors one at a time: it forms
// the factor's r2 or exponent again in float64 (as the leaf kernels recompute d in their sweep), and its weight
//   w_ij = G_ij coef_t prod_{f' != f} v_f' phi_f'
// by MULTIPLYING the others -- never dividing the term by phi_f, which underflows to zero.  With w in the place of G
// the leaf kernels' closed forms follow unchanged (gp_kernel.hip, gp_periodic.hip): the sums for the variance, the
// scale_mixture and a scalar lengthscale per tile, then one sweep over the factor's features for the row gradient and
// the ARD lengthscale and period sums.  A single-factor term skips pass 1.
//   The row gradient of all factors goes to ONE float64 array [64, U] in LDS: per feature the 16 lanes of a row add
// theirs on DPP and lane tx = 0, the only writer of that row, adds the sum times the factor's scale (2 v / l_k, or
// -2 pi v / (p_k l_k^2)) -- the scale differs per factor, so it is applied before the add and the finalize only sums
// the splits.  Parameter sums go wave by wave to per-wave float64 accumulators (one writer per entry) and from there
// to one scalar record per workgroup, laid out factor by factor; the finalize adds the records in a fixed order in
// float64, applies the leaf kernels' factors and rounds once.  gZ is a second launch with the roles exchanged; with
// z = x (null) one launch gives x both roles through the weight (G_ij + G_ji).
//
// gfx950 cross-compile (hipcc -O3, -Rpass-analysis=kernel-resource-usage): no instantiation uses scratch; LDS is
// dynamic; the register table is in the README entry "Gaussian processes".
#include "gp_compose_plan.h"
#include "gp_families.h"
#include "gp_host.h"
#include "gp_periodic_dev.h"

namespace pa {

typedef pa_gp_compose_spec GpxSpec;

// the periodic factor as a family of its exponent e = sum_k s^2 / l_k^2: f = exp(-2 e); ``df`` is f itself, the
// weight W = G K of gp_periodic.hip
template <typename T>
struct GpxPeriodic {
  __device__ __forceinline__ static void eval(double e, T, T& f, T& df, T& da) {
    f = gp_exp_of<T>(-2.0 * e);
    df = f;
    da = T(0);
  }
};

// body(family) under a switch that is uniform over the workgroup
template <typename T, typename F>
__device__ __forceinline__ void gpx_with_family(int kind, F&& body) {
  switch (kind) {
    case PA_GP_RBF: body(GpRbf<T>()); break;
    case PA_GP_RATIONAL_QUADRATIC: body(GpRq<T>()); break;
    case PA_GP_EXPONENTIAL: body(GpExponential<T>()); break;
    case PA_GP_MATERN32: body(GpMatern32<T>()); break;
    case PA_GP_MATERN52: body(GpMatern52<T>()); break;
    default: body(GpxPeriodic<T>()); break;
  }
}

// per factor and feature, in float64: 1 / l_k, or 1 / p_k and 1 / l_k^2, at par[2 col0 + k] and par[2 col0 + D + k]
template <typename T>
__device__ __forceinline__ void gpx_stage_parameters(const GpxSpec& s, double* par) {
  for (int f = 0; f < s.n_factors; ++f) {
    const pa_gp_factor& fa = s.factor[f];
    const T* ls = (const T*)fa.lengthscale;
    const T* period = (const T*)fa.aux;
    const int D = fa.D;
    double* pa0 = par + 2 * fa.col0;
    for (int k = threadIdx.x; k < D; k += GPK_THREADS) {
      const double l = (double)ls[fa.n_ls == 1 ? 0 : k];
      if (fa.kind == PA_GP_PERIODIC) {
        pa0[k] = 1.0 / (double)period[fa.n_aux == 1 ? 0 : k];
        pa0[D + k] = 1.0 / (l * l);
      } else {
        pa0[k] = 1.0 / l;
        pa0[D + k] = 0.0;
      }
    }
  }
}

// r2 (gp_kernel.hip's gp_r2_tile) or the periodic exponent sum_k s^2 / l_k^2 (gp_periodic.hip's gpp_exponent_tile) of
// the thread's 4 x 4 entries over the factor's columns, in float64 for both dtypes
template <typename T>
__device__ __forceinline__ void gpx_distance_tile(const T* xs, const T* zs, const uint8_t* cols, const double* pa0, int D,
                                                  bool periodic, int stride, int ty, int tx, double (&acc)[4][4]) {
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[r][c] = 0.0;
  for (int k = 0; k < D; ++k) {
    const int col = cols[k];
    const double ia = pa0[k], il2 = pa0[D + k];
    double xv[4], zv[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) xv[r] = (double)xs[(4 * ty + r) * stride + col];
#pragma unroll
    for (int c = 0; c < 4; ++c) zv[c] = (double)zs[(4 * tx + c) * stride + col];
    if (!periodic) {
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const double d = (xv[r] - zv[c]) * ia;
          acc[r][c] = fma(d, d, acc[r][c]);
        }
    } else {
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const double u = (xv[r] - zv[c]) * ia;
          const double sn = gpp_sinpi_reduced<T>(u - rint(u));
          acc[r][c] = fma(sn * sn, il2, acc[r][c]);
        }
    }
  }
}

// v_f phi_f of the thread's 4 x 4 entries times ``into``
template <typename T>
__device__ __forceinline__ void gpx_multiply_factor(const GpxSpec& s, int f, const T* xs, const T* zs, const double* par,
                                                    int stride, int ty, int tx, T (&into)[4][4]) {
  const pa_gp_factor& fa = s.factor[f];
  double e[4][4];
  gpx_distance_tile(xs, zs, s.cols + fa.col0, par + 2 * fa.col0, (int)fa.D, fa.kind == PA_GP_PERIODIC, stride, ty, tx, e);
  const T var = ((const T*)fa.variance)[0];
  const T alpha = fa.kind == PA_GP_RATIONAL_QUADRATIC ? ((const T*)fa.aux)[0] : T(1);
  gpx_with_family<T>(fa.kind, [&](auto fam) {
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        T fv, df, da;
        decltype(fam)::eval(e[r][c], alpha, fv, df, da);
        into[r][c] *= var * fv;
      }
  });
}

// ---- forward ---------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(GPK_THREADS) void gp_compose_fwd_kernel(const GpxSpec s, const T* __restrict__ x,
                                                                     const T* __restrict__ z, T* __restrict__ K, int64_t N,
                                                                     int64_t M, int64_t col_tiles) {
  extern __shared__ __attribute__((aligned(16))) unsigned char gp_lds[];
  const int U = s.U, stride = gpk_lds_stride(U);
  T* xs = reinterpret_cast<T*>(gp_lds);
  T* zs = xs + GPK_TILE * stride;
  double* par = reinterpret_cast<double*>(gp_lds + gpk_lds_head_bytes(U, sizeof(T)));      // [2 sum_d]
  const int64_t rt = (int64_t)blockIdx.x / col_tiles, ct = (int64_t)blockIdx.x - rt * col_tiles;
  const int64_t i0 = rt * GPK_TILE, j0 = ct * GPK_TILE;
  gp_stage(x, i0, N, U, stride, xs);
  gp_stage(z, j0, M, U, stride, zs);
  gpx_stage_parameters<T>(s, par);
  __syncthreads();
  const int ty = threadIdx.x >> 4, tx = threadIdx.x & 15;
  T sum[4][4];
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int c = 0; c < 4; ++c) sum[r][c] = (T)s.bias;
  int f = 0;
  for (int t = 0; t < s.n_terms; ++t) {
    T prod[4][4];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int c = 0; c < 4; ++c) prod[r][c] = (T)s.coef[t];
    for (int fi = 0; fi < s.term_count[t]; ++fi, ++f) gpx_multiply_factor<T>(s, f, xs, zs, par, stride, ty, tx, prod);
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int c = 0; c < 4; ++c) sum[r][c] += prod[r][c];
  }
  const int64_t j = j0 + 4 * tx;
  const bool vec = (M & 3) == 0 && j + 3 < M && (uintptr_t)K % sizeof(Vec4<T>) == 0;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int64_t i = i0 + 4 * ty + r;
    if (i >= N) continue;
    Vec4<T> out;
#pragma unroll
    for (int c = 0; c < 4; ++c) out.v[c] = sum[r][c];
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
struct GpxBwdArgs {
  const T *xr, *xc;            // the points that get a gradient [R, U], the points that are walked [C, U]
  const T* G;                  // G(i, j) = G[i * g_sr + j * g_sc], one of the strides is 1
  int64_t g_sr, g_sc;
  int splits, want_rows, want_scalars;
  unsigned want_ls, want_aux;  // bit f: factor f's lengthscale / period gradient is wanted
  int64_t R, C, tiles_per_split, col_tiles;
  double *row_rec, *sc_rec;    // [splits, R, U], [workgroups, gpx_record_doubles]
};

// One factor of one term on one tile: its weight from G and the product of the others, the per-tile scalar sums, the
// sweep over its features.  ``others``: coef_t prod_{f' != f} v_f' phi_f' of the thread's entries.
template <typename T, bool SYM>
__device__ __forceinline__ void gpx_factor_backward(const GpxSpec& s, const GpxBwdArgs<T>& a, int f, const T* xs, const T* zs,
                                                    const double* par, double* acc, double* ls_acc, double* p_acc,
                                                    double* sc_acc, const T (&g)[4][4], const T (&gs)[SYM ? 4 : 1][4],
                                                    const T (&others)[4][4], int stride, int ty, int tx) {
  const pa_gp_factor& fa = s.factor[f];
  const int D = fa.D, U = s.U, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const bool periodic = fa.kind == PA_GP_PERIODIC;
  const uint8_t* cols = s.cols + fa.col0;
  const double* pa0 = par + 2 * fa.col0;
  const T alpha = fa.kind == PA_GP_RATIONAL_QUADRATIC ? ((const T*)fa.aux)[0] : T(1);
  T ws[4][4], wr[SYM ? 4 : 1][4];                  // the weight of the parameter sums, and of the rows when z = x
  T t_var = T(0), t_alpha = T(0), t_ls = T(0);
  {
    double e[4][4];
    gpx_distance_tile(xs, zs, cols, pa0, D, periodic, stride, ty, tx, e);
    gpx_with_family<T>(fa.kind, [&](auto fam) {
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          T fv, df, da;
          decltype(fam)::eval(e[r][c], alpha, fv, df, da);
          const T w = g[r][c] * others[r][c];      // zero outside [R, C]: padded entries weigh nothing
          ws[r][c] = w * df;
          if constexpr (SYM) wr[r][c] = gs[r][c] * others[r][c] * df;
          t_var += w * fv;
          t_alpha += w * da;
          t_ls += ws[r][c] * (T)e[r][c];
        }
    });
  }
  if (a.want_scalars) {
    const double v0 = wave_sum((double)t_var), v1 = wave_sum((double)t_alpha), v2 = wave_sum((double)t_ls);
    if (lane == 0) {
      double* sc = sc_acc + (wave * GPX_MAX_FACTORS + f) * GPX_SCALARS;
      sc[0] += v0, sc[1] += v1, sc[2] += v2;
    }
  }
  const bool ard = a.want_scalars && ((a.want_ls >> f) & 1) && fa.n_ls != 1;
  const bool want_period = a.want_scalars && periodic && ((a.want_aux >> f) & 1);
  if (!(a.want_rows || ard || want_period)) return;
  const double var = (double)((const T*)fa.variance)[0];
  for (int k = 0; k < D; ++k) {
    const int col = cols[k];
    T p[4], ql = T(0), qp = T(0);
    double row_scale;
    if (!periodic) {
      const T il = (T)pa0[k];
      row_scale = 2.0 * var * pa0[k];
      T xv[4], zv[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) xv[r] = xs[(4 * ty + r) * stride + col];
#pragma unroll
      for (int c = 0; c < 4; ++c) zv[c] = zs[(4 * tx + c) * stride + col];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        p[r] = T(0);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const T d = (xv[r] - zv[c]) * il;
          p[r] += (SYM ? wr[SYM ? r : 0][c] : ws[r][c]) * d;
          ql += ws[r][c] * d * d;
        }
      }
    } else {
      const double ip = pa0[k];
      row_scale = -2.0 * 3.14159265358979323846 * var * ip * pa0[D + k];
      double xv[4], zv[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) xv[r] = (double)xs[(4 * ty + r) * stride + col];
#pragma unroll
      for (int c = 0; c < 4; ++c) zv[c] = (double)zs[(4 * tx + c) * stride + col];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        p[r] = T(0);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const double u = (xv[r] - zv[c]) * ip;
          T sn, co;
          gpp_sincospi((T)(u - rint(u)), sn, co);
          const T s2t = T(2) * sn * co;            // sin(2 theta)
          const T w = ws[r][c];
          p[r] += (SYM ? wr[SYM ? r : 0][c] : w) * s2t;
          ql += w * sn * sn;
          qp += w * s2t * (T)(3.14159265358979323846 * u);
        }
      }
    }
    if (a.want_rows) {
#pragma unroll
      for (int r = 0; r < 4; ++r) gp_row_add(p[r], row_scale, acc, (4 * ty + r) * U + col, tx);
    }
    if (ard) gp_wave_add(ql, ls_acc, wave * s.sum_d + fa.col0 + k, lane);
    if (want_period) gp_wave_add(qp, p_acc, wave * s.sum_d + fa.col0 + k, lane);
  }
}

// SYM: z = x, the row gradient's weight carries (G_ij + G_ji)
template <typename T, bool SYM>
__global__ __launch_bounds__(GPK_THREADS) void gp_compose_bwd_kernel(const GpxSpec s, const GpxBwdArgs<T> a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char gp_lds[];
  const int U = s.U, stride = gpk_lds_stride(U), sum_d = s.sum_d;
  T* xs = reinterpret_cast<T*>(gp_lds);
  T* zs = xs + GPK_TILE * stride;
  double* par = reinterpret_cast<double*>(gp_lds + gpk_lds_head_bytes(U, sizeof(T)));      // [2 sum_d]
  double* acc = par + 2 * sum_d;                                                             // [64, U]
  double* ls_acc = acc + GPK_TILE * U;                                                       // [4, sum_d]
  double* p_acc = ls_acc + GPK_WAVES * sum_d;                                                // [4, sum_d]
  double* sc_acc = p_acc + GPK_WAVES * sum_d;                                                // [4, 8, 3]
  const int tid = threadIdx.x, ty = tid >> 4, tx = tid & 15;
  const int64_t rb = (int64_t)blockIdx.x / a.splits;
  const int split = (int)((int64_t)blockIdx.x - rb * a.splits);
  const int64_t i0 = rb * GPK_TILE;
  gp_stage(a.xr, i0, a.R, U, stride, xs);
  gpx_stage_parameters<T>(s, par);
  const int zeros = GPK_TILE * U + 2 * GPK_WAVES * sum_d + GPK_WAVES * GPX_MAX_FACTORS * GPX_SCALARS;
  for (int e = tid; e < zeros; e += GPK_THREADS) acc[e] = 0.0;
  int64_t ct_end = (int64_t)(split + 1) * a.tiles_per_split;
  if (ct_end > a.col_tiles) ct_end = a.col_tiles;
  for (int64_t ct = (int64_t)split * a.tiles_per_split; ct < ct_end; ++ct) {
    const int64_t j0 = ct * GPK_TILE;
    __syncthreads();                               // the previous tile's reads of zs are over
    gp_stage(a.xc, j0, a.C, U, stride, zs);
    __syncthreads();
    T g[4][4], gs[SYM ? 4 : 1][4];
    gp_load_g(a, a.g_sr, a.g_sc, i0, j0, ty, tx, g);
    if constexpr (SYM) {
      gp_load_g(a, a.g_sc, a.g_sr, i0, j0, ty, tx, gs);      // G(j, i)
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) gs[r][c] += g[r][c];
    }
    int f0 = 0;
    for (int t = 0; t < s.n_terms; ++t) {
      const int count = s.term_count[t];
      const T coef = (T)s.coef[t];
      // pass 1 pushes the term's values v_f phi_f in at the front: v0 is the last factor's, ones fill what is unused
      T v0[4][4], v1[4][4], v2[4][4];
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) v0[r][c] = v1[r][c] = v2[r][c] = T(1);
      if (count > 1) {
        for (int fi = 0; fi < count; ++fi) {
#pragma unroll
          for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int c = 0; c < 4; ++c) v2[r][c] = v1[r][c], v1[r][c] = v0[r][c], v0[r][c] = T(1);
          gpx_multiply_factor<T>(s, f0 + fi, xs, zs, par, stride, ty, tx, v0);
        }
      }
      // pass 2 takes the factors from the last to the first: the current one's value sits in v0, the OTHERS are v1 and
      // v2, and a rotation brings the next one to the front.  Every index is static, so the values stay in registers,
      // and there is one copy of the factor's code.
      for (int fi = count - 1; fi >= 0; --fi) {
        T others[4][4];
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            others[r][c] = coef * v1[r][c] * v2[r][c];
            const T front = v0[r][c];
            v0[r][c] = v1[r][c], v1[r][c] = v2[r][c], v2[r][c] = front;
          }
        gpx_factor_backward<T, SYM>(s, a, f0 + fi, xs, zs, par, acc, ls_acc, p_acc, sc_acc, g, gs, others, stride, ty, tx);
      }
      f0 += count;
    }
  }
  __syncthreads();
  if (a.want_rows) gp_copy_row_record(acc, a.row_rec, split, a.R, i0, U);
  if (a.want_scalars) {
    double* sc = a.sc_rec + (int64_t)blockIdx.x * gpx_record_doubles(s.n_factors, sum_d);
    for (int f = 0; f < s.n_factors; ++f) {
      const pa_gp_factor& fa = s.factor[f];
      const int D = fa.D;
      double* out = sc + gpx_record_base(f, fa.col0);
      for (int e = tid; e < GPX_SCALARS + 2 * D; e += GPK_THREADS) {
        const double* src;
        int step;
        if (e < GPX_SCALARS) src = sc_acc + f * GPX_SCALARS + e, step = GPX_MAX_FACTORS * GPX_SCALARS;
        else if (e < GPX_SCALARS + D) src = ls_acc + fa.col0 + (e - GPX_SCALARS), step = sum_d;
        else src = p_acc + fa.col0 + (e - GPX_SCALARS - D), step = sum_d;
        out[e] = gp_fold_waves(src, 0, step);
      }
    }
  }
}

// records -> gradients, float64 sums in a fixed order.  Blocks [0, row_fin_blocks): g_rows[i, k] = sum_split rec[split,
// i, k] (the factors' scales are in the records).  Then one block per reduced output, factor by factor: variance,
// scale_mixture, lengthscale (n_ls of them), period (n_aux, Periodic only).
template <typename T>
struct GpxFinArgs {
  const double *row_rec, *sc_rec;
  int splits;
  int64_t R, workgroups, row_fin_blocks;
  T* g_rows;
  pa_gp_compose_grads g;
};

GPK_HD inline int gpx_fin_outputs(const pa_gp_factor& fa) {
  return 2 + fa.n_ls + (fa.kind == PA_GP_PERIODIC ? fa.n_aux : 0);
}

template <typename T>
__global__ __launch_bounds__(GPK_THREADS) void gp_compose_fin_kernel(const GpxSpec s, const GpxFinArgs<T> a) {
  __shared__ double red[GPK_WAVES];
  if ((int64_t)blockIdx.x < a.row_fin_blocks) {
    const int64_t e = (int64_t)blockIdx.x * GPK_THREADS + threadIdx.x, total = a.R * s.U;
    if (e >= total) return;
    a.g_rows[e] = (T)gp_sum_splits(a.row_rec, a.splits, total, e);
    return;
  }
  int which = (int)((int64_t)blockIdx.x - a.row_fin_blocks), f = 0;
  while (f < s.n_factors - 1 && which >= gpx_fin_outputs(s.factor[f])) which -= gpx_fin_outputs(s.factor[f]), ++f;
  const pa_gp_factor& fa = s.factor[f];
  const int D = fa.D, rec = gpx_record_doubles(s.n_factors, s.sum_d), base = gpx_record_base(f, fa.col0);
  const bool periodic = fa.kind == PA_GP_PERIODIC;
  const T *ls = (const T*)fa.lengthscale, *period = (const T*)fa.aux;
  const double var = (double)((const T*)fa.variance)[0];
  const auto l_of = [&](int k) { return (double)ls[fa.n_ls == 1 ? 0 : k]; };
  T* out;
  double sum = 0.0;
  if (which < 2 + fa.n_ls) {
    int slot;
    double scale;
    if (which == 0) {
      out = (T*)a.g.g_variance[f], slot = 0, scale = 1.0;
    } else if (which == 1) {
      out = fa.kind == PA_GP_RATIONAL_QUADRATIC ? (T*)a.g.g_aux[f] : nullptr, slot = 1, scale = var;
    } else {
      const int j = which - 2;
      const double l = l_of(j);
      out = a.g.g_lengthscale[f] ? (T*)a.g.g_lengthscale[f] + j : nullptr;
      slot = fa.n_ls == 1 ? 2 : GPX_SCALARS + j;
      if (periodic) scale = fa.n_ls == 1 ? 4.0 * var / l : 4.0 * var / (l * l * l);
      else scale = -2.0 * var / l;
    }
    if (out == nullptr) return;                   // (uniform over the block)
    for (int64_t w = threadIdx.x; w < a.workgroups; w += GPK_THREADS) sum += a.sc_rec[w * rec + base + slot];
    sum *= scale;
  } else {
    const int first = which - 2 - fa.n_ls;
    out = a.g.g_aux[f] ? (T*)a.g.g_aux[f] + first : nullptr;
    if (out == nullptr) return;
    const int last = fa.n_aux == 1 ? D : first + 1;      // a scalar period takes the sum over the features as well
    for (int64_t w = threadIdx.x; w < a.workgroups; w += GPK_THREADS)
      for (int k = first; k < last; ++k)
        sum += 2.0 * var / ((double)period[fa.n_aux == 1 ? 0 : k] * l_of(k) * l_of(k)) *
               a.sc_rec[w * rec + base + GPX_SCALARS + D + k];
  }
  sum = block_sum_f64_waves(sum, red, GPK_WAVES);
  if (threadIdx.x == 0) *out = (T)sum;
}

// ---- launchers -----------------------------------------------------------------------------------------------------
template <typename T>
static int gpx_fwd_launch(const GpxSpec& s, const void* x, const void* z, void* K, int64_t N, int64_t M, hipStream_t st) {
  const int64_t col_tiles = gpk_tiles(M), tiles = gpk_tiles(N) * col_tiles;
  PA_REQUIRE(tiles <= GPK_MAX_WORKGROUPS, "pa_gp_compose_fwd: %lld tiles over the grid limit", (long long)tiles);
  return gp_launch("gp_compose_fwd_kernel", gp_compose_fwd_kernel<T>, tiles, GPK_THREADS,
                   gpx_fwd_lds_bytes(s.U, s.sum_d, sizeof(T)), st, s, (const T*)x, (const T*)(z ? z : x), (T*)K, N, M, col_tiles);
}

template <typename T>
static int gpx_bwd_side(const GpxSpec& s, const GpkLaunchPlan& pl, const T* xr, const T* xc, const T* G, int64_t g_sr,
                        int64_t g_sc, bool sym, const pa_gp_compose_grads& gr, bool scalars, double* ws, T* g_rows,
                        hipStream_t st) {
  PA_REQUIRE(pl.workgroups <= GPK_MAX_WORKGROUPS, "pa_gp_compose_bwd: %lld workgroups over the grid limit",
             (long long)pl.workgroups);
  GpxBwdArgs<T> a;
  a.xr = xr, a.xc = xc, a.G = G, a.g_sr = g_sr, a.g_sc = g_sc, a.splits = pl.splits;
  a.want_rows = pl.row_records ? 1 : 0, a.want_scalars = scalars ? 1 : 0, a.want_ls = 0, a.want_aux = 0;
  int fin_outputs = 0;
  for (int f = 0; f < s.n_factors; ++f) {
    if (gr.g_lengthscale[f]) a.want_ls |= 1u << f;
    if (gr.g_aux[f]) a.want_aux |= 1u << f;
    fin_outputs += gpx_fin_outputs(s.factor[f]);
  }
  a.R = pl.rows, a.C = pl.cols, a.tiles_per_split = pl.tiles_per_split, a.col_tiles = pl.col_tiles;
  a.row_rec = ws, a.sc_rec = ws + pl.row_doubles;
  int rc = gp_launch("gp_compose_bwd_kernel", sym ? gp_compose_bwd_kernel<T, true> : gp_compose_bwd_kernel<T, false>,
                     pl.workgroups, GPK_THREADS, gpx_bwd_lds_bytes(s.U, s.sum_d, sizeof(T)), st, s, a);
  if (rc != PA_OK) return rc;
  GpxFinArgs<T> f;
  f.row_rec = a.row_rec, f.sc_rec = a.sc_rec, f.splits = pl.splits, f.R = pl.rows, f.workgroups = pl.workgroups;
  f.row_fin_blocks = pl.row_records ? (pl.rows * s.U + GPK_THREADS - 1) / GPK_THREADS : 0;
  f.g_rows = g_rows, f.g = gr;
  const int64_t blocks = f.row_fin_blocks + (scalars ? fin_outputs : 0);
  if (blocks == 0) return PA_OK;
  PA_REQUIRE(blocks <= GPK_MAX_WORKGROUPS, "pa_gp_compose_bwd: finalize grid of %lld blocks", (long long)blocks);
  return gp_launch("gp_compose_fin_kernel", gp_compose_fin_kernel<T>, blocks, GPK_THREADS, 0, st, s, f);
}

template <typename T>
static int gpx_bwd_launch(const GpxSpec& s, const GpkCallPlan& cp, const void* x, const void* z, const void* G, int64_t M,
                          void* gx, void* gz, const pa_gp_compose_grads& gr, bool any_scalar, void* workspace,
                          hipStream_t st) {
  return gp_bwd_two_sided<T>(cp, x, z, M, gx, gz, any_scalar, workspace,
                             [&](const GpkLaunchPlan& pl, const T* xr, const T* xc, int64_t g_sr, int64_t g_sc, bool sym,
                                 bool scalars, double* ws, T* g_rows) {
                               return gpx_bwd_side<T>(s, pl, xr, xc, (const T*)G, g_sr, g_sc, sym, gr, scalars, ws, g_rows, st);
                             });
}

static int gpx_check(const char* who, int dtype, const pa_gp_compose_spec* spec, const void* x, const void* z, int64_t N,
                     int64_t M) {
  PA_REQUIRE(dtype == PA_F32 || dtype == PA_F64, "%s: dtype %d", who, dtype);
  PA_REQUIRE(spec != nullptr, "%s: null descriptor", who);
  if (!gpx_supported(*spec, dtype == PA_F32 ? 4 : 8))
    return fail(PA_ERR_UNSUPPORTED, "%s: a descriptor of %d terms, %d factors, U=%d, sum D=%d outside the caps", who,
                spec->n_terms, spec->n_factors, spec->U, spec->sum_d);
  PA_REQUIRE(N >= 0 && M >= 0 && N < GPK_MAX_POINTS && M < GPK_MAX_POINTS, "%s: N=%lld M=%lld", who, (long long)N,
             (long long)M);
  PA_REQUIRE(z != nullptr || N == M, "%s: z = x needs M = N, got N=%lld M=%lld", who, (long long)N, (long long)M);
  PA_REQUIRE(N == 0 || x != nullptr, "%s: null input", who);
  for (int f = 0; f < spec->n_factors; ++f) {
    const pa_gp_factor& fa = spec->factor[f];
    PA_REQUIRE(fa.variance != nullptr && fa.lengthscale != nullptr && (fa.n_aux == 0) == (fa.aux == nullptr),
               "%s: factor %d: null parameter, or an aux that its kind %d does not take", who, f, (int)fa.kind);
  }
  return PA_OK;
}

}  // namespace pa

extern "C" {

int pa_gp_compose_fwd(int dtype, const pa_gp_compose_spec* spec, const void* x, const void* z, void* K, int64_t N,
                      int64_t M, pa_stream_t stream) {
  int rc = pa::gpx_check("pa_gp_compose_fwd", dtype, spec, x, z, N, M);
  if (rc != PA_OK) return rc;
  if (N == 0 || M == 0) return PA_OK;
  PA_REQUIRE(K != nullptr, "pa_gp_compose_fwd: null output");
  hipStream_t st = pa::as_stream(stream);
  if (dtype == PA_F32) return pa::gpx_fwd_launch<float>(*spec, x, z, K, N, M, st);
  return pa::gpx_fwd_launch<double>(*spec, x, z, K, N, M, st);
}

size_t pa_gp_compose_bwd_workspace(const pa_gp_compose_spec* spec, int64_t N, int64_t M, int z_null, int want_gx,
                                   int want_gz, int forced_splits) {
  if (spec == nullptr || !pa::gpx_spec_ok(*spec) || N <= 0 || M <= 0 || N >= pa::GPK_MAX_POINTS || M >= pa::GPK_MAX_POINTS)
    return 0;
  return pa::gpk_call_plan(N, M, spec->U, pa::gpx_record_doubles(spec->n_factors, spec->sum_d), z_null != 0, want_gx != 0,
                           want_gz != 0, pa::cu_count(), forced_splits)
      .bytes;
}

int pa_gp_compose_bwd(int dtype, const pa_gp_compose_spec* spec, const void* x, const void* z, const void* G, int64_t N,
                      int64_t M, void* gx, void* gz, const pa_gp_compose_grads* grads, int forced_splits,
                      void* workspace, size_t workspace_bytes, pa_stream_t stream) {
  int rc = pa::gpx_check("pa_gp_compose_bwd", dtype, spec, x, z, N, M);
  if (rc != PA_OK) return rc;
  PA_REQUIRE(grads != nullptr, "pa_gp_compose_bwd: null grads");
  bool any_scalar = false;
  for (int f = 0; f < spec->n_factors; ++f) {
    const pa_gp_factor& fa = spec->factor[f];
    PA_REQUIRE(grads->g_aux[f] == nullptr || fa.n_aux != 0, "pa_gp_compose_bwd: g_aux for factor %d of kind %d", f,
               (int)fa.kind);
    any_scalar = any_scalar || grads->g_variance[f] || grads->g_lengthscale[f] || grads->g_aux[f];
  }
  bool launch;
  rc = pa::gp_bwd_preamble("pa_gp_compose_bwd", z, gz, forced_splits, gx || gz || any_scalar, N, M, G, &launch);
  if (rc != PA_OK || !launch) return rc;
  const pa::GpkCallPlan cp =
      pa::gpk_call_plan(N, M, spec->U, pa::gpx_record_doubles(spec->n_factors, spec->sum_d), z == nullptr, gx != nullptr,
                        gz != nullptr, pa::cu_count(), forced_splits);
  rc = pa::gp_workspace_check("pa_gp_compose_bwd", workspace, workspace_bytes, cp.bytes);
  if (rc != PA_OK) return rc;
  hipStream_t st = pa::as_stream(stream);
  if (dtype == PA_F32)
    return pa::gpx_bwd_launch<float>(*spec, cp, x, z, G, M, gx, gz, *grads, any_scalar, workspace, st);
  return pa::gpx_bwd_launch<double>(*spec, cp, x, z, G, M, gx, gz, *grads, any_scalar, workspace, st);
}

}  // extern "C"
