// gp_kernel.hip -- the stationary covariance matrix of a Gaussian-process model and its gradient, by DIRECT
// DIFFERENCES: K[i, j] = variance * f(r2_ij), r2_ij = sum_k ((x_ik - z_jk) / l_k)^2, for the five families RBF,
// RationalQuadratic, Exponential, Matern32, Matern52 (r = sqrt(r2 + 1e-12), the reference's guard), f32 and f64,
// D <= 64.  The forward is ONE launch that writes K once; the backward is one pass over the incoming gradient G per
// side that wants a gradient, plus a fixed-order finalize.  No float atomics: bit-reproducible from call to call.
//
// Reference path replaced: pyro/contrib/gp/kernels/isotropic.py: r2 = X2 - 2 X Z^T + Z2, clamped, then four to eight
// element-wise torch passes over [N, M], doubled and kept alive by autograd.  The expansion cancels in float32 (see
// the README entry); differences do not, so r2 >= 0 needs no clamp here.
//
// Tiles.  A workgroup of 256 threads takes a 64 x 64 tile; thread (ty, tx) = (tid / 16, tid % 16) owns rows 4 ty + r
// and columns 4 tx + c, r, c < 4, in registers.  The x and z rows of the tile are staged in LDS UNSCALED, beside
// 1 / l_k in float64: the difference is formed first and scaled after, d = (x - z) * (1 / l).  (Scaling the points
// first would round x / l at the magnitude of x: with inputs shifted by 1e3 that alone is an error of 3e-5 in d in
// float32, the cancellation this kernel exists to avoid.)  r2 is formed in float64 for both dtypes (gp_r2_tile); the
// gradient pass forms d again in the tensor's dtype, where nothing magnifies its rounding.  The row stride in LDS is
// D | 1, odd, so the 16 columns a wave reads sit in 16 different banks and the 4 rows are broadcasts.  A thread's 4 columns are adjacent: K is stored, and G
// loaded, as one 16- or 32-byte vector per row where M allows it, 256 contiguous bytes per 16 lanes in f32.
// Parameters are read through their device pointers, by the kernels.
//
// Backward.  Nothing of the forward is kept: r2 and f are recomputed from the inputs (a model adds noise to the
// diagonal of K in place before its Cholesky).  With w_ij = G_ij f'(r2_ij):
//   gX_ik = (2 variance / l_k) sum_j w_ij d_ijk        g_l_k = -(2 variance / l_k) sum_ij w_ij d_ijk^2
//   g_variance = sum_ij G_ij f_ij                       g_alpha = variance sum_ij G_ij f_ij (u / (1 + u) - log1p(u))
// (u = r2 / (2 alpha); a scalar lengthscale takes sum_k d^2 = r2, so it needs no per-feature pass.)  The grid is
// row blocks x column splits (gp_kernel_plan.h: the splits fill the device when the rows alone are few); a workgroup
// walks the column tiles of its split.  Per tile and feature a thread forms sum_c w d over its 4 columns, the 16
// lanes of a row add theirs on DPP, and lane tx = 0 adds the result to the row's float64 accumulator in LDS (one
// writer per entry).  At the end the workgroup leaves one record [64, D] in slot ``split`` of the workspace and
// one scalar record {variance, alpha, scalar lengthscale, lengthscale_k}; the finalize kernel adds records in a
// fixed order in float64, applies 2 variance / l_k, and rounds once to the tensor's dtype.  gZ is a second launch of
// the same kernel with the roles of x and z exchanged (G read through transposed strides).  With z = x (null) one
// launch gives x both roles: the weight of the row gradient is (G_ij + G_ji) f', G is read twice.
//
// gfx950 cross-compile (hipcc -O3, -Rpass-analysis=kernel-resource-usage): no instantiation uses scratch; LDS is
// dynamic (gp_kernel_plan.h); forward 62 (f32) / 80 (f64) VGPRs, 8 / 6 waves per SIMD; backward 186-214 (f32, 2
// waves) and 255-256 with up to 100 AGPRs (f64, 2 or 1 waves); the table is in the README entry "Gaussian processes".
#include "common.h"
#include "gp_kernel_plan.h"

namespace pa {

template <typename T>
struct alignas(4 * sizeof(T)) Vec4 {
  T v[4];
};

// ---- the families: f(r2) and f'(r2) = df / d(r2), the guard inside --------------------------------------------------
template <typename T>
__device__ __forceinline__ T gp_exp(T v) {
  if constexpr (sizeof(T) == 4) return expf(v);
  else return exp(v);
}
template <typename T>
__device__ __forceinline__ T gp_sqrt(T v) {
  if constexpr (sizeof(T) == 4) return sqrtf(v);
  else return sqrt(v);
}
template <typename T>
__device__ __forceinline__ T gp_log1p(T v) {
  if constexpr (sizeof(T) == 4) return log1pf(v);
  else return log1p(v);
}

// exp(a) for an argument held in float64.  In float32 the argument is split into its rounded value and the remainder,
// exp(hi + lo) = exp(hi) (1 + lo): rounding a = -r2 / 2 to float32 alone would cost |a| 2^-24 relative (4e-6 at r2 = 130).
template <typename T>
__device__ __forceinline__ T gp_exp_of(double a) {
  if constexpr (sizeof(T) == 8) {
    return exp(a);
  } else {
    const float hi = (float)a, lo = (float)(a - (double)hi);
    return expf(hi) * (1.0f + lo);
  }
}

// eval(r2 in float64, alpha) -> f, df = df / d(r2), da = df / d(alpha)
template <typename T>
struct GpRbf {
  __device__ __forceinline__ static void eval(double r2, T, T& f, T& df, T& da) {
    f = gp_exp_of<T>(-0.5 * r2);
    df = T(-0.5) * f;
    da = T(0);
  }
};
template <typename T>
struct GpRq {
  __device__ __forceinline__ static void eval(double r2d, T alpha, T& f, T& df, T& da) {
    const T u = (T)r2d / (T(2) * alpha), l1 = gp_log1p(u);
    f = gp_exp(-alpha * l1);
    df = T(-0.5) * f / (T(1) + u);
    da = f * (u / (T(1) + u) - l1);
  }
};
template <typename T>
struct GpExponential {
  __device__ __forceinline__ static void eval(double r2, T, T& f, T& df, T& da) {
    const double r = sqrt(r2 + 1e-12);
    f = gp_exp_of<T>(-r);
    df = T(-0.5) * f / (T)r;
    da = T(0);
  }
};
template <typename T>
struct GpMatern32 {
  __device__ __forceinline__ static void eval(double r2, T, T& f, T& df, T& da) {
    const double sr = 1.7320508075688772935 * sqrt(r2 + 1e-12);
    const T e = gp_exp_of<T>(-sr);
    f = (T(1) + (T)sr) * e;
    df = T(-1.5) * e;
    da = T(0);
  }
};
template <typename T>
struct GpMatern52 {
  __device__ __forceinline__ static void eval(double r2, T, T& f, T& df, T& da) {
    const double r = sqrt(r2 + 1e-12), sr = 2.2360679774997896964 * r;
    const T e = gp_exp_of<T>(-sr);
    f = (T(1) + (T)sr + T(5.0 / 3.0) * (T)r2) * e;
    df = e * (T(-5.0 / 6.0) - T(5.0 * 2.2360679774997896964 / 6.0) * (T)(r2 / r));
    da = T(0);
  }
};

// ---- staging: rows [first, first + 64) of p [n, D] into tile [64, stride], zeros past the end ----------------------
template <typename T>
__device__ __forceinline__ void gp_stage(const T* __restrict__ p, int64_t first, int64_t n, int D, int stride, T* tile) {
  const int total = GPK_TILE * D;
  for (int e = threadIdx.x; e < total; e += GPK_THREADS) {
    const int row = e / D, k = e - row * D;
    const int64_t i = first + row;
    tile[row * stride + k] = i < n ? p[i * D + k] : T(0);
  }
}

template <typename T>
__device__ __forceinline__ void gp_inverse_lengthscale(const T* __restrict__ ls, int n_ls, int D, double* inv_l) {
  for (int k = threadIdx.x; k < D; k += GPK_THREADS) inv_l[k] = 1.0 / (double)ls[n_ls == 1 ? 0 : k];
}

// r2 of the thread's 4 x 4 entries, in float64 for both dtypes: the difference, its scaling by 1 / l and the sum over
// the features.  f(r2) = exp(-r2 / 2) magnifies a relative error of r2 by r2 / 2: in float32 the two roundings of
// d = (x - z) / l and a sequential sum of 64 squares are 3e-5 relative in f at r2 = 130, as much as or more than the
// float32 restatement on the CPU carries.  The float32 inputs are exact in float64, so r2 is that of the inputs
// as given, to float64 rounding, and stays in float64 up to the exponential (gp_exp_of).
template <typename T>
__device__ __forceinline__ void gp_r2_tile(const T* xs, const T* zs, const double* inv_l, int D, int stride, int ty,
                                           int tx, double (&acc)[4][4]) {
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[r][c] = 0.0;
  for (int k = 0; k < D; ++k) {
    const double il = inv_l[k];
    double xv[4], zv[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) xv[r] = (double)xs[(4 * ty + r) * stride + k];
#pragma unroll
    for (int c = 0; c < 4; ++c) zv[c] = (double)zs[(4 * tx + c) * stride + k];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const double d = (xv[r] - zv[c]) * il;
        acc[r][c] = fma(d, d, acc[r][c]);
      }
  }
}

// ---- forward ---------------------------------------------------------------------------------------------------------
template <typename T, template <typename> class FAM>
__global__ __launch_bounds__(GPK_THREADS) void gp_kernel_fwd_kernel(const T* __restrict__ x, const T* __restrict__ z,
                                                                    const T* __restrict__ ls, int n_ls,
                                                                    const T* __restrict__ variance,
                                                                    const T* __restrict__ alpha_p, T* __restrict__ K,
                                                                    int64_t N, int64_t M, int D, int64_t col_tiles) {
  extern __shared__ __attribute__((aligned(16))) unsigned char gp_lds[];
  const int stride = gpk_lds_stride(D);
  T* xs = reinterpret_cast<T*>(gp_lds);
  T* zs = xs + GPK_TILE * stride;
  double* inv_l = reinterpret_cast<double*>(gp_lds + gpk_lds_head_bytes(D, sizeof(T)));      // [D]
  const int64_t rt = (int64_t)blockIdx.x / col_tiles, ct = (int64_t)blockIdx.x - rt * col_tiles;
  const int64_t i0 = rt * GPK_TILE, j0 = ct * GPK_TILE;
  gp_stage(x, i0, N, D, stride, xs);
  gp_stage(z, j0, M, D, stride, zs);
  gp_inverse_lengthscale(ls, n_ls, D, inv_l);
  __syncthreads();
  const int ty = threadIdx.x >> 4, tx = threadIdx.x & 15;
  double r2[4][4];
  gp_r2_tile(xs, zs, inv_l, D, stride, ty, tx, r2);
  const T var = variance[0], alpha = alpha_p ? alpha_p[0] : T(1);
  const int64_t j = j0 + 4 * tx;
  const bool vec = (M & 3) == 0 && j + 3 < M && (uintptr_t)K % sizeof(Vec4<T>) == 0;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int64_t i = i0 + 4 * ty + r;
    if (i >= N) continue;
    Vec4<T> out;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      T f, df, da;
      FAM<T>::eval(r2[r][c], alpha, f, df, da);
      out.v[c] = var * f;
    }
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
// sum over the 16 lanes of a DPP row (the lanes that share ty); every lane of the wave must be active
template <typename T>
__device__ __forceinline__ T gp_row16_sum(T v) {
  v += dpp_get<0xB1>(v);
  v += dpp_get<0x4E>(v);
  v += dpp_get<0x141>(v);
  v += dpp_get<0x140>(v);
  return v;
}

template <typename T>
struct GpBwdArgs {
  const T *xr, *xc;            // the points that get a gradient [R, D], the points that are walked [C, D]
  const T* G;                  // G(i, j) = G[i * g_sr + j * g_sc], one of the strides is 1
  int64_t g_sr, g_sc;
  int sym;                     // z = x: the row gradient's weight is (G_ij + G_ji) f'
  const T *ls, *variance, *alpha;
  int n_ls, D, splits;
  int want_rows, want_ls, want_scalars;
  int64_t R, C, tiles_per_split, col_tiles;
  double *row_rec, *sc_rec;    // [splits, R, D], [workgroups, GPK_SCALARS + D]
};

template <typename T>
__device__ __forceinline__ void gp_load_g(const GpBwdArgs<T>& a, int64_t sr, int64_t sc, int64_t i0, int64_t j0, int ty,
                                          int tx, T (&g)[4][4]) {
  // G(i, j) at i * sr + j * sc for the thread's 4 x 4 entries, zero outside [R, C]
  const int64_t i = i0 + 4 * ty, j = j0 + 4 * tx;
  const bool inside = i + 3 < a.R && j + 3 < a.C && (uintptr_t)a.G % sizeof(Vec4<T>) == 0;
  if (sc == 1 && inside && (sr & 3) == 0) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const Vec4<T> v = *reinterpret_cast<const Vec4<T>*>(a.G + (i + r) * sr + j);
#pragma unroll
      for (int c = 0; c < 4; ++c) g[r][c] = v.v[c];
    }
  } else if (sr == 1 && inside && (sc & 3) == 0) {
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const Vec4<T> v = *reinterpret_cast<const Vec4<T>*>(a.G + (j + c) * sc + i);
#pragma unroll
      for (int r = 0; r < 4; ++r) g[r][c] = v.v[r];
    }
  } else {
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int c = 0; c < 4; ++c) g[r][c] = (i + r < a.R && j + c < a.C) ? a.G[(i + r) * sr + (j + c) * sc] : T(0);
  }
}

template <typename T, template <typename> class FAM>
__global__ __launch_bounds__(GPK_THREADS) void gp_kernel_bwd_kernel(const GpBwdArgs<T> a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char gp_lds[];
  __shared__ double red[GPK_THREADS / 64];
  const int D = a.D, stride = gpk_lds_stride(D);
  T* xs = reinterpret_cast<T*>(gp_lds);
  T* zs = xs + GPK_TILE * stride;
  double* inv_l = reinterpret_cast<double*>(gp_lds + gpk_lds_head_bytes(D, sizeof(T)));      // [D]
  double* acc = inv_l + D;                                                                       // [64, D]
  double* ls_acc = acc + GPK_TILE * D;                                                                      // [4, D]
  const int tid = threadIdx.x, ty = tid >> 4, tx = tid & 15, lane = tid & 63, wave = tid >> 6;
  const int64_t rb = (int64_t)blockIdx.x / a.splits;
  const int split = (int)((int64_t)blockIdx.x - rb * a.splits);
  const int64_t i0 = rb * GPK_TILE;
  gp_stage(a.xr, i0, a.R, D, stride, xs);
  gp_inverse_lengthscale(a.ls, a.n_ls, D, inv_l);
  for (int e = tid; e < GPK_TILE * D + (GPK_THREADS / 64) * D; e += GPK_THREADS) acc[e] = 0.0;
  const T alpha = a.alpha ? a.alpha[0] : T(1);
  const bool ard = a.want_ls && a.n_ls != 1;
  double s_var = 0.0, s_alpha = 0.0, s_ls = 0.0;
  int64_t ct_end = (int64_t)(split + 1) * a.tiles_per_split;
  if (ct_end > a.col_tiles) ct_end = a.col_tiles;
  for (int64_t ct = (int64_t)split * a.tiles_per_split; ct < ct_end; ++ct) {
    const int64_t j0 = ct * GPK_TILE;
    __syncthreads();                               // the previous tile's reads of zs are over
    gp_stage(a.xc, j0, a.C, D, stride, zs);
    __syncthreads();
    double r2[4][4];
    T g[4][4], wr[4][4], ws[4][4];
    gp_r2_tile(xs, zs, inv_l, D, stride, ty, tx, r2);
    gp_load_g(a, a.g_sr, a.g_sc, i0, j0, ty, tx, g);
    if (a.sym) gp_load_g(a, a.g_sc, a.g_sr, i0, j0, ty, tx, wr);      // G(j, i)
    T t_var = T(0), t_alpha = T(0), t_ls = T(0);
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        T f, df, da;
        FAM<T>::eval(r2[r][c], alpha, f, df, da);
        const T gij = g[r][c];                     // zero outside [R, C]: padded entries weigh nothing
        ws[r][c] = gij * df;
        wr[r][c] = a.sym ? (gij + wr[r][c]) * df : ws[r][c];
        t_var += gij * f;
        t_alpha += gij * da;
        t_ls += ws[r][c] * (T)r2[r][c];
      }
    s_var += (double)t_var, s_alpha += (double)t_alpha, s_ls += (double)t_ls;
    if (a.want_rows || ard) {
      for (int k = 0; k < D; ++k) {
        const T il = (T)inv_l[k];
        T xv[4], zv[4], p[4], q = T(0);
#pragma unroll
        for (int r = 0; r < 4; ++r) xv[r] = xs[(4 * ty + r) * stride + k];
#pragma unroll
        for (int c = 0; c < 4; ++c) zv[c] = zs[(4 * tx + c) * stride + k];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          p[r] = T(0);
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            const T d = (xv[r] - zv[c]) * il;
            p[r] += wr[r][c] * d;
            q += ws[r][c] * d * d;
          }
        }
        if (a.want_rows) {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const T total = gp_row16_sum(p[r]);
            if (tx == 0) acc[(4 * ty + r) * D + k] += (double)total;
          }
        }
        if (ard) {
          const T total = wave_sum(q);
          if (lane == 0) ls_acc[wave * D + k] += (double)total;
        }
      }
    }
  }
  __syncthreads();
  if (a.want_rows) {
    const int64_t rows_here = a.R - i0 < GPK_TILE ? a.R - i0 : GPK_TILE;
    double* rec = a.row_rec + ((int64_t)split * a.R + i0) * D;
    for (int64_t e = tid; e < rows_here * D; e += GPK_THREADS) rec[e] = acc[e];
  }
  double* sc = a.sc_rec + (int64_t)blockIdx.x * (GPK_SCALARS + D);
  if (a.want_scalars) {
    const double v0 = block_sum_f64_waves(s_var, red, GPK_THREADS / 64);
    const double v1 = block_sum_f64_waves(s_alpha, red, GPK_THREADS / 64);
    const double v2 = block_sum_f64_waves(s_ls, red, GPK_THREADS / 64);
    if (tid == 0) sc[0] = v0, sc[1] = v1, sc[2] = v2;
    if (ard)
      for (int k = tid; k < D; k += GPK_THREADS)
        sc[GPK_SCALARS + k] = (ls_acc[k] + ls_acc[D + k]) + (ls_acc[2 * D + k] + ls_acc[3 * D + k]);
  }
}

// records -> gradients, float64 sums in a fixed order.  Blocks [0, row_blocks_fin): g_rows[i, k] = (2 variance / l_k)
// sum_split rec[split, i, k].  Then one block per reduced output: lengthscale (n_ls of them), variance, alpha.
template <typename T>
struct GpFinArgs {
  const double *row_rec, *sc_rec;
  const T *ls, *variance;
  int n_ls, D, splits;
  int64_t R, workgroups, row_fin_blocks;
  T *g_rows, *g_ls, *g_var, *g_alpha;
};

template <typename T>
__global__ __launch_bounds__(GPK_THREADS) void gp_kernel_fin_kernel(const GpFinArgs<T> a) {
  __shared__ double red[GPK_THREADS / 64];
  const double var = (double)a.variance[0];
  if ((int64_t)blockIdx.x < a.row_fin_blocks) {
    const int64_t e = (int64_t)blockIdx.x * GPK_THREADS + threadIdx.x, total = a.R * a.D;
    if (e >= total) return;
    const int k = (int)(e % a.D);
    double s = 0.0;
    for (int sp = 0; sp < a.splits; ++sp) s += a.row_rec[(int64_t)sp * total + e];
    a.g_rows[e] = (T)(2.0 * var / (double)a.ls[a.n_ls == 1 ? 0 : k] * s);
    return;
  }
  const int which = (int)((int64_t)blockIdx.x - a.row_fin_blocks);      // 0 .. n_ls - 1: lengthscale; then variance, alpha
  int slot;
  T* out;
  if (which < a.n_ls) slot = a.n_ls == 1 ? 2 : GPK_SCALARS + which, out = a.g_ls ? a.g_ls + which : nullptr;
  else if (which == a.n_ls) slot = 0, out = a.g_var;
  else slot = 1, out = a.g_alpha;
  if (out == nullptr) return;                     // (uniform over the block)
  double s = 0.0;
  for (int64_t w = threadIdx.x; w < a.workgroups; w += GPK_THREADS) s += a.sc_rec[w * (GPK_SCALARS + a.D) + slot];
  s = block_sum_f64_waves(s, red, GPK_THREADS / 64);
  if (threadIdx.x == 0) {
    if (which < a.n_ls) s *= -2.0 * var / (double)a.ls[which];
    else if (which > a.n_ls) s *= var;
    *out = (T)s;
  }
}

// ---- launchers -----------------------------------------------------------------------------------------------------
template <typename T, template <typename> class FAM>
static int gp_fwd_launch(const void* x, const void* z, const void* ls, int n_ls, const void* variance, const void* alpha,
                         void* K, int64_t N, int64_t M, int D, hipStream_t st) {
  const int64_t col_tiles = gpk_tiles(M), tiles = gpk_tiles(N) * col_tiles;
  PA_REQUIRE(tiles <= GPK_MAX_WORKGROUPS, "pa_gp_kernel_fwd: %lld tiles over the grid limit", (long long)tiles);
  const size_t lds = gpk_fwd_lds_bytes(D, sizeof(T));
  auto k = gp_kernel_fwd_kernel<T, FAM>;
  if (lds > 48 * 1024) (void)hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  hipLaunchKernelGGL(k, dim3((unsigned)tiles), dim3(GPK_THREADS), lds, st, (const T*)x, (const T*)(z ? z : x), (const T*)ls,
                     n_ls, (const T*)variance, (const T*)alpha, (T*)K, N, M, D, col_tiles);
  return check_launch("gp_kernel_fwd_kernel");
}

template <typename T, template <typename> class FAM>
static int gp_bwd_side(const GpkLaunchPlan& pl, const T* xr, const T* xc, const T* G, int64_t g_sr, int64_t g_sc, int sym,
                       const T* ls, int n_ls, const T* variance, const T* alpha, bool want_ls, bool scalars, double* ws,
                       T* g_rows, T* g_ls, T* g_var, T* g_alpha, hipStream_t st) {
  PA_REQUIRE(pl.workgroups <= GPK_MAX_WORKGROUPS, "pa_gp_kernel_bwd: %lld workgroups over the grid limit",
             (long long)pl.workgroups);
  GpBwdArgs<T> a;
  a.xr = xr, a.xc = xc, a.G = G, a.g_sr = g_sr, a.g_sc = g_sc, a.sym = sym;
  a.ls = ls, a.variance = variance, a.alpha = alpha, a.n_ls = n_ls, a.D = pl.D, a.splits = pl.splits;
  a.want_rows = pl.row_records ? 1 : 0, a.want_ls = want_ls && scalars ? 1 : 0, a.want_scalars = scalars ? 1 : 0;
  a.R = pl.rows, a.C = pl.cols, a.tiles_per_split = pl.tiles_per_split, a.col_tiles = pl.col_tiles;
  a.row_rec = ws, a.sc_rec = ws + pl.row_doubles;
  const size_t lds = gpk_bwd_lds_bytes(pl.D, sizeof(T));
  auto k = gp_kernel_bwd_kernel<T, FAM>;
  if (lds > 48 * 1024) (void)hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  hipLaunchKernelGGL(k, dim3((unsigned)pl.workgroups), dim3(GPK_THREADS), lds, st, a);
  int rc = check_launch("gp_kernel_bwd_kernel");
  if (rc != PA_OK) return rc;
  GpFinArgs<T> f;
  f.row_rec = a.row_rec, f.sc_rec = a.sc_rec, f.ls = ls, f.variance = variance, f.n_ls = n_ls, f.D = pl.D;
  f.splits = pl.splits, f.R = pl.rows, f.workgroups = pl.workgroups;
  f.row_fin_blocks = pl.row_records ? (pl.rows * pl.D + GPK_THREADS - 1) / GPK_THREADS : 0;
  f.g_rows = g_rows, f.g_ls = g_ls, f.g_var = g_var, f.g_alpha = g_alpha;
  const int64_t blocks = f.row_fin_blocks + (scalars ? n_ls + 2 : 0);
  if (blocks == 0) return PA_OK;
  PA_REQUIRE(blocks <= GPK_MAX_WORKGROUPS, "pa_gp_kernel_bwd: finalize grid of %lld blocks", (long long)blocks);
  hipLaunchKernelGGL(gp_kernel_fin_kernel<T>, dim3((unsigned)blocks), dim3(GPK_THREADS), 0, st, f);
  return check_launch("gp_kernel_fin_kernel");
}

template <typename T, template <typename> class FAM>
static int gp_bwd_launch(const GpkCallPlan& cp, const void* x, const void* z, const void* ls, int n_ls, const void* variance,
                         const void* alpha, const void* G, int64_t N, int64_t M, void* gx, void* gz, void* g_ls, void* g_var,
                         void* g_alpha, void* workspace, hipStream_t st) {
  double* ws = (double*)workspace;
  const bool want_ls = g_ls != nullptr, any_scalar = g_ls || g_var || g_alpha;
  if (cp.run_x) {
    int rc = gp_bwd_side<T, FAM>(cp.x, (const T*)x, (const T*)(z ? z : x), (const T*)G, M, 1, z ? 0 : 1, (const T*)ls, n_ls,
                                 (const T*)variance, (const T*)alpha, want_ls, any_scalar, ws, (T*)gx, (T*)g_ls,
                                 (T*)g_var, (T*)g_alpha, st);
    if (rc != PA_OK) return rc;
  }
  if (cp.run_z) {
    const bool scalars = any_scalar && !cp.run_x;
    int rc = gp_bwd_side<T, FAM>(cp.z, (const T*)z, (const T*)x, (const T*)G, 1, M, 0, (const T*)ls, n_ls,
                                 (const T*)variance, (const T*)alpha, want_ls, scalars, ws + cp.z_offset_doubles, (T*)gz,
                                 (T*)g_ls, (T*)g_var, (T*)g_alpha, st);
    if (rc != PA_OK) return rc;
  }
  return PA_OK;
}

#define GPK_DISPATCH(CALL, ...)                                                       \
  switch (family) {                                                                   \
    case PA_GP_RBF: return CALL<T, GpRbf>(__VA_ARGS__);                               \
    case PA_GP_RATIONAL_QUADRATIC: return CALL<T, GpRq>(__VA_ARGS__);                 \
    case PA_GP_EXPONENTIAL: return CALL<T, GpExponential>(__VA_ARGS__);               \
    case PA_GP_MATERN32: return CALL<T, GpMatern32>(__VA_ARGS__);                     \
    default: return CALL<T, GpMatern52>(__VA_ARGS__);                                 \
  }

template <typename T>
static int gp_fwd_family(int family, const void* x, const void* z, const void* ls, int n_ls, const void* variance,
                         const void* alpha, void* K, int64_t N, int64_t M, int D, hipStream_t st) {
  GPK_DISPATCH(gp_fwd_launch, x, z, ls, n_ls, variance, alpha, K, N, M, D, st)
}
template <typename T>
static int gp_bwd_family(int family, const GpkCallPlan& cp, const void* x, const void* z, const void* ls, int n_ls,
                         const void* variance, const void* alpha, const void* G, int64_t N, int64_t M, void* gx, void* gz,
                         void* g_ls, void* g_var, void* g_alpha, void* workspace, hipStream_t st) {
  GPK_DISPATCH(gp_bwd_launch, cp, x, z, ls, n_ls, variance, alpha, G, N, M, gx, gz, g_ls, g_var, g_alpha, workspace, st)
}

static int gp_check(const char* who, int dtype, int family, const void* x, const void* ls, int n_ls, const void* variance,
                    const void* alpha, const void* z, int64_t N, int64_t M, int64_t D) {
  PA_REQUIRE(dtype == PA_F32 || dtype == PA_F64, "%s: dtype %d", who, dtype);
  if (!(D >= 1 && D <= GPK_MAX_D))
    return fail(PA_ERR_UNSUPPORTED, "%s: D=%lld outside [1, %d]", who, (long long)D, GPK_MAX_D);
  PA_REQUIRE(gpk_shape_ok(family, N, M, D, n_ls), "%s: family=%d N=%lld M=%lld D=%lld n_ls=%d", who, family, (long long)N,
             (long long)M, (long long)D, n_ls);
  PA_REQUIRE(z != nullptr || N == M, "%s: z = x needs M = N, got N=%lld M=%lld", who, (long long)N, (long long)M);
  PA_REQUIRE(ls != nullptr && variance != nullptr && (N == 0 || x != nullptr), "%s: null input", who);
  PA_REQUIRE(family != PA_GP_RATIONAL_QUADRATIC || alpha != nullptr, "%s: RationalQuadratic needs scale_mixture", who);
  return PA_OK;
}

}  // namespace pa

extern "C" {

int pa_gp_kernel_fwd(int dtype, int family, const void* x, const void* z, const void* lengthscale, int n_ls,
                     const void* variance, const void* alpha, void* K, int64_t N, int64_t M, int64_t D,
                     pa_stream_t stream) {
  int rc = pa::gp_check("pa_gp_kernel_fwd", dtype, family, x, lengthscale, n_ls, variance, alpha, z, N, M, D);
  if (rc != PA_OK) return rc;
  if (N == 0 || M == 0) return PA_OK;
  PA_REQUIRE(K != nullptr, "pa_gp_kernel_fwd: null output");
  hipStream_t st = pa::as_stream(stream);
  if (dtype == PA_F32)
    return pa::gp_fwd_family<float>(family, x, z, lengthscale, n_ls, variance, alpha, K, N, M, (int)D, st);
  return pa::gp_fwd_family<double>(family, x, z, lengthscale, n_ls, variance, alpha, K, N, M, (int)D, st);
}

size_t pa_gp_kernel_bwd_workspace(int64_t N, int64_t M, int64_t D, int z_null, int want_gx, int want_gz,
                                  int forced_splits) {
  if (!pa::gpk_shape_ok(0, N, M, D, 1) || N == 0 || M == 0) return 0;
  return pa::gpk_call_plan(N, M, (int)D, z_null != 0, want_gx != 0, want_gz != 0, pa::cu_count(), forced_splits).bytes;
}

int pa_gp_kernel_bwd(int dtype, int family, const void* x, const void* z, const void* lengthscale, int n_ls,
                     const void* variance, const void* alpha, const void* G, int64_t N, int64_t M, int64_t D, void* gx,
                     void* gz, void* g_lengthscale, void* g_variance, void* g_alpha, int forced_splits, void* workspace,
                     size_t workspace_bytes, pa_stream_t stream) {
  int rc = pa::gp_check("pa_gp_kernel_bwd", dtype, family, x, lengthscale, n_ls, variance, alpha, z, N, M, D);
  if (rc != PA_OK) return rc;
  PA_REQUIRE(gz == nullptr || z != nullptr, "pa_gp_kernel_bwd: gz without a z (with z = x, gx takes both roles)");
  PA_REQUIRE(g_alpha == nullptr || family == PA_GP_RATIONAL_QUADRATIC, "pa_gp_kernel_bwd: g_alpha for family %d", family);
  PA_REQUIRE(forced_splits >= 0, "pa_gp_kernel_bwd: forced_splits=%d", forced_splits);
  if (!(gx || gz || g_lengthscale || g_variance || g_alpha)) return PA_OK;
  PA_REQUIRE(N > 0 && M > 0, "pa_gp_kernel_bwd: an empty matrix has zero gradients; the caller fills them");
  PA_REQUIRE(G != nullptr, "pa_gp_kernel_bwd: null G");
  const pa::GpkCallPlan cp =
      pa::gpk_call_plan(N, M, (int)D, z == nullptr, gx != nullptr, gz != nullptr, pa::cu_count(), forced_splits);
  // the records of BOTH launches fit the workspace that was handed in (not merely the one sized by the caller's flags)
  PA_REQUIRE(workspace != nullptr && cp.bytes <= workspace_bytes && (uintptr_t)workspace % 8 == 0,
             "pa_gp_kernel_bwd: workspace of %zu bytes, the plan needs %zu (8-byte aligned)", workspace_bytes, cp.bytes);
  PA_REQUIRE((!cp.run_x || (cp.x.row_doubles + cp.x.scalar_doubles) * sizeof(double) == cp.x.bytes) &&
                 (!cp.run_z || cp.z_offset_doubles * sizeof(double) + cp.z.bytes == cp.bytes),
             "pa_gp_kernel_bwd: inconsistent plan");
  hipStream_t st = pa::as_stream(stream);
  if (dtype == PA_F32)
    return pa::gp_bwd_family<float>(family, cp, x, z, lengthscale, n_ls, variance, alpha, G, N, M, gx, gz, g_lengthscale,
                                    g_variance, g_alpha, workspace, st);
  return pa::gp_bwd_family<double>(family, cp, x, z, lengthscale, n_ls, variance, alpha, G, N, M, gx, gz, g_lengthscale,
                                   g_variance, g_alpha, workspace, st);
}

}  // extern "C"
