// gp_wrap.hip -- a stationary covariance matrix under an output transform and a vertical scaling, and its gradient:
//   K[i, j] = a_i * q(variance * f(r2_ij)) * b_j,   r2_ij = sum_k ((x_ik - z_jk) / l_k)^2
// f one of the five families of gp_kernel.hip or cos(r) (GpCosine, dispatched here alone), q the identity, exp, or a
// polynomial with at most 8 constant coefficients, a [N] and b [M] optional device vectors.  gp.kernels.Cosine, Exponent,
// Warping (owarping_coef) and VerticalScaling over a stationary leaf are this kernel; the arithmetic of r2 and of f is
// gp_kernel.hip's: direct differences of the points staged UNSCALED, difference, sum of squares and the argument of f in
// float64 for f32 and f64 alike, r = sqrt(r2 + 1e-12).  The forward is ONE launch that writes K once; the backward is
// one pass over the incoming gradient G per side that wants a gradient plus a fixed-order finalize.  No float atomics:
// bit-reproducible from call to call.
//
// Reference path replaced: pyro/contrib/gp/kernels/kernel.py: Exponent, Warping and VerticalScaling apply two to
// 2 len(coef) element-wise torch passes to the child's [N, M] matrix, and autograd keeps the exponential, every Horner
// intermediate and the scaled products alive.  Here nothing of size [N, M] is kept.
//
// Variants.  q and the presence of a / b are COMPILE-TIME parameters (Q, AB) beside the family: the pair loop has no
// branch on them.  q travels by value in the kernel arguments (GpwQ: 8 float64 coefficients, zero above the degree, so
// that Horner's rule always takes 7 steps and needs no count); nothing is copied to the device.  The plain families
// without a transform or a scaling are gp_kernel.hip's and are not instantiated here.
//
// Tiles: gp_tile.h's 64 x 64 frame, thread (ty, tx) owns rows 4 ty + r and columns 4 tx + c.  The tile's 64 + 64 scales
// are staged in LDS between the point tiles and the float64 words (gp_wrap_plan.h); with z = x one vector serves both.
//
// Backward.  Everything is recomputed from the inputs (a model adds noise to the diagonal of K in place).  With
// k0 = variance f, e_ij = a_i b_j q'(k0_ij) and G'_ij = G_ij e_ij, the machinery of gp_kernel.hip runs on G' unchanged:
//   gX_ik = (2 variance / l_k) sum_j G'_ij f' d_ijk      g_l_k = -(2 variance / l_k) sum_ij G'_ij f' d_ijk^2
//   g_variance = sum_ij G'_ij f_ij                        g_alpha = variance sum_ij G'_ij df/dalpha
// and the gradient of the scale is one more column of the row accumulator, [64, D + 1] float64 with one writer per entry:
//   g_a_i = sum_j G_ij q(k0_ij) b_j
// The second-side launch (roles of x and z, and of a and b, exchanged; G read through transposed strides) gives gZ and
// g_b.  With z = x one launch gives x and a both roles: the row weights take G_ij + G_ji.  Records per (row block,
// column split) are summed in split order in float64 by the finalize kernel.
//
// gfx950 cross-compile (hipcc -O3, -Rpass-analysis=kernel-resource-usage): no instantiation uses scratch; the table is
// in the README entry "Gaussian processes".
#include "gp_families.h"
#include "gp_host.h"
#include "gp_tile.h"
#include "gp_wrap_plan.h"

namespace pa {

struct GpwQ {
  double coef[GPW_MAX_COEF];      // q(k) = sum_c coef[c] k^c, zero above the degree
};

template <typename T>
__device__ __forceinline__ T gpw_fma(T a, T b, T c) {
  if constexpr (sizeof(T) == 4) return fmaf(a, b, c);
  else return fma(a, b, c);
}

// q(k0) and q'(k0) of the compile-time variant Q
template <typename T, int Q>
__device__ __forceinline__ void gpw_q(const GpwQ& p, T k0, T& q, T& dq) {
  if constexpr (Q == GPW_Q_IDENTITY) {
    q = k0, dq = T(1);
  } else if constexpr (Q == GPW_Q_EXP) {
    q = gp_exp(k0), dq = q;
  } else {
    q = (T)p.coef[GPW_MAX_COEF - 1], dq = T(0);
#pragma unroll
    for (int c = GPW_MAX_COEF - 2; c >= 0; --c) {
      dq = gpw_fma(dq, k0, q);
      q = gpw_fma(q, k0, (T)p.coef[c]);
    }
  }
}

// the scales of rows [first, first + 64) of s [n], zeros past the end (a padded row or column weighs nothing)
template <typename T>
__device__ __forceinline__ void gpw_stage_scale(const T* __restrict__ s, int64_t first, int64_t n, T* tile) {
  if (threadIdx.x < GPK_TILE) {
    const int64_t i = first + threadIdx.x;
    tile[threadIdx.x] = i < n ? s[i] : T(0);
  }
}

// ---- forward ---------------------------------------------------------------------------------------------------------
template <typename T>
struct GpwFwdArgs {
  const T *x, *z, *ls, *variance, *alpha, *sa, *sb;      // sa [N], sb [M]: read by the AB variants only
  int n_ls, D;
  int64_t N, M, col_tiles;
  GpwQ qp;
  T* K;
};

template <typename T, template <typename> class FAM, int Q, bool AB>
__global__ __launch_bounds__(GPK_THREADS) void gp_wrap_fwd_kernel(const GpwFwdArgs<T> a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char gp_lds[];
  const int D = a.D, stride = gpk_lds_stride(D);
  T* xs = reinterpret_cast<T*>(gp_lds);
  T* zs = xs + GPK_TILE * stride;
  T* as = zs + GPK_TILE * stride;                                                              // [64]
  T* bs = as + GPK_TILE;                                                                       // [64]
  double* inv_l = reinterpret_cast<double*>(gp_lds + gpw_lds_head_bytes(D, sizeof(T)));      // [D]
  const int64_t rt = (int64_t)blockIdx.x / a.col_tiles, ct = (int64_t)blockIdx.x - rt * a.col_tiles;
  const int64_t i0 = rt * GPK_TILE, j0 = ct * GPK_TILE;
  gp_stage(a.x, i0, a.N, D, stride, xs);
  gp_stage(a.z, j0, a.M, D, stride, zs);
  if constexpr (AB) {
    gpw_stage_scale(a.sa, i0, a.N, as);
    gpw_stage_scale(a.sb, j0, a.M, bs);
  }
  gp_inverse_lengthscale(a.ls, a.n_ls, D, inv_l);
  __syncthreads();
  const int ty = threadIdx.x >> 4, tx = threadIdx.x & 15;
  double r2[4][4];
  gp_r2_tile(xs, zs, inv_l, D, stride, ty, tx, r2);
  const T var = a.variance[0], alpha = a.alpha ? a.alpha[0] : T(1);
  T bv[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) bv[c] = AB ? bs[4 * tx + c] : T(1);
  const int64_t j = j0 + 4 * tx;
  const bool vec = (a.M & 3) == 0 && j + 3 < a.M && (uintptr_t)a.K % sizeof(Vec4<T>) == 0;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int64_t i = i0 + 4 * ty + r;
    if (i >= a.N) continue;
    const T av = AB ? as[4 * ty + r] : T(1);
    Vec4<T> out;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      T f, df, da, qv, dq;
      FAM<T>::eval(r2[r][c], alpha, f, df, da);
      gpw_q<T, Q>(a.qp, var * f, qv, dq);
      out.v[c] = AB ? av * qv * bv[c] : qv;
    }
    T* dst = a.K + i * a.M + j;
    if (vec) {
      *reinterpret_cast<Vec4<T>*>(dst) = out;
    } else {
#pragma unroll
      for (int c = 0; c < 4; ++c)
        if (j + c < a.M) dst[c] = out.v[c];
    }
  }
}

// ---- backward ----------------------------------------------------------------------------------------------------------
template <typename T>
struct GpwBwdArgs {
  const T *xr, *xc;            // the points that get a gradient [R, D], the points that are walked [C, D]
  const T *sr, *sc;            // their scales [R], [C] (AB variants)
  const T* G;                  // G(i, j) = G[i * g_sr + j * g_sc], one of the strides is 1
  int64_t g_sr, g_sc;
  int sym;                     // z = x: the row weights take G_ij + G_ji
  const T *ls, *variance, *alpha;
  int n_ls, D, splits;
  int want_rows, want_scale, want_ls, want_scalars;
  int64_t R, C, tiles_per_split, col_tiles;
  GpwQ qp;
  double *row_rec, *sc_rec;    // [splits, R, D + 1], [workgroups, GPK_SCALARS + D]
};

template <typename T, template <typename> class FAM, int Q, bool AB>
__global__ __launch_bounds__(GPK_THREADS) void gp_wrap_bwd_kernel(const GpwBwdArgs<T> a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char gp_lds[];
  __shared__ double red[GPK_WAVES];
  const int D = a.D, stride = gpk_lds_stride(D), W = gpw_row_width(D);
  T* xs = reinterpret_cast<T*>(gp_lds);
  T* zs = xs + GPK_TILE * stride;
  T* as = zs + GPK_TILE * stride;                                                              // [64] rows' scales
  T* bs = as + GPK_TILE;                                                                       // [64] the column tile's
  double* inv_l = reinterpret_cast<double*>(gp_lds + gpw_lds_head_bytes(D, sizeof(T)));      // [D]
  double* acc = inv_l + D;                                                                     // [64, D + 1]
  double* ls_acc = acc + GPK_TILE * W;                                                         // [4, D]
  const int tid = threadIdx.x, ty = tid >> 4, tx = tid & 15, lane = tid & 63, wave = tid >> 6;
  const int64_t rb = (int64_t)blockIdx.x / a.splits;
  const int split = (int)((int64_t)blockIdx.x - rb * a.splits);
  const int64_t i0 = rb * GPK_TILE;
  gp_stage(a.xr, i0, a.R, D, stride, xs);
  if constexpr (AB) gpw_stage_scale(a.sr, i0, a.R, as);
  gp_inverse_lengthscale(a.ls, a.n_ls, D, inv_l);
  for (int e = tid; e < GPK_TILE * W + GPK_WAVES * D; e += GPK_THREADS) acc[e] = 0.0;
  const T var = a.variance[0], alpha = a.alpha ? a.alpha[0] : T(1);
  const bool ard = a.want_ls && a.n_ls != 1;
  double s_var = 0.0, s_alpha = 0.0, s_ls = 0.0;
  int64_t ct_end = (int64_t)(split + 1) * a.tiles_per_split;
  if (ct_end > a.col_tiles) ct_end = a.col_tiles;
  for (int64_t ct = (int64_t)split * a.tiles_per_split; ct < ct_end; ++ct) {
    const int64_t j0 = ct * GPK_TILE;
    __syncthreads();                               // the previous tile's reads of zs and bs are over
    gp_stage(a.xc, j0, a.C, D, stride, zs);
    if constexpr (AB) gpw_stage_scale(a.sc, j0, a.C, bs);
    __syncthreads();
    double r2[4][4];
    T g[4][4], wr[4][4], ws[4][4], bv[4], ps[4];
    gp_r2_tile(xs, zs, inv_l, D, stride, ty, tx, r2);
    gp_load_g(a, a.g_sr, a.g_sc, i0, j0, ty, tx, g);
    if (a.sym) gp_load_g(a, a.g_sc, a.g_sr, i0, j0, ty, tx, wr);      // G(j, i)
#pragma unroll
    for (int c = 0; c < 4; ++c) bv[c] = AB ? bs[4 * tx + c] : T(1);
    T t_var = T(0), t_alpha = T(0), t_ls = T(0);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const T av = AB ? as[4 * ty + r] : T(1);
      ps[r] = T(0);
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        T f, df, da, qv, dq;
        FAM<T>::eval(r2[r][c], alpha, f, df, da);
        gpw_q<T, Q>(a.qp, var * f, qv, dq);
        const T e = AB ? av * bv[c] * dq : dq;     // d K_ij / d k0_ij
        const T gij = g[r][c];                     // zero outside [R, C]: padded entries weigh nothing
        const T both = a.sym ? gij + wr[r][c] : gij;
        const T ge = gij * e;
        ws[r][c] = ge * df;
        wr[r][c] = both * e * df;
        if constexpr (AB) ps[r] += both * qv * bv[c];
        t_var += ge * f;
        t_alpha += ge * da;
        t_ls += ws[r][c] * (T)r2[r][c];
      }
    }
    s_var += (double)t_var, s_alpha += (double)t_alpha, s_ls += (double)t_ls;
    if constexpr (AB) {
      if (a.want_scale) {
#pragma unroll
        for (int r = 0; r < 4; ++r) gp_row_add(ps[r], acc, (4 * ty + r) * W + D, tx);
      }
    }
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
          for (int r = 0; r < 4; ++r) gp_row_add(p[r], acc, (4 * ty + r) * W + k, tx);
        }
        if (ard) gp_wave_add(q, ls_acc, wave * D + k, lane);
      }
    }
  }
  __syncthreads();
  if (a.want_rows || a.want_scale) gp_copy_row_record(acc, a.row_rec, split, a.R, i0, W);
  double* sc = a.sc_rec + (int64_t)blockIdx.x * gpk_record_doubles(D);
  if (a.want_scalars) {
    const double v0 = block_sum_f64_waves(s_var, red, GPK_WAVES);
    const double v1 = block_sum_f64_waves(s_alpha, red, GPK_WAVES);
    const double v2 = block_sum_f64_waves(s_ls, red, GPK_WAVES);
    if (tid == 0) sc[0] = v0, sc[1] = v1, sc[2] = v2;
    if (ard)
      for (int k = tid; k < D; k += GPK_THREADS) sc[GPK_SCALARS + k] = gp_fold_waves(ls_acc, k, D);
  }
}

// records -> gradients, float64 sums in a fixed order.  Blocks [0, row_fin_blocks): entry (i, k) of the row records
// [splits, R, D + 1]: k < D is g_rows[i, k] = (2 variance / l_k) sum_split, k = D is g_scale[i] = sum_split.  Then one
// block per reduced output: lengthscale (n_ls of them), variance, alpha.
template <typename T>
struct GpwFinArgs {
  const double *row_rec, *sc_rec;
  const T *ls, *variance;
  int n_ls, D, splits;
  int64_t R, workgroups, row_fin_blocks;
  T *g_rows, *g_scale, *g_ls, *g_var, *g_alpha;
};

template <typename T>
__global__ __launch_bounds__(GPK_THREADS) void gp_wrap_fin_kernel(const GpwFinArgs<T> a) {
  __shared__ double red[GPK_WAVES];
  const double var = (double)a.variance[0];
  if ((int64_t)blockIdx.x < a.row_fin_blocks) {
    const int W = gpw_row_width(a.D);
    const int64_t e = (int64_t)blockIdx.x * GPK_THREADS + threadIdx.x, total = a.R * W;
    if (e >= total) return;
    const int64_t i = e / W;
    const int k = (int)(e - i * W);
    if (k < a.D ? a.g_rows == nullptr : a.g_scale == nullptr) return;
    const double s = gp_sum_splits(a.row_rec, a.splits, total, e);
    if (k < a.D) a.g_rows[i * a.D + k] = (T)(2.0 * var / (double)a.ls[a.n_ls == 1 ? 0 : k] * s);
    else a.g_scale[i] = (T)s;
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
  for (int64_t w = threadIdx.x; w < a.workgroups; w += GPK_THREADS) s += a.sc_rec[w * gpk_record_doubles(a.D) + slot];
  s = block_sum_f64_waves(s, red, GPK_WAVES);
  if (threadIdx.x == 0) {
    if (which < a.n_ls) s *= -2.0 * var / (double)a.ls[which];
    else if (which > a.n_ls) s *= var;
    *out = (T)s;
  }
}

// ---- launchers -----------------------------------------------------------------------------------------------------
// one call of an entry point, as the entry point received it
struct GpwCall {
  const void *x, *z, *ls, *variance, *alpha, *a, *b, *G;
  int n_ls, D, forced_splits;
  int64_t N, M;
  GpwQ qp;
  void *K, *gx, *gz, *g_ls, *g_var, *g_alpha, *g_a, *g_b, *workspace;
  const GpkCallPlan* cp;
  hipStream_t st;
};

template <typename T, template <typename> class FAM, int Q, bool AB>
static int gpw_fwd_launch(const GpwCall& c) {
  GpwFwdArgs<T> a;
  a.x = (const T*)c.x, a.z = (const T*)(c.z ? c.z : c.x), a.ls = (const T*)c.ls, a.variance = (const T*)c.variance;
  a.alpha = (const T*)c.alpha, a.sa = (const T*)c.a, a.sb = (const T*)(c.z ? c.b : c.a);
  a.n_ls = c.n_ls, a.D = c.D, a.N = c.N, a.M = c.M, a.col_tiles = gpk_tiles(c.M), a.qp = c.qp, a.K = (T*)c.K;
  const int64_t tiles = gpk_tiles(c.N) * a.col_tiles;
  PA_REQUIRE(tiles <= GPK_MAX_WORKGROUPS, "pa_gp_wrap_fwd: %lld tiles over the grid limit", (long long)tiles);
  return gp_launch("gp_wrap_fwd_kernel", gp_wrap_fwd_kernel<T, FAM, Q, AB>, tiles, GPK_THREADS,
                   gpw_fwd_lds_bytes(c.D, sizeof(T)), c.st, a);
}

// one side: the main launch and its finalize
template <typename T, template <typename> class FAM, int Q, bool AB>
static int gpw_bwd_side(const GpwCall& c, const GpkLaunchPlan& pl, const void* xr, const void* xc, const void* sr,
                        const void* sc, int64_t g_sr, int64_t g_sc, bool sym, bool scalars, double* ws, void* g_rows,
                        void* g_scale) {
  PA_REQUIRE(pl.workgroups <= GPK_MAX_WORKGROUPS, "pa_gp_wrap_bwd: %lld workgroups over the grid limit",
             (long long)pl.workgroups);
  GpwBwdArgs<T> a;
  a.xr = (const T*)xr, a.xc = (const T*)xc, a.sr = (const T*)sr, a.sc = (const T*)sc, a.G = (const T*)c.G;
  a.g_sr = g_sr, a.g_sc = g_sc, a.sym = sym ? 1 : 0;
  a.ls = (const T*)c.ls, a.variance = (const T*)c.variance, a.alpha = (const T*)c.alpha;
  a.n_ls = c.n_ls, a.D = pl.D, a.splits = pl.splits;
  a.want_rows = g_rows ? 1 : 0, a.want_scale = g_scale ? 1 : 0;
  a.want_ls = c.g_ls && scalars ? 1 : 0, a.want_scalars = scalars ? 1 : 0;
  a.R = pl.rows, a.C = pl.cols, a.tiles_per_split = pl.tiles_per_split, a.col_tiles = pl.col_tiles, a.qp = c.qp;
  a.row_rec = ws, a.sc_rec = ws + pl.row_doubles;
  PA_REQUIRE(pl.row_records || !(g_rows || g_scale), "pa_gp_wrap_bwd: a row gradient without row records");
  int rc = gp_launch("gp_wrap_bwd_kernel", gp_wrap_bwd_kernel<T, FAM, Q, AB>, pl.workgroups, GPK_THREADS,
                     gpw_bwd_lds_bytes(pl.D, sizeof(T)), c.st, a);
  if (rc != PA_OK) return rc;
  GpwFinArgs<T> f;
  f.row_rec = a.row_rec, f.sc_rec = a.sc_rec, f.ls = a.ls, f.variance = a.variance, f.n_ls = c.n_ls, f.D = pl.D;
  f.splits = pl.splits, f.R = pl.rows, f.workgroups = pl.workgroups;
  f.row_fin_blocks = (g_rows || g_scale) ? (pl.rows * gpw_row_width(pl.D) + GPK_THREADS - 1) / GPK_THREADS : 0;
  f.g_rows = (T*)g_rows, f.g_scale = (T*)g_scale;
  f.g_ls = (T*)c.g_ls, f.g_var = (T*)c.g_var, f.g_alpha = (T*)c.g_alpha;
  const int64_t blocks = f.row_fin_blocks + (scalars ? c.n_ls + 2 : 0);
  if (blocks == 0) return PA_OK;
  PA_REQUIRE(blocks <= GPK_MAX_WORKGROUPS, "pa_gp_wrap_bwd: finalize grid of %lld blocks", (long long)blocks);
  return gp_launch("gp_wrap_fin_kernel", gp_wrap_fin_kernel<T>, blocks, GPK_THREADS, 0, c.st, f);
}

// x's launch, then, for a z of its own that wants a gradient, z's with the roles of x and z and of a and b exchanged.
// With z = x (null) x's launch gives x and a both roles.  The reduced gradients come from the first launch that runs.
template <typename T, template <typename> class FAM, int Q, bool AB>
static int gpw_bwd_launch(const GpwCall& c) {
  const GpkCallPlan& cp = *c.cp;
  const bool any_scalar = c.g_ls || c.g_var || c.g_alpha, sym = c.z == nullptr;
  double* ws = (double*)c.workspace;
  if (cp.run_x) {
    int rc = gpw_bwd_side<T, FAM, Q, AB>(c, cp.x, c.x, sym ? c.x : c.z, c.a, sym ? c.a : c.b, c.M, 1, sym, any_scalar, ws,
                                         c.gx, c.g_a);
    if (rc != PA_OK) return rc;
  }
  if (cp.run_z)
    return gpw_bwd_side<T, FAM, Q, AB>(c, cp.z, c.z, c.x, c.b, c.a, 1, c.M, false, any_scalar && !cp.run_x,
                                       ws + cp.z_offset_doubles, c.gz, c.g_b);
  return PA_OK;
}

// variant = q + 3 * (a and b given).  PLAIN: whether <identity, no scaling> exists for the family (GpCosine alone).
// <f64, polynomial, scaled> is not built: its backward needs more than the 512 registers of a lane (RationalQuadratic
// and Cosine spill to scratch, the others come within 12 to 62 of the limit), so the classes keep that case in torch.
#define GPW_VARIANT_DISPATCH(CALL, FAM, PLAIN)                                                                     \
  switch (variant) {                                                                                               \
    case 0:                                                                                                        \
      if constexpr (PLAIN) return CALL<T, FAM, GPW_Q_IDENTITY, false>(c);                                          \
      else return fail(PA_ERR_INVALID, "pa_gp_wrap: family %d without a transform is pa_gp_kernel's", family);     \
    case 1: return CALL<T, FAM, GPW_Q_EXP, false>(c);                                                              \
    case 2: return CALL<T, FAM, GPW_Q_POLY, false>(c);                                                             \
    case 3: return CALL<T, FAM, GPW_Q_IDENTITY, true>(c);                                                          \
    case 4: return CALL<T, FAM, GPW_Q_EXP, true>(c);                                                               \
    default:                                                                                                       \
      if constexpr (sizeof(T) == 4) return CALL<T, FAM, GPW_Q_POLY, true>(c);                                      \
      else return fail(PA_ERR_UNSUPPORTED, "pa_gp_wrap: f64 with a polynomial and a scaling is not built");        \
  }
#define GPW_FAMILY_DISPATCH(CALL)                                                        \
  switch (family) {                                                                      \
    case PA_GP_RBF: GPW_VARIANT_DISPATCH(CALL, GpRbf, false)                             \
    case PA_GP_RATIONAL_QUADRATIC: GPW_VARIANT_DISPATCH(CALL, GpRq, false)               \
    case PA_GP_EXPONENTIAL: GPW_VARIANT_DISPATCH(CALL, GpExponential, false)             \
    case PA_GP_MATERN32: GPW_VARIANT_DISPATCH(CALL, GpMatern32, false)                   \
    case PA_GP_MATERN52: GPW_VARIANT_DISPATCH(CALL, GpMatern52, false)                   \
    default: GPW_VARIANT_DISPATCH(CALL, GpCosine, true)                                  \
  }

template <typename T>
static int gpw_fwd_family(int family, int variant, const GpwCall& c) {
  GPW_FAMILY_DISPATCH(gpw_fwd_launch)
}
template <typename T>
static int gpw_bwd_family(int family, int variant, const GpwCall& c) {
  GPW_FAMILY_DISPATCH(gpw_bwd_launch)
}

static int gpw_check(const char* who, int dtype, int family, int q, const double* coef, int n_coef, const GpwCall& c,
                     int64_t D) {
  PA_REQUIRE(dtype == PA_F32 || dtype == PA_F64, "%s: dtype %d", who, dtype);
  if (!(D >= 1 && D <= GPK_MAX_D))
    return fail(PA_ERR_UNSUPPORTED, "%s: D=%lld outside [1, %d]", who, (long long)D, GPK_MAX_D);
  if (!gpw_supported(dtype == PA_F32 ? 4 : 8, q, n_coef, c.a != nullptr))
    return fail(PA_ERR_UNSUPPORTED, "%s: %d coefficients outside [1, %d], or f64 with a polynomial and a scaling", who, n_coef,
                GPW_MAX_COEF);
  PA_REQUIRE(gpw_family_ok(family) && gpk_shape_ok(0, c.N, c.M, D, c.n_ls), "%s: family=%d N=%lld M=%lld D=%lld n_ls=%d", who,
             family, (long long)c.N, (long long)c.M, (long long)D, c.n_ls);
  PA_REQUIRE(gpw_variant_ok(family, q, c.a != nullptr), "%s: family=%d q=%d%s is not a variant of this kernel", who, family, q,
             c.a ? " scaled" : "");
  PA_REQUIRE(q != GPW_Q_POLY || coef != nullptr, "%s: null coefficients", who);
  PA_REQUIRE(c.z != nullptr || c.N == c.M, "%s: z = x needs M = N, got N=%lld M=%lld", who, (long long)c.N, (long long)c.M);
  PA_REQUIRE(c.ls != nullptr && c.variance != nullptr && (c.N == 0 || c.x != nullptr), "%s: null input", who);
  PA_REQUIRE((family == PA_GP_RATIONAL_QUADRATIC) == (c.alpha != nullptr), "%s: scale_mixture goes with RationalQuadratic",
             who);
  PA_REQUIRE((c.b != nullptr) == (c.a != nullptr && c.z != nullptr), "%s: a [N] and, with a z of its own, b [M], or neither",
             who);
  return PA_OK;
}

static GpwQ gpw_q_of(int q, const double* coef, int n_coef) {
  GpwQ p;
  for (int i = 0; i < GPW_MAX_COEF; ++i) p.coef[i] = (q == GPW_Q_POLY && i < n_coef) ? coef[i] : 0.0;
  return p;
}

}  // namespace pa

extern "C" {

int pa_gp_wrap_fwd(int dtype, int family, int q, const double* coef, int n_coef, const void* x, const void* z,
                   const void* lengthscale, int n_ls, const void* variance, const void* alpha, const void* a, const void* b,
                   void* K, int64_t N, int64_t M, int64_t D, pa_stream_t stream) {
  pa::GpwCall c = {};
  c.x = x, c.z = z, c.ls = lengthscale, c.variance = variance, c.alpha = alpha, c.a = a, c.b = b;
  c.n_ls = n_ls, c.D = (int)D, c.N = N, c.M = M, c.K = K;
  int rc = pa::gpw_check("pa_gp_wrap_fwd", dtype, family, q, coef, n_coef, c, D);
  if (rc != PA_OK) return rc;
  if (N == 0 || M == 0) return PA_OK;
  PA_REQUIRE(K != nullptr, "pa_gp_wrap_fwd: null output");
  c.qp = pa::gpw_q_of(q, coef, n_coef);
  c.st = pa::as_stream(stream);
  const int variant = q + 3 * (a != nullptr);
  if (dtype == PA_F32) return pa::gpw_fwd_family<float>(family, variant, c);
  return pa::gpw_fwd_family<double>(family, variant, c);
}

size_t pa_gp_wrap_bwd_workspace(int64_t N, int64_t M, int64_t D, int z_null, int rows_x, int rows_z, int forced_splits) {
  if (!pa::gpk_shape_ok(0, N, M, D, 1) || N == 0 || M == 0) return 0;
  return pa::gpw_call_plan(N, M, (int)D, z_null != 0, rows_x != 0, rows_z != 0, pa::cu_count(), forced_splits).bytes;
}

int pa_gp_wrap_bwd(int dtype, int family, int q, const double* coef, int n_coef, const void* x, const void* z,
                   const void* lengthscale, int n_ls, const void* variance, const void* alpha, const void* a, const void* b,
                   const void* G, int64_t N, int64_t M, int64_t D, void* gx, void* gz, void* g_lengthscale, void* g_variance,
                   void* g_alpha, void* g_a, void* g_b, int forced_splits, void* workspace, size_t workspace_bytes,
                   pa_stream_t stream) {
  pa::GpwCall c = {};
  c.x = x, c.z = z, c.ls = lengthscale, c.variance = variance, c.alpha = alpha, c.a = a, c.b = b, c.G = G;
  c.n_ls = n_ls, c.D = (int)D, c.forced_splits = forced_splits, c.N = N, c.M = M;
  c.gx = gx, c.gz = gz, c.g_ls = g_lengthscale, c.g_var = g_variance, c.g_alpha = g_alpha, c.g_a = g_a, c.g_b = g_b;
  c.workspace = workspace;
  int rc = pa::gpw_check("pa_gp_wrap_bwd", dtype, family, q, coef, n_coef, c, D);
  if (rc != PA_OK) return rc;
  PA_REQUIRE(g_alpha == nullptr || family == PA_GP_RATIONAL_QUADRATIC, "pa_gp_wrap_bwd: g_alpha for family %d", family);
  PA_REQUIRE((g_a == nullptr || a != nullptr) && (g_b == nullptr || b != nullptr), "pa_gp_wrap_bwd: g_a / g_b without a / b");
  bool launch;
  rc = pa::gp_bwd_preamble("pa_gp_wrap_bwd", z, gz ? gz : g_b, forced_splits,
                           gx || gz || g_lengthscale || g_variance || g_alpha || g_a || g_b, N, M, G, &launch);
  if (rc != PA_OK || !launch) return rc;
  const pa::GpkCallPlan cp = pa::gpw_call_plan(N, M, (int)D, z == nullptr, gx || g_a, gz || g_b, pa::cu_count(), forced_splits);
  rc = pa::gp_workspace_check("pa_gp_wrap_bwd", workspace, workspace_bytes, cp.bytes);
  if (rc != PA_OK) return rc;
  PA_REQUIRE((!cp.run_x || (cp.x.row_doubles + cp.x.scalar_doubles) * sizeof(double) == cp.x.bytes) &&
                 (!cp.run_z || cp.z_offset_doubles * sizeof(double) + cp.z.bytes == cp.bytes),
             "pa_gp_wrap_bwd: inconsistent plan");
  c.cp = &cp;
  c.qp = pa::gpw_q_of(q, coef, n_coef);
  c.st = pa::as_stream(stream);
  const int variant = q + 3 * (a != nullptr);
  if (dtype == PA_F32) return pa::gpw_bwd_family<float>(family, variant, c);
  return pa::gpw_bwd_family<double>(family, variant, c);
}

}  // extern "C"
