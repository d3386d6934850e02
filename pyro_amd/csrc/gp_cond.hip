// gp_cond.hip -- the per-point marginals of a sparse variational GP's conditional, streamed over the points, so that
// Kuf [M, N], W = Luu^-1 Kuf and W S [N, M Q] are never formed.  With k_n = Kuf[:, n], Kuf[i, n] = variance f(r2(xu_i, x_n)):
//   loc[n, q] = k_n . a[:, q]            a [M, Q]
//   s[n, j]   = |P_j k_n|^2              P [J, M, M], J = 1 + Q, P_0 lower triangular (Luu^-1)
// and their gradient given g_loc [N, Q], g_s [N, J]:
//   ga = Kuf g_loc,   Aw_j = Kuf diag(g_s[:, j]) Kuf^T   (float64 for both dtypes, so that gP_j = 2 P_j Aw_j is M x M
//   algebra for the caller),
//   G = dL/dKuf = a g_loc^T + sum_j (2 P_j^T P_j) Kuf diag(g_s[:, j]),  chained to x, xu and the kernel's parameters.
// G exists one [32 points, 32 rows] block at a time in registers.  f32 and f64, the five stationary families of
// gp_kernel.hip, 1 <= D <= 64, 1 <= Q <= 16, M <= 512 (f32) / 256 (f64).  No float atomics: partial records in float64,
// summed in a fixed order; bit-reproducible.
//
// Reference path replaced: pyro/contrib/gp/util.py conditional(..., full_cov=False) as VariationalSparseGP calls it:
// Kuf, Luu^-1 Kuf, W S and their squares, all [M, N] or larger and all kept by autograd, a dozen launches each way.
//
// r2 is gp_sgpr.hip's (gp_sparse_dev.h, with the wave's block and the staging) and the family functions are
// gp_families.h's, the ones every covariance kernel evaluates: the difference first, its square summed in float64 up
// to the exponential.  The matrix primitive (gpc_mac) is gp_sgpr.hip's gps_mac with two
// additions: the rows of A may be clamped (the caller discards the rows past the limit) and may carry a weight.  In f32
// it is v_mfma_f32_32x32x2_f32, in f64 the same register layout filled by VALU FMAs (v_mfma_f64_16x16x4_f64 has not
// been tried here; whether it pays is not measured).
//
// Forward.  One workgroup per tile of 32 points; no splits, no records.  x rows into LDS, Kuf[:, tile] [M, 32] generated
// into LDS (row stride 33), then the four waves share the pairs (j, 32-row block of P_j): Y = P_j[rows, :] Kuf[:, tile],
// inner length M -- for j = 0 only up to the block's last column, P_0 being lower triangular.  P comes TRANSPOSED
// (Pt_j = P_j^T), so that the 32 rows an operand needs at one inner index are 32 consecutive words, read through L2.
// A lane holds one point and 16 rows of Y: the squared norm is an in-lane sum and one exchange between the half-waves.
// Each wave adds into its own float64 [J, 32] in LDS; the four are summed in wave order.  loc rides along on the VALU.
//
// Backward, launch one.  gp_sgpr's forward frame with j as one more grid dimension: workgroup (j, block pair I <= J',
// split of N); the column tile is weighted by g_s[n, j] as it is generated; ga rides along for j = 0 on the diagonal.
// The finalize kernel takes both triangles of Aw_j from the upper one.
//
// Backward, launch two.  gp_sgpr's backward frame: workgroup (chunk of 128 inducing rows, split of N), all of
// Kuf[:, 32 points] in LDS.  G^T [32 points, 32 rows] is ONE accumulator over all j -- the weight g_s[n, j] goes onto
// the Kuf operand as it is read from LDS, B2_j = 2 P_j^T P_j (symmetric, formed by the caller) is read as its own
// transpose -- then a g_loc^T as Q more inner steps.  From there as gp_sgpr.hip: f' for the lane's 16 entries, float64
// [128, D] accumulators in LDS with one writer per entry, per-chunk partials of gx, scalar records, a finalize kernel.
#include "gp_cond_plan.h"
#include "gp_families.h"
#include "gp_host.h"
#include "gp_sparse_dev.h"

namespace pa {

// C += diag(w) A B.  A(i, k) = A[min(i, a_rows - 1) * a_si + k * a_sk], i < 32: rows past a_rows repeat the last one and
// the caller discards them.  WEIGHTED: w_i = w[i * w_s], else 1.  B(k, j) = B[k * b_sk + j * b_sj], read only where b_ok
// (the lane's column j = lane % 32 exists), zero otherwise; k < K
template <typename T, bool WEIGHTED>
__device__ __forceinline__ void gpc_mac(GpsAcc<T>& acc, const T* A, int a_si, int a_sk, int a_rows, const T* w, int w_s,
                                        const T* B, int b_sk, int b_sj, int K, bool b_ok, int lane) {
  const int col = lane & 31, half = lane >> 5;
  if constexpr (sizeof(T) == 4) {
    const int arow = (col < a_rows ? col : a_rows - 1) * a_si;
    float wi = 1.0f;
    if constexpr (WEIGHTED) wi = w[col * w_s];
#pragma unroll 4
    for (int k0 = 0; k0 < K; k0 += 2) {
      const int k = k0 + half;
      const bool in = k < K;
      float av = in ? A[arow + k * a_sk] : 0.0f;
      if constexpr (WEIGHTED) av *= wi;
      const float bv = (in && b_ok) ? B[k * b_sk + col * b_sj] : 0.0f;
      acc.c = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc.c, 0, 0, 0);
    }
  } else {
    int arow[16];
    double wi[16];
#pragma unroll
    for (int v = 0; v < 16; ++v) {
      const int r = gps_row(v, lane);
      arow[v] = (r < a_rows ? r : a_rows - 1) * a_si;
      if constexpr (WEIGHTED) wi[v] = w[r * w_s];
    }
#pragma unroll 2
    for (int k = 0; k < K; ++k) {
      const double bv = b_ok ? B[k * b_sk + col * b_sj] : 0.0;
#pragma unroll
      for (int v = 0; v < 16; ++v) {
        double av = A[arow[v] + k * a_sk];
        if constexpr (WEIGHTED) av *= wi[v];
        acc.c[v] = fma(av, bv, acc.c[v]);
      }
    }
  }
}

// ---- forward ---------------------------------------------------------------------------------------------------------
template <typename T>
struct GpcFwdArgs {
  const T *x, *xu, *a, *Pt, *ls, *variance, *alpha;      // a [M, Q], Pt [J, M, M] with Pt_j = P_j^T
  int n_ls, D, Q, M, row_blocks;
  int64_t N;
  T *loc, *s;                                            // [N, Q], [N, J]
};

template <typename T, template <typename> class FAM>
__global__ __launch_bounds__(GPS_THREADS) void gp_cond_fwd_kernel(const GpcFwdArgs<T> a) {
  constexpr int WAVES = GPS_THREADS / 64;
  extern __shared__ __attribute__((aligned(16))) unsigned char gpc_lds[];
  const int D = a.D, Q = a.Q, J = Q + 1, M = a.M, RB = a.row_blocks, stride = gps_lds_stride(D);
  double* inv_l = reinterpret_cast<double*>(gpc_lds);      // [D]
  double* sred = inv_l + D;                                // [WAVES, J, TN]
  T* ks = reinterpret_cast<T*>(sred + WAVES * J * GPS_TN); // [RB * 32, KS]: Kuf[:, tile], zero rows past M
  T* xs = ks + RB * GPS_SUB * GPS_KS;                      // [TN, stride]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int p = tid & 31, g8 = tid >> 5;
  const int64_t n0 = (int64_t)blockIdx.x * GPS_TN;
  gps_stage(a.x, n0, a.N, GPS_TN, D, stride, xs);
  for (int k = tid; k < D; k += GPS_THREADS) inv_l[k] = 1.0 / (double)a.ls[a.n_ls == 1 ? 0 : k];
  for (int e = tid; e < WAVES * J * GPS_TN; e += GPS_THREADS) sred[e] = 0.0;
  const T var = a.variance[0], alpha = a.alpha ? a.alpha[0] : T(1);
  __syncthreads();
  const bool p_in = n0 + p < a.N;
  for (int i = g8; i < RB * GPS_SUB; i += 8) {
    T f = T(0), df, da;
    if (p_in && i < M) {
      FAM<T>::eval(gps_r2(a.xu + (int64_t)i * D, xs + p * stride, inv_l, D), alpha, f, df, da);
      f *= var;
    }
    ks[i * GPS_KS + p] = f;
  }
  __syncthreads();
  for (int t = wave; t < J * RB; t += WAVES) {      // (wave-uniform)
    const int j = t / RB, r0 = (t - j * RB) * GPS_SUB;
    const int K = (j == 0 && r0 + GPS_SUB < M) ? r0 + GPS_SUB : M;      // P_0[row, k] = 0 for k > row
    GpsAcc<T> y;
    gps_clear(y);
    gpc_mac<T, false>(y, a.Pt + (int64_t)j * M * M + r0, 1, M, M - r0, nullptr, 0, ks, GPS_KS, 1, K, true, lane);
    T ss = T(0);
#pragma unroll
    for (int v = 0; v < 16; ++v)
      if (r0 + gps_row(v, lane) < M) ss += y.c[v] * y.c[v];
    ss += __shfl_xor(ss, 32);
    if (lane < 32) sred[(wave * J + j) * GPS_TN + lane] += (double)ss;      // this wave's own [J, 32]
  }
  if (p_in) {
    for (int q = g8; q < Q; q += 8) {
      double sum = 0.0;
      for (int i = 0; i < M; ++i) sum += (double)(ks[i * GPS_KS + p] * a.a[i * Q + q]);
      a.loc[(n0 + p) * Q + q] = (T)sum;
    }
  }
  __syncthreads();
  for (int e = tid; e < J * GPS_TN; e += GPS_THREADS) {
    const int j = e / GPS_TN, pp = e - j * GPS_TN;
    if (n0 + pp >= a.N) continue;
    double sum = 0.0;
    for (int w = 0; w < WAVES; ++w) sum += sred[(w * J + j) * GPS_TN + pp];
    a.s[(n0 + pp) * J + j] = (T)sum;
  }
}

// ---- backward, launch one: Aw [J, M, M] and ga [M, Q] ---------------------------------------------------------------
template <typename T>
struct GpcGramArgs {
  const T *x, *xu, *g_loc, *g_s, *ls, *variance, *alpha;
  int n_ls, D, Q, blocks, pairs, splits, rec_dim;
  int64_t N, M, steps, steps_per_split;
  double *a_rec, *b_rec;      // [J, pairs, splits, rec_dim, rec_dim], [blocks, splits, rec_dim, Q]
};

template <typename T, template <typename> class FAM, int TM>
__global__ __launch_bounds__(GPS_THREADS) void gp_cond_gram_kernel(const GpcGramArgs<T> a) {
  constexpr int NB = TM / GPS_SUB, NT = NB * NB / 4, QG = GPS_THREADS / TM, NQ = GPS_MAX_Q / QG;
  extern __shared__ __attribute__((aligned(16))) unsigned char gpc_lds[];
  const int D = a.D, Q = a.Q, Jn = Q + 1, stride = gps_lds_stride(D);
  double* inv_l = reinterpret_cast<double*>(gpc_lds);      // [D]
  T* xui = reinterpret_cast<T*>(inv_l + D);                // [TM, stride]
  T* xuj = xui + TM * stride;                              // [TM, stride]
  T* xs = xuj + TM * stride;                               // [TN, stride]
  T* ksi = xs + GPS_TN * stride;                           // [TM, KS]: Kuf_I
  T* ksj = ksi + TM * GPS_KS;                              // [TM, KS]: Kuf_J' diag(g_s[:, j])
  T* rs = ksj + TM * GPS_KS;                               // [TN, Q]: g_loc
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int unit = (int)(blockIdx.x / a.splits), split = (int)(blockIdx.x - (unsigned)unit * a.splits);
  const int j = unit / a.pairs, pair = unit - j * a.pairs;
  int I = 0, rem = pair;
  while (rem >= a.blocks - I) rem -= a.blocks - I, ++I;
  const int Jb = I + rem;
  const bool diag = I == Jb, with_b = diag && j == 0;
  gps_stage(a.xu, (int64_t)I * TM, a.M, TM, D, stride, xui);
  if (!diag) gps_stage(a.xu, (int64_t)Jb * TM, a.M, TM, D, stride, xuj);
  for (int k = tid; k < D; k += GPS_THREADS) inv_l[k] = 1.0 / (double)a.ls[a.n_ls == 1 ? 0 : k];
  const T var = a.variance[0], alpha = a.alpha ? a.alpha[0] : T(1);
  GpsAcc<T> acc[NT];
#pragma unroll
  for (int u = 0; u < NT; ++u) gps_clear(acc[u]);
  double bacc[NQ];
#pragma unroll
  for (int u = 0; u < NQ; ++u) bacc[u] = 0.0;
  const int rd = a.rec_dim;
  double* rec = a.a_rec + (((int64_t)j * a.pairs + pair) * a.splits + split) * rd * rd;
  bool flushed = false;
  auto flush = [&]() {
#pragma unroll
    for (int u = 0; u < NT; ++u) {
      const int t = wave * NT + u, rb = t / NB, cb = t - rb * NB;
#pragma unroll
      for (int v = 0; v < 16; ++v) {
        const int li = rb * GPS_SUB + gps_row(v, lane), lj = cb * GPS_SUB + (lane & 31);
        if (li < rd && lj < rd) rec[li * rd + lj] = (flushed ? rec[li * rd + lj] : 0.0) + (double)acc[u].c[v];
      }
      gps_clear(acc[u]);
    }
    flushed = true;
  };
  const int p = tid & 31, row0 = tid >> 5;      // generation: point p, rows row0 + 8 e
  const int brow = tid % TM, bq0 = tid / TM;    // ga: row brow, columns bq0 + QG u
  int64_t s_end = (int64_t)(split + 1) * a.steps_per_split;
  if (s_end > a.steps) s_end = a.steps;
  int since = 0;
  for (int64_t s = (int64_t)split * a.steps_per_split; s < s_end; ++s) {
    const int64_t n0 = s * GPS_TN;
    __syncthreads();      // the previous step's reads of xs, rs and the Kuf tiles are over
    gps_stage(a.x, n0, a.N, GPS_TN, D, stride, xs);
    if (with_b) gps_stage(a.g_loc, n0, a.N, GPS_TN, Q, Q, rs);
    __syncthreads();
    const bool p_in = n0 + p < a.N;
    const T gw = p_in ? a.g_s[(n0 + p) * Jn + j] : T(0);
    for (int e = 0; e < TM / 8; ++e) {
      const int row = row0 + 8 * e;
      T ki = T(0), kj = T(0), df, da;
      if (p_in && (int64_t)I * TM + row < a.M) {
        FAM<T>::eval(gps_r2(xui + row * stride, xs + p * stride, inv_l, D), alpha, ki, df, da);
        ki *= var;
      }
      ksi[row * GPS_KS + p] = ki;
      if (diag) {
        kj = ki;
      } else if (p_in && (int64_t)Jb * TM + row < a.M) {
        FAM<T>::eval(gps_r2(xuj + row * stride, xs + p * stride, inv_l, D), alpha, kj, df, da);
        kj *= var;
      }
      ksj[row * GPS_KS + p] = kj * gw;
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < NT; ++u) {
      const int t = wave * NT + u, rb = t / NB, cb = t - rb * NB;
      if ((int64_t)I * TM + rb * GPS_SUB >= a.M || (int64_t)Jb * TM + cb * GPS_SUB >= a.M) continue;      // (wave-uniform)
      gpc_mac<T, false>(acc[u], ksi + rb * GPS_SUB * GPS_KS, GPS_KS, 1, GPS_SUB, nullptr, 0, ksj + cb * GPS_SUB * GPS_KS, 1,
                        GPS_KS, GPS_TN, true, lane);
    }
    if (with_b) {
#pragma unroll
      for (int u = 0; u < NQ; ++u) {
        const int q = bq0 + QG * u;
        if (q >= Q) continue;
        T sum = T(0);      // 32 products in the tensor's dtype, then float64
        for (int pp = 0; pp < GPS_TN; ++pp) sum += ksi[brow * GPS_KS + pp] * rs[pp * Q + q];
        bacc[u] += (double)sum;
      }
    }
    since += GPS_TN;
    if (since >= GPS_FLUSH && s + 1 < s_end) flush(), since = 0;
  }
  flush();
  if (with_b && brow < rd) {
    double* brec = a.b_rec + ((int64_t)I * a.splits + split) * rd * Q;
#pragma unroll
    for (int u = 0; u < NQ; ++u) {
      const int q = bq0 + QG * u;
      if (q < Q) brec[brow * Q + q] = bacc[u];
    }
  }
}

// records -> Aw (both triangles of every Aw_j from the upper one; left in float64: the caller's P_j Aw_j is a sum of M
// signed terms) and ga, float64 sums over the splits in order
template <typename T>
__global__ __launch_bounds__(GPS_THREADS) void gp_cond_gram_fin_kernel(const double* __restrict__ a_rec,
                                                                       const double* __restrict__ b_rec, double* __restrict__ Aw,
                                                                       T* __restrict__ ga, int M, int Q, int tm, int blocks,
                                                                       int pairs, int splits, int rd, int a_blocks) {
  if ((int)blockIdx.x < a_blocks) {
    const int64_t e = (int64_t)blockIdx.x * GPS_THREADS + threadIdx.x;
    if (e >= (int64_t)(Q + 1) * M * M) return;
    const int j = (int)(e / ((int64_t)M * M)), ij = (int)(e - (int64_t)j * M * M);
    int i = ij / M, c = ij - i * M;
    if (i > c) {
      const int t = i;
      i = c, c = t;
    }
    const int I = i / tm, Jb = c / tm;
    const int pair = I * blocks - I * (I - 1) / 2 + (Jb - I);
    const double* rec = a_rec + ((int64_t)j * pairs + pair) * splits * rd * rd + (i - I * tm) * rd + (c - Jb * tm);
    double s = 0.0;
    for (int sp = 0; sp < splits; ++sp) s += rec[(int64_t)sp * rd * rd];
    Aw[e] = s;
    return;
  }
  const int e = ((int)blockIdx.x - a_blocks) * GPS_THREADS + threadIdx.x;
  if (e >= M * Q) return;
  const int i = e / Q, q = e - i * Q, I = i / tm;
  const double* rec = b_rec + (int64_t)I * splits * rd * Q + (i - I * tm) * Q + q;
  double s = 0.0;
  for (int sp = 0; sp < splits; ++sp) s += rec[(int64_t)sp * rd * Q];
  ga[e] = (T)s;
}

// ---- backward, launch two: the chain through variance f'(r2) --------------------------------------------------------
template <typename T>
struct GpcChainArgs {
  const T *x, *xu, *a, *B2, *g_loc, *g_s, *ls, *variance, *alpha;      // B2 [J, M, M] = 2 P_j^T P_j (symmetric)
  int n_ls, D, Q, M, splits;
  int want_rows, want_ls, want_scalars, want_gx;
  int64_t N, steps, steps_per_split;
  double *row_rec, *sc_rec, *gx_rec;      // [splits, M, D], [workgroups, SCALARS + D], [chunks, N, D]
};

template <typename T, template <typename> class FAM>
__global__ __launch_bounds__(GPS_THREADS) void gp_cond_chain_kernel(const GpcChainArgs<T> a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char gpc_lds[];
  __shared__ double red[GPS_THREADS / 64];
  const int D = a.D, Q = a.Q, J = Q + 1, M = a.M, stride = gps_lds_stride(D);
  const int ks_rows = (M > GPS_BWD_ROWS ? M : GPS_BWD_ROWS) + 1;
  double* inv_l = reinterpret_cast<double*>(gpc_lds);      // [D]
  double* acc = inv_l + D;                                 // [BWD_ROWS, D]
  double* ls_acc = acc + GPS_BWD_ROWS * D;                 // [waves, D]
  T* ks = reinterpret_cast<T*>(ls_acc + (GPS_THREADS / 64) * D);      // [ks_rows, KS]: Kuf[:, step], later w of the chunk
  T* xs = ks + ks_rows * GPS_KS;                           // [TN, stride]
  T* gl = xs + GPS_TN * stride;                            // [TN, Q]: g_loc
  T* gw = gl + GPS_TN * Q;                                 // [TN, J]: g_s
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, col = lane & 31;
  const int chunk = (int)(blockIdx.x / a.splits), split = (int)(blockIdx.x - (unsigned)chunk * a.splits);
  const int c0 = chunk * GPS_BWD_ROWS, i0 = c0 + wave * GPS_SUB, i = i0 + col;
  const bool wave_on = i0 < M, row_ok = i < M;
  const int rows_here = M - c0 < GPS_BWD_ROWS ? M - c0 : GPS_BWD_ROWS;
  const T* xu_i = a.xu + (int64_t)(row_ok ? i : M - 1) * D;
  for (int k = tid; k < D; k += GPS_THREADS) inv_l[k] = 1.0 / (double)a.ls[a.n_ls == 1 ? 0 : k];
  for (int e = tid; e < GPS_BWD_ROWS * D + (GPS_THREADS / 64) * D; e += GPS_THREADS) acc[e] = 0.0;
  const T var = a.variance[0], alpha = a.alpha ? a.alpha[0] : T(1);
  const bool ard = a.want_ls && a.n_ls != 1;
  const int p = tid & 31, g8 = tid >> 5;
  double s_var = 0.0, s_alpha = 0.0, s_ls = 0.0;
  int64_t s_end = (int64_t)(split + 1) * a.steps_per_split;
  if (s_end > a.steps) s_end = a.steps;
  for (int64_t s = (int64_t)split * a.steps_per_split; s < s_end; ++s) {
    const int64_t n0 = s * GPS_TN;
    __syncthreads();      // the previous step's reads of ks, xs, gl, gw are over
    gps_stage(a.x, n0, a.N, GPS_TN, D, stride, xs);
    gps_stage(a.g_loc, n0, a.N, GPS_TN, Q, Q, gl);
    gps_stage(a.g_s, n0, a.N, GPS_TN, J, J, gw);
    __syncthreads();
    const bool p_in = n0 + p < a.N;
    for (int jr = g8; jr < M; jr += 8) {
      T f = T(0), df, da;
      if (p_in) {
        FAM<T>::eval(gps_r2(a.xu + (int64_t)jr * D, xs + p * stride, inv_l, D), alpha, f, df, da);
        f *= var;
      }
      ks[jr * GPS_KS + p] = f;
    }
    __syncthreads();
    T w[16];
    if (wave_on) {
      // G^T [32 points, 32 rows] = sum_j diag(g_s[step, j]) Kuf[:, step]^T B2_j[:, rows] + g_loc[step] a[rows]^T
      GpsAcc<T> g;
      gps_clear(g);
      for (int j = 0; j < J; ++j)
        gpc_mac<T, true>(g, ks, 1, GPS_KS, GPS_TN, gw + j, J, a.B2 + (int64_t)j * M * M + i0, M, 1, M, row_ok, lane);
      gpc_mac<T, false>(g, gl, Q, 1, GPS_TN, nullptr, 0, a.a + (int64_t)i0 * Q, 1, Q, Q, row_ok, lane);
      T t_var = T(0), t_alpha = T(0), t_ls = T(0);
#pragma unroll
      for (int v = 0; v < 16; ++v) {
        const int pv = gps_row(v, lane);
        const T gv = (row_ok && n0 + pv < a.N) ? g.c[v] : T(0);      // padded entries weigh nothing
        const double r2 = gps_r2(xu_i, xs + pv * stride, inv_l, D);
        T f, df, da;
        FAM<T>::eval(r2, alpha, f, df, da);
        w[v] = gv * var * df;
        t_var += gv * f;
        t_alpha += gv * da;
        t_ls += w[v] * (T)r2;
      }
      s_var += (double)t_var, s_alpha += (double)t_alpha, s_ls += (double)t_ls;
      if (a.want_rows || ard) {
        for (int k = 0; k < D; ++k) {
          const T il = (T)inv_l[k], xi = xu_i[k];
          T sum = T(0), q2 = T(0);
#pragma unroll
          for (int v = 0; v < 16; ++v) {
            const T d = (xi - xs[gps_row(v, lane) * stride + k]) * il;
            sum += w[v] * d;
            q2 += w[v] * d * d;
          }
          if (a.want_rows) {
            sum += __shfl_xor(sum, 32);
            if (lane < 32 && row_ok) acc[(i - c0) * D + k] += (double)sum;      // one writer per entry
          }
          if (ard) {
            const T total = wave_sum(q2);
            if (lane == 0) ls_acc[wave * D + k] += (double)total;
          }
        }
      }
    } else {
#pragma unroll
      for (int v = 0; v < 16; ++v) w[v] = T(0);
    }
    if (a.want_gx) {      // (uniform over the workgroup)
      __syncthreads();    // every read of Kuf[:, step] is over: the tile now carries w of the chunk's rows
#pragma unroll
      for (int v = 0; v < 16; ++v) ks[(wave * GPS_SUB + col) * GPS_KS + gps_row(v, lane)] = w[v];
      __syncthreads();
      if (p_in) {
        for (int k = g8; k < D; k += 8) {
          const double il = inv_l[k];
          const T xv = xs[p * stride + k];
          double sum = 0.0;
          for (int li = 0; li < rows_here; ++li)
            sum += (double)(ks[li * GPS_KS + p] * ((a.xu[(int64_t)(c0 + li) * D + k] - xv) * (T)il));
          a.gx_rec[((int64_t)chunk * a.N + n0 + p) * D + k] = sum;
        }
      }
    }
  }
  __syncthreads();
  if (a.want_rows) {
    double* rec = a.row_rec + ((int64_t)split * M + c0) * D;
    for (int e = tid; e < rows_here * D; e += GPS_THREADS) rec[e] = acc[e];
  }
  if (a.want_scalars) {
    double* sc = a.sc_rec + (int64_t)blockIdx.x * (GPS_SCALARS + D);
    const double v0 = block_sum_f64_waves(s_var, red, GPS_THREADS / 64);
    const double v1 = block_sum_f64_waves(s_alpha, red, GPS_THREADS / 64);
    const double v2 = block_sum_f64_waves(s_ls, red, GPS_THREADS / 64);
    if (tid == 0) sc[0] = v0, sc[1] = v1, sc[2] = v2;
    if (ard)
      for (int k = tid; k < D; k += GPS_THREADS)
        sc[GPS_SCALARS + k] = (ls_acc[k] + ls_acc[D + k]) + (ls_acc[2 * D + k] + ls_acc[3 * D + k]);
  }
}

// records -> gradients, float64 sums in a fixed order.  Blocks [0, xu_blocks): gxu[i, k] = (2 variance / l_k) sum over
// the splits; [.., + x_blocks): gx[n, k] = -(2 variance / l_k) sum over the chunks; then one block per reduced output:
// lengthscale (n_ls of them), variance, alpha.  w carries the variance already (w = G variance f').
template <typename T>
struct GpcFinArgs {
  const double *row_rec, *sc_rec, *gx_rec;
  const T *ls, *variance;
  int n_ls, D, M, splits, chunks;
  int64_t N, workgroups, xu_blocks, x_blocks;
  T *gxu, *gx, *g_ls, *g_var, *g_alpha;
};

template <typename T>
__global__ __launch_bounds__(GPS_THREADS) void gp_cond_chain_fin_kernel(const GpcFinArgs<T> a) {
  __shared__ double red[GPS_THREADS / 64];
  const int64_t blk = blockIdx.x;
  if (blk < a.xu_blocks) {
    const int64_t e = blk * GPS_THREADS + threadIdx.x, total = (int64_t)a.M * a.D;
    if (e >= total) return;
    double s = 0.0;
    for (int sp = 0; sp < a.splits; ++sp) s += a.row_rec[(int64_t)sp * total + e];
    a.gxu[e] = (T)(2.0 / (double)a.ls[a.n_ls == 1 ? 0 : (int)(e % a.D)] * s);
    return;
  }
  if (blk < a.xu_blocks + a.x_blocks) {
    const int64_t e = (blk - a.xu_blocks) * GPS_THREADS + threadIdx.x, total = a.N * a.D;
    if (e >= total) return;
    double s = 0.0;
    for (int c = 0; c < a.chunks; ++c) s += a.gx_rec[(int64_t)c * total + e];
    a.gx[e] = (T)(-2.0 / (double)a.ls[a.n_ls == 1 ? 0 : (int)(e % a.D)] * s);
    return;
  }
  const int which = (int)(blk - a.xu_blocks - a.x_blocks);      // 0 .. n_ls - 1: lengthscale; then variance, alpha
  int slot;
  T* out;
  if (which < a.n_ls) slot = a.n_ls == 1 ? 2 : GPS_SCALARS + which, out = a.g_ls ? a.g_ls + which : nullptr;
  else if (which == a.n_ls) slot = 0, out = a.g_var;
  else slot = 1, out = a.g_alpha;
  if (out == nullptr) return;      // (uniform over the block)
  double s = 0.0;
  for (int64_t wg = threadIdx.x; wg < a.workgroups; wg += GPS_THREADS) s += a.sc_rec[wg * (GPS_SCALARS + a.D) + slot];
  s = block_sum_f64_waves(s, red, GPS_THREADS / 64);
  if (threadIdx.x == 0) {
    if (which < a.n_ls) s *= -2.0 / (double)a.ls[which];
    else if (which > a.n_ls) s *= (double)a.variance[0];
    *out = (T)s;
  }
}

// ---- launchers -------------------------------------------------------------------------------------------------------
struct GpcIn {
  const void *x, *xu, *a, *P, *ls, *variance, *alpha, *g_loc, *g_s;      // P: Pt (forward) or B2 (backward)
  int n_ls;
  int64_t N, M;
};

template <typename T, template <typename> class FAM>
static int gpc_fwd_launch(const GpcFwdPlan& pl, const GpcIn& in, void* loc, void* s, hipStream_t st) {
  GpcFwdArgs<T> a;
  a.x = (const T*)in.x, a.xu = (const T*)in.xu, a.a = (const T*)in.a, a.Pt = (const T*)in.P, a.ls = (const T*)in.ls;
  a.variance = (const T*)in.variance, a.alpha = (const T*)in.alpha, a.n_ls = in.n_ls, a.D = pl.D, a.Q = pl.Q;
  a.M = (int)in.M, a.row_blocks = pl.row_blocks, a.N = in.N, a.loc = (T*)loc, a.s = (T*)s;
  return gp_launch("gp_cond_fwd_kernel", gp_cond_fwd_kernel<T, FAM>, pl.workgroups, GPS_THREADS, pl.lds_bytes, st, a);
}

struct GpcBwdOut {
  void *gx, *gxu, *g_ls, *g_var, *g_alpha, *ga, *Aw;
};

template <typename T, template <typename> class FAM>
static int gpc_bwd_launch(const GpcBwdPlan& pl, const GpcIn& in, const GpcBwdOut& o, void* workspace, hipStream_t st) {
  double* ws = (double*)workspace;
  const int64_t N = in.N, M = in.M;
  int rc;
  if (o.ga != nullptr || o.Aw != nullptr) {
    GpcGramArgs<T> a;
    a.x = (const T*)in.x, a.xu = (const T*)in.xu, a.g_loc = (const T*)in.g_loc, a.g_s = (const T*)in.g_s;
    a.ls = (const T*)in.ls, a.variance = (const T*)in.variance, a.alpha = (const T*)in.alpha, a.n_ls = in.n_ls;
    a.D = pl.D, a.Q = pl.Q, a.blocks = pl.blocks, a.pairs = pl.pairs, a.splits = pl.splits1, a.rec_dim = pl.rec_dim;
    a.N = N, a.M = M, a.steps = pl.steps, a.steps_per_split = pl.per_split1;
    a.a_rec = ws, a.b_rec = ws + pl.a_doubles;
    constexpr int TM = sizeof(T) == 4 ? 128 : 64;
    rc = gp_launch("gp_cond_gram_kernel", gp_cond_gram_kernel<T, FAM, TM>, pl.workgroups1, GPS_THREADS, pl.lds1_bytes, st, a);
    if (rc != PA_OK) return rc;
    const int a_blocks = (int)gps_div_up((int64_t)pl.J * M * M, GPS_THREADS);
    const int b_blocks = (int)gps_div_up(M * pl.Q, GPS_THREADS);
    hipLaunchKernelGGL(gp_cond_gram_fin_kernel<T>, dim3((unsigned)(a_blocks + b_blocks)), dim3(GPS_THREADS), 0, st,
                       a.a_rec, a.b_rec, (double*)o.Aw, (T*)o.ga, (int)M, pl.Q, pl.tm, pl.blocks, pl.pairs, pl.splits1,
                       pl.rec_dim, a_blocks);
    rc = check_launch("gp_cond_gram_fin_kernel");
    if (rc != PA_OK) return rc;
  }
  const bool scalars = o.g_ls || o.g_var || o.g_alpha;
  if (!(scalars || o.gx || o.gxu)) return PA_OK;
  GpcChainArgs<T> c;
  c.x = (const T*)in.x, c.xu = (const T*)in.xu, c.a = (const T*)in.a, c.B2 = (const T*)in.P, c.g_loc = (const T*)in.g_loc;
  c.g_s = (const T*)in.g_s, c.ls = (const T*)in.ls, c.variance = (const T*)in.variance, c.alpha = (const T*)in.alpha;
  c.n_ls = in.n_ls, c.D = pl.D, c.Q = pl.Q, c.M = (int)M, c.splits = pl.splits2, c.want_rows = pl.want_gxu ? 1 : 0;
  c.want_ls = o.g_ls ? 1 : 0, c.want_scalars = scalars ? 1 : 0, c.want_gx = pl.want_gx ? 1 : 0, c.N = N;
  c.steps = pl.steps, c.steps_per_split = pl.per_split2;
  c.row_rec = ws + pl.a_doubles + pl.b_doubles, c.sc_rec = c.row_rec + pl.row_doubles;
  c.gx_rec = c.sc_rec + pl.scalar_doubles;
  rc = gp_launch("gp_cond_chain_kernel", gp_cond_chain_kernel<T, FAM>, pl.workgroups2, GPS_THREADS, pl.lds2_bytes, st, c);
  if (rc != PA_OK) return rc;
  GpcFinArgs<T> f;
  f.row_rec = c.row_rec, f.sc_rec = c.sc_rec, f.gx_rec = c.gx_rec, f.ls = c.ls, f.variance = c.variance, f.n_ls = in.n_ls;
  f.D = pl.D, f.M = (int)M, f.splits = pl.splits2, f.chunks = pl.chunks, f.N = N, f.workgroups = pl.workgroups2;
  f.xu_blocks = pl.want_gxu ? gps_div_up(M * pl.D, GPS_THREADS) : 0;
  f.x_blocks = pl.want_gx ? gps_div_up(N * pl.D, GPS_THREADS) : 0;
  f.gxu = (T*)o.gxu, f.gx = (T*)o.gx, f.g_ls = (T*)o.g_ls, f.g_var = (T*)o.g_var, f.g_alpha = (T*)o.g_alpha;
  const int64_t blocks = f.xu_blocks + f.x_blocks + (scalars ? in.n_ls + 2 : 0);
  PA_REQUIRE(blocks <= GPS_MAX_WORKGROUPS, "pa_gp_cond_bwd: finalize grid of %lld blocks", (long long)blocks);
  hipLaunchKernelGGL(gp_cond_chain_fin_kernel<T>, dim3((unsigned)blocks), dim3(GPS_THREADS), 0, st, f);
  return check_launch("gp_cond_chain_fin_kernel");
}

template <typename T>
static int gpc_fwd_family(int family, const GpcFwdPlan& pl, const GpcIn& in, void* loc, void* s, hipStream_t st) {
  GP_FAMILY_DISPATCH(gpc_fwd_launch, pl, in, loc, s, st)
}
template <typename T>
static int gpc_bwd_family(int family, const GpcBwdPlan& pl, const GpcIn& in, const GpcBwdOut& o, void* workspace,
                          hipStream_t st) {
  GP_FAMILY_DISPATCH(gpc_bwd_launch, pl, in, o, workspace, st)
}

static int gpc_check(const char* who, int dtype, int family, const GpcIn& in, int64_t D, int64_t Q) {
  PA_REQUIRE(dtype == PA_F32 || dtype == PA_F64, "%s: dtype %d", who, dtype);
  const size_t elem = dtype == PA_F32 ? 4 : 8;
  PA_REQUIRE(family >= 0 && family < GPS_FAMILIES && in.N >= 0 && in.M >= 0 && in.N < GPS_MAX_POINTS &&
                 (in.n_ls == 1 || in.n_ls == D),
             "%s: family=%d N=%lld M=%lld n_ls=%d", who, family, (long long)in.N, (long long)in.M, in.n_ls);
  if (!gpc_shape_ok(family, in.N, in.M, D, Q, in.n_ls, elem))
    return fail(PA_ERR_UNSUPPORTED, "%s: M=%lld D=%lld Q=%lld outside M <= %d, 1 <= D <= %d, 1 <= Q <= %d", who,
                (long long)in.M, (long long)D, (long long)Q, gps_max_m(elem), GPS_MAX_D, GPS_MAX_Q);
  PA_REQUIRE(in.ls != nullptr && in.variance != nullptr && (in.N == 0 || in.x != nullptr) &&
                 (in.M == 0 || (in.xu != nullptr && in.a != nullptr && in.P != nullptr)),
             "%s: null input", who);
  PA_REQUIRE(family != PA_GP_RATIONAL_QUADRATIC || in.alpha != nullptr, "%s: RationalQuadratic needs scale_mixture", who);
  return PA_OK;
}

}  // namespace pa

extern "C" {

size_t pa_gp_cond_workspace(int dtype, int64_t N, int64_t M, int64_t D, int64_t Q, int want_gx, int want_gxu,
                            int forced_splits) {
  const size_t elem = dtype == PA_F32 ? 4 : 8;
  if (!pa::gpc_shape_ok(0, N, M, D, Q, 1, elem) || N == 0 || M == 0) return 0;
  return pa::gpc_bwd_plan(N, M, (int)D, (int)Q, elem, want_gx != 0, want_gxu != 0, pa::cu_count(), forced_splits).bytes;
}

int pa_gp_cond_fwd(int dtype, int family, const void* x, const void* xu, const void* a, const void* Pt,
                   const void* lengthscale, int n_ls, const void* variance, const void* alpha, void* loc, void* s,
                   int64_t N, int64_t M, int64_t D, int64_t Q, pa_stream_t stream) {
  const pa::GpcIn in = {x, xu, a, Pt, lengthscale, variance, alpha, nullptr, nullptr, n_ls, N, M};
  int rc = pa::gpc_check("pa_gp_cond_fwd", dtype, family, in, D, Q);
  if (rc != PA_OK) return rc;
  if (N == 0 || M == 0) return PA_OK;      // (no launch: the caller fills the zeros)
  PA_REQUIRE(loc != nullptr && s != nullptr, "pa_gp_cond_fwd: null output");
  const size_t elem = dtype == PA_F32 ? 4 : 8;
  const pa::GpcFwdPlan pl = pa::gpc_fwd_plan(N, M, (int)D, (int)Q, elem);
  PA_REQUIRE(pl.workgroups <= pa::GPS_MAX_WORKGROUPS && pl.lds_bytes <= pa::GPC_MAX_LDS, "pa_gp_cond_fwd: inconsistent plan");
  hipStream_t st = pa::as_stream(stream);
  if (dtype == PA_F32) return pa::gpc_fwd_family<float>(family, pl, in, loc, s, st);
  return pa::gpc_fwd_family<double>(family, pl, in, loc, s, st);
}

int pa_gp_cond_bwd(int dtype, int family, const void* x, const void* xu, const void* a, const void* B2,
                   const void* lengthscale, int n_ls, const void* variance, const void* alpha, const void* g_loc,
                   const void* g_s, int64_t N, int64_t M, int64_t D, int64_t Q, void* gx, void* gxu, void* g_lengthscale,
                   void* g_variance, void* g_alpha, void* ga, void* Aw, int forced_splits, void* workspace,
                   size_t workspace_bytes, pa_stream_t stream) {
  const pa::GpcIn in = {x, xu, a, B2, lengthscale, variance, alpha, g_loc, g_s, n_ls, N, M};
  int rc = pa::gpc_check("pa_gp_cond_bwd", dtype, family, in, D, Q);
  if (rc != PA_OK) return rc;
  PA_REQUIRE(g_alpha == nullptr || family == PA_GP_RATIONAL_QUADRATIC, "pa_gp_cond_bwd: g_alpha for family %d", family);
  PA_REQUIRE(forced_splits >= 0, "pa_gp_cond_bwd: forced_splits=%d", forced_splits);
  PA_REQUIRE((ga == nullptr) == (Aw == nullptr), "pa_gp_cond_bwd: ga and Aw come together");
  if (!(gx || gxu || g_lengthscale || g_variance || g_alpha || ga)) return PA_OK;
  if (N == 0 || M == 0) return PA_OK;      // (no launch: the caller fills the zeros)
  PA_REQUIRE(g_loc != nullptr && g_s != nullptr, "pa_gp_cond_bwd: null g_loc or g_s");
  const size_t elem = dtype == PA_F32 ? 4 : 8;
  const pa::GpcBwdPlan pl =
      pa::gpc_bwd_plan(N, M, (int)D, (int)Q, elem, gx != nullptr, gxu != nullptr, pa::cu_count(), forced_splits);
  rc = pa::gp_workspace_check("pa_gp_cond_bwd", workspace, workspace_bytes, pl.bytes);
  if (rc != PA_OK) return rc;
  PA_REQUIRE(pl.workgroups1 <= pa::GPS_MAX_WORKGROUPS && pl.workgroups2 <= pa::GPS_MAX_WORKGROUPS &&
                 pl.lds1_bytes <= pa::GPC_MAX_LDS && pl.lds2_bytes <= pa::GPC_MAX_LDS,
             "pa_gp_cond_bwd: inconsistent plan");
  const pa::GpcBwdOut o = {gx, gxu, g_lengthscale, g_variance, g_alpha, ga, Aw};
  hipStream_t st = pa::as_stream(stream);
  if (dtype == PA_F32) return pa::gpc_bwd_family<float>(family, pl, in, o, workspace, st);
  return pa::gpc_bwd_family<double>(family, pl, in, o, workspace, st);
}

}  // extern "C"
