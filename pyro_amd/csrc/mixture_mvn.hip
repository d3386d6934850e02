// mixture_mvn.hip -- the mixture leaf for a full-covariance MultivariateNormal observation, without the [K, N, D]
// frame.
//
// Reference path replaced: TraceEnum_ELBO on `MultivariateNormal(locs[z], scale_tril=L[z])` observed under the data
// plate (pyro/infer/traceenum_elbo.py:112-214, pyro/ops/contract.py:79-160): torch's MultivariateNormal.log_prob
// forms diff = x - loc as a [K, N, D] tensor, runs a batched triangular solve over it, adds the log-determinant, and
// the sum-product takes logsumexp over K and the plate sum; autograd keeps and walks those [K, N, D] tensors again.
//
// Here, per parameter set b (vectorised particles / chains), with W_k = L_k^-1 (lower triangular), d = x_n - mu_k
// formed per component BEFORE the product (W x - W mu cancels when |x| >> the spread), z = W_k d:
//   t_nk = a_k + sum_i log W_k,ii - D/2 log 2 pi - |z|^2 / 2,      S = sum_n logsumexp_k t_nk
// and, with r_nk = softmax_k t_nk, the statistics every gradient follows from (torch takes the chain rule on the
// tiny [B, K, D, D] results):
//   R_k = sum_n r_nk (= dS/da_k),   m_k = sum_n r_nk z_nk,   G_k = sum_n r_nk z_nk d_nk^T (lower triangle).
// The row-tile kernel accumulates C_k = sum_n r_nk d_nk d_nk^T (symmetric: the lower triangle only) and
// s_k = sum_n r_nk d_nk; the last launch forms m_k = W_k s_k and G_k = W_k C_k in double.
//
// Three launches:
//   1. lse:      one thread per row; W_k, mu_k and the constant of each k staged in LDS (every lane reads the same
//                word: a broadcast), z = W d on the VALU in registers, the row's logsumexp online.  Writes the row's
//                logsumexp (B N values of the input dtype: the only per-row buffer) and one double per workgroup.
//   2. stats:    one workgroup per (row chunk, k, b); recomputes t_nk, r_nk = exp(t_nk - lse_n), stages r and d of a
//                tile of TR rows in LDS (column-major, padded), then 136 threads each own a TB x TB block of the
//                lower triangle of C (TB = DP / 16), DP threads own s and one owns R.  Per-tile sums in the input
//                dtype, across tiles in double.  One record of 1 + DP + DP^2 doubles per workgroup.
//   3. finalize: per (k, b) the records added in chunk order, then m = W s and G = W C; block (0, b) adds the
//                lse partials in order.  No atomics anywhere: two runs give identical bits.
// Nothing of size K N is written.  D is padded to DP in {8, 16, 32, 64} with zeros; the rows past D are skipped.
//
// Workspace (pa_mixture_mvn_workspace(K, D, B)), in doubles:
//   B * G1(B) + B * K * C(K, B) * (1 + DP + DP^2),   G1(B) = max(1, ceil(2048 / B)),  C(K, B) = max(1, ceil(1024 / (K B)))
// i.e. at most (2048 + B) + (1024 + K B)(1 + DP + DP^2) doubles: 34.1 MB at K = D = 64, B = 1.  The launch
// takes G1 and C no larger than that (fewer for small N) and checks that its records fit.
//
// Matrix cores: not used yet -- every D runs on the VALU (FMAs with W broadcast from LDS), so there is no D crossover
// in this version.  Measured, N = 1e6, f32, the leaf call alone (three launches, workspace and wrapper; median of
// 5 blocks of 10 calls), with the fraction of the f32 matrix peak (157.3 TFLOP/s) at 4 N K D^2 FLOP:
//   K = 16: D = 2 0.47 ms, D = 8 0.67 ms (3.9 %), D = 32 3.11 ms (13.4 %), D = 64 16.2 ms (10.3 %);
//   K = 64: D = 32 11.8 ms (14.1 %), D = 64 62.6 ms (10.7 %).
// At D <= 8 the leaf is bound by its launches and the per-k LDS staging, not by the products; from D = 16 on it is
// bound by VALU issue and the LDS reads of W (one ds_read per four FMAs).  An MFMA (f32 32x32x2, exact f32) form of
// both forward products and of the C accumulation is the next step for D >= 16: it would keep this record layout,
// and its gain is bounded by the 10-14 % of peak measured here.
#include "common.h"
#include "dist_fam.h"
#include "mixture_mvn.h"

namespace pa {

template <typename T, int DP>
__global__ __launch_bounds__(MVN_THREADS) void mixture_mvn_lse_kernel(const T* __restrict__ x, int64_t N, int D,
                                                                      int K, const T* __restrict__ a, int64_t a_bs,
                                                                      const T* __restrict__ loc, int64_t l_sk,
                                                                      int64_t l_bs, const T* __restrict__ w,
                                                                      int64_t w_sk, int64_t w_bs,
                                                                      T* __restrict__ lse,
                                                                      double* __restrict__ spart) {
  const int64_t b = blockIdx.y;
  a += b * a_bs;
  loc += b * l_bs;
  w += b * w_bs;
  __shared__ T Ws[DP * DP];
  __shared__ T mus[DP];
  __shared__ T ck[1];
  __shared__ double red[MVN_THREADS / 64];
  const int tid = threadIdx.x;
  const T ninf = -t_inf<T>();
  double acc = 0.0;
  for (int64_t base = (int64_t)blockIdx.x * MVN_THREADS; base < N; base += (int64_t)gridDim.x * MVN_THREADS) {
    const int64_t n = base + tid;
    const bool valid = n < N;
    const T* xr = x + (valid ? n : N - 1) * D;
    T xv[DP];
#pragma unroll
    for (int j = 0; j < DP; ++j) xv[j] = j < D ? xr[j] : T(0);
    T m = ninf, s = T(0);
    for (int k = 0; k < K; ++k) {
      mvn_stage<T, DP>(Ws, mus, ck, a, loc, l_sk, w, w_sk, D, k);
      T d[DP];
#pragma unroll
      for (int j = 0; j < DP; ++j) d[j] = xv[j] - mus[j];
      const T t = ck[0] - T(0.5) * mvn_quad<T, DP>(Ws, d, D);
      // online logsumexp: a term of -inf (a component switched off) adds nothing, NaN propagates
      if (t > m) {
        s = s * t_exp(m - t) + T(1);
        m = t;
      } else if (!(t == ninf)) {
        s += t_exp(t - m);
      }
    }
    const T l = s > T(0) ? m + t_log(s) : (s == T(0) ? ninf : s);
    if (valid) {
      lse[b * N + n] = l;
      acc += (double)l;
    }
  }
  const double tot = block_sum_f64(acc, red);
  if (tid == 0) spart[b * gridDim.x + blockIdx.x] = tot;
}

template <typename T, int DP, int TR>
__global__ __launch_bounds__(MVN_THREADS) void mixture_mvn_stats_kernel(const T* __restrict__ x, int64_t N, int D,
                                                                        int K, const T* __restrict__ a,
                                                                        int64_t a_bs, const T* __restrict__ loc,
                                                                        int64_t l_sk, int64_t l_bs,
                                                                        const T* __restrict__ w, int64_t w_sk,
                                                                        int64_t w_bs, const T* __restrict__ lse,
                                                                        int64_t rows_per, double* __restrict__ rec) {
  constexpr int TB = DP >= 16 ? DP / 16 : 1;        // edge of a thread's block of C
  constexpr int NB = DP / TB;                       // blocks per edge (<= 16)
  constexpr int NLOW = NB * (NB + 1) / 2;           // blocks on or below the diagonal (<= 136)
  constexpr int TRP = TR + 16 / (int)sizeof(T);     // (padded: the rows of dT start in different banks)
  static_assert(NLOW + DP + 1 <= MVN_THREADS && TR <= MVN_THREADS && TR % 4 == 0, "thread roles");
  const int k = blockIdx.y, c = blockIdx.x;
  const int64_t b = blockIdx.z;
  a += b * a_bs;
  loc += b * l_bs;
  w += b * w_bs;
  lse += b * N;
  __shared__ T Ws[DP * DP];
  __shared__ T mus[DP];
  __shared__ T ck[1];
  __shared__ __attribute__((aligned(16))) T dT[DP * TRP];   // d of the tile's rows, [feature][row]
  __shared__ __attribute__((aligned(16))) T rs[TR];         // their responsibilities for k
  mvn_stage<T, DP>(Ws, mus, ck, a, loc, l_sk, w, w_sk, D, k);
  const int tid = threadIdx.x;
  const T ninf = -t_inf<T>();
  int bi = 0, bj = tid;                             // tid < NLOW: block (bi, bj) of C, bj <= bi
  while (bj > bi && bi < NB) bj -= ++bi;
  double cacc[TB][TB];
#pragma unroll
  for (int u = 0; u < TB; ++u)
#pragma unroll
    for (int v = 0; v < TB; ++v) cacc[u][v] = 0.0;
  double sacc = 0.0;                                // s_i (NLOW <= tid < NLOW + DP) or R (tid == NLOW + DP)
  const int64_t r0 = (int64_t)c * rows_per;
  const int64_t r1 = r0 + rows_per < N ? r0 + rows_per : N;
  for (int64_t base = r0; base < r1; base += TR) {
    if (tid < TR) {
      const int64_t n = base + tid;
      const bool valid = n < r1;
      const T* xr = x + (valid ? n : r0) * D;
      T d[DP];
#pragma unroll
      for (int j = 0; j < DP; ++j) d[j] = (j < D ? xr[j] : T(0)) - mus[j];
      const T t = ck[0] - T(0.5) * mvn_quad<T, DP>(Ws, d, D);
      const T l = valid ? lse[n] : ninf;
      // (a row whose every term is -inf has no responsibilities; NaN in a row propagates)
      const T r = l == ninf ? T(0) : t_exp(t - l);
#pragma unroll
      // (r == 0 exactly -- a dead row, a switched-off component: nothing of the row enters C or s, whatever d is
      //  there (0 * inf); a NaN r is handed on)
      for (int j = 0; j < DP; ++j) dT[j * TRP + tid] = (valid && r != T(0)) ? d[j] : T(0);
      rs[tid] = r;
    }
    __syncthreads();
    if (tid < NLOW) {
      T cf[TB][TB];
#pragma unroll
      for (int u = 0; u < TB; ++u)
#pragma unroll
        for (int v = 0; v < TB; ++v) cf[u][v] = T(0);
      for (int n = 0; n < TR; n += 4) {
        T r4[4], di[TB][4], dj[TB][4];
#pragma unroll
        for (int q = 0; q < 4; ++q) r4[q] = rs[n + q];
#pragma unroll
        for (int u = 0; u < TB; ++u)
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            di[u][q] = r4[q] * dT[(bi * TB + u) * TRP + n + q];
            dj[u][q] = dT[(bj * TB + u) * TRP + n + q];
          }
#pragma unroll
        for (int u = 0; u < TB; ++u)
#pragma unroll
          for (int v = 0; v < TB; ++v)
#pragma unroll
            for (int q = 0; q < 4; ++q) cf[u][v] += di[u][q] * dj[v][q];
      }
#pragma unroll
      for (int u = 0; u < TB; ++u)
#pragma unroll
        for (int v = 0; v < TB; ++v) cacc[u][v] += (double)cf[u][v];
    } else if (tid <= NLOW + DP) {
      const int i = tid - NLOW;
      T s = T(0);
      if (i < DP) {
        for (int n = 0; n < TR; ++n) s += rs[n] * dT[i * TRP + n];
      } else {
        for (int n = 0; n < TR; ++n) s += rs[n];
      }
      sacc += (double)s;
    }
    __syncthreads();
  }
  // record [0] = R, [1 + i] = s_i, [1 + DP + i DP + j] = C_ij for the blocks on or below the diagonal
  double* out = rec + (((int64_t)b * K + k) * gridDim.x + c) * mvn_record(DP);
  if (tid < NLOW) {
#pragma unroll
    for (int u = 0; u < TB; ++u)
#pragma unroll
      for (int v = 0; v < TB; ++v) out[1 + DP + (bi * TB + u) * DP + bj * TB + v] = cacc[u][v];
  } else if (tid < NLOW + DP) {
    out[1 + tid - NLOW] = sacc;
  } else if (tid == NLOW + DP) {
    out[0] = sacc;
  }
}

// out[b][0] = S, [1 + k] = R_k, [1 + K + k D + i] = m_ki, [1 + K + K D + (k D + i) D + j] = G_kij (zero above the
// diagonal); the partials added in index order
template <typename T>
__global__ __launch_bounds__(MVN_THREADS) void mixture_mvn_finalize_kernel(const double* __restrict__ spart, int g1,
                                                                           const double* __restrict__ rec,
                                                                           int chunks, int K, int D, int DP,
                                                                           const T* __restrict__ w, int64_t w_sk,
                                                                           int64_t w_bs, double* __restrict__ out) {
  __shared__ double acc[1 + MVN_MAXD + MVN_MAXD * MVN_MAXD];
  __shared__ double red[MVN_THREADS / 64];
  const int k = blockIdx.x, tid = threadIdx.x;
  const int64_t b = blockIdx.y;
  const int J = (int)mvn_record(DP);
  const double* rp = rec + ((int64_t)b * K + k) * chunks * J;
  for (int e = tid; e < J; e += MVN_THREADS) {
    const int q = e - 1 - DP, i = q / DP, j = q % DP;
    if (!(e <= D || (q >= 0 && i < D && j <= i))) continue;
    double v = 0.0;
    for (int cc = 0; cc < chunks; ++cc) v += rp[(int64_t)cc * J + e];
    acc[e] = v;
  }
  __syncthreads();
  const int64_t JO = 1 + K + (int64_t)K * D + (int64_t)K * D * D;
  double* o = out + b * JO;
  const T* wk = w + b * w_bs + (int64_t)k * w_sk;
  if (tid == 0) o[1 + k] = acc[0];
  for (int i = tid; i < D; i += MVN_THREADS) {
    double m = 0.0;
    for (int l = 0; l <= i; ++l) m += (double)wk[i * D + l] * acc[1 + l];
    o[1 + K + (int64_t)k * D + i] = m;
  }
  for (int e = tid; e < D * D; e += MVN_THREADS) {
    const int i = e / D, j = e % D;
    double g = 0.0;
    if (j <= i)
      for (int l = 0; l <= i; ++l) g += (double)wk[i * D + l] * acc[1 + DP + (l >= j ? l * DP + j : j * DP + l)];
    o[1 + K + (int64_t)K * D + (int64_t)k * D * D + e] = g;
  }
  if (k == 0) {
    double v = 0.0;
    for (int q = tid; q < g1; q += MVN_THREADS) v += spart[b * g1 + q];
    v = block_sum_f64(v, red);
    if (tid == 0) o[0] = v;
  }
}

template <typename T, int DP>
static int mixture_mvn_launch(const T* x, int64_t N, int D, int K, int64_t B, const T* a, int64_t a_bs, const T* loc,
                              int64_t l_sk, int64_t l_bs, const T* w, int64_t w_sk, int64_t w_bs, T* row_lse,
                              double* ws, size_t ws_bytes, double* out, hipStream_t s) {
  // (f64 at DP = 64: a 128-row tile keeps the LDS image of d within 64 KB)
  constexpr int TR = (sizeof(T) == 8 && DP == 64) ? 128 : 256;
  int64_t g1 = (N + MVN_THREADS - 1) / MVN_THREADS;
  if (g1 > mvn_lse_blocks_max(B)) g1 = mvn_lse_blocks_max(B);
  int64_t chunks = (N + TR - 1) / TR;
  if (chunks > mvn_chunks_max(K, B)) chunks = mvn_chunks_max(K, B);
  int64_t rows_per = (N + chunks - 1) / chunks;
  rows_per = (rows_per + TR - 1) / TR * TR;
  const int64_t need = (B * g1 + B * K * chunks * mvn_record(DP)) * (int64_t)sizeof(double);
  PA_REQUIRE((size_t)need <= ws_bytes, "mixture_mvn_fwd_bwd: records need %lld bytes, workspace has %zu",
             (long long)need, ws_bytes);
  double* spart = ws;
  double* rec = ws + B * g1;
  hipLaunchKernelGGL((mixture_mvn_lse_kernel<T, DP>), dim3((unsigned)g1, (unsigned)B), dim3(MVN_THREADS), 0, s, x,
                     N, D, K, a, a_bs, loc, l_sk, l_bs, w, w_sk, w_bs, row_lse, spart);
  hipLaunchKernelGGL((mixture_mvn_stats_kernel<T, DP, TR>), dim3((unsigned)chunks, (unsigned)K, (unsigned)B),
                     dim3(MVN_THREADS), 0, s, x, N, D, K, a, a_bs, loc, l_sk, l_bs, w, w_sk, w_bs,
                     (const T*)row_lse, rows_per, rec);
  hipLaunchKernelGGL((mixture_mvn_finalize_kernel<T>), dim3((unsigned)K, (unsigned)B), dim3(MVN_THREADS), 0, s,
                     (const double*)spart, (int)g1, (const double*)rec, (int)chunks, K, D, DP, w, w_sk, w_bs, out);
  return check_launch("mixture_mvn_kernel");
}

template <typename T>
static int mixture_mvn_t(const T* x, int64_t N, int D, int K, int64_t B, const T* a, int64_t a_bs, const T* loc,
                         int64_t l_sk, int64_t l_bs, const T* w, int64_t w_sk, int64_t w_bs, T* row_lse, double* ws,
                         size_t ws_bytes, double* out, hipStream_t s) {
  switch (mvn_padded_d(D)) {
#define PA_MVN_CASE(DP_)                                                                                        \
  case DP_:                                                                                                     \
    return mixture_mvn_launch<T, DP_>(x, N, D, K, B, a, a_bs, loc, l_sk, l_bs, w, w_sk, w_bs, row_lse, ws,      \
                                      ws_bytes, out, s);
    PA_MVN_CASE(8) PA_MVN_CASE(16) PA_MVN_CASE(32) PA_MVN_CASE(64)
#undef PA_MVN_CASE
  }
  return fail(PA_ERR_UNSUPPORTED, "mixture_mvn_fwd_bwd: D=%d", D);
}

}  // namespace pa

extern "C" {

int64_t pa_mixture_mvn_layout(int K, int D) {
  if (K < 1 || K > pa::MVN_MAXK || D < 1 || D > pa::MVN_MAXD) return 0;
  return 1 + K + (int64_t)K * D + (int64_t)K * D * D;
}

size_t pa_mixture_mvn_workspace(int K, int D, int64_t B) {
  if (K < 1 || K > pa::MVN_MAXK || D < 1 || D > pa::MVN_MAXD || B < 1 || B > 65535) return 0;
  const int DP = pa::mvn_padded_d(D);
  return (size_t)(B * pa::mvn_lse_blocks_max(B) + B * K * pa::mvn_chunks_max(K, B) * pa::mvn_record(DP)) *
         sizeof(double);
}

int pa_mixture_mvn_fwd_bwd(int dtype, const void* x, int64_t N, int D, int K, int64_t B, const void* a,
                           int64_t a_batch_stride, const void* loc, int64_t loc_stride_k, int64_t loc_batch_stride,
                           const void* w, int64_t w_stride_k, int64_t w_batch_stride, void* row_lse,
                           void* workspace, size_t workspace_bytes, double* out, pa_stream_t stream) {
  PA_REQUIRE(K >= 1 && K <= pa::MVN_MAXK && D >= 1 && D <= pa::MVN_MAXD,
             "mixture_mvn_fwd_bwd: K=%d (<= %d), D=%d (<= %d)", K, pa::MVN_MAXK, D, pa::MVN_MAXD);
  PA_REQUIRE(B >= 1 && B <= 65535, "mixture_mvn_fwd_bwd: B=%lld outside [1, 65535]", (long long)B);
  PA_REQUIRE(N >= 1 && x && a && loc && w && row_lse && out && workspace,
             "mixture_mvn_fwd_bwd: NULL pointer or N < 1");
  PA_REQUIRE(a_batch_stride >= 0 && loc_stride_k >= 0 && loc_batch_stride >= 0 && w_stride_k >= 0 &&
                 w_batch_stride >= 0, "mixture_mvn_fwd_bwd: negative stride");
  PA_REQUIRE(workspace_bytes >= pa_mixture_mvn_workspace(K, D, B), "mixture_mvn_fwd_bwd: workspace too small");
  hipStream_t s = pa::as_stream(stream);
  if (dtype == PA_F32)
    return pa::mixture_mvn_t<float>((const float*)x, N, D, K, B, (const float*)a, a_batch_stride,
                                    (const float*)loc, loc_stride_k, loc_batch_stride, (const float*)w, w_stride_k,
                                    w_batch_stride, (float*)row_lse, (double*)workspace, workspace_bytes, out, s);
  if (dtype == PA_F64)
    return pa::mixture_mvn_t<double>((const double*)x, N, D, K, B, (const double*)a, a_batch_stride,
                                     (const double*)loc, loc_stride_k, loc_batch_stride, (const double*)w,
                                     w_stride_k, w_batch_stride, (double*)row_lse, (double*)workspace,
                                     workspace_bytes, out, s);
  return pa::fail(PA_ERR_UNSUPPORTED, "mixture_mvn_fwd_bwd: dtype %d", dtype);
}

}  // extern "C"
