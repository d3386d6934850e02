// mixture_rows.hip -- the mixture leaf of mixture.hip when the assignment's log-weights differ from row to row.
//
// Reference path replaced: TraceEnum_ELBO on a plated mixture whose enumerated Categorical has per-row probabilities
// (a gating network `Categorical(logits=X @ W + b)`, grouped weights `Categorical(theta[group])`, soft or one-hot
// labels): pyro/infer/traceenum_elbo.py:112-214 adds the site's [K, N] log-probabilities
// (pyro/poutine/trace_struct.py:248-288) to the observed site's [K, N] log_prob, reduces by logsumexp over K
// (pyro/ops/contract.py:79-160 -> pyro/ops/einsum/torch_log.py:14-55) and sums over the plate; autograd keeps the
// [K, N] frame and walks it again for every operand.
//
// Here:   S[b] = sum_n log sum_k exp(a[b][n][k] + log p(x_n | p0[b][k], p1[b][k]))
// and in the same pass
//         dS/da[b][n][k] = r_nk  (written once, in a's dtype; not at all when the caller passes no buffer),
//         dS/dp0[b][k] = sum_n r_nk d log p / d p0,   dS/dp1[b][k] likewise.
// With per-row weights a K N input and a K N output are intrinsic: a is read once, x is read once, r is written once.
// Lane layout (mixture_lanes.h): KP lanes hold one row's K terms, 64 / KP rows per wave and iteration.  The
// Categorical's own factor is a transposed view of row-major [N, K] logits (strides k: 1, n: K): consecutive lanes
// then read consecutive addresses of a, and write consecutive addresses of the row-major r.  Any other non-negative
// strides are correct but uncoalesced.
// Reduction: S and the parameter gradients per lane in T, across lanes and waves in double, workgroup (wave)
// partials added in a fixed order by a second small launch (bit-reproducible).
#include "common.h"
#include "dist_fam.h"
#include "mixture_lanes.h"

namespace pa {

constexpr int MIXR_U = 4;     // iterations whose loads of x and a are requested together

// (mix_row of mixture_lanes.h: a row whose every term is -inf has lse = -inf and r = 0; a NaN term makes lse and every
//  r of the row NaN)

template <int DIST, typename T, int KP>
__global__ __launch_bounds__(MIX_THREADS) void mixture_rows_kernel(const T* __restrict__ x, int64_t N, int K,
                                                                   const T* __restrict__ a, int64_t a_sk,
                                                                   int64_t a_sn, int64_t a_bs,
                                                                   const T* __restrict__ p0, int64_t s0,
                                                                   const T* __restrict__ p1, int64_t s1,
                                                                   int64_t p0_bs, int64_t p1_bs,
                                                                   T* __restrict__ da, double* __restrict__ partial) {
  // blockIdx.y: one of B parameter sets over the SAME data
  a += (int64_t)blockIdx.y * a_bs;
  p0 += (int64_t)blockIdx.y * p0_bs;
  if (p1 != nullptr) p1 += (int64_t)blockIdx.y * p1_bs;
  if (da != nullptr) da += (int64_t)blockIdx.y * N * K;       // r[b][n][k], row-major
  constexpr int RPW = 64 / KP;                     // rows per wave and iteration
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int k = lane & (KP - 1), slot = lane / KP;
  const bool kok = k < K;
  const T ninf = -t_inf<T>();
  const int64_t a_k = kok ? (int64_t)k * a_sk : 0;
  const T p0k = p0[kok ? (int64_t)k * s0 : 0];
  const T p1k = p1 != nullptr ? p1[kok ? (int64_t)k * s1 : 0] : T(0);
  T acc_s = T(0), acc_0 = T(0), acc_1 = T(0);
  const int64_t step = (int64_t)gridDim.x * (MIX_THREADS / 64) * RPW;
  // (a wave's iteration reads 64 values of a and 64 / KP of x: four iterations' loads are requested together,
  //  otherwise every iteration waits out a memory round trip)
  for (int64_t base0 = ((int64_t)blockIdx.x * (MIX_THREADS / 64) + wave) * RPW; base0 < N; base0 += MIXR_U * step) {
    T xs[MIXR_U], as[MIXR_U];
#pragma unroll
    for (int u = 0; u < MIXR_U; ++u) {
      const int64_t row = base0 + u * step + slot;
      const int64_t rc = row < N ? row : N - 1;
      xs[u] = x[rc];
      as[u] = a[rc * a_sn + a_k];
    }
#pragma unroll
    for (int u = 0; u < MIXR_U; ++u) {
      const int64_t base = base0 + u * step;
      if (base >= N) break;                          // (wave-uniform)
      const int64_t row = base + slot;
      const bool valid = row < N;
      const T xv = xs[u];
      const T t = kok ? as[u] + Fam<DIST, T>::lp(xv, p0k, p1k) : ninf;
      T lse, r;
      mix_row<KP>(t, kok, lse, r);
      if (!valid) r = T(0);
      if (da != nullptr && valid && kok) da[row * K + k] = r;
      T dv, g0, g1;
      Fam<DIST, T>::grad(xv, p0k, p1k, dv, g0, g1);
      acc_s += (valid && k == 0) ? lse : T(0);
      // (r == 0 exactly: no gradient, whatever the family's derivative is there; a NaN r is handed on)
      acc_0 += r == T(0) ? T(0) : r * g0;
      acc_1 += r == T(0) ? T(0) : r * g1;
    }
  }
  // lanes of the same k (the wave's RPW row slots), in double
  double ds = (double)acc_s, ds0 = (double)acc_0, ds1 = (double)acc_1;
#pragma unroll
  for (int o = KP; o < 64; o <<= 1) {
    ds += __shfl_xor(ds, o, 64);
    ds0 += __shfl_xor(ds0, o, 64);
    ds1 += __shfl_xor(ds1, o, 64);
  }
  __shared__ double red[MIX_THREADS / 64][3][MIX_MAXK];
  if (lane < KP) {
    red[wave][0][lane] = ds;
    red[wave][1][lane] = ds0;
    red[wave][2][lane] = ds1;
  }
  __syncthreads();
  // partial[block][0] = sum of the rows' logsumexp; [1 + q * KP + k], q = 0, 1: the two gradient sums
  constexpr int J = 1 + 2 * KP;
  for (int j = threadIdx.x; j < J; j += MIX_THREADS) {
    const int q = j == 0 ? 0 : 1 + (j - 1) / KP, kk = j == 0 ? 0 : (j - 1) % KP;
    double v = 0.0;
#pragma unroll
    for (int w = 0; w < MIX_THREADS / 64; ++w) v += red[w][q][kk];
    partial[((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * J + j] = v;
  }
}

// ---- a diagonal Normal over D <= 8 features inside the logsumexp (mixture_diag_kernel with per-row weights) -------
// The features of a row stay with the lane that holds (row, k); every WAVE writes its own partial.  Partial / padded
// output layout per set: [0] = S, [1 + k * DD + d] = dS/dloc_kd, [1 + KP * DD + k * DD + d] = dS/dscale_kd.
template <typename T, int KP, int DD>
__global__ __launch_bounds__(MIX_THREADS) void mixture_rows_diag_kernel(const T* __restrict__ x, int64_t N, int D,
                                                                        int K, const T* __restrict__ a,
                                                                        int64_t a_sk, int64_t a_sn, int64_t a_bs,
                                                                        const T* __restrict__ loc, int64_t l_sk,
                                                                        int64_t l_sd, int64_t l_bs,
                                                                        const T* __restrict__ scl, int64_t s_sk,
                                                                        int64_t s_sd, int64_t s_bs,
                                                                        T* __restrict__ da,
                                                                        double* __restrict__ partial) {
  a += (int64_t)blockIdx.y * a_bs;
  loc += (int64_t)blockIdx.y * l_bs;
  scl += (int64_t)blockIdx.y * s_bs;
  if (da != nullptr) da += (int64_t)blockIdx.y * N * K;
  constexpr int RPW = 64 / KP;
  constexpr int JP = 1 + 2 * KP * DD;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int k = lane & (KP - 1), slot = lane / KP;
  const bool kok = k < K;
  const T ninf = -t_inf<T>();
  const int64_t a_k = kok ? (int64_t)k * a_sk : 0;
  T mu[DD], inv[DD];
  T ck = T(0);                                      // - sum_d log scale_d - D / 2 log 2 pi
#pragma unroll
  for (int d = 0; d < DD; ++d) {
    const bool dok = d < D;
    mu[d] = loc[(kok ? (int64_t)k * l_sk : 0) + (dok ? (int64_t)d * l_sd : 0)];
    const T sg = scl[(kok ? (int64_t)k * s_sk : 0) + (dok ? (int64_t)d * s_sd : 0)];
    inv[d] = dok ? pos_rcp(sg) : T(0);
    if (dok) ck -= pos_log(sg) + Consts<T>::half_log_2pi;
  }
  T acc_s = T(0), acc_l[DD], acc_c[DD];
#pragma unroll
  for (int d = 0; d < DD; ++d) acc_l[d] = acc_c[d] = T(0);
  const int64_t nwaves = (int64_t)gridDim.x * (MIX_THREADS / 64);
  const int64_t step = nwaves * RPW;
  for (int64_t base0 = ((int64_t)blockIdx.x * (MIX_THREADS / 64) + wave) * RPW; base0 < N; base0 += MIXR_U * step) {
    T xs[MIXR_U][DD], as[MIXR_U];
#pragma unroll
    for (int u = 0; u < MIXR_U; ++u) {
      const int64_t row = base0 + u * step + slot;
      const int64_t rc = row < N ? row : N - 1;
      const T* xr = x + rc * D;
#pragma unroll
      for (int d = 0; d < DD; ++d) xs[u][d] = xr[d < D ? d : 0];
      as[u] = a[rc * a_sn + a_k];
    }
#pragma unroll
    for (int u = 0; u < MIXR_U; ++u) {
      const int64_t base = base0 + u * step;
      if (base >= N) break;                          // (wave-uniform)
      const int64_t row = base + slot;
      const bool valid = row < N;
      T z[DD];
      T q = T(0);
#pragma unroll
      for (int d = 0; d < DD; ++d) {
        z[d] = d < D ? (xs[u][d] - mu[d]) * inv[d] : T(0);       // (nothing past D, whatever x[row][0] is)
        q += z[d] * z[d];
      }
      const T t = kok ? as[u] + ck - T(0.5) * q : ninf;
      T lse, r;
      mix_row<KP>(t, kok, lse, r);
      if (!valid) r = T(0);
      if (da != nullptr && valid && kok) da[row * K + k] = r;
      acc_s += (valid && k == 0) ? lse : T(0);
      // (r == 0 exactly: no gradient, whatever z is there; a NaN r is handed on)
      const bool none = r == T(0);
#pragma unroll
      for (int d = 0; d < DD; ++d) {
        const T w = r * inv[d];
        acc_l[d] += none ? T(0) : w * z[d];                        // r (x - loc) / scale^2
        acc_c[d] += none ? T(0) : w * (z[d] * z[d] - T(1));        // r ((x - loc)^2 / scale^2 - 1) / scale
      }
    }
  }
  const int64_t gw = (int64_t)blockIdx.x * (MIX_THREADS / 64) + wave;
  double* out = partial + ((int64_t)blockIdx.y * nwaves + gw) * JP;
  auto over_slots = [&](T v) {
    double dv = (double)v;
#pragma unroll
    for (int o = KP; o < 64; o <<= 1) dv += __shfl_xor(dv, o, 64);
    return dv;
  };
  const double ds = over_slots(acc_s);
  if (lane == 0) out[0] = ds;
#pragma unroll
  for (int d = 0; d < DD; ++d) {
    const double dl = over_slots(acc_l[d]), dc = over_slots(acc_c[d]);
    if (lane < KP) {
      out[1 + lane * DD + d] = dl;
      out[1 + KP * DD + lane * DD + d] = dc;
    }
  }
}

// out[b][j] = the partials added in index order (16 segments per output in parallel, eight loads in flight).  A copy
// of mixture_sum_partials_kernel of mixture.hip: without relocatable device code a launch cannot cross the files.
__global__ __launch_bounds__(1024) void mixture_rows_sum_partials_kernel(const double* __restrict__ partial,
                                                                         int nparts, int J,
                                                                         double* __restrict__ out) {
  __shared__ double seg[16][64];
  const int jj = threadIdx.x & 63, sg = threadIdx.x >> 6;
  const int j = blockIdx.x * 64 + jj;
  partial += (int64_t)blockIdx.y * nparts * J;
  out += (int64_t)blockIdx.y * J;
  double v = 0.0;
  if (j < J) {
    const int per = (nparts + 15) / 16;
    const int b0 = sg * per, b1 = b0 + per < nparts ? b0 + per : nparts;
    int b = b0;
    for (; b + 8 <= b1; b += 8) {
      double q[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) q[u] = partial[(int64_t)(b + u) * J + j];
#pragma unroll
      for (int u = 0; u < 8; ++u) v += q[u];
    }
    for (; b < b1; ++b) v += partial[(int64_t)b * J + j];
  }
  seg[sg][jj] = v;
  __syncthreads();
  if (sg == 0 && j < J) {
    double t = 0.0;
#pragma unroll
    for (int q = 0; q < 16; ++q) t += seg[q][jj];
    out[j] = t;
  }
}

static int mixr_kp(int K) {
  int KP = 1;
  while (KP < K) KP <<= 1;
  return KP;
}

// workgroups per parameter set: >= 8 iterations per wave, at most `per_cu` workgroups per CU over all sets
static int mixr_grid(int64_t N, int KP, int64_t B, int per_cu) {
  const int64_t rows_per_block = (int64_t)(MIX_THREADS / 64) * (64 / KP);
  int64_t g = (N + rows_per_block * 8 - 1) / (rows_per_block * 8);
  int64_t cap = ((int64_t)cu_count() * per_cu + B - 1) / B;
  if (cap < 1) cap = 1;
  if (g > cap) g = cap;
  return (int)(g < 1 ? 1 : g);
}

template <int DIST, typename T>
static int mixture_rows_launch(const T* x, int64_t N, int K, int64_t B, const T* a, int64_t a_sk, int64_t a_sn,
                               int64_t a_bs, const T* p0, int64_t s0, const T* p1, int64_t s1, int64_t p0_bs,
                               int64_t p1_bs, T* da, double* partial, double* out, hipStream_t s) {
  const int KP = mixr_kp(K);
  const int grid = mixr_grid(N, KP, B, 4);
#define PA_MIXR_CASE(KP_)                                                                              \
  if (KP == KP_)                                                                                       \
    hipLaunchKernelGGL((mixture_rows_kernel<DIST, T, KP_>), dim3((unsigned)grid, (unsigned)B),         \
                       dim3(MIX_THREADS), 0, s, x, N, K, a, a_sk, a_sn, a_bs, p0, s0, p1, s1, p0_bs,   \
                       p1_bs, da, partial);
  PA_MIXR_CASE(1) PA_MIXR_CASE(2) PA_MIXR_CASE(4) PA_MIXR_CASE(8) PA_MIXR_CASE(16) PA_MIXR_CASE(32) PA_MIXR_CASE(64)
#undef PA_MIXR_CASE
  const int J = 1 + 2 * KP;
  hipLaunchKernelGGL(mixture_rows_sum_partials_kernel, dim3((unsigned)((J + 63) / 64), (unsigned)B), dim3(1024), 0,
                     s, partial, grid, J, out);
  return check_launch("mixture_rows_kernel");
}

template <typename T>
static int mixture_rows_t(int dist, const T* x, int64_t N, int K, int64_t B, const T* a, int64_t a_sk, int64_t a_sn,
                          int64_t a_bs, const T* p0, int64_t s0, const T* p1, int64_t s1, int64_t p0_bs,
                          int64_t p1_bs, T* da, double* partial, double* out, hipStream_t s) {
#define PA_MIXR_FAM(ID)                                                                                \
  case ID:                                                                                             \
    return mixture_rows_launch<ID, T>(x, N, K, B, a, a_sk, a_sn, a_bs, p0, s0, p1, s1, p0_bs, p1_bs, da, partial, \
                                      out, s);
  switch (dist) {
    PA_MIXR_FAM(PA_DIST_NORMAL)
    PA_MIXR_FAM(PA_DIST_LOG_NORMAL)
    PA_MIXR_FAM(PA_DIST_EXPONENTIAL)
    PA_MIXR_FAM(PA_DIST_BERNOULLI_LOGITS)
    PA_MIXR_FAM(PA_DIST_POISSON)
    PA_MIXR_FAM(PA_DIST_GAMMA)
    default: return fail(PA_ERR_UNSUPPORTED, "mixture_rows_fwd_bwd: distribution id %d not implemented", dist);
  }
#undef PA_MIXR_FAM
}

static bool mixture_rows_family(int dist) {
  return dist == PA_DIST_NORMAL || dist == PA_DIST_LOG_NORMAL || dist == PA_DIST_EXPONENTIAL ||
         dist == PA_DIST_BERNOULLI_LOGITS || dist == PA_DIST_POISSON || dist == PA_DIST_GAMMA;
}

template <typename T, int KP>
static int mixture_rows_diag_launch(const T* x, int64_t N, int D, int K, int64_t B, const T* a, int64_t a_sk,
                                    int64_t a_sn, int64_t a_bs, const T* loc, int64_t l_sk, int64_t l_sd,
                                    int64_t l_bs, const T* scl, int64_t s_sk, int64_t s_sd, int64_t s_bs, T* da,
                                    double* partial, double* out, hipStream_t s) {
  const int DD = D <= 2 ? 2 : D <= 4 ? 4 : 8;
  const int grid = mixr_grid(N, KP, B, 2);         // (every wave writes a partial: fewer, longer waves)
  const int nparts = grid * (MIX_THREADS / 64);
  const int JP = 1 + 2 * KP * DD;
#define PA_MIXRD_CASE(DD_)                                                                             \
  if (DD == DD_)                                                                                       \
    hipLaunchKernelGGL((mixture_rows_diag_kernel<T, KP, DD_>), dim3((unsigned)grid, (unsigned)B),      \
                       dim3(MIX_THREADS), 0, s, x, N, D, K, a, a_sk, a_sn, a_bs, loc, l_sk, l_sd, l_bs, scl, s_sk, \
                       s_sd, s_bs, da, partial);
  PA_MIXRD_CASE(2) PA_MIXRD_CASE(4) PA_MIXRD_CASE(8)
#undef PA_MIXRD_CASE
  hipLaunchKernelGGL(mixture_rows_sum_partials_kernel, dim3((unsigned)((JP + 63) / 64), (unsigned)B), dim3(1024), 0,
                     s, partial, nparts, JP, out);
  return check_launch("mixture_rows_diag_kernel");
}

template <typename T>
static int mixture_rows_diag_t(const T* x, int64_t N, int D, int K, int64_t B, const T* a, int64_t a_sk,
                               int64_t a_sn, int64_t a_bs, const T* loc, int64_t l_sk, int64_t l_sd, int64_t l_bs,
                               const T* scl, int64_t s_sk, int64_t s_sd, int64_t s_bs, T* da, double* partial,
                               double* out, hipStream_t s) {
  const int KP = mixr_kp(K);
#define PA_MIXRD_K(KP_)                                                                                \
  if (KP == KP_)                                                                                       \
    return mixture_rows_diag_launch<T, KP_>(x, N, D, K, B, a, a_sk, a_sn, a_bs, loc, l_sk, l_sd, l_bs, scl, s_sk, \
                                            s_sd, s_bs, da, partial, out, s);
  PA_MIXRD_K(1) PA_MIXRD_K(2) PA_MIXRD_K(4) PA_MIXRD_K(8) PA_MIXRD_K(16) PA_MIXRD_K(32) PA_MIXRD_K(64)
#undef PA_MIXRD_K
  return fail(PA_ERR_UNSUPPORTED, "mixture_rows_diag_normal_fwd_bwd: K=%d", K);
}

}  // namespace pa

extern "C" {

int pa_mixture_rows_layout(int K, int* kp_out) {
  if (K < 1 || K > pa::MIX_MAXK) return 0;
  const int KP = pa::mixr_kp(K);
  if (kp_out) *kp_out = KP;
  return 1 + 2 * KP;
}

size_t pa_mixture_rows_workspace(int K, int64_t B) {
  if (K < 1 || K > pa::MIX_MAXK || B < 1 || B > 65535) return 0;
  // (at most cu_count * 4 + B workgroups over all parameter sets)
  return ((size_t)pa::cu_count() * 4 + (size_t)B) * (size_t)(1 + 2 * pa::mixr_kp(K)) * sizeof(double);
}

int pa_mixture_rows_fwd_bwd(int dtype, int dist, const void* x, int64_t N, int K, int64_t B, const void* a,
                            int64_t a_stride_k, int64_t a_stride_n, int64_t a_batch_stride, const void* p0,
                            int64_t p0_stride, int64_t p0_batch_stride, const void* p1, int64_t p1_stride,
                            int64_t p1_batch_stride, void* da, void* workspace, size_t workspace_bytes,
                            double* out_padded, pa_stream_t stream) {
  if (K < 1 || K > pa::MIX_MAXK || B < 1 || B > 65535 || !pa::mixture_rows_family(dist) ||
      (dtype != PA_F32 && dtype != PA_F64))
    return pa::fail(PA_ERR_UNSUPPORTED, "mixture_rows_fwd_bwd: K=%d (1..%d), B=%lld (1..65535), family %d, dtype %d",
                    K, pa::MIX_MAXK, (long long)B, dist, dtype);
  PA_REQUIRE(N >= 1 && x && a && p0 && out_padded && workspace, "mixture_rows_fwd_bwd: NULL pointer or N < 1");
  PA_REQUIRE(a_stride_k >= 0 && a_stride_n >= 0 && a_batch_stride >= 0 && p0_stride >= 0 && p1_stride >= 0 &&
                 p0_batch_stride >= 0 && p1_batch_stride >= 0, "mixture_rows_fwd_bwd: negative stride");
  PA_REQUIRE(workspace_bytes >= pa_mixture_rows_workspace(K, B), "mixture_rows_fwd_bwd: workspace too small");
  PA_REQUIRE(pa::dist_nparams(dist) == 1 || p1 != nullptr, "mixture_rows_fwd_bwd: the family takes two parameters");
  hipStream_t s = pa::as_stream(stream);
  if (dtype == PA_F32)
    return pa::mixture_rows_t<float>(dist, (const float*)x, N, K, B, (const float*)a, a_stride_k, a_stride_n,
                                     a_batch_stride, (const float*)p0, p0_stride, (const float*)p1, p1_stride,
                                     p0_batch_stride, p1_batch_stride, (float*)da, (double*)workspace, out_padded, s);
  return pa::mixture_rows_t<double>(dist, (const double*)x, N, K, B, (const double*)a, a_stride_k, a_stride_n,
                                    a_batch_stride, (const double*)p0, p0_stride, (const double*)p1, p1_stride,
                                    p0_batch_stride, p1_batch_stride, (double*)da, (double*)workspace, out_padded, s);
}

static int mixture_rows_diag_padded(int K, int D, int* kp, int* dd) {
  const int KP = pa::mixr_kp(K);
  const int DD = D <= 2 ? 2 : D <= 4 ? 4 : 8;
  if (kp) *kp = KP;
  if (dd) *dd = DD;
  return 1 + 2 * KP * DD;
}

int pa_mixture_rows_diag_normal_layout(int K, int D, int* kp_out, int* dd_out) {
  if (K < 1 || K > pa::MIX_MAXK || D < 1 || D > 8) return 0;
  return mixture_rows_diag_padded(K, D, kp_out, dd_out);
}

size_t pa_mixture_rows_diag_normal_workspace(int K, int D, int64_t B) {
  if (K < 1 || K > pa::MIX_MAXK || D < 1 || D > 8 || B < 1 || B > 65535) return 0;
  const int JP = mixture_rows_diag_padded(K, D, nullptr, nullptr);
  return ((size_t)pa::cu_count() * 2 + (size_t)B) * (pa::MIX_THREADS / 64) * (size_t)JP * sizeof(double);
}

int pa_mixture_rows_diag_normal_fwd_bwd(int dtype, const void* x, int64_t N, int D, int K, int64_t B, const void* a,
                                        int64_t a_stride_k, int64_t a_stride_n, int64_t a_batch_stride,
                                        const void* loc, int64_t loc_stride_k, int64_t loc_stride_d,
                                        int64_t loc_batch_stride, const void* scale, int64_t scale_stride_k,
                                        int64_t scale_stride_d, int64_t scale_batch_stride, void* da,
                                        void* workspace, size_t workspace_bytes, double* out_padded,
                                        pa_stream_t stream) {
  if (K < 1 || K > pa::MIX_MAXK || D < 1 || D > 8 || B < 1 || B > 65535 || (dtype != PA_F32 && dtype != PA_F64))
    return pa::fail(PA_ERR_UNSUPPORTED,
                    "mixture_rows_diag_normal_fwd_bwd: K=%d (1..%d), D=%d (1..8), B=%lld (1..65535), dtype %d", K,
                    pa::MIX_MAXK, D, (long long)B, dtype);
  PA_REQUIRE(N >= 1 && x && a && loc && scale && out_padded && workspace,
             "mixture_rows_diag_normal_fwd_bwd: NULL pointer or N < 1");
  PA_REQUIRE(a_stride_k >= 0 && a_stride_n >= 0 && a_batch_stride >= 0 && loc_stride_k >= 0 && loc_stride_d >= 0 &&
                 loc_batch_stride >= 0 && scale_stride_k >= 0 && scale_stride_d >= 0 && scale_batch_stride >= 0,
             "mixture_rows_diag_normal_fwd_bwd: negative stride");
  PA_REQUIRE(workspace_bytes >= pa_mixture_rows_diag_normal_workspace(K, D, B),
             "mixture_rows_diag_normal_fwd_bwd: workspace too small");
  hipStream_t s = pa::as_stream(stream);
  if (dtype == PA_F32)
    return pa::mixture_rows_diag_t<float>((const float*)x, N, D, K, B, (const float*)a, a_stride_k, a_stride_n,
                                          a_batch_stride, (const float*)loc, loc_stride_k, loc_stride_d,
                                          loc_batch_stride, (const float*)scale, scale_stride_k, scale_stride_d,
                                          scale_batch_stride, (float*)da, (double*)workspace, out_padded, s);
  return pa::mixture_rows_diag_t<double>((const double*)x, N, D, K, B, (const double*)a, a_stride_k, a_stride_n,
                                         a_batch_stride, (const double*)loc, loc_stride_k, loc_stride_d,
                                         loc_batch_stride, (const double*)scale, scale_stride_k, scale_stride_d,
                                         scale_batch_stride, (double*)da, (double*)workspace, out_padded, s);
}

}  // extern "C"
