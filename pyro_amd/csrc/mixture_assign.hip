// mixture_assign.hip -- which component does each row of a plated mixture belong to: the most probable one, or one
// drawn from the row's posterior, in one pass over the data.
//
// Reference path replaced: infer_discrete on a plated mixture (pyro/infer/discrete.py _sample_posterior_from_trace):
// the enumerated Categorical's [K, N] log-probabilities and the observed site's [K, N] log_prob are added, and the map
// / sample einsum backends (pyro/ops/einsum/torch_map.py, torch_sample.py) reduce the [K, N] frame over K by argmax
// or by a Categorical draw from its softmax.
//
// Here, for every parameter set b and row n, with t_k = a[b][n][k] + log p(x[n] | p0[b][k], p1[b][k]):
//   mode 0:  z[b][n] = the smallest k with t_k = max_k t_k;
//   mode 1:  z[b][n] = the smallest k with c_k > u c_{K-1}, where e_k = exp(t_k - max_k t_k), c_k = e_0 + .. + e_k
//            added in index order (a sequence that never decreases, whatever the rounding) and u = element b N + n of
//            the Philox uniform stream (seed, offset) in x's dtype -- the mapping of pa_philox_uniform --, clamped to
//            the largest k with e_k > 0 (u c_{K-1} may round up to c_{K-1}).
// A row without a finite maximum to speak of -- every term -inf, or a NaN among them -- gets 0.
// Lane layout (mixture_lanes.h): KP lanes hold one row's K terms, 64 / KP rows per wave and iteration, four
// iterations' loads in flight; the lane that owns k = 0 writes the row's z.  Nothing of size K N exists, nothing is
// reduced across rows: one launch, no workspace, bit-reproducible.
#include "common.h"
#include "dist_fam.h"
#include "mixture_lanes.h"
#include "mixture_assign.h"

namespace pa {

constexpr int MIXA_U = 4;     // iterations whose loads of x and a are requested together

// one row's component from its KP lanes' terms (t = -inf on padded lanes); every lane of the row returns it.
// Indices travel as T through the DPP all-reduce (<= 64: exact).
template <int KP, typename T>
__device__ __forceinline__ int mixa_row(T t, bool kok, int k, int K, int lane, int mode, T u) {
  const T ninf = -t_inf<T>();
  const T m = mix_allreduce<KP>(t, [](T p, T q) { return mixa_max(p, q); });
  if (mode == 0) {
    const T first = mix_allreduce<KP>((kok && t == m) ? T(k) : T(KP), [](T p, T q) { return mixa_min(p, q); });
    return first < T(K) ? (int)first : 0;            // (a NaN maximum equals no term)
  }
  const bool dead = m != m || m == ninf;
  const T e = (dead || !kok) ? T(0) : (t == m ? T(1) : t_exp(t - m));
  // c_k = e_0 + .. + e_k in index order: lane k takes the first k + 1 of the row's values as they are handed round
  T c = T(0);
  const int first_lane = lane & ~(KP - 1);
  for (int j = 0; j < K; ++j) {                      // (K: wave-uniform)
    const T ej = __shfl(e, first_lane + j, 64);
    c += j <= k ? ej : T(0);
  }
  const T thr = u * __shfl(c, first_lane + K - 1, 64);
  const T first = mix_allreduce<KP>((kok && c > thr) ? T(k) : T(KP), [](T p, T q) { return mixa_min(p, q); });
  const T last = mix_allreduce<KP>((kok && e > T(0)) ? T(k) : T(-1), [](T p, T q) { return mix_max(p, q); });
  const int zi = (int)mixa_min(first, last);
  return (dead || zi < 0) ? 0 : zi;
}

template <int DIST, typename T, int KP>
__global__ __launch_bounds__(MIX_THREADS) void mixture_assign_kernel(const T* __restrict__ x, int64_t N, int K,
                                                                     const T* __restrict__ a, int64_t a_sk,
                                                                     int64_t a_sn, int64_t a_bs,
                                                                     const T* __restrict__ p0, int64_t s0,
                                                                     const T* __restrict__ p1, int64_t s1,
                                                                     int64_t p0_bs, int64_t p1_bs, int mode,
                                                                     uint64_t seed, uint64_t offset,
                                                                     const uint64_t* __restrict__ offset_dev,
                                                                     int64_t* __restrict__ z) {
  // blockIdx.y: one of B parameter sets over the SAME data
  a += (int64_t)blockIdx.y * a_bs;
  p0 += (int64_t)blockIdx.y * p0_bs;
  if (p1 != nullptr) p1 += (int64_t)blockIdx.y * p1_bs;
  z += (int64_t)blockIdx.y * N;
  if (offset_dev) offset += *offset_dev;
  constexpr int RPW = 64 / KP;                     // rows per wave and iteration
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int k = lane & (KP - 1), slot = lane / KP;
  const bool kok = k < K;
  const T ninf = -t_inf<T>();
  const int64_t a_k = kok ? (int64_t)k * a_sk : 0;
  const T p0k = p0[kok ? (int64_t)k * s0 : 0];
  const T p1k = p1 != nullptr ? p1[kok ? (int64_t)k * s1 : 0] : T(0);
  const int64_t step = (int64_t)gridDim.x * (MIX_THREADS / 64) * RPW;
  for (int64_t base0 = ((int64_t)blockIdx.x * (MIX_THREADS / 64) + wave) * RPW; base0 < N; base0 += MIXA_U * step) {
    T xs[MIXA_U], as[MIXA_U];
#pragma unroll
    for (int u = 0; u < MIXA_U; ++u) {
      const int64_t row = base0 + u * step + slot;
      const int64_t rc = row < N ? row : N - 1;      // (a row past the end reads the last one and writes nothing)
      xs[u] = x[rc];
      as[u] = a[rc * a_sn + a_k];
    }
#pragma unroll
    for (int u = 0; u < MIXA_U; ++u) {
      const int64_t base = base0 + u * step;
      if (base >= N) break;                          // (wave-uniform)
      const int64_t row = base + slot;
      const bool valid = row < N;
      const T t = kok ? as[u] + Fam<DIST, T>::lp(xs[u], p0k, p1k) : ninf;
      const T un = mode == 0 ? T(0)
                             : mixa_uniform(T(0), seed, offset, (uint64_t)blockIdx.y * (uint64_t)N +
                                                                    (uint64_t)(valid ? row : N - 1));
      const int zi = mixa_row<KP>(t, kok, k, K, lane, mode, un);
      if (valid && k == 0) z[row] = (int64_t)zi;
    }
  }
}

// ---- a diagonal Normal over D <= 8 features: the features of a row stay with the lane that holds (row, k) ---------
template <typename T, int KP, int DD>
__global__ __launch_bounds__(MIX_THREADS) void mixture_assign_diag_kernel(const T* __restrict__ x, int64_t N, int D,
                                                                          int K, const T* __restrict__ a,
                                                                          int64_t a_sk, int64_t a_sn, int64_t a_bs,
                                                                          const T* __restrict__ loc, int64_t l_sk,
                                                                          int64_t l_sd, int64_t l_bs,
                                                                          const T* __restrict__ scl, int64_t s_sk,
                                                                          int64_t s_sd, int64_t s_bs, int mode,
                                                                          uint64_t seed, uint64_t offset,
                                                                          const uint64_t* __restrict__ offset_dev,
                                                                          int64_t* __restrict__ z) {
  a += (int64_t)blockIdx.y * a_bs;
  loc += (int64_t)blockIdx.y * l_bs;
  scl += (int64_t)blockIdx.y * s_bs;
  z += (int64_t)blockIdx.y * N;
  if (offset_dev) offset += *offset_dev;
  constexpr int RPW = 64 / KP;
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
  const int64_t step = (int64_t)gridDim.x * (MIX_THREADS / 64) * RPW;
  for (int64_t base0 = ((int64_t)blockIdx.x * (MIX_THREADS / 64) + wave) * RPW; base0 < N; base0 += MIXA_U * step) {
    T xs[MIXA_U][DD], as[MIXA_U];
#pragma unroll
    for (int u = 0; u < MIXA_U; ++u) {
      const int64_t row = base0 + u * step + slot;
      const int64_t rc = row < N ? row : N - 1;
      const T* xr = x + rc * D;
#pragma unroll
      for (int d = 0; d < DD; ++d) xs[u][d] = xr[d < D ? d : 0];
      as[u] = a[rc * a_sn + a_k];
    }
#pragma unroll
    for (int u = 0; u < MIXA_U; ++u) {
      const int64_t base = base0 + u * step;
      if (base >= N) break;                          // (wave-uniform)
      const int64_t row = base + slot;
      const bool valid = row < N;
      T q = T(0);
#pragma unroll
      for (int d = 0; d < DD; ++d) {
        const T zd = d < D ? (xs[u][d] - mu[d]) * inv[d] : T(0);    // (nothing past D, whatever x[row][0] is)
        q += zd * zd;
      }
      const T t = kok ? as[u] + ck - T(0.5) * q : ninf;
      const T un = mode == 0 ? T(0)
                             : mixa_uniform(T(0), seed, offset, (uint64_t)blockIdx.y * (uint64_t)N +
                                                                    (uint64_t)(valid ? row : N - 1));
      const int zi = mixa_row<KP>(t, kok, k, K, lane, mode, un);
      if (valid && k == 0) z[row] = (int64_t)zi;
    }
  }
}

static int mixa_kp(int K) {
  int KP = 1;
  while (KP < K) KP <<= 1;
  return KP;
}

// workgroups per parameter set: >= 8 iterations per wave, at most four workgroups per CU over all sets
static int mixa_grid(int64_t N, int KP, int64_t B) {
  const int64_t rows_per_block = (int64_t)(MIX_THREADS / 64) * (64 / KP);
  int64_t g = (N + rows_per_block * 8 - 1) / (rows_per_block * 8);
  int64_t cap = ((int64_t)cu_count() * 4 + B - 1) / B;
  if (cap < 1) cap = 1;
  if (g > cap) g = cap;
  return (int)(g < 1 ? 1 : g);
}

template <int DIST, typename T>
static int mixture_assign_launch(const T* x, int64_t N, int K, int64_t B, const T* a, int64_t a_sk, int64_t a_sn,
                                 int64_t a_bs, const T* p0, int64_t s0, const T* p1, int64_t s1, int64_t p0_bs,
                                 int64_t p1_bs, int mode, uint64_t seed, uint64_t offset, const uint64_t* offset_dev,
                                 int64_t* z, hipStream_t s) {
  const int KP = mixa_kp(K);
  const int grid = mixa_grid(N, KP, B);
#define PA_MIXA_CASE(KP_)                                                                              \
  if (KP == KP_)                                                                                       \
    hipLaunchKernelGGL((mixture_assign_kernel<DIST, T, KP_>), dim3((unsigned)grid, (unsigned)B),       \
                       dim3(MIX_THREADS), 0, s, x, N, K, a, a_sk, a_sn, a_bs, p0, s0, p1, s1, p0_bs,   \
                       p1_bs, mode, seed, offset, offset_dev, z);
  PA_MIXA_CASE(1) PA_MIXA_CASE(2) PA_MIXA_CASE(4) PA_MIXA_CASE(8) PA_MIXA_CASE(16) PA_MIXA_CASE(32) PA_MIXA_CASE(64)
#undef PA_MIXA_CASE
  return check_launch("mixture_assign_kernel");
}

template <typename T>
static int mixture_assign_t(int dist, const T* x, int64_t N, int K, int64_t B, const T* a, int64_t a_sk, int64_t a_sn,
                            int64_t a_bs, const T* p0, int64_t s0, const T* p1, int64_t s1, int64_t p0_bs,
                            int64_t p1_bs, int mode, uint64_t seed, uint64_t offset, const uint64_t* offset_dev,
                            int64_t* z, hipStream_t s) {
#define PA_MIXA_FAM(ID)                                                                                \
  case ID:                                                                                             \
    return mixture_assign_launch<ID, T>(x, N, K, B, a, a_sk, a_sn, a_bs, p0, s0, p1, s1, p0_bs, p1_bs, mode, seed, \
                                        offset, offset_dev, z, s);
  switch (dist) {
    PA_MIXA_FAM(PA_DIST_NORMAL)
    PA_MIXA_FAM(PA_DIST_LOG_NORMAL)
    PA_MIXA_FAM(PA_DIST_EXPONENTIAL)
    PA_MIXA_FAM(PA_DIST_BERNOULLI_LOGITS)
    PA_MIXA_FAM(PA_DIST_POISSON)
    PA_MIXA_FAM(PA_DIST_GAMMA)
    default: return fail(PA_ERR_UNSUPPORTED, "mixture_assign: distribution id %d not implemented", dist);
  }
#undef PA_MIXA_FAM
}

static bool mixture_assign_family(int dist) {
  return dist == PA_DIST_NORMAL || dist == PA_DIST_LOG_NORMAL || dist == PA_DIST_EXPONENTIAL ||
         dist == PA_DIST_BERNOULLI_LOGITS || dist == PA_DIST_POISSON || dist == PA_DIST_GAMMA;
}

template <typename T, int KP>
static int mixture_assign_diag_launch(const T* x, int64_t N, int D, int K, int64_t B, const T* a, int64_t a_sk,
                                      int64_t a_sn, int64_t a_bs, const T* loc, int64_t l_sk, int64_t l_sd,
                                      int64_t l_bs, const T* scl, int64_t s_sk, int64_t s_sd, int64_t s_bs, int mode,
                                      uint64_t seed, uint64_t offset, const uint64_t* offset_dev, int64_t* z,
                                      hipStream_t s) {
  const int DD = D <= 2 ? 2 : D <= 4 ? 4 : 8;
  const int grid = mixa_grid(N, KP, B);
#define PA_MIXAD_CASE(DD_)                                                                             \
  if (DD == DD_)                                                                                       \
    hipLaunchKernelGGL((mixture_assign_diag_kernel<T, KP, DD_>), dim3((unsigned)grid, (unsigned)B),    \
                       dim3(MIX_THREADS), 0, s, x, N, D, K, a, a_sk, a_sn, a_bs, loc, l_sk, l_sd, l_bs, scl, s_sk, \
                       s_sd, s_bs, mode, seed, offset, offset_dev, z);
  PA_MIXAD_CASE(2) PA_MIXAD_CASE(4) PA_MIXAD_CASE(8)
#undef PA_MIXAD_CASE
  return check_launch("mixture_assign_diag_kernel");
}

template <typename T>
static int mixture_assign_diag_t(const T* x, int64_t N, int D, int K, int64_t B, const T* a, int64_t a_sk,
                                 int64_t a_sn, int64_t a_bs, const T* loc, int64_t l_sk, int64_t l_sd, int64_t l_bs,
                                 const T* scl, int64_t s_sk, int64_t s_sd, int64_t s_bs, int mode, uint64_t seed,
                                 uint64_t offset, const uint64_t* offset_dev, int64_t* z, hipStream_t s) {
  const int KP = mixa_kp(K);
#define PA_MIXAD_K(KP_)                                                                                \
  if (KP == KP_)                                                                                       \
    return mixture_assign_diag_launch<T, KP_>(x, N, D, K, B, a, a_sk, a_sn, a_bs, loc, l_sk, l_sd, l_bs, scl, s_sk, \
                                              s_sd, s_bs, mode, seed, offset, offset_dev, z, s);
  PA_MIXAD_K(1) PA_MIXAD_K(2) PA_MIXAD_K(4) PA_MIXAD_K(8) PA_MIXAD_K(16) PA_MIXAD_K(32) PA_MIXAD_K(64)
#undef PA_MIXAD_K
  return fail(PA_ERR_UNSUPPORTED, "mixture_assign_diag_normal: K=%d", K);
}

}  // namespace pa

extern "C" {

int pa_mixture_assign(int dtype, int dist, const void* x, int64_t N, int K, int64_t B, const void* a,
                      int64_t a_stride_k, int64_t a_stride_n, int64_t a_batch_stride, const void* p0,
                      int64_t p0_stride, int64_t p0_batch_stride, const void* p1, int64_t p1_stride,
                      int64_t p1_batch_stride, int mode, uint64_t seed, uint64_t offset, const uint64_t* offset_dev,
                      int64_t* z, pa_stream_t stream) {
  if (K < 1 || K > pa::MIX_MAXK || B < 1 || B > 65535 || !pa::mixture_assign_family(dist) ||
      (dtype != PA_F32 && dtype != PA_F64))
    return pa::fail(PA_ERR_UNSUPPORTED, "mixture_assign: K=%d (1..%d), B=%lld (1..65535), family %d, dtype %d", K,
                    pa::MIX_MAXK, (long long)B, dist, dtype);
  PA_REQUIRE(mode == 0 || mode == 1, "mixture_assign: mode %d (0: most probable, 1: draw)", mode);
  PA_REQUIRE(N >= 1 && x && a && p0 && z, "mixture_assign: NULL pointer or N < 1");
  PA_REQUIRE(a_stride_k >= 0 && a_stride_n >= 0 && a_batch_stride >= 0 && p0_stride >= 0 && p1_stride >= 0 &&
                 p0_batch_stride >= 0 && p1_batch_stride >= 0, "mixture_assign: negative stride");
  PA_REQUIRE(pa::dist_nparams(dist) == 1 || p1 != nullptr, "mixture_assign: the family takes two parameters");
  hipStream_t s = pa::as_stream(stream);
  if (dtype == PA_F32)
    return pa::mixture_assign_t<float>(dist, (const float*)x, N, K, B, (const float*)a, a_stride_k, a_stride_n,
                                       a_batch_stride, (const float*)p0, p0_stride, (const float*)p1, p1_stride,
                                       p0_batch_stride, p1_batch_stride, mode, seed, offset, offset_dev, z, s);
  return pa::mixture_assign_t<double>(dist, (const double*)x, N, K, B, (const double*)a, a_stride_k, a_stride_n,
                                      a_batch_stride, (const double*)p0, p0_stride, (const double*)p1, p1_stride,
                                      p0_batch_stride, p1_batch_stride, mode, seed, offset, offset_dev, z, s);
}

int pa_mixture_assign_diag_normal(int dtype, const void* x, int64_t N, int D, int K, int64_t B, const void* a,
                                  int64_t a_stride_k, int64_t a_stride_n, int64_t a_batch_stride, const void* loc,
                                  int64_t loc_stride_k, int64_t loc_stride_d, int64_t loc_batch_stride,
                                  const void* scale, int64_t scale_stride_k, int64_t scale_stride_d,
                                  int64_t scale_batch_stride, int mode, uint64_t seed, uint64_t offset,
                                  const uint64_t* offset_dev, int64_t* z, pa_stream_t stream) {
  if (K < 1 || K > pa::MIX_MAXK || D < 1 || D > 8 || B < 1 || B > 65535 || (dtype != PA_F32 && dtype != PA_F64))
    return pa::fail(PA_ERR_UNSUPPORTED,
                    "mixture_assign_diag_normal: K=%d (1..%d), D=%d (1..8), B=%lld (1..65535), dtype %d", K,
                    pa::MIX_MAXK, D, (long long)B, dtype);
  PA_REQUIRE(mode == 0 || mode == 1, "mixture_assign_diag_normal: mode %d (0: most probable, 1: draw)", mode);
  PA_REQUIRE(N >= 1 && x && a && loc && scale && z, "mixture_assign_diag_normal: NULL pointer or N < 1");
  PA_REQUIRE(a_stride_k >= 0 && a_stride_n >= 0 && a_batch_stride >= 0 && loc_stride_k >= 0 && loc_stride_d >= 0 &&
                 loc_batch_stride >= 0 && scale_stride_k >= 0 && scale_stride_d >= 0 && scale_batch_stride >= 0,
             "mixture_assign_diag_normal: negative stride");
  hipStream_t s = pa::as_stream(stream);
  if (dtype == PA_F32)
    return pa::mixture_assign_diag_t<float>((const float*)x, N, D, K, B, (const float*)a, a_stride_k, a_stride_n,
                                            a_batch_stride, (const float*)loc, loc_stride_k, loc_stride_d,
                                            loc_batch_stride, (const float*)scale, scale_stride_k, scale_stride_d,
                                            scale_batch_stride, mode, seed, offset, offset_dev, z, s);
  return pa::mixture_assign_diag_t<double>((const double*)x, N, D, K, B, (const double*)a, a_stride_k, a_stride_n,
                                           a_batch_stride, (const double*)loc, loc_stride_k, loc_stride_d,
                                           loc_batch_stride, (const double*)scale, scale_stride_k, scale_stride_d,
                                           scale_batch_stride, mode, seed, offset, offset_dev, z, s);
}

}  // extern "C"
