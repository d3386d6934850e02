// mixture_assign_wide.hip -- which component does each row of a plated mixture belong to, for the two wide leaves:
// an event-shaped element-wise observation `Fam(p0[z], p1[z]).to_event(1)` over D <= 1024 features (the families of
// mixture_event.hip) and a full-covariance MultivariateNormal over D <= 64 features (mixture_mvn.hip).
//
// Reference path replaced: infer_discrete on such a mixture (pyro/infer/discrete.py _sample_posterior_from_trace):
// the observed site's log_prob builds the [K, N, D] frame (torch's Independent.log_prob, or MultivariateNormal's
// diff and batched triangular solve), the enumerated Categorical's log-probabilities are added, and the map / sample
// einsum backends (pyro/ops/einsum/torch_map.py, torch_sample.py) reduce the [K, N] frame over K.
//
// Here, for every parameter set b and row n, with t_k = a[b][k] + log p(x[n] | component k of set b), the rule of
// mixture_assign.hip, decided in double:
//   mode 0:  z[b][n] = the smallest k with t_k = max_k t_k;
//   mode 1:  z[b][n] = the smallest k with c_k > u c_{K-1}, e_k = exp(t_k - max_k t_k), c_k = e_0 + .. + e_k in index
//            order, u = element b N + n of the Philox uniform stream (seed, offset) in x's dtype (mixa_uniform),
//            clamped to the largest k with e_k > 0.
// A row with every term -inf, or a NaN among them, gets 0; rows past N write nothing.
//
// One launch each, one thread per row, rows in tiles of 256, the score pass of the leaves' lse launches:
//   event: c_k = a_k + sum_d kc(p_kd) in double by every workgroup for itself (one wave per component, lanes over
//          the features; what the leaf's prep launch does once: K D evaluations against the 256 K D element terms of
//          a tile), then ev_rows per chunk of 16 components: x and the staged parameters through LDS in chunks of
//          features, t_nk per chunk in the input dtype, across chunks in double;
//   mvn:   mvn_stage / mvn_quad per component: W_k, mu_k and the constant in LDS, d = x - mu before the product, the
//          row's x and d in registers, t_nk in the input dtype as in the leaf.
// Mode 0 keeps the running maximum and its index.  Mode 1 needs all K scores at once: they stay in the row's
// thread, in REGISTERS, written by compile-time index (a chunk's 16 doubles, or one score, selected into its place
// with v_cndmask: 2 x 16 NKC selects per chunk of 16 D element terms, KP per component of D (D + 1) / 2 FMAs), and
// the kernels are instantiated per padded K (event: NKC = 1, 2, 4 chunks of 16; mvn: KP = 16, 32, 64) and per mode,
// so that mode 0 and small K do not pay for the registers of K = 64.  LDS was not taken: 256 rows x 64 scores are
// 64 KB (f32 scores) to 128 KB (doubles).  No workspace, nothing of size K N in global memory, no atomics, nothing
// reduced across rows: two runs give identical bits.
//
// Footprint (hipcc -Rpass-analysis=kernel-resource-usage, gfx950, VGPRs + AGPRs per lane; a workgroup of 256 threads is
// one wave on each SIMD, so waves per SIMD = workgroups per CU; LDS never binds before the registers do):
//   event, LDS 17.6 KB (one data value per element) or 18.6 KB (Normal, LogNormal, Bernoulli):
//     mode 0:          123 .. 209 (Bernoulli f32 172, Gamma f64 178)          2 to 4 waves per SIMD
//     mode 1, NKC 1:   141 .. 221 (Bernoulli f32 193, Gamma f64 199)          2 to 3
//     mode 1, NKC 2:   239 .. 256 + 40 (Bernoulli f32 256 + 24)               1 to 2
//     mode 1, NKC 4:   256 + 20 .. 256 + 124 (Bernoulli f32 256 + 90)         1
//   mvn, LDS DP^2 + DP + 1 values (f32 DP = 64: 16.3 KB, f64: 32.5 KB), DP = 8 / 16 / 32 / 64:
//     f32 mode 0:        58 / 89 / 175 / 256 + 4                              8 / 5 / 2 / 1
//     f32 mode 1, KP 16: 95 / 124 / 209 / 256 + 14                            5 / 4 / 2 / 1
//     f32 mode 1, KP 64: 206 / 210 / 256 + 15 / 256 + 63                      2 / 2 / 1 / 1
//     f64 mode 0:        94 / 134 / 213 / 256 + 120                           5 / 3 / 2 / 1
//     f64 mode 1, KP 16: 149 / 187 / 256 + 1 / 256 + 176                      3 / 2 / 1 / 1
//     f64 mode 1, KP 64: 255 / 256 + 28 / 256 + 98 / 512 and 80 bytes of scratch per lane    2 / 1 / 1 / 1
// Scratch is used by that last instantiation only (float64 draws with D > 32 and K > 32: the row's x and d are 256
// registers by themselves, as in the leaf).  With the workgroup as the unit of the barrier-separated staging, the
// compiler spends the registers a 256-thread launch bound leaves it on hoisted LDS reads; a draw over more than 16
// components therefore runs at one wave per SIMD, which is where the leaves' lse launches already are at f64.
#include "common.h"
#include "dist_fam.h"
#include "mixture_assign.h"
#include "mixture_event.h"
#include "mixture_mvn.h"

namespace pa {

// mode 0, one score after the other in index order: the first maximum and whether a NaN was among them
struct MixwBest {
  double m;
  int arg;
  bool nan;
  __device__ __forceinline__ void init() { m = -t_inf<double>(); arg = 0; nan = false; }
  __device__ __forceinline__ void take(double t, int k) {
    if (t != t) {
      nan = true;
    } else if (t > m) {
      m = t;
      arg = k;
    }
  }
  __device__ __forceinline__ int get() const { return nan ? 0 : arg; }
};

// mode 1 from a row's NK scores (-inf past K) in index order
template <int NK, typename S>
__device__ __forceinline__ int mixw_draw(S (&ts)[NK], int K, double u) {
  const double ninf = -t_inf<double>();
  double m = ninf;
  bool nan = false;
#pragma unroll
  for (int k = 0; k < NK; ++k) {
    const double t = (double)ts[k];
    nan = nan || t != t;
    m = t > m ? t : m;
  }
  if (nan || m == ninf) return 0;
  auto term = [&](int k) {
    const double t = (double)ts[k];
    return t == m ? 1.0 : exp(t - m);
  };
  double tot = 0.0;
#pragma unroll
  for (int k = 0; k < NK; ++k) {
    if (k < K) tot += term(k);                       // (K: uniform over the workgroup)
  }
  const double thr = u * tot;
  double c = 0.0;
  int first = NK, last = -1;
#pragma unroll
  for (int k = 0; k < NK; ++k) {
    if (k < K) {
      const double e = term(k);
      c += e;
      if (c > thr && first == NK) first = k;
      if (e > 0.0) last = k;
    }
  }
  const int zi = first < last ? first : last;
  return zi < 0 ? 0 : zi;
}

template <int F, typename T, int NKC, int MODE>
__global__ __launch_bounds__(EV_THREADS) void mixture_assign_event_kernel(const T* __restrict__ x, int64_t N, int D,
                                                                          int K, const T* __restrict__ a,
                                                                          int64_t a_bs, EvParams P, uint64_t seed,
                                                                          uint64_t offset,
                                                                          const uint64_t* __restrict__ offset_dev,
                                                                          int64_t* __restrict__ z) {
  using E = Ev<F, T>;
  constexpr int DC = ev_dc<T, E::NX>();
  __shared__ T xs[E::NX * DC * EV_TRP];
  __shared__ __attribute__((aligned(16))) T ps[E::NP * EV_KC * DC];
  __shared__ double cks[EV_MAXK];
  const int64_t b = blockIdx.y;
  const T* p0 = (const T*)P.p0 + b * P.p0_b;
  const T* p1 = P.p1 ? (const T*)P.p1 + b * P.p1_b : nullptr;
  a += b * a_bs;
  z += b * N;
  if (offset_dev) offset += *offset_dev;
  const int tid = threadIdx.x, lane = tid & 63;
  for (int k = tid >> 6; k < K; k += EV_THREADS / 64) {
    const T* q0 = p0 + k * P.p0_k;
    const T* q1 = p1 ? p1 + k * P.p1_k : nullptr;
    double v = 0.0;
    for (int d = lane; d < D; d += 64) v += E::kc((double)q0[d * P.p0_d], q1 ? (double)q1[d * P.p1_d] : 0.0);
    v = wave_sum(v);
    if (lane == 0) cks[k] = (double)a[k] + v;
  }
  __syncthreads();
  for (int64_t base = (int64_t)blockIdx.x * EV_TR; base < N; base += (int64_t)gridDim.x * EV_TR) {
    const int64_t n = base + tid;
    int zi;
    if constexpr (MODE == 0) {
      MixwBest best;
      best.init();
      for (int kc0 = 0; kc0 < K; kc0 += EV_KC) {
        double t[EV_KC], q;
        ev_rows<F, T>(x, N, D, K, kc0, base, p0, P.p0_k, P.p0_d, p1, P.p1_k, P.p1_d, cks, xs, ps, t, false, q);
#pragma unroll
        for (int k = 0; k < EV_KC; ++k)
          if (kc0 + k < K) best.take(t[k], kc0 + k);
      }
      zi = best.get();
    } else {
      double ts[NKC * EV_KC];
#pragma unroll
      for (int k = 0; k < NKC * EV_KC; ++k) ts[k] = -t_inf<double>();
#pragma unroll 1
      for (int c = 0; c < NKC; ++c) {
        if (c * EV_KC >= K) break;                   // (uniform over the workgroup)
        double t[EV_KC], q;
        ev_rows<F, T>(x, N, D, K, c * EV_KC, base, p0, P.p0_k, P.p0_d, p1, P.p1_k, P.p1_d, cks, xs, ps, t, false, q);
#pragma unroll
        for (int j = 0; j < NKC; ++j)
#pragma unroll
          for (int k = 0; k < EV_KC; ++k) ts[j * EV_KC + k] = j == c ? t[k] : ts[j * EV_KC + k];
      }
      const T u = mixa_uniform(T(0), seed, offset, (uint64_t)b * (uint64_t)N + (uint64_t)(n < N ? n : N - 1));
      zi = mixw_draw(ts, K, (double)u);
    }
    if (n < N) z[n] = (int64_t)zi;
  }
}

template <typename T, int DP, int KP, int MODE>
__global__ __launch_bounds__(MVN_THREADS) void mixture_assign_mvn_kernel(const T* __restrict__ x, int64_t N, int D,
                                                                         int K, const T* __restrict__ a, int64_t a_bs,
                                                                         const T* __restrict__ loc, int64_t l_sk,
                                                                         int64_t l_bs, const T* __restrict__ w,
                                                                         int64_t w_sk, int64_t w_bs, uint64_t seed,
                                                                         uint64_t offset,
                                                                         const uint64_t* __restrict__ offset_dev,
                                                                         int64_t* __restrict__ z) {
  const int64_t b = blockIdx.y;
  a += b * a_bs;
  loc += b * l_bs;
  w += b * w_bs;
  z += b * N;
  if (offset_dev) offset += *offset_dev;
  __shared__ T Ws[DP * DP];
  __shared__ T mus[DP];
  __shared__ T ck[1];
  const int tid = threadIdx.x;
  for (int64_t base = (int64_t)blockIdx.x * MVN_THREADS; base < N; base += (int64_t)gridDim.x * MVN_THREADS) {
    const int64_t n = base + tid;
    const bool valid = n < N;
    const T* xr = x + (valid ? n : N - 1) * D;        // (a row past the end reads the last one and writes nothing)
    T xv[DP];
#pragma unroll
    for (int j = 0; j < DP; ++j) xv[j] = j < D ? xr[j] : T(0);
    MixwBest best;
    best.init();
    T ts[KP];
#pragma unroll
    for (int j = 0; j < KP; ++j) ts[j] = -t_inf<T>();
    for (int k = 0; k < K; ++k) {
      mvn_stage<T, DP>(Ws, mus, ck, a, loc, l_sk, w, w_sk, D, k);
      T d[DP];
#pragma unroll
      for (int j = 0; j < DP; ++j) d[j] = xv[j] - mus[j];
      const T t = ck[0] - T(0.5) * mvn_quad<T, DP>(Ws, d, D);
      if constexpr (MODE == 0) {
        best.take((double)t, k);
      } else {
#pragma unroll
        for (int j = 0; j < KP; ++j) ts[j] = j == k ? t : ts[j];
      }
    }
    int zi;
    if constexpr (MODE == 0) {
      zi = best.get();
    } else {
      const T u = mixa_uniform(T(0), seed, offset, (uint64_t)b * (uint64_t)N + (uint64_t)(valid ? n : N - 1));
      zi = mixw_draw(ts, K, (double)u);
    }
    if (valid) z[n] = (int64_t)zi;
  }
}

template <int F, typename T>
static int mixture_assign_event_f(const T* x, int64_t N, int D, int K, int64_t B, const T* a, int64_t a_bs,
                                  const EvParams& P, int mode, uint64_t seed, uint64_t offset,
                                  const uint64_t* offset_dev, int64_t* z, hipStream_t s) {
  int64_t g = (N + EV_TR - 1) / EV_TR;
  if (g > ev_lse_blocks_max(B)) g = ev_lse_blocks_max(B);
  const dim3 grid((unsigned)g, (unsigned)B);
#define PA_MIXW_EV(NKC_, MODE_)                                                                                   \
  hipLaunchKernelGGL((mixture_assign_event_kernel<F, T, NKC_, MODE_>), grid, dim3(EV_THREADS), 0, s, x, N, D, K, \
                     a, a_bs, P, seed, offset, offset_dev, z)
  if (mode == 0) PA_MIXW_EV(1, 0);
  else if (K <= EV_KC) PA_MIXW_EV(1, 1);
  else if (K <= 2 * EV_KC) PA_MIXW_EV(2, 1);
  else PA_MIXW_EV(4, 1);
#undef PA_MIXW_EV
  return check_launch("mixture_assign_event_kernel");
}

template <typename T>
static int mixture_assign_event_t(int dist, const T* x, int64_t N, int D, int K, int64_t B, const T* a, int64_t a_bs,
                                  const EvParams& P, int mode, uint64_t seed, uint64_t offset,
                                  const uint64_t* offset_dev, int64_t* z, hipStream_t s) {
  switch (dist) {
#define PA_MIXW_CASE(F_) \
  case F_: return mixture_assign_event_f<F_, T>(x, N, D, K, B, a, a_bs, P, mode, seed, offset, offset_dev, z, s);
    PA_MIXW_CASE(PA_DIST_NORMAL) PA_MIXW_CASE(PA_DIST_LOG_NORMAL) PA_MIXW_CASE(PA_DIST_EXPONENTIAL)
    PA_MIXW_CASE(PA_DIST_BERNOULLI_LOGITS) PA_MIXW_CASE(PA_DIST_POISSON) PA_MIXW_CASE(PA_DIST_GAMMA)
#undef PA_MIXW_CASE
  }
  return fail(PA_ERR_UNSUPPORTED, "mixture_assign_event: distribution %d", dist);
}

template <typename T, int DP>
static int mixture_assign_mvn_launch(const T* x, int64_t N, int D, int K, int64_t B, const T* a, int64_t a_bs,
                                     const T* loc, int64_t l_sk, int64_t l_bs, const T* w, int64_t w_sk, int64_t w_bs,
                                     int mode, uint64_t seed, uint64_t offset, const uint64_t* offset_dev, int64_t* z,
                                     hipStream_t s) {
  int64_t g = (N + MVN_THREADS - 1) / MVN_THREADS;
  if (g > mvn_lse_blocks_max(B)) g = mvn_lse_blocks_max(B);
  const dim3 grid((unsigned)g, (unsigned)B);
#define PA_MIXW_MVN(KP_, MODE_)                                                                                    \
  hipLaunchKernelGGL((mixture_assign_mvn_kernel<T, DP, KP_, MODE_>), grid, dim3(MVN_THREADS), 0, s, x, N, D, K, a, \
                     a_bs, loc, l_sk, l_bs, w, w_sk, w_bs, seed, offset, offset_dev, z)
  if (mode == 0) PA_MIXW_MVN(1, 0);
  else if (K <= 16) PA_MIXW_MVN(16, 1);
  else if (K <= 32) PA_MIXW_MVN(32, 1);
  else PA_MIXW_MVN(64, 1);
#undef PA_MIXW_MVN
  return check_launch("mixture_assign_mvn_kernel");
}

template <typename T>
static int mixture_assign_mvn_t(const T* x, int64_t N, int D, int K, int64_t B, const T* a, int64_t a_bs,
                                const T* loc, int64_t l_sk, int64_t l_bs, const T* w, int64_t w_sk, int64_t w_bs,
                                int mode, uint64_t seed, uint64_t offset, const uint64_t* offset_dev, int64_t* z,
                                hipStream_t s) {
  switch (mvn_padded_d(D)) {
#define PA_MIXW_CASE(DP_)                                                                                        \
  case DP_:                                                                                                      \
    return mixture_assign_mvn_launch<T, DP_>(x, N, D, K, B, a, a_bs, loc, l_sk, l_bs, w, w_sk, w_bs, mode, seed, \
                                             offset, offset_dev, z, s);
    PA_MIXW_CASE(8) PA_MIXW_CASE(16) PA_MIXW_CASE(32) PA_MIXW_CASE(64)
#undef PA_MIXW_CASE
  }
  return fail(PA_ERR_UNSUPPORTED, "mixture_assign_mvn: D=%d", D);
}

}  // namespace pa

extern "C" {

int pa_mixture_assign_event(int dtype, int dist, const void* x, int64_t N, int D, int K, int64_t B, const void* a,
                            int64_t a_batch_stride, const void* p0, int64_t p0_stride_k, int64_t p0_stride_d,
                            int64_t p0_batch_stride, const void* p1, int64_t p1_stride_k, int64_t p1_stride_d,
                            int64_t p1_batch_stride, int mode, uint64_t seed, uint64_t offset,
                            const uint64_t* offset_dev, int64_t* z, pa_stream_t stream) {
  if (!pa::ev_family(dist) || K < 1 || K > pa::EV_MAXK || D < 1 || D > pa::EV_MAXD || B < 1 || B > 65535 ||
      (dtype != PA_F32 && dtype != PA_F64))
    return pa::fail(PA_ERR_UNSUPPORTED,
                    "mixture_assign_event: family %d, K=%d (1..%d), D=%d (1..%d), B=%lld (1..65535), dtype %d", dist,
                    K, pa::EV_MAXK, D, pa::EV_MAXD, (long long)B, dtype);
  PA_REQUIRE(mode == 0 || mode == 1, "mixture_assign_event: mode %d (0: most probable, 1: draw)", mode);
  PA_REQUIRE(N >= 1 && x && a && p0 && z, "mixture_assign_event: NULL pointer or N < 1");
  PA_REQUIRE((p1 != nullptr) == (pa::ev_npar(dist) == 2), "mixture_assign_event: p1 %s for distribution %d",
             p1 ? "given" : "missing", dist);
  PA_REQUIRE(a_batch_stride >= 0 && p0_stride_k >= 0 && p0_stride_d >= 0 && p0_batch_stride >= 0 &&
                 p1_stride_k >= 0 && p1_stride_d >= 0 && p1_batch_stride >= 0,
             "mixture_assign_event: negative stride");
  const pa::EvParams P{p0, p0_stride_k, p0_stride_d, p0_batch_stride, p1, p1_stride_k, p1_stride_d, p1_batch_stride};
  hipStream_t s = pa::as_stream(stream);
  if (dtype == PA_F32)
    return pa::mixture_assign_event_t<float>(dist, (const float*)x, N, D, K, B, (const float*)a, a_batch_stride, P,
                                             mode, seed, offset, offset_dev, z, s);
  return pa::mixture_assign_event_t<double>(dist, (const double*)x, N, D, K, B, (const double*)a, a_batch_stride, P,
                                            mode, seed, offset, offset_dev, z, s);
}

int pa_mixture_assign_mvn(int dtype, const void* x, int64_t N, int D, int K, int64_t B, const void* a,
                          int64_t a_batch_stride, const void* loc, int64_t loc_stride_k, int64_t loc_batch_stride,
                          const void* w, int64_t w_stride_k, int64_t w_batch_stride, int mode, uint64_t seed,
                          uint64_t offset, const uint64_t* offset_dev, int64_t* z, pa_stream_t stream) {
  if (K < 1 || K > pa::MVN_MAXK || D < 1 || D > pa::MVN_MAXD || B < 1 || B > 65535 ||
      (dtype != PA_F32 && dtype != PA_F64))
    return pa::fail(PA_ERR_UNSUPPORTED,
                    "mixture_assign_mvn: K=%d (1..%d), D=%d (1..%d), B=%lld (1..65535), dtype %d", K, pa::MVN_MAXK,
                    D, pa::MVN_MAXD, (long long)B, dtype);
  PA_REQUIRE(mode == 0 || mode == 1, "mixture_assign_mvn: mode %d (0: most probable, 1: draw)", mode);
  PA_REQUIRE(N >= 1 && x && a && loc && w && z, "mixture_assign_mvn: NULL pointer or N < 1");
  PA_REQUIRE(a_batch_stride >= 0 && loc_stride_k >= 0 && loc_batch_stride >= 0 && w_stride_k >= 0 &&
                 w_batch_stride >= 0, "mixture_assign_mvn: negative stride");
  hipStream_t s = pa::as_stream(stream);
  if (dtype == PA_F32)
    return pa::mixture_assign_mvn_t<float>((const float*)x, N, D, K, B, (const float*)a, a_batch_stride,
                                           (const float*)loc, loc_stride_k, loc_batch_stride, (const float*)w,
                                           w_stride_k, w_batch_stride, mode, seed, offset, offset_dev, z, s);
  return pa::mixture_assign_mvn_t<double>((const double*)x, N, D, K, B, (const double*)a, a_batch_stride,
                                          (const double*)loc, loc_stride_k, loc_batch_stride, (const double*)w,
                                          w_stride_k, w_batch_stride, mode, seed, offset, offset_dev, z, s);
}

}  // extern "C"
