// mixture_event.h -- the event-shaped mixture leaf's split of the log density (Ev<F, T>), its tile sizes and the
// score pass ev_rows: shared by mixture_event.hip (lse and stats launches) and mixture_assign_wide.hip.
#pragma once
#include "common.h"
#include "dist_fam.h"

namespace pa {

constexpr int EV_THREADS = 256;         // = the rows of a tile (one thread per row in the t pass)
constexpr int EV_TR = EV_THREADS;
constexpr int EV_KC = 16;               // components per chunk
constexpr int EV_MAXK = 64;
constexpr int EV_MAXD = 1024;
constexpr int EV_LSE_BLOCKS = 2048;     // launch 2: workgroups over all parameter sets (at most, plus B)
constexpr int EV_STAT_BLOCKS = 1024;    // launch 3: workgroups over all (k chunk, feature block, b) (at most, plus)
constexpr double EV_REC_CAP = 40.0 * 1024 * 1024;   // bytes of stats records (unless one chunk needs more)

// ---- per-family split of the log density ---------------------------------------------------------------------------
// NX data values staged per element (x, log x), NP parameters staged per (k, d), NS sums per (k, d), NPAR gradients.
// data(x, v), par(p0, p1, q): the staged values; elem(v, q): the (n, k, d) term; row(v): the (n, d) term;
// kc(p0, p1): the (k, d) term; stat(v, q, r, s): s += r * statistic; grad(R, s, p0, p1, g): dS/dp0, dS/dp1.
// Zero data and zero parameters give elem = 0 and row = 0 (the padding).
template <int F, typename T> struct Ev;

template <typename T> __device__ __forceinline__ T ev_softplus(T l) {
  return (l > T(0) ? l : T(0)) + t_log1p(t_exp(-t_abs(l)));
}

template <typename T> struct Ev<PA_DIST_BERNOULLI_LOGITS, T> {
  static constexpr int NX = 1, NP = 2, NS = 1, NPAR = 1;
  static __device__ __forceinline__ void data(T x, T* v) { v[0] = x; }
  static __device__ __forceinline__ void par(T l, T, T* q) { q[0] = l; q[1] = -ev_softplus(l); }
  static __device__ __forceinline__ T elem(const T* v, const T* q) { return fma(v[0], q[0], q[1]); }
  static __device__ __forceinline__ T row(const T*) { return T(0); }
  static __device__ __forceinline__ double kc(double, double) { return 0.0; }
  static __device__ __forceinline__ void stat(const T* v, const T*, T r, T* s) { s[0] += r * v[0]; }
  static __device__ __forceinline__ void grad(double R, const double* s, double l, double, double* g) {
    const double e = exp(-fabs(l));
    g[0] = s[0] - R * (l >= 0.0 ? 1.0 / (1.0 + e) : e / (1.0 + e));
  }
};

template <typename T> struct Ev<PA_DIST_POISSON, T> {
  static constexpr int NX = 1, NP = 1, NS = 1, NPAR = 1;
  static __device__ __forceinline__ void data(T x, T* v) { v[0] = x; }
  static __device__ __forceinline__ void par(T lam, T, T* q) { q[0] = t_log(lam); }
  static __device__ __forceinline__ T elem(const T* v, const T* q) { return v[0] != T(0) ? v[0] * q[0] : T(0); }
  static __device__ __forceinline__ T row(const T* v) { return v[0] == T(0) ? T(0) : -t_lgamma(v[0] + T(1)); }
  static __device__ __forceinline__ double kc(double lam, double) { return -lam; }
  static __device__ __forceinline__ void stat(const T* v, const T*, T r, T* s) { s[0] += r * v[0]; }
  static __device__ __forceinline__ void grad(double R, const double* s, double lam, double, double* g) {
    g[0] = s[0] / lam - R;
  }
};

template <typename T> struct Ev<PA_DIST_EXPONENTIAL, T> {
  static constexpr int NX = 1, NP = 1, NS = 1, NPAR = 1;
  static __device__ __forceinline__ void data(T x, T* v) { v[0] = x; }
  static __device__ __forceinline__ void par(T lam, T, T* q) { q[0] = -lam; }
  static __device__ __forceinline__ T elem(const T* v, const T* q) { return v[0] * q[0]; }
  static __device__ __forceinline__ T row(const T*) { return T(0); }
  static __device__ __forceinline__ double kc(double lam, double) { return log(lam); }
  static __device__ __forceinline__ void stat(const T* v, const T*, T r, T* s) { s[0] += r * v[0]; }
  static __device__ __forceinline__ void grad(double R, const double* s, double lam, double, double* g) {
    g[0] = R / lam - s[0];
  }
};

template <typename T> struct Ev<PA_DIST_GAMMA, T> {
  static constexpr int NX = 2, NP = 2, NS = 2, NPAR = 2;
  static __device__ __forceinline__ void data(T x, T* v) { v[0] = x; v[1] = t_log(x); }
  static __device__ __forceinline__ void par(T al, T be, T* q) { q[0] = al - T(1); q[1] = -be; }
  static __device__ __forceinline__ T elem(const T* v, const T* q) {
    return (q[0] != T(0) ? q[0] * v[1] : T(0)) + q[1] * v[0];      // xlogy(al - 1, x) - be x
  }
  static __device__ __forceinline__ T row(const T*) { return T(0); }
  static __device__ __forceinline__ double kc(double al, double be) { return t_xlogy(al, be) - t_lgamma(al); }
  static __device__ __forceinline__ void stat(const T* v, const T* q, T r, T* s) {
    s[0] += r * ((q[0] == T(0) && v[0] == T(0)) ? T(0) : v[1]);    // d xlogy(al - 1, x) / d al
    s[1] += r * v[0];
  }
  static __device__ __forceinline__ void grad(double R, const double* s, double al, double be, double* g) {
    g[0] = R * (t_xlogy_dx(al, be) - t_digamma(al)) + s[0];
    g[1] = R * (al / be) - s[1];
  }
};

template <typename T> struct Ev<PA_DIST_NORMAL, T> {
  static constexpr int NX = 1, NP = 2, NS = 2, NPAR = 2;
  static __device__ __forceinline__ void data(T x, T* v) { v[0] = x; }
  static __device__ __forceinline__ void par(T mu, T sg, T* q) { q[0] = mu; q[1] = T(1) / sg; }
  static __device__ __forceinline__ T elem(const T* v, const T* q) {
    const T z = (v[0] - q[0]) * q[1];
    return T(-0.5) * z * z;
  }
  static __device__ __forceinline__ T row(const T*) { return T(0); }
  static __device__ __forceinline__ double kc(double, double sg) { return -log(sg) - Consts<double>::half_log_2pi; }
  static __device__ __forceinline__ void stat(const T* v, const T* q, T r, T* s) {
    const T z = (v[0] - q[0]) * q[1], rz = r * z;
    s[0] += rz;
    s[1] += rz * z;
  }
  static __device__ __forceinline__ void grad(double R, const double* s, double, double sg, double* g) {
    g[0] = s[0] / sg;
    g[1] = (s[1] - R) / sg;
  }
};

template <typename T> struct Ev<PA_DIST_LOG_NORMAL, T> : Ev<PA_DIST_NORMAL, T> {
  static __device__ __forceinline__ void data(T x, T* v) { v[0] = t_log(x); }
  static __device__ __forceinline__ T row(const T* v) { return -v[0]; }
};

static int ev_npar(int F) { return F == PA_DIST_NORMAL || F == PA_DIST_LOG_NORMAL || F == PA_DIST_GAMMA ? 2 : 1; }
static bool ev_family(int F) {
  return F == PA_DIST_NORMAL || F == PA_DIST_LOG_NORMAL || F == PA_DIST_EXPONENTIAL ||
         F == PA_DIST_BERNOULLI_LOGITS || F == PA_DIST_POISSON || F == PA_DIST_GAMMA;
}

// ---- sizes ---------------------------------------------------------------------------------------------------------
static int ev_block_d(int D) { return D <= 16 ? 16 : D <= 64 ? 64 : 256; }
__host__ __device__ inline int64_t ev_record(int DB, int NS) { return EV_KC + (int64_t)EV_KC * DB * NS; }
static int64_t ev_lse_blocks_max(int64_t B) { int64_t g = (EV_LSE_BLOCKS + B - 1) / B; return g < 1 ? 1 : g; }
static int64_t ev_chunks_max(int K, int D, int64_t B, int NS) {
  const int DB = ev_block_d(D);
  const int64_t groups = B * ((K + EV_KC - 1) / EV_KC) * ((D + DB - 1) / DB);
  int64_t c = (EV_STAT_BLOCKS + groups - 1) / groups;
  const int64_t cap = (int64_t)(EV_REC_CAP / (8.0 * (double)groups * (double)ev_record(DB, NS)));
  if (c > cap) c = cap;
  return c < 1 ? 1 : c;
}

// the rows of a tile and the chunks of features staged per pass (each LDS image about 16 KB)
template <typename T, int NX> constexpr int ev_dc() { return (sizeof(T) == 4 ? 16 : 8) / NX; }
constexpr int EV_TRP = EV_TR + 1;        // (padded: the staging writes of a row's features land in distinct banks)

struct EvParams {
  const void* p0;
  int64_t p0_k, p0_d, p0_b;
  const void* p1;
  int64_t p1_k, p1_d, p1_b;
};

// t_nk (k < EV_KC; in double) of row row0 + threadIdx.x for the components kc0 ..  kc0 + EV_KC - 1 of set b (whose
// parameter pointers are already offset), over all D features; x and the staged parameters pass through LDS in
// chunks of DC features.  With `want_row`, q = sum_d row(x_nd) too.  Every thread of the workgroup calls it.
template <int F, typename T>
__device__ __forceinline__ void ev_rows(const T* __restrict__ x, int64_t N, int D, int K, int kc0, int64_t row0,
                                        const T* __restrict__ p0, int64_t p0k, int64_t p0d, const T* __restrict__ p1,
                                        int64_t p1k, int64_t p1d, const double* __restrict__ ck, T* xs, T* ps,
                                        double (&t)[EV_KC], bool want_row, double& q) {
  using E = Ev<F, T>;
  constexpr int NX = E::NX, NP = E::NP, DC = ev_dc<T, NX>();
  const int tid = threadIdx.x;
#pragma unroll
  for (int k = 0; k < EV_KC; ++k) t[k] = kc0 + k < K ? ck[kc0 + k] : -(double)t_inf<T>();
  q = 0.0;
  for (int d0 = 0; d0 < D; d0 += DC) {
    __syncthreads();                               // (the previous chunk's readers are done)
    for (int e = tid; e < EV_TR * DC; e += EV_THREADS) {
      const int r = e / DC, c = e % DC;
      const int64_t n = row0 + r;
      const int d = d0 + c;
      T v[NX];
#pragma unroll
      for (int j = 0; j < NX; ++j) v[j] = T(0);
      if (n < N && d < D) E::data(x[n * D + d], v);
#pragma unroll
      for (int j = 0; j < NX; ++j) xs[(j * DC + c) * EV_TRP + r] = v[j];
    }
    for (int e = tid; e < EV_KC * DC; e += EV_THREADS) {
      const int k = e / DC, c = e % DC, kk = kc0 + k, d = d0 + c;
      T qv[NP];
#pragma unroll
      for (int j = 0; j < NP; ++j) qv[j] = T(0);
      if (kk < K && d < D) E::par(p0[kk * p0k + d * p0d], p1 ? p1[kk * p1k + d * p1d] : T(0), qv);
#pragma unroll
      for (int j = 0; j < NP; ++j) ps[(j * EV_KC + k) * DC + c] = qv[j];
    }
    __syncthreads();
    T tc[EV_KC], qc = T(0);
#pragma unroll
    for (int k = 0; k < EV_KC; ++k) tc[k] = T(0);
#pragma unroll
    for (int c = 0; c < DC; ++c) {
      T v[NX];
#pragma unroll
      for (int j = 0; j < NX; ++j) v[j] = xs[(j * DC + c) * EV_TRP + tid];
      if (want_row) qc += E::row(v);
#pragma unroll
      for (int k = 0; k < EV_KC; ++k) {
        T qv[NP];
#pragma unroll
        for (int j = 0; j < NP; ++j) qv[j] = ps[(j * EV_KC + k) * DC + c];   // (one address per wave: broadcast)
        tc[k] += E::elem(v, qv);
      }
    }
#pragma unroll
    for (int k = 0; k < EV_KC; ++k) t[k] += (double)tc[k];
    q += (double)qc;
  }
}

}  // namespace pa
