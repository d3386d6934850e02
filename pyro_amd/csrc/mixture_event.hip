// mixture_event.hip -- the mixture leaf for an event-shaped element-wise observation `Fam(p0[z], p1[z]).to_event(1)`
// over D <= 1024 features (Normal, LogNormal, Exponential, Bernoulli, Poisson, Gamma), without the [K, N, D] frame.
//
// Reference path replaced: TraceEnum_ELBO on such a site observed under the data plate with z enumerated
// (pyro/infer/traceenum_elbo.py:112-214, pyro/ops/contract.py:79-160): torch's Independent.log_prob builds the
// [K, N, D] element-wise log densities and sums the event dim, the sum-product takes logsumexp over K and the plate
// sum, and autograd keeps and walks those [K, N, D] tensors again.
//
// Here, per parameter set b (vectorised particles / chains):
//   t_nk = a_k + sum_d lp(x_nd | p0_kd, p1_kd),   S = sum_n logsumexp_k t_nk,   r_nk = softmax_k t_nk,
//   dS/da_k = R_k = sum_n r_nk,   dS/dp_kd = sum_n r_nk dlp/dp (x_nd | p0_kd, p1_kd).
// lp splits into a term of (n, k, d) -- the only one evaluated per element --, a term of (k, d) summed once per
// component into c_k = a_k + sum_d kc(p_kd) (double), and a term of (n, d) summed per row (it shifts every t_nk of
// a row alike: the row's logsumexp, never r).  The gradients follow from R_k and at most two sums per (k, d):
//   Bernoulli(l)   elem fma(x, l, -softplus(l)) (x l - softplus(l) rounded once: no cancellation at |l| >> 1)
//                  s = sum r x                      dl = s - R sigmoid(l)
//   Poisson(lam)   elem xlogy(x, lam), kc -lam, row -lgamma(x + 1)
//                  s = sum r x                      dlam = s / lam - R
//   Exponential    elem -lam x, kc log lam          s = sum r x           dlam = R / lam - s
//   Gamma(al, be)  elem xlogy(al - 1, x) - be x, kc xlogy(al, be) - lgamma(al)
//                  s0 = sum r log x, s1 = sum r x   dal = R (log be - psi(al)) + s0,  dbe = R al / be - s1
//   Normal(mu, sg) elem -z^2 / 2, z = (x - mu) / sg (centred: x - mu first), kc -log sg - log(2 pi) / 2
//                  s0 = sum r z, s1 = sum r z^2     dmu = s0 / sg,  dsg = (s1 - R) / sg
//   LogNormal      as Normal on log x, row -log x
// (xlogy and its derivative as dist_fam.h states them for torch: 0 at a zero coefficient unless the log's argument is
// NaN.)
//
// Five launches:
//   1. prep:     one workgroup per (k, b): c_k in double.
//   2. lse:      one thread per row, rows in tiles of 256; the tile's x and the staged parameters of 16 components
//                pass through LDS in chunks of features (one global read of x per 16 components); t_nk of the 16
//                components in registers (per chunk in the input dtype, across chunks in double), logsumexp over
//                k online in double.  Writes the row's logsumexp without the row term (B N doubles: the only per-row
//                buffer) and one double per workgroup: sum_n (lse_n + row term).
//   3. stats:    one workgroup per (row chunk, 16-component chunk, feature block of DB in {16, 64, 256}, b):
//                recomputes t_nk of its components for a tile of 256 rows (as launch 2), stages r_nk in LDS, then
//                each thread owns DB / 16 (k, d) pairs of the block and adds r times the statistic over the tile's
//                rows (x staged again, per sub-tile), in the input dtype per sub-tile and in double across them.
//                One record per workgroup: R (feature block 0) and the sums of its pairs.
//   3b. redo:    launch 3 again for the workgroups whose record came out non-finite, without the rows and components
//                whose responsibility is exactly 0 (see mixture_event_stats_kernel); the others leave at once.
//   4. finalize: one wave per (k, 64 features, b): the records added in chunk order in double and the chain rule
//                in double with the parameters; wave (0, 0, b) adds the lse partials in a fixed order.  No atomics
//                anywhere: two runs give identical bits.
// Nothing of size K N is written.  Features past D, components past K and rows past N are staged as zeros that
// every family's element term maps to 0.
//
// Workspace (pa_mixture_event_workspace(dist, K, D, B)), in doubles:
//   B K + B G1(B) + B nkc ndb C (16 + 16 DB NS),    G1(B) = max(1, ceil(2048 / B)),
//   C = max(1, min(ceil(1024 / (nkc ndb B)), floor(40 MiB / (8 B nkc ndb (16 + 16 DB NS))))),
// nkc = ceil(K / 16), ndb = ceil(D / DB), NS = sums per pair (1 or 2): at K = 64, D = 1024, B = 1 (NS = 2) 38 chunks,
// 41.0 MB in all; at most 42 MB for any K, D at B = 1 (the records' 40 MiB cap).  The launch takes G1 and C no
// larger than that (fewer for small N) and checks that its records fit.
//
// All arithmetic runs on the VALU (f32 MFMA issues at the f32 vector rate on gfx950: MI355X_MICROARCH.md).  Measured
// (rocprofv3, f32, Bernoulli N = 1e5, K = 16, D = 784): lse 0.50 ms, stats 2.20 ms, finalize 0.11 ms: bound by VALU /
// LDS issue at 1-2 waves per SIMD, not HBM (x streams at 0.6 TB/s); the stats launch repeats the t pass once per
// feature block (4x at D = 784), the first thing to take out.
#include "common.h"
#include "dist_fam.h"
#include "mixture_event.h"

namespace pa {

template <int F, typename T>
__global__ __launch_bounds__(EV_THREADS) void mixture_event_prep_kernel(int D, int K, const T* __restrict__ a,
                                                                        int64_t a_bs, EvParams P,
                                                                        double* __restrict__ ck) {
  __shared__ double red[EV_THREADS / 64];
  const int k = blockIdx.x;
  const int64_t b = blockIdx.y;
  const T* p0 = (const T*)P.p0 + b * P.p0_b + k * P.p0_k;
  const T* p1 = P.p1 ? (const T*)P.p1 + b * P.p1_b + k * P.p1_k : nullptr;
  double v = 0.0;
  for (int d = threadIdx.x; d < D; d += EV_THREADS)
    v += Ev<F, T>::kc((double)p0[d * P.p0_d], p1 ? (double)p1[d * P.p1_d] : 0.0);
  v = block_sum_f64(v, red);
  if (threadIdx.x == 0) ck[b * K + k] = (double)a[b * a_bs + k] + v;
}

template <int F, typename T>
__global__ __launch_bounds__(EV_THREADS) void mixture_event_lse_kernel(const T* __restrict__ x, int64_t N, int D,
                                                                       int K, EvParams P,
                                                                       const double* __restrict__ ck,
                                                                       double* __restrict__ lse,
                                                                       double* __restrict__ spart) {
  using E = Ev<F, T>;
  constexpr int DC = ev_dc<T, E::NX>();
  __shared__ T xs[E::NX * DC * EV_TRP];
  __shared__ __attribute__((aligned(16))) T ps[E::NP * EV_KC * DC];
  __shared__ double red[EV_THREADS / 64];
  const int64_t b = blockIdx.y;
  const T* p0 = (const T*)P.p0 + b * P.p0_b;
  const T* p1 = P.p1 ? (const T*)P.p1 + b * P.p1_b : nullptr;
  ck += b * K;
  const int tid = threadIdx.x;
  const double ninf = -t_inf<double>();
  double acc = 0.0;
  for (int64_t base = (int64_t)blockIdx.x * EV_TR; base < N; base += (int64_t)gridDim.x * EV_TR) {
    const int64_t n = base + tid;
    double m = ninf, s = 0.0;
    double qrow = 0.0;
    for (int kc0 = 0; kc0 < K; kc0 += EV_KC) {
      double t[EV_KC], q;
      ev_rows<F, T>(x, N, D, K, kc0, base, p0, P.p0_k, P.p0_d, p1, P.p1_k, P.p1_d, ck, xs, ps, t, kc0 == 0, q);
      if (kc0 == 0) qrow = q;
#pragma unroll
      for (int k = 0; k < EV_KC; ++k) {
        if (kc0 + k >= K) continue;
        const double tk = t[k];
        // online logsumexp (in double: t_nk is a double): a term of -inf (a component switched off) adds nothing,
        // NaN propagates
        if (tk > m) {
          s = s * exp(m - tk) + 1.0;
          m = tk;
        } else if (!(tk == ninf)) {
          s += exp(tk - m);
        }
      }
    }
    const double l = s > 0.0 ? m + log(s) : (s == 0.0 ? ninf : s);
    if (n < N) {
      // (a row term that makes the row's logsumexp NaN -- LogNormal at x = 0: -inf - log 0 -- makes it a NaN row for
      //  the statistics as well, as a NaN term does)
      const double lq = l + qrow;
      lse[b * N + n] = lq != lq ? lq : l;
      acc += lq;
    }
  }
  const double tot = block_sum_f64(acc, red);
  if (tid == 0) spart[b * gridDim.x + blockIdx.x] = tot;
}

// REDO (the launch after the plain one): r == 0 exactly -- a dead row, a switched-off or collapsed component -- adds
// no statistic, whatever the staged value is there; the plain sums form 0 * inf for it (Gamma at x = 0, Normal at
// x = inf).  A workgroup of the REDO launch leaves at once unless its record came out non-finite, and then adds it
// again with the zero responsibilities left out (a NaN r is handed on either way).  The guard is not inside the plain
// sums because it changes how the compiler packs and fuses their float32 multiply-adds, hence the last bits of ordinary
// data.
template <int F, typename T, int DB, bool REDO>
__global__ __launch_bounds__(EV_THREADS) void mixture_event_stats_kernel(const T* __restrict__ x, int64_t N, int D,
                                                                         int K, EvParams P,
                                                                         const double* __restrict__ ck,
                                                                         const double* __restrict__ lse,
                                                                         int64_t rows_per,
                                                                         int ndb, double* __restrict__ rec) {
  using E = Ev<F, T>;
  constexpr int NX = E::NX, NP = E::NP, NS = E::NS, DC = ev_dc<T, NX>();
  constexpr int TB = ev_dc<T, NX>();                    // rows per sub-tile of the statistics pass
  constexpr int PPT = EV_KC * DB / EV_THREADS;          // (k, d) pairs per thread
  constexpr int KSTEP = EV_THREADS / DB;                // components between a thread's pairs
  constexpr int XA = NX * DC * EV_TRP, XB = NX * TB * DB;
  static_assert(PPT * EV_THREADS == EV_KC * DB && TB * DB <= EV_TR * DC, "thread roles");
  __shared__ T xs[XA > XB ? XA : XB];                   // the t pass's x image, then the sub-tile's
  __shared__ __attribute__((aligned(16))) T ps[NP * EV_KC * DC];
  __shared__ __attribute__((aligned(16))) T rs[EV_KC * EV_TR];   // r of the tile, [k][row]
  const int c = blockIdx.x, kc = blockIdx.y / ndb, db = blockIdx.y % ndb;
  const int64_t b = blockIdx.z;
  const int kc0 = kc * EV_KC, d0b = db * DB;
  const T* p0 = (const T*)P.p0 + b * P.p0_b;
  const T* p1 = P.p1 ? (const T*)P.p1 + b * P.p1_b : nullptr;
  ck += b * K;
  lse += b * N;
  const int tid = threadIdx.x;
  const T ninf = -t_inf<T>();
  const int dl = tid % DB, d = d0b + dl, k0 = tid / DB;
  // the staged parameters of the thread's pairs (k0 + j KSTEP, d)
  T qp[PPT][NP];
#pragma unroll
  for (int j = 0; j < PPT; ++j) {
    const int kk = kc0 + k0 + j * KSTEP;
#pragma unroll
    for (int i = 0; i < NP; ++i) qp[j][i] = T(0);
    if (kk < K && d < D) E::par(p0[kk * P.p0_k + d * P.p0_d], p1 ? p1[kk * P.p1_k + d * P.p1_d] : T(0), qp[j]);
  }
  if constexpr (REDO) {                                 // (the record the plain launch wrote: R only in block 0)
    const double* was = rec + (((b * (int64_t)gridDim.y) + blockIdx.y) * gridDim.x + c) * ev_record(DB, NS);
    int odd = 0;
    for (int64_t e = tid + (db == 0 ? 0 : EV_KC); e < ev_record(DB, NS); e += EV_THREADS) {
      const double o = was[e];
      odd |= !(o - o == 0.0);
    }
    if (!__syncthreads_or(odd)) return;                 // (uniform over the workgroup)
  }
  double sacc[PPT][NS];
#pragma unroll
  for (int j = 0; j < PPT; ++j)
#pragma unroll
    for (int i = 0; i < NS; ++i) sacc[j][i] = 0.0;
  double racc = 0.0;                                    // R of component kc0 + tid (tid < EV_KC, block 0)
  const int64_t r0 = (int64_t)c * rows_per;
  const int64_t r1 = r0 + rows_per < N ? r0 + rows_per : N;
  for (int64_t base = r0; base < r1; base += EV_TR) {
    {
      double t[EV_KC], q;
      ev_rows<F, T>(x, r1, D, K, kc0, base, p0, P.p0_k, P.p0_d, p1, P.p1_k, P.p1_d, ck, xs, ps, t, false, q);
      const int64_t n = base + tid;
      const double l = n < r1 ? lse[n] : -t_inf<double>();
#pragma unroll
      for (int k = 0; k < EV_KC; ++k) {
        // (a row whose every term is -inf has no responsibilities; NaN in a row propagates)
        const T r = (l == -t_inf<double>() || kc0 + k >= K) ? T(0) : (T)exp(t[k] - l);
        rs[k * EV_TR + tid] = r;
      }
    }
    __syncthreads();
    if (db == 0 && tid < EV_KC) {
      double sr = 0.0;
      for (int n = 0; n < EV_TR; ++n) sr += (double)rs[tid * EV_TR + n];
      racc += sr;
    }
    for (int s0 = 0; s0 < EV_TR; s0 += TB) {
      if (base + s0 >= r1) break;                       // (uniform over the workgroup)
      __syncthreads();                                  // (the previous readers of xs are done)
      for (int e = tid; e < TB * DB; e += EV_THREADS) {
        const int rr = e / DB, cc = e % DB;
        const int64_t n = base + s0 + rr;
        T v[NX];
#pragma unroll
        for (int j = 0; j < NX; ++j) v[j] = T(0);
        if (n < r1 && d0b + cc < D) E::data(x[n * D + d0b + cc], v);
#pragma unroll
        for (int j = 0; j < NX; ++j) xs[(j * TB + rr) * DB + cc] = v[j];
      }
      __syncthreads();
      if (d < D) {
        T sp[PPT][NS];
#pragma unroll
        for (int j = 0; j < PPT; ++j)
#pragma unroll
          for (int i = 0; i < NS; ++i) sp[j][i] = T(0);
#pragma unroll
        for (int rr = 0; rr < TB; ++rr) {
          T v[NX];
#pragma unroll
          for (int i = 0; i < NX; ++i) v[i] = xs[(i * TB + rr) * DB + dl];
#pragma unroll
          for (int j = 0; j < PPT; ++j) {
            if constexpr (REDO) {
              const T r = rs[(k0 + j * KSTEP) * EV_TR + s0 + rr];
              if (r != T(0)) E::stat(v, qp[j], r, sp[j]);
            } else {
              E::stat(v, qp[j], rs[(k0 + j * KSTEP) * EV_TR + s0 + rr], sp[j]);
            }
          }
        }
#pragma unroll
        for (int j = 0; j < PPT; ++j)
#pragma unroll
          for (int i = 0; i < NS; ++i) sacc[j][i] += (double)sp[j][i];
      }
    }
  }
  // record: [k] = R_k (feature block 0), [EV_KC + (k DB + dl) NS + i] = the sums of pair (k, dl)
  double* out = rec + (((b * (int64_t)gridDim.y) + blockIdx.y) * gridDim.x + c) * ev_record(DB, NS);
  if (db == 0 && tid < EV_KC) out[tid] = racc;
#pragma unroll
  for (int j = 0; j < PPT; ++j)
#pragma unroll
    for (int i = 0; i < NS; ++i) out[EV_KC + ((int64_t)(k0 + j * KSTEP) * DB + dl) * NS + i] = sacc[j][i];
}

// out[b][0] = S, [1 + k] = R_k, [1 + K + k D + d] = dS/dp0_kd, [1 + K + K D + k D + d] = dS/dp1_kd (two-parameter
// families).  One wave per (k, 64 features, b): each lane adds the records of its feature in chunk order; R_k and S
// are lane-strided sums closed by the fixed DPP tree of wave_sum.  Deterministic.
constexpr int EV_FIN_THREADS = 64;
template <int F, typename T>
__global__ __launch_bounds__(EV_FIN_THREADS) void mixture_event_finalize_kernel(const double* __restrict__ spart,
                                                                                int g1, const double* __restrict__ rec,
                                                                                int chunks, int K, int D, int DB,
                                                                                int ndb, EvParams P,
                                                                                double* __restrict__ out) {
  using E = Ev<F, T>;
  constexpr int NS = E::NS;
  const int k = blockIdx.x, lane = threadIdx.x, kc = k / EV_KC, kl = k % EV_KC;
  const int64_t b = blockIdx.z;
  const int64_t J = ev_record(DB, NS);
  const int nkc = (K + EV_KC - 1) / EV_KC;
  const int64_t JO = 1 + K + (int64_t)K * D * E::NPAR;
  double* o = out + b * JO;
  auto recp = [&](int dbk, int cc) { return rec + ((((b * nkc) + kc) * ndb + dbk) * (int64_t)chunks + cc) * J; };
  double R = 0.0;
  for (int cc = lane; cc < chunks; cc += EV_FIN_THREADS) R += recp(0, cc)[kl];
  R = wave_sum(R);
  if (blockIdx.y == 0 && lane == 0) o[1 + k] = R;
  const int d = blockIdx.y * EV_FIN_THREADS + lane;
  if (d < D) {
    const int dbk = d / DB, dl = d % DB;
    double s[NS];
#pragma unroll
    for (int i = 0; i < NS; ++i) s[i] = 0.0;
    for (int cc = 0; cc < chunks; ++cc) {
      const double* rp = recp(dbk, cc) + EV_KC + ((int64_t)kl * DB + dl) * NS;
#pragma unroll
      for (int i = 0; i < NS; ++i) s[i] += rp[i];
    }
    const T* p0 = (const T*)P.p0 + b * P.p0_b + k * P.p0_k;
    const T* p1 = P.p1 ? (const T*)P.p1 + b * P.p1_b + k * P.p1_k : nullptr;
    double g[2];
    E::grad(R, s, (double)p0[d * P.p0_d], p1 ? (double)p1[d * P.p1_d] : 0.0, g);
    // (R == 0 exactly: no row has a responsibility for k, so there is no gradient, whatever the chain rule's factors
    //  are there -- 0 / 0 at a Poisson rate of 0; a NaN R is handed on)
    if (R == 0.0) g[0] = g[1] = 0.0;
    o[1 + K + (int64_t)k * D + d] = g[0];
    if (E::NPAR == 2) o[1 + K + (int64_t)K * D + (int64_t)k * D + d] = g[1];
  }
  if (k == 0 && blockIdx.y == 0) {
    double v = 0.0;
    for (int q = lane; q < g1; q += EV_FIN_THREADS) v += spart[b * g1 + q];
    v = wave_sum(v);
    if (lane == 0) o[0] = v;
  }
}

template <int F, typename T, int DB>
static int mixture_event_launch(const T* x, int64_t N, int D, int K, int64_t B, const T* a, int64_t a_bs,
                                const EvParams& P, double* row_lse, double* ws, size_t ws_bytes, double* out,
                                hipStream_t s) {
  constexpr int NS = Ev<F, T>::NS;
  const int nkc = (K + EV_KC - 1) / EV_KC, ndb = (D + DB - 1) / DB;
  int64_t g1 = (N + EV_TR - 1) / EV_TR;
  if (g1 > ev_lse_blocks_max(B)) g1 = ev_lse_blocks_max(B);
  int64_t chunks = (N + EV_TR - 1) / EV_TR;
  if (chunks > ev_chunks_max(K, D, B, NS)) chunks = ev_chunks_max(K, D, B, NS);
  int64_t rows_per = (N + chunks - 1) / chunks;
  rows_per = (rows_per + EV_TR - 1) / EV_TR * EV_TR;
  const int64_t need = (B * K + B * g1 + B * nkc * ndb * chunks * ev_record(DB, NS)) * (int64_t)sizeof(double);
  PA_REQUIRE((size_t)need <= ws_bytes, "mixture_event_fwd_bwd: records need %lld bytes, workspace has %zu",
             (long long)need, ws_bytes);
  PA_REQUIRE(chunks <= 65535 && (int64_t)nkc * ndb <= 65535, "mixture_event_fwd_bwd: grid");
  double* ck = ws;
  double* spart = ws + B * K;
  double* rec = spart + B * g1;
  hipLaunchKernelGGL((mixture_event_prep_kernel<F, T>), dim3((unsigned)K, (unsigned)B), dim3(EV_THREADS), 0, s, D, K,
                     a, a_bs, P, ck);
  hipLaunchKernelGGL((mixture_event_lse_kernel<F, T>), dim3((unsigned)g1, (unsigned)B), dim3(EV_THREADS), 0, s, x, N,
                     D, K, P, (const double*)ck, row_lse, spart);
  hipLaunchKernelGGL((mixture_event_stats_kernel<F, T, DB, false>),
                     dim3((unsigned)chunks, (unsigned)(nkc * ndb), (unsigned)B), dim3(EV_THREADS), 0, s, x, N, D, K, P,
                     (const double*)ck, (const double*)row_lse, rows_per, ndb, rec);
  hipLaunchKernelGGL((mixture_event_stats_kernel<F, T, DB, true>),
                     dim3((unsigned)chunks, (unsigned)(nkc * ndb), (unsigned)B), dim3(EV_THREADS), 0, s, x, N, D, K, P,
                     (const double*)ck, (const double*)row_lse, rows_per, ndb, rec);
  hipLaunchKernelGGL((mixture_event_finalize_kernel<F, T>),
                     dim3((unsigned)K, (unsigned)((D + EV_FIN_THREADS - 1) / EV_FIN_THREADS), (unsigned)B),
                     dim3(EV_FIN_THREADS), 0, s,
                     (const double*)spart, (int)g1, (const double*)rec, (int)chunks, K, D, DB, ndb, P, out);
  return check_launch("mixture_event_kernel");
}

template <int F, typename T>
static int mixture_event_f(const T* x, int64_t N, int D, int K, int64_t B, const T* a, int64_t a_bs,
                           const EvParams& P, double* row_lse, double* ws, size_t ws_bytes, double* out,
                           hipStream_t s) {
  switch (ev_block_d(D)) {
    case 16: return mixture_event_launch<F, T, 16>(x, N, D, K, B, a, a_bs, P, row_lse, ws, ws_bytes, out, s);
    case 64: return mixture_event_launch<F, T, 64>(x, N, D, K, B, a, a_bs, P, row_lse, ws, ws_bytes, out, s);
    default: return mixture_event_launch<F, T, 256>(x, N, D, K, B, a, a_bs, P, row_lse, ws, ws_bytes, out, s);
  }
}

template <typename T>
static int mixture_event_t(int dist, const T* x, int64_t N, int D, int K, int64_t B, const T* a, int64_t a_bs,
                           const EvParams& P, double* row_lse, double* ws, size_t ws_bytes, double* out,
                           hipStream_t s) {
  switch (dist) {
#define PA_EV_CASE(F_) \
  case F_: return mixture_event_f<F_, T>(x, N, D, K, B, a, a_bs, P, row_lse, ws, ws_bytes, out, s);
    PA_EV_CASE(PA_DIST_NORMAL) PA_EV_CASE(PA_DIST_LOG_NORMAL) PA_EV_CASE(PA_DIST_EXPONENTIAL)
    PA_EV_CASE(PA_DIST_BERNOULLI_LOGITS) PA_EV_CASE(PA_DIST_POISSON) PA_EV_CASE(PA_DIST_GAMMA)
#undef PA_EV_CASE
  }
  return fail(PA_ERR_UNSUPPORTED, "mixture_event_fwd_bwd: distribution %d", dist);
}

}  // namespace pa

extern "C" {

int64_t pa_mixture_event_layout(int dist, int K, int D) {
  if (!pa::ev_family(dist) || K < 1 || K > pa::EV_MAXK || D < 1 || D > pa::EV_MAXD) return 0;
  return 1 + K + (int64_t)K * D * pa::ev_npar(dist);
}

size_t pa_mixture_event_workspace(int dist, int K, int D, int64_t B) {
  if (!pa::ev_family(dist) || K < 1 || K > pa::EV_MAXK || D < 1 || D > pa::EV_MAXD || B < 1 || B > 65535) return 0;
  const int NS = pa::ev_npar(dist) == 2 ? 2 : 1;
  const int DB = pa::ev_block_d(D);
  const int64_t groups = B * ((K + pa::EV_KC - 1) / pa::EV_KC) * ((D + DB - 1) / DB);
  return (size_t)(B * K + B * pa::ev_lse_blocks_max(B) +
                  groups * pa::ev_chunks_max(K, D, B, NS) * pa::ev_record(DB, NS)) * sizeof(double);
}

int pa_mixture_event_fwd_bwd(int dtype, int dist, const void* x, int64_t N, int D, int K, int64_t B, const void* a,
                             int64_t a_batch_stride, const void* p0, int64_t p0_stride_k, int64_t p0_stride_d,
                             int64_t p0_batch_stride, const void* p1, int64_t p1_stride_k, int64_t p1_stride_d,
                             int64_t p1_batch_stride, void* row_lse, void* workspace, size_t workspace_bytes,
                             double* out, pa_stream_t stream) {
  PA_REQUIRE(pa::ev_family(dist), "mixture_event_fwd_bwd: distribution %d", dist);
  PA_REQUIRE(K >= 1 && K <= pa::EV_MAXK && D >= 1 && D <= pa::EV_MAXD,
             "mixture_event_fwd_bwd: K=%d (<= %d), D=%d (<= %d)", K, pa::EV_MAXK, D, pa::EV_MAXD);
  PA_REQUIRE(B >= 1 && B <= 65535, "mixture_event_fwd_bwd: B=%lld outside [1, 65535]", (long long)B);
  PA_REQUIRE(N >= 1 && x && a && p0 && row_lse && out && workspace, "mixture_event_fwd_bwd: NULL pointer or N < 1");
  PA_REQUIRE((p1 != nullptr) == (pa::ev_npar(dist) == 2), "mixture_event_fwd_bwd: p1 %s for distribution %d",
             p1 ? "given" : "missing", dist);
  PA_REQUIRE(a_batch_stride >= 0 && p0_stride_k >= 0 && p0_stride_d >= 0 && p0_batch_stride >= 0 &&
                 p1_stride_k >= 0 && p1_stride_d >= 0 && p1_batch_stride >= 0,
             "mixture_event_fwd_bwd: negative stride");
  PA_REQUIRE(workspace_bytes >= pa_mixture_event_workspace(dist, K, D, B),
             "mixture_event_fwd_bwd: workspace too small");
  const pa::EvParams P{p0, p0_stride_k, p0_stride_d, p0_batch_stride, p1, p1_stride_k, p1_stride_d, p1_batch_stride};
  hipStream_t s = pa::as_stream(stream);
  if (dtype == PA_F32)
    return pa::mixture_event_t<float>(dist, (const float*)x, N, D, K, B, (const float*)a, a_batch_stride, P,
                                      (double*)row_lse, (double*)workspace, workspace_bytes, out, s);
  if (dtype == PA_F64)
    return pa::mixture_event_t<double>(dist, (const double*)x, N, D, K, B, (const double*)a, a_batch_stride, P,
                                       (double*)row_lse, (double*)workspace, workspace_bytes, out, s);
  return pa::fail(PA_ERR_UNSUPPORTED, "mixture_event_fwd_bwd: dtype %d", dtype);
}

}  // extern "C"
