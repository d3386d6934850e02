// gaussian_hmm.hip -- a linear-Gaussian state-space likelihood and its gradient in ONE launch.
//
// Reference path replaced: GaussianHMM.log_prob (pyro/distributions/hmm.py:434-741) eliminates the time axis with
// sequential_gaussian_tensordot (pyro/ops/gaussian.py): O(log T) rounds of batched Cholesky-based Gaussian
// contractions, and autograd differentiates through every one of them -- hundreds of small launches per gradient
// for a few hundred steps.  Here (row vectors, as the reference writes the model)
//     z_0 ~ N(m0, P0),   z_t = z_{t-1} F_t + N(q_t, Q_t),   x_t = z_t H_t + N(r_t, R_t),   t = 1..T
// one wave per sequence runs the Kalman filter forward and, when gradients are asked for, the adjoint of that filter
// backward in the same launch: the derivative of the filter's own arithmetic, step by step.  (Until the edge tests the
// sweep was the Rauch-Tung-Striebel smoother with the expected complete-data score as the gradient -- Fisher's
// identity: exact, but differences sandwiched between Q^-1, R^-1 and P0^-1, which cost float32 up to all of its digits
// when R is small or P0 large and a factor of ten where the hidden dimension exceeds the observed one.)
//
// Forward: the filter of gaussian_hmm.h (GhFilter: the recurrence, where P^p is symmetrised, the bad-pivot rule), shared
// with gaussian_hmm_sample.hip; per step this kernel adds  log_prob += -|v|^2 / 2 - sum log diag L - obs / 2 log 2 pi.
// A sequence the filter marks (a non-positive or NaN pivot of S) has NaN log_prob, filter outputs and gradients, no
// other sequence sees it.  The backward sweep marks a sequence the same way on a bad pivot of P^p, Q, R or P0
// (gradients only: log_prob is what the forward pass alone gives).
//
// Backward, per step t = T..1, from the filtered (m_{t-1}, P_{t-1}) kept in the workspace (hidden + hidden^2
// elements per step; the predicted moments, S, the gain K = P^p H S^-1 and w = S^-1 y are recomputed), with
// (mu, M) = d l_{>t} / d (m_t, P_t) carried down (zero at t = T; at the end the gradients of m0 and P0):
//     rho = w - K^T mu = d/dr = -d/dx,   Sigma = (rho rho^T - S^-1) / 2 + K^T (M - mu mu^T / 2) K = d/dR,
//     d/dH = m^p rho^T + (P^p mu) w^T + 2 P^p H Sigma - 2 P^p M K,
//     lambda = H rho + mu = d/dq,   Lambda = H Sigma H^T + sym(mu (H w)^T) + M - M K H^T - H K^T M = d/dQ,
//     d/dF = m_{t-1} lambda^T + 2 P_{t-1} F Lambda,   mu <- F lambda,   M <- F Lambda F^T.
// No inverse but S^-1 enters; the sums accumulate in double also for float32.  The pivots of P^p, Q, R and P0 are
// still checked (a Cholesky sweep over a copy) for the NaN convention above.  A parameter with step stride 0 has its
// gradient summed over the steps in registers, in the order of the sweep (t = T down to 1) -- a fixed order, no
// atomics: bit-reproducible.
//
// Mapping: the block is ONE wave; every matrix lives in LDS with row stride MD + 1 (MD = 8 or 16: the padded
// dimension; the odd stride keeps both the row- and the column-indexed accesses of the 64 lanes off each other's
// banks), a lane owns MD^2 / 64 elements of every matrix product, the triangular solves give a lane one right-hand
// side each.  The next step's x, heterogeneous parameters and (backward) filtered moments are loaded into registers
// while the current step computes and are written to LDS at the top of the next step.
//
// The Student-t variant (template parameter ST; pa_gamma_gaussian_hmm_fwd_bwd, reference: GammaGaussianHMM.log_prob,
// pyro/distributions/hmm.py:744-940): every covariance of the model divided by one s ~ Gamma(a, b) per series.  The
// filter's means, gains and P / P^p ratios do not depend on s, so the forward pass is the same filter at unit scale; it
// keeps  quad = sum_t |v_t|^2  and  logdet = sum_t sum log diag L_t  apart (both in double) and writes them instead of
// log_prob, which the caller forms:  lgamma(a + n/2) - lgamma(a) + a log b - (a + n/2) log(b + quad/2) - logdet -
// n/2 log 2 pi,  n = T obs.  With w = (a + n/2) / (b + quad/2) held constant, the gradient with respect to m0, F, q,
// H, r, x is that of the GAUSSIAN model at P0 / w, Q_t / w, R_t / w, and with respect to P0, Q_t, R_t it is 1 / w times
// that model's with respect to its scaled covariance.  So the wave forms w from its series' a, b and runs the sweep
// below unchanged: P0, Q, R and the filtered covariances read back from the workspace are multiplied by 1 / w on their
// way into LDS, the three covariance gradients on their way out.  d/da and d/db are closed forms of quad, the caller's.
//
// gfx950 cross-compile (hipcc -O3, -Rpass-analysis=kernel-resource-usage), one wave of 64 lanes per block:
//     instantiation    VGPRs      SGPRs  scratch   LDS bytes   waves / SIMD
//     <float , 8>      135        106    0         5832        3
//     <float , 16>     256 + 5    106    0         21384       1
//     <double, 8>      168        106    0         11664       2
//     <double, 16>     256 + 60   106    0         42768       1
// (+ n: accumulation registers the 16-wide instantiations use as spill space; nothing goes to scratch memory)
// With the Student-t template parameter the four Gaussian instantiations <., ., false> compile to the same figures
// (135 / 256 + 5 / 168 / 256 + 60 VGPRs, 106 SGPRs, scratch 0, the same LDS); the Student-t ones:
//     <float , 8 , true>   161        106    0         5832        3
//     <float , 16, true>   256 + 8    106    0         21384       1
//     <double, 8 , true>   170        106    0         11664       2
//     <double, 16, true>   256 + 61   106    0         42768       1
#include <limits>

#include "common.h"
#include "gaussian_hmm.h"

namespace pa {

struct GhmmArgs {
  GhModel m;
  int grads;
  void *lp, *fm, *fP, *g_m0, *g_P0, *g_F, *g_q, *g_Q, *g_H, *g_r, *g_R, *g_x, *ws;
  // the Student-t variant alone: the Gamma's concentration and rate ([B | 1], batch stride 0 or 1); it writes quad
  // and logdet instead of lp
  const void *ga, *gb;
  int64_t ga_sb, gb_sb;
  void *quad, *logdet;
};

// ST: the Student-t variant (see the top of the file)
template <typename T, int MD, bool ST>
__global__ __launch_bounds__(64) void gaussian_hmm_kernel(const GhmmArgs a) {
  constexpr int LD = MD + 1, MS = MD * LD, EPL = MD * MD / 64;
  constexpr int NMAT = 19, NVEC = 11;
  __shared__ T sm[NMAT * MS + NVEC * MD + 2];
  const int lane = threadIdx.x;
  const int64_t b = blockIdx.x;
  GhFilter<T, MD> f(a.m, sm, sm + NMAT * MS, sm + NMAT * MS + NVEC * MD, lane, b);
  // the filter's matrices (backward: sP = P_{t-1}, sPp late R^-1 V, sA = G^T, sB and sC temporaries) ...
  T *const sP = f.sP, *const sF = f.sF, *const sQ = f.sQ, *const sH = f.sH, *const sR = f.sR, *const sPp = f.sPp,
    *const sL = f.sL, *const sA = f.sA, *const sB = f.sB, *const sC = f.sC;
  T* const sX = sC + MS;       // ... and the sweep's behind them: cross-covariance C_t
  T* const sPs = sX + MS;      // smoothed covariance Ps_t
  T* const sPm = sPs + MS;     // Ps_{t-1}
  T* const sM = sPm + MS;
  T* const sE = sM + MS;
  T* const sQi = sE + MS;      // Q^-1 (at the end: P0^-1)
  T* const sRi = sQi + MS;     // R^-1
  T* const sN = sRi + MS;
  T* const sV = sN + MS;
  T *const vm = f.vm, *const vq = f.vq, *const vr = f.vr, *const vx = f.vx, *const vmp = f.vmp;
  T* const vzs = f.vy + MD;    // zbar_t
  T* const vzp = vzs + MD;     // zbar_{t-1}
  T* const vd = vzp + MD;
  T* const ve = vd + MD;       // ebar
  T* const vu = ve + MD;       // ubar

  const int h = a.m.h, o = a.m.o, Tn = a.m.T, hh = h * h, ho = h * o, oo = o * o;
  const T NaN = std::numeric_limits<T>::quiet_NaN();
  const auto& lhh = f.lhh;
  const auto& lho = f.lho;
  const auto& loo = f.loo;
  bool& bad = f.bad;
  const int64_t wstep = h + hh;
  T* wsb = a.grads ? (T*)a.ws + b * (int64_t)Tn * wstep : nullptr;

  // ---- forward: the Kalman filter ----------------------------------------------------------------------------
  f.start();
  double lp = 0.0;               // (in double also for float32: T terms of one sign, |log_prob| grows with T)
  double quad = 0.0, lds = 0.0;  // (ST: the two halves of lp kept apart)
  const T half_log_2pi_o = T(0.91893853320467274178) * T(o);
  for (int t = 0; t < Tn; ++t) {
    const T logdet = f.step(t, a.grads ? wsb + (int64_t)t * wstep : nullptr);
    if constexpr (ST) {
      quad += (double)f.sc[0];
      lds += (double)logdet;
    } else {
      lp += (double)(T(-0.5) * f.sc[0] - logdet - half_log_2pi_o);
    }
  }
  __syncthreads();
  if constexpr (ST) {
    if (lane == 0) {
      ((T*)a.quad)[b] = bad ? NaN : (T)quad;
      ((T*)a.logdet)[b] = bad ? NaN : (T)lds;
    }
  } else {
    if (lane == 0) ((T*)a.lp)[b] = bad ? NaN : (T)lp;
  }
  if (a.fm && lane < h) ((T*)a.fm)[b * h + lane] = bad ? NaN : vm[lane];
  if (a.fP) {
#pragma unroll
    for (int k = 0; k < EPL; ++k)
      if (lhh[k] >= 0) ((T*)a.fP)[b * hh + lane + 64 * k] = bad ? NaN : sP[lhh[k]];
  }
  if (!a.grads) return;

  // ---- backward: the Rauch-Tung-Striebel sweep and the expected complete-data score ---------------------------
  T* const gm0 = (T*)a.g_m0 + b * h;
  T* const gP0 = (T*)a.g_P0 + b * hh;
  const int64_t TF = a.m.F_ss ? Tn : 1, Tq = a.m.q_ss ? Tn : 1, TQ = a.m.Q_ss ? Tn : 1, TH = a.m.H_ss ? Tn : 1,
                Tr = a.m.r_ss ? Tn : 1, TR = a.m.R_ss ? Tn : 1;
  T* const gF = (T*)a.g_F + b * TF * hh;
  T* const gq = (T*)a.g_q + b * Tq * h;
  T* const gQ = (T*)a.g_Q + b * TQ * hh;
  T* const gH = (T*)a.g_H + b * TH * ho;
  T* const gr = (T*)a.g_r + b * Tr * o;
  T* const gR = (T*)a.g_R + b * TR * oo;
  T* const gx = (T*)a.g_x + b * (int64_t)Tn * o;
  // every gradient element is written by ONE lane (element e by lane e % 64, a vector's by lane e): the NaN fill
  // of a marked sequence comes after that lane's own stores in program order
  auto fill_nan = [&]() {
    if (lane < h) gm0[lane] = NaN;
    for (int64_t t = 0; t < Tq; ++t)
      if (lane < h) gq[t * h + lane] = NaN;
    for (int64_t t = 0; t < Tr; ++t)
      if (lane < o) gr[t * o + lane] = NaN;
    for (int64_t t = 0; t < Tn; ++t)
      if (lane < o) gx[t * o + lane] = NaN;
#pragma unroll
    for (int k = 0; k < EPL; ++k) {
      const int e = lane + 64 * k;
      if (lhh[k] >= 0) {
        gP0[e] = NaN;
        for (int64_t t = 0; t < TF; ++t) gF[t * hh + e] = NaN;
        for (int64_t t = 0; t < TQ; ++t) gQ[t * hh + e] = NaN;
      }
      if (lho[k] >= 0)
        for (int64_t t = 0; t < TH; ++t) gH[t * ho + e] = NaN;
      if (loo[k] >= 0)
        for (int64_t t = 0; t < TR; ++t) gR[t * oo + e] = NaN;
    }
  };
  if (bad) {
    fill_nan();
    return;
  }
  // a pivot check alone: the Cholesky sweep over a copy of the n x n matrix ``src`` in sL; ends with a barrier
  auto check_pivots = [&](const T* src, int n, const int (&own)[EPL]) {
#pragma unroll
    for (int k = 0; k < EPL; ++k)
      if (own[k] >= 0) sL[own[k]] = src[own[k]];
    __syncthreads();
    gh_cholesky<T, MD>(sL, n, lane, bad);
    __syncthreads();
  };

  using AT = double;             // the sweep's sums accumulate in double, also for float32
  T* const sMa = sPs;            // M = d l_{>t} / d P_t, carried down the sweep
  T* const sLa = sPm;            // Lambda = d l / d P^p_t
  T* const sFL = sM;             // F Lambda
  T* const sPH = sE;             // P^p H
  T* const sK = sB;              // the gain K = P^p H S^-1
  T* const sMK = sQi;            // M K
  T* const sSi = sRi;            // S^-1
  T* const sSg = sV;             // Sigma = d l / d S_t
  T* const sHS = sX;             // H Sigma
  T* const vw = f.vy;            // S^-1 y
  T* const vmu = vzs;            // mu = d l_{>t} / d m_t, carried down the sweep
  T* const vla = vzp;            // lambda = d l / d m^p_t
  T* const vpm = vd;             // P^p mu
  T* const vhw = ve;             // H w
  T* const vrho = vu;            // rho = w - K^T mu

  // ST: the sweep is the Gaussian model's at P0 / w, Q_t / w, R_t / w with w = (a + n / 2) / (b + quad / 2) held
  // constant; iw = 1 / w scales those three and the filtered covariances on their way into LDS and the three
  // covariance gradients on their way out.  (A lane scales the elements it wrote itself: no barrier in between.)
  T iw = T(1);
  if constexpr (ST) {
    const double ca = ((const T*)a.ga)[b * a.ga_sb], cb = ((const T*)a.gb)[b * a.gb_sb];
    iw = (T)((cb + 0.5 * quad) / (ca + 0.5 * (double)Tn * (double)o));
#pragma unroll
    for (int k = 0; k < EPL; ++k) {          // the time-homogeneous ones: in LDS since the first step of the filter
      if (!a.m.Q_ss && lhh[k] >= 0) sQ[lhh[k]] *= iw;
      if (!a.m.R_ss && loo[k] >= 0) sR[loo[k]] *= iw;
    }
  }
  if (lane < h) vmu[lane] = T(0);
#pragma unroll
  for (int k = 0; k < EPL; ++k)
    if (lhh[k] >= 0) sMa[lhh[k]] = T(0);
  __syncthreads();
  if (!a.m.Q_ss) check_pivots(sQ, h, lhh);
  if (!a.m.R_ss) check_pivots(sR, o, loo);

  T aF[EPL], aQ[EPL], aH[EPL], aR[EPL], aq = T(0), ar = T(0);
#pragma unroll
  for (int k = 0; k < EPL; ++k) aF[k] = aQ[k] = aH[k] = aR[k] = T(0);

  auto load_filtered = [&](int t) {          // (m_{t-1}, P_{t-1}) of 0-based step t
    if (t == 0) {
      if (lane < h) f.pm = f.m0b[lane];
#pragma unroll
      for (int k = 0; k < EPL; ++k)
        if (lhh[k] >= 0) f.pP[k] = f.P0b[lane + 64 * k];
    } else {
      const T* w = wsb + (int64_t)(t - 1) * wstep;
      if (lane < h) f.pm = w[lane];
#pragma unroll
      for (int k = 0; k < EPL; ++k)
        if (lhh[k] >= 0) f.pP[k] = w[h + lane + 64 * k];
    }
  };
  // (the forward pass wrote the workspace with the lanes that read it back here: same lane, same address)
  f.load_params(Tn - 1, false, true);
  load_filtered(Tn - 1);
  for (int t = Tn - 1; t >= 0; --t) {
    __syncthreads();
    f.commit_params(false, true);
    if (lane < h) vm[lane] = f.pm;
#pragma unroll
    for (int k = 0; k < EPL; ++k) {
      if (lhh[k] >= 0) sP[lhh[k]] = ST ? f.pP[k] * iw : f.pP[k];
      if constexpr (ST) {
        if (a.m.Q_ss && lhh[k] >= 0) sQ[lhh[k]] = f.pQ[k] * iw;
        if (a.m.R_ss && loo[k] >= 0) sR[loo[k]] = f.pR[k] * iw;
      }
    }
    if (t > 0) {
      f.load_params(t - 1, false, true);
      load_filtered(t - 1);
    }
    __syncthreads();
    if (a.m.Q_ss) check_pivots(sQ, h, lhh);
    if (a.m.R_ss) check_pivots(sR, o, loo);
    f.predict(sL);                                                 // vmp, sPp (and a copy in sL), sA = F^T P_{t-1}
    gh_cholesky<T, MD>(sL, h, lane, bad);                          // (the pivots of P^p)
    __syncthreads();
    // the step's update once more: y, P^p H, S = L L^T, K, w = S^-1 y, S^-1
    if (lane < o) {
      T s = vx[lane] - vr[lane];
      for (int j = 0; j < h; ++j) s -= vmp[j] * sH[j * LD + lane];
      vw[lane] = s;
    }
#pragma unroll
    for (int k = 0; k < EPL; ++k) {
      if (lho[k] >= 0) {
        const int j = lho[k] / LD, c = lho[k] % LD;
        T s = T(0);
        for (int i = 0; i < h; ++i) s += sPp[j * LD + i] * sH[i * LD + c];
        sPH[lho[k]] = s;
        sK[lho[k]] = s;
      }
      if (loo[k] >= 0) sSi[loo[k]] = loo[k] / LD == loo[k] % LD ? T(1) : T(0);
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < EPL; ++k)
      if (loo[k] >= 0) {
        const int r_ = loo[k] / LD, c = loo[k] % LD;
        T s = sR[loo[k]];
        for (int j = 0; j < h; ++j) s += sH[j * LD + r_] * sPH[j * LD + c];
        sL[loo[k]] = s;
      }
    __syncthreads();
    gh_cholesky<T, MD>(sL, o, lane, bad);
    if (lane < h) {                                              // row j of K
      gh_forward_sub<T, LD>(sL, sK + lane * LD, 1, o);
      gh_backward_sub<T, LD>(sL, sK + lane * LD, 1, o);
    } else if (lane == h) {
      gh_forward_sub<T, LD>(sL, vw, 1, o);
      gh_backward_sub<T, LD>(sL, vw, 1, o);
    } else if (lane <= h + o) {
      gh_forward_sub<T, LD>(sL, sSi + (lane - h - 1), LD, o);
      gh_backward_sub<T, LD>(sL, sSi + (lane - h - 1), LD, o);
    }
    __syncthreads();
    if (lane < o) {                                              // rho = w - K^T mu
      AT s = vw[lane];
      for (int j = 0; j < h; ++j) s -= (AT)sK[j * LD + lane] * vmu[j];
      vrho[lane] = s;
    }
    if (lane < h) {                                              // H w, P^p mu
      AT s = AT(0), s2 = AT(0);
      for (int c = 0; c < o; ++c) s += (AT)sH[lane * LD + c] * vw[c];
      for (int i = 0; i < h; ++i) s2 += (AT)sPp[lane * LD + i] * vmu[i];
      vhw[lane] = s;
      vpm[lane] = s2;
    }
#pragma unroll
    for (int k = 0; k < EPL; ++k)
      if (lho[k] >= 0) {                                         // M K
        const int j = lho[k] / LD, c = lho[k] % LD;
        AT s = AT(0);
        for (int i = 0; i < h; ++i) s += (AT)sMa[j * LD + i] * sK[i * LD + c];
        sMK[lho[k]] = s;
      }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < EPL; ++k)
      if (loo[k] >= 0) {                 // Sigma = (rho rho^T - S^-1) / 2 + K^T (M - mu mu^T / 2) K
        const int r_ = loo[k] / LD, c = loo[k] % LD;
        const AT kr = (AT)vw[r_] - vrho[r_], kc = (AT)vw[c] - vrho[c];
        AT s = AT(0.5) * ((AT)vrho[r_] * vrho[c] - sSi[loo[k]] - kr * kc);
        for (int j = 0; j < h; ++j) s += (AT)sK[j * LD + r_] * sMK[j * LD + c];
        sSg[loo[k]] = s;
      }
    if (lane < h) {                                              // lambda = H rho + mu
      AT s = vmu[lane];
      for (int c = 0; c < o; ++c) s += (AT)sH[lane * LD + c] * vrho[c];
      vla[lane] = s;
    }
    __syncthreads();
    if (lane < o) {                                              // d/dr = rho = -d/dx
      const T s = vrho[lane];
      if (a.m.r_ss) gr[(int64_t)t * o + lane] = s; else ar += s;
      gx[(int64_t)t * o + lane] = -s;
    }
    if (lane < h) {                                              // d/dq = lambda
      const T s = vla[lane];
      if (a.m.q_ss) gq[(int64_t)t * h + lane] = s; else aq += s;
    }
#pragma unroll
    for (int k = 0; k < EPL; ++k) {
      const int e = lane + 64 * k;
      if (loo[k] >= 0) {                                         // d/dR = Sigma
        const T s = ST ? sSg[loo[k]] * iw : sSg[loo[k]];
        if (a.m.R_ss) gR[(int64_t)t * oo + e] = s; else aR[k] += s;
      }
      if (lho[k] >= 0) {
        const int j = lho[k] / LD, c = lho[k] % LD;
        // d/dH = m^p rho^T + (P^p mu) w^T + 2 P^p H Sigma - 2 P^p M K;  sHS = H Sigma
        AT s = (AT)vmp[j] * vrho[c] + (AT)vpm[j] * vw[c], s2 = AT(0), s3 = AT(0);
        for (int i = 0; i < o; ++i) {
          s2 += (AT)sPH[j * LD + i] * sSg[i * LD + c];
          s3 += (AT)sH[j * LD + i] * sSg[i * LD + c];
        }
        for (int i = 0; i < h; ++i) s2 -= (AT)sPp[j * LD + i] * sMK[i * LD + c];
        s += AT(2) * s2;
        if (a.m.H_ss) gH[(int64_t)t * ho + e] = s; else aH[k] += s;
        sHS[lho[k]] = s3;
      }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < EPL; ++k) {
      const int e = lane + 64 * k;
      if (lhh[k] >= 0) {
        // Lambda = H Sigma H^T + (mu (H w)^T + (H w) mu^T) / 2 + M - M K H^T - H K^T M = d/dQ
        const int j = lhh[k] / LD, c = lhh[k] % LD;
        AT s = sMa[lhh[k]] + AT(0.5) * ((AT)vmu[j] * vhw[c] + (AT)vhw[j] * vmu[c]);
        for (int i = 0; i < o; ++i)
          s += ((AT)sHS[j * LD + i] - sMK[j * LD + i]) * sH[c * LD + i] - (AT)sMK[c * LD + i] * sH[j * LD + i];
        sLa[lhh[k]] = s;
        if constexpr (ST) s *= iw;
        if (a.m.Q_ss) gQ[(int64_t)t * hh + e] = s; else aQ[k] += s;
      }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < EPL; ++k)
      if (lhh[k] >= 0) {                                         // F Lambda
        const int j = lhh[k] / LD, c = lhh[k] % LD;
        AT s = AT(0);
        for (int i = 0; i < h; ++i) s += (AT)sF[j * LD + i] * sLa[i * LD + c];
        sFL[lhh[k]] = s;
      }
    __syncthreads();
    T nM[EPL];
    AT nmu = AT(0);
#pragma unroll
    for (int k = 0; k < EPL; ++k) {
      const int e = lane + 64 * k;
      nM[k] = T(0);
      if (lhh[k] >= 0) {                 // d/dF = m_{t-1} lambda^T + 2 P_{t-1} F Lambda;  M_{t-1} = F Lambda F^T
        const int j = lhh[k] / LD, c = lhh[k] % LD;
        AT s = AT(0), s2 = AT(0);
        for (int i = 0; i < h; ++i) {
          s += (AT)sP[j * LD + i] * sFL[i * LD + c];
          s2 += (AT)sFL[j * LD + i] * sF[c * LD + i];
        }
        s = (AT)vm[j] * vla[c] + AT(2) * s;
        if (a.m.F_ss) gF[(int64_t)t * hh + e] = s; else aF[k] += s;
        nM[k] = s2;
      }
    }
    if (lane < h)                                                // mu_{t-1} = F lambda
      for (int c = 0; c < h; ++c) nmu += (AT)sF[lane * LD + c] * vla[c];
    __syncthreads();
    if (lane < h) vmu[lane] = nmu;
#pragma unroll
    for (int k = 0; k < EPL; ++k)
      if (lhh[k] >= 0) sMa[lhh[k]] = nM[k];
  }
  __syncthreads();
  // the step-summed gradients of the time-homogeneous parameters
  if (!a.m.q_ss && lane < h) gq[lane] = aq;
  if (!a.m.r_ss && lane < o) gr[lane] = ar;
#pragma unroll
  for (int k = 0; k < EPL; ++k) {
    const int e = lane + 64 * k;
    if (lhh[k] >= 0) {
      if (!a.m.F_ss) gF[e] = aF[k];
      if (!a.m.Q_ss) gQ[e] = aQ[k];
    }
    if (lho[k] >= 0 && !a.m.H_ss) gH[e] = aH[k];
    if (loo[k] >= 0 && !a.m.R_ss) gR[e] = aR[k];
  }
  // the initial state: (mu_0, M_0) are its gradients; sP holds P0 since step 1 of the sweep
  if (lane < h) gm0[lane] = vmu[lane];
#pragma unroll
  for (int k = 0; k < EPL; ++k)
    if (lhh[k] >= 0) gP0[lane + 64 * k] = ST ? sMa[lhh[k]] * iw : sMa[lhh[k]];
  check_pivots(sP, h, lhh);
  if (bad) fill_nan();
}

// what the two entry points share: the checks, the workspace and the launch (``who`` names the entry point in errors)
static int ghmm_launch(const char* who, bool student, int dtype, GhmmArgs& a, int64_t B, int64_t T, int64_t hidden,
                       int64_t obs, size_t workspace_bytes, pa_stream_t stream) {
  const GhModel& m = a.m;
  PA_REQUIRE(dtype == PA_F32 || dtype == PA_F64, "%s: bad dtype %d", who, dtype);
  PA_REQUIRE(B >= 0 && T >= 1 && hidden >= 1 && obs >= 1, "%s: bad shape B=%lld T=%lld hidden=%lld obs=%lld", who,
             (long long)B, (long long)T, (long long)hidden, (long long)obs);
  if (hidden > GH_MAXHIDDEN || obs > GH_MAXOBS)
    return fail(PA_ERR_UNSUPPORTED, "%s: hidden=%lld obs=%lld over the limit of %d / %d", who, (long long)hidden,
                (long long)obs, GH_MAXHIDDEN, GH_MAXOBS);
  PA_REQUIRE(B < (int64_t(1) << 31) && T < (int64_t(1) << 31), "%s: shape too large", who);
  if (B == 0) return PA_OK;
  PA_REQUIRE(m.m0 && m.P0 && m.F && m.q && m.Q && m.H && m.r && m.R && m.x, "%s: NULL pointer", who);
  if (student) {
    PA_REQUIRE(a.ga && a.gb && a.quad && a.logdet, "%s: NULL pointer", who);
    PA_REQUIRE((a.ga_sb == 0 || a.ga_sb == 1) && (a.gb_sb == 0 || a.gb_sb == 1),
               "%s: concentration and rate are [B | 1], batch stride 0 or 1", who);
  } else {
    PA_REQUIRE(a.lp, "%s: NULL pointer", who);
  }
  PA_REQUIRE((a.fm == nullptr) == (a.fP == nullptr), "%s: filter mean and covariance go together", who);
  const int ng = (a.g_m0 != nullptr) + (a.g_P0 != nullptr) + (a.g_F != nullptr) + (a.g_q != nullptr) +
                 (a.g_Q != nullptr) + (a.g_H != nullptr) + (a.g_r != nullptr) + (a.g_R != nullptr) +
                 (a.g_x != nullptr);
  PA_REQUIRE(ng == 0 || ng == 9, "%s: all nine gradient pointers or none", who);
  PA_REQUIRE(m.m0_sb >= 0 && m.P0_sb >= 0 && m.F_sb >= 0 && m.F_ss >= 0 && m.q_sb >= 0 && m.q_ss >= 0 &&
                 m.Q_sb >= 0 && m.Q_ss >= 0 && m.H_sb >= 0 && m.H_ss >= 0 && m.r_sb >= 0 && m.r_ss >= 0 &&
                 m.R_sb >= 0 && m.R_ss >= 0,
             "%s: negative stride", who);
  const size_t need = pa_gaussian_hmm_workspace(dtype, B, T, hidden, obs, ng != 0);
  PA_REQUIRE(need == 0 || (a.ws && workspace_bytes >= need), "%s: workspace too small", who);
  a.grads = ng != 0;
  hipStream_t s = as_stream(stream);
  const bool small = hidden <= 8 && obs <= 8;
#define PA_GH_LAUNCH(T_, MD_)                                                                             \
  do {                                                                                                    \
    if (student) hipLaunchKernelGGL((gaussian_hmm_kernel<T_, MD_, true>), dim3((unsigned)B), dim3(64), 0, s, a); \
    else hipLaunchKernelGGL((gaussian_hmm_kernel<T_, MD_, false>), dim3((unsigned)B), dim3(64), 0, s, a); \
  } while (0)
  if (dtype == PA_F32) {
    if (small) PA_GH_LAUNCH(float, 8); else PA_GH_LAUNCH(float, 16);
  } else {
    if (small) PA_GH_LAUNCH(double, 8); else PA_GH_LAUNCH(double, 16);
  }
#undef PA_GH_LAUNCH
  return check_launch("gaussian_hmm_kernel");
}

}  // namespace pa

extern "C" {

size_t pa_gaussian_hmm_workspace(int dtype, int64_t B, int64_t T, int64_t hidden, int64_t obs, int need_grads) {
  (void)obs;
  if (!need_grads || B <= 0 || T <= 0 || hidden <= 0) return 0;
  return (size_t)(B * T * (hidden + hidden * hidden)) * (dtype == PA_F32 ? 4 : 8);
}

int pa_gaussian_hmm_fwd_bwd(int dtype, const void* m0, int64_t m0_stride_batch, const void* P0,
                            int64_t P0_stride_batch, const void* F, int64_t F_stride_batch, int64_t F_stride_step,
                            const void* q, int64_t q_stride_batch, int64_t q_stride_step, const void* Q,
                            int64_t Q_stride_batch, int64_t Q_stride_step, const void* H, int64_t H_stride_batch,
                            int64_t H_stride_step, const void* r, int64_t r_stride_batch, int64_t r_stride_step,
                            const void* R, int64_t R_stride_batch, int64_t R_stride_step, const void* x, int64_t B,
                            int64_t T, int64_t hidden, int64_t obs, void* log_prob, void* filter_mean,
                            void* filter_cov, void* grad_m0, void* grad_P0, void* grad_F, void* grad_q, void* grad_Q,
                            void* grad_H, void* grad_r, void* grad_R, void* grad_x, void* workspace,
                            size_t workspace_bytes, pa_stream_t stream) {
  pa::GhmmArgs a{{m0, P0, F, q, Q, H, r, R, x,
                  m0_stride_batch, P0_stride_batch, F_stride_batch, F_stride_step, q_stride_batch, q_stride_step,
                  Q_stride_batch, Q_stride_step, H_stride_batch, H_stride_step, r_stride_batch, r_stride_step,
                  R_stride_batch, R_stride_step, (int)T, (int)hidden, (int)obs},
                 0,
                 log_prob, filter_mean, filter_cov, grad_m0, grad_P0, grad_F, grad_q, grad_Q, grad_H, grad_r, grad_R,
                 grad_x, workspace,
                 nullptr, nullptr, 0, 0, nullptr, nullptr};
  return pa::ghmm_launch("gaussian_hmm", false, dtype, a, B, T, hidden, obs, workspace_bytes, stream);
}

int pa_gamma_gaussian_hmm_fwd_bwd(int dtype, const void* concentration, int64_t concentration_stride_batch,
                                  const void* rate, int64_t rate_stride_batch, const void* m0,
                                  int64_t m0_stride_batch, const void* P0, int64_t P0_stride_batch, const void* F,
                                  int64_t F_stride_batch, int64_t F_stride_step, const void* q, int64_t q_stride_batch,
                                  int64_t q_stride_step, const void* Q, int64_t Q_stride_batch, int64_t Q_stride_step,
                                  const void* H, int64_t H_stride_batch, int64_t H_stride_step, const void* r,
                                  int64_t r_stride_batch, int64_t r_stride_step, const void* R, int64_t R_stride_batch,
                                  int64_t R_stride_step, const void* x, int64_t B, int64_t T, int64_t hidden,
                                  int64_t obs, void* quad, void* logdet, void* filter_mean, void* filter_cov,
                                  void* grad_m0, void* grad_P0, void* grad_F, void* grad_q, void* grad_Q, void* grad_H,
                                  void* grad_r, void* grad_R, void* grad_x, void* workspace, size_t workspace_bytes,
                                  pa_stream_t stream) {
  pa::GhmmArgs a{{m0, P0, F, q, Q, H, r, R, x,
                  m0_stride_batch, P0_stride_batch, F_stride_batch, F_stride_step, q_stride_batch, q_stride_step,
                  Q_stride_batch, Q_stride_step, H_stride_batch, H_stride_step, r_stride_batch, r_stride_step,
                  R_stride_batch, R_stride_step, (int)T, (int)hidden, (int)obs},
                 0,
                 nullptr, filter_mean, filter_cov, grad_m0, grad_P0, grad_F, grad_q, grad_Q, grad_H, grad_r, grad_R,
                 grad_x, workspace,
                 concentration, rate, concentration_stride_batch, rate_stride_batch, quad, logdet};
  return pa::ghmm_launch("gamma_gaussian_hmm", true, dtype, a, B, T, hidden, obs, workspace_bytes, stream);
}

}  // extern "C"
