// gaussian_hmm.hip -- a linear-Gaussian state-space likelihood and its gradient in ONE launch.
//
// Reference path replaced: GaussianHMM.log_prob (pyro/distributions/hmm.py:434-741) eliminates the time axis with
// sequential_gaussian_tensordot (pyro/ops/gaussian.py): O(log T) rounds of batched Cholesky-based Gaussian
// contractions, and autograd differentiates through every one of them -- hundreds of small launches per gradient
// for a few hundred steps.  Here (row vectors, as the reference writes the model)
//     z_0 ~ N(m0, P0),   z_t = z_{t-1} F_t + N(q_t, Q_t),   x_t = z_t H_t + N(r_t, R_t),   t = 1..T
// one wave per sequence runs the Kalman filter forward and, when gradients are asked for, the Rauch-Tung-Striebel
// sweep backward in the same launch.  The expected complete-data score under the smoothed posterior IS the gradient
// of the log-likelihood (Fisher's identity) -- the relation logchain.hip uses for the discrete chain: the posteriors
// are the gradient.
//
// Forward: the filter of gaussian_hmm.h (GhFilter: the recurrence, where P^p is symmetrised, the bad-pivot rule), shared
// with gaussian_hmm_sample.hip; per step this kernel adds  log_prob += -|v|^2 / 2 - sum log diag L - obs / 2 log 2 pi.
// A sequence the filter marks (a non-positive or NaN pivot of S) has NaN log_prob, filter outputs and gradients, no
// other sequence sees it.  The backward sweep marks a sequence the same way on a bad pivot of P^p, Q, R or P0
// (gradients only: log_prob is what the forward pass alone gives).
//
// Backward, per step t = T..1, from the filtered (m_{t-1}, P_{t-1}) kept in the workspace (hidden + hidden^2
// elements per step; the predicted moments are recomputed): smoother gain G = P_{t-1} F (P^p)^-1,
//     zbar_{t-1} = m_{t-1} + G (zbar_t - m^p),  Ps_{t-1} = sym(P_{t-1} + G (Ps_t - P^p) G^T),  C = G Ps_t,
// and the gradient rows of include/pyro_amd.h.  A parameter with step stride 0 has its gradient summed over the
// steps in registers, in the order of the sweep (t = T down to 1) -- a fixed order, no atomics: bit-reproducible.
//
// Mapping: the block is ONE wave; every matrix lives in LDS with row stride MD + 1 (MD = 8 or 16: the padded
// dimension; the odd stride keeps both the row- and the column-indexed accesses of the 64 lanes off each other's
// banks), a lane owns MD^2 / 64 elements of every matrix product, the triangular solves give a lane one right-hand
// side each.  The next step's x, heterogeneous parameters and (backward) filtered moments are loaded into registers
// while the current step computes and are written to LDS at the top of the next step.
//
// gfx950 cross-compile (hipcc -O3, -Rpass-analysis=kernel-resource-usage), one wave of 64 lanes per block:
//     instantiation    VGPRs      SGPRs  scratch   LDS bytes   waves / SIMD
//     <float , 8>      132        106    0         5832        3
//     <float , 16>     256 + 12   106    0         21384       1
//     <double, 8>      172        106    0         11664       2
//     <double, 16>     256 + 65   106    0         42768       1
// (+ n: accumulation registers the 16-wide instantiations use as spill space; nothing goes to scratch memory)
#include <limits>

#include "common.h"
#include "gaussian_hmm.h"

namespace pa {

struct GhmmArgs {
  GhModel m;
  int grads;
  void *lp, *fm, *fP, *g_m0, *g_P0, *g_F, *g_q, *g_Q, *g_H, *g_r, *g_R, *g_x, *ws;
};

template <typename T, int MD>
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
  const T half_log_2pi_o = T(0.91893853320467274178) * T(o);
  for (int t = 0; t < Tn; ++t) {
    const T logdet = f.step(t, a.grads ? wsb + (int64_t)t * wstep : nullptr);
    lp += (double)(T(-0.5) * f.sc[0] - logdet - half_log_2pi_o);
  }
  __syncthreads();
  if (lane == 0) ((T*)a.lp)[b] = bad ? NaN : (T)lp;
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
  // dst = src^-1 for a symmetric positive definite n x n matrix whose elements ``own`` lists (sL is the scratch)
  auto spd_inverse = [&](const T* src, T* dst, int n, const int (&own)[EPL]) {
#pragma unroll
    for (int k = 0; k < EPL; ++k)
      if (own[k] >= 0) {
        sL[own[k]] = src[own[k]];
        dst[own[k]] = own[k] / LD == own[k] % LD ? T(1) : T(0);
      }
    __syncthreads();
    gh_cholesky<T, MD>(sL, n, lane, bad);
    if (lane < n) {
      gh_forward_sub<T, LD>(sL, dst + lane, LD, n);
      gh_backward_sub<T, LD>(sL, dst + lane, LD, n);
    }
    __syncthreads();
  };

  if (lane < h) vzs[lane] = vm[lane];
#pragma unroll
  for (int k = 0; k < EPL; ++k)
    if (lhh[k] >= 0) sPs[lhh[k]] = sP[lhh[k]];
  __syncthreads();
  if (!a.m.Q_ss) spd_inverse(sQ, sQi, h, lhh);
  if (!a.m.R_ss) spd_inverse(sR, sRi, o, loo);

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
    for (int k = 0; k < EPL; ++k)
      if (lhh[k] >= 0) sP[lhh[k]] = f.pP[k];
    if (t > 0) {
      f.load_params(t - 1, false, true);
      load_filtered(t - 1);
    }
    __syncthreads();
    if (a.m.Q_ss) spd_inverse(sQ, sQi, h, lhh);
    if (a.m.R_ss) spd_inverse(sR, sRi, o, loo);
    f.predict(sL);                                                 // vmp, sPp (= sL), sA = F^T P_{t-1}
    gh_cholesky<T, MD>(sL, h, lane, bad);
    if (lane < h) {                                              // column i of sA <- (P^p)^-1 column: sA[j, i] = G[i, j]
      gh_forward_sub<T, LD>(sL, sA + lane, LD, h);
      gh_backward_sub<T, LD>(sL, sA + lane, LD, h);
      vd[lane] = vzs[lane] - vmp[lane];
    }
#pragma unroll
    for (int k = 0; k < EPL; ++k)
      if (lhh[k] >= 0) sB[lhh[k]] = sPs[lhh[k]] - sPp[lhh[k]];
    __syncthreads();
    if (lane < h) {                                              // zbar_{t-1}
      T s = vm[lane];
      for (int j = 0; j < h; ++j) s += sA[j * LD + lane] * vd[j];
      vzp[lane] = s;
    }
#pragma unroll
    for (int k = 0; k < EPL; ++k)
      if (lhh[k] >= 0) {                                         // sC = G (Ps_t - P^p), sX = C_t = G Ps_t
        const int i = lhh[k] / LD, c = lhh[k] % LD;
        T s = T(0), s2 = T(0);
        for (int j = 0; j < h; ++j) {
          const T g = sA[j * LD + i];
          s += g * sB[j * LD + c];
          s2 += g * sPs[j * LD + c];
        }
        sC[lhh[k]] = s;
        sX[lhh[k]] = s2;
      }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < EPL; ++k)
      if (lhh[k] >= 0) {                                         // sB = P_{t-1} + G (Ps_t - P^p) G^T
        const int i = lhh[k] / LD, c = lhh[k] % LD;
        T s = sP[lhh[k]];
        for (int j = 0; j < h; ++j) s += sC[i * LD + j] * sA[j * LD + c];
        sB[lhh[k]] = s;
      }
    if (lane < h) {                                              // ebar
      T s = vzs[lane] - vq[lane];
      for (int i = 0; i < h; ++i) s -= vzp[i] * sF[i * LD + lane];
      ve[lane] = s;
    }
    if (lane < o) {                                              // ubar
      T s = vx[lane] - vr[lane];
      for (int j = 0; j < h; ++j) s -= vzs[j] * sH[j * LD + lane];
      vu[lane] = s;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < EPL; ++k)
      if (lhh[k] >= 0) {                                         // Ps_{t-1}, symmetrised
        const int i = lhh[k] / LD, c = lhh[k] % LD;
        sPm[lhh[k]] = T(0.5) * (sB[i * LD + c] + sB[c * LD + i]);
      }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < EPL; ++k) {
      if (lhh[k] >= 0) {                                         // sM = Ps_{t-1} F
        const int i = lhh[k] / LD, c = lhh[k] % LD;
        T s = T(0);
        for (int j = 0; j < h; ++j) s += sPm[i * LD + j] * sF[j * LD + c];
        sM[lhh[k]] = s;
      }
      if (lho[k] >= 0) {                                         // sN = Ps_t H
        const int j = lho[k] / LD, c = lho[k] % LD;
        T s = T(0);
        for (int i = 0; i < h; ++i) s += sPs[j * LD + i] * sH[i * LD + c];
        sN[lho[k]] = s;
      }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < EPL; ++k) {
      if (lhh[k] >= 0) {
        const int j = lhh[k] / LD, c = lhh[k] % LD;
        // sC = C - Ps_{t-1} F + zbar_{t-1} ebar^T                       ([old, new])
        sC[lhh[k]] = sX[lhh[k]] - sM[lhh[k]] + vzp[j] * ve[c];
        // sE = Ps_t - F^T C - C^T F + F^T Ps_{t-1} F + ebar ebar^T - Q
        T s = sPs[lhh[k]] + ve[j] * ve[c] - sQ[lhh[k]];
        for (int i = 0; i < h; ++i)
          s += sF[i * LD + j] * (sM[i * LD + c] - sX[i * LD + c]) - sX[i * LD + j] * sF[i * LD + c];
        sE[lhh[k]] = s;
      }
      if (lho[k] >= 0) {                                         // sB = -Ps_t H + zbar_t ubar^T
        const int j = lho[k] / LD, c = lho[k] % LD;
        sB[lho[k]] = vzs[j] * vu[c] - sN[lho[k]];
      }
      if (loo[k] >= 0) {                                         // sV = H^T Ps_t H + ubar ubar^T - R
        const int r_ = loo[k] / LD, c = loo[k] % LD;
        T s = vu[r_] * vu[c] - sR[loo[k]];
        for (int j = 0; j < h; ++j) s += sH[j * LD + r_] * sN[j * LD + c];
        sV[loo[k]] = s;
      }
    }
    __syncthreads();
    if (lane < h) {                                              // d/dq = Q^-1 ebar
      T s = T(0);
      for (int c = 0; c < h; ++c) s += sQi[lane * LD + c] * ve[c];
      if (a.m.q_ss) gq[(int64_t)t * h + lane] = s; else aq += s;
    }
    if (lane < o) {                                              // d/dr = R^-1 ubar = -d/dx
      T s = T(0);
      for (int c = 0; c < o; ++c) s += sRi[lane * LD + c] * vu[c];
      if (a.m.r_ss) gr[(int64_t)t * o + lane] = s; else ar += s;
      gx[(int64_t)t * o + lane] = -s;
    }
#pragma unroll
    for (int k = 0; k < EPL; ++k) {
      const int e = lane + 64 * k;
      if (lhh[k] >= 0) {
        const int j = lhh[k] / LD, c = lhh[k] % LD;
        T s = T(0), s2 = T(0);
        for (int i = 0; i < h; ++i) {
          s += sC[j * LD + i] * sQi[i * LD + c];                 // d/dF = (...) Q^-1
          s2 += sQi[j * LD + i] * sE[i * LD + c];                // sM = Q^-1 E
        }
        if (a.m.F_ss) gF[(int64_t)t * hh + e] = s; else aF[k] += s;
        sM[lhh[k]] = s2;
      }
      if (lho[k] >= 0) {                                         // d/dH = (...) R^-1
        const int j = lho[k] / LD, c = lho[k] % LD;
        T s = T(0);
        for (int i = 0; i < o; ++i) s += sB[j * LD + i] * sRi[i * LD + c];
        if (a.m.H_ss) gH[(int64_t)t * ho + e] = s; else aH[k] += s;
      }
      if (loo[k] >= 0) {                                         // sPp = R^-1 V
        const int r_ = loo[k] / LD, c = loo[k] % LD;
        T s = T(0);
        for (int i = 0; i < o; ++i) s += sRi[r_ * LD + i] * sV[i * LD + c];
        sPp[loo[k]] = s;
      }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < EPL; ++k) {
      const int e = lane + 64 * k;
      if (lhh[k] >= 0) {                                         // d/dQ = Q^-1 E Q^-1 / 2
        const int j = lhh[k] / LD, c = lhh[k] % LD;
        T s = T(0);
        for (int i = 0; i < h; ++i) s += sM[j * LD + i] * sQi[i * LD + c];
        s *= T(0.5);
        if (a.m.Q_ss) gQ[(int64_t)t * hh + e] = s; else aQ[k] += s;
        sPs[lhh[k]] = sPm[lhh[k]];                               // (Ps_t was last read before the barrier above)
      }
      if (loo[k] >= 0) {                                         // d/dR = R^-1 V R^-1 / 2
        const int r_ = loo[k] / LD, c = loo[k] % LD;
        T s = T(0);
        for (int i = 0; i < o; ++i) s += sPp[r_ * LD + i] * sRi[i * LD + c];
        s *= T(0.5);
        if (a.m.R_ss) gR[(int64_t)t * oo + e] = s; else aR[k] += s;
      }
    }
    if (lane < h) vzs[lane] = vzp[lane];
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
  // the initial state: (vm, sP) hold (m0, P0) since step 1 of the sweep, (vzs, sPs) = (zbar_0, Ps_0)
  spd_inverse(sP, sQi, h, lhh);
  if (lane < h) vd[lane] = vzs[lane] - vm[lane];
  __syncthreads();
#pragma unroll
  for (int k = 0; k < EPL; ++k)
    if (lhh[k] >= 0) {
      const int j = lhh[k] / LD, c = lhh[k] % LD;
      sB[lhh[k]] = sPs[lhh[k]] + vd[j] * vd[c] - sP[lhh[k]];
    }
  if (lane < h) {
    T s = T(0);
    for (int c = 0; c < h; ++c) s += sQi[lane * LD + c] * vd[c];
    gm0[lane] = s;
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < EPL; ++k)
    if (lhh[k] >= 0) {
      const int j = lhh[k] / LD, c = lhh[k] % LD;
      T s = T(0);
      for (int i = 0; i < h; ++i) s += sQi[j * LD + i] * sB[i * LD + c];
      sA[lhh[k]] = s;
    }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < EPL; ++k)
    if (lhh[k] >= 0) {
      const int j = lhh[k] / LD, c = lhh[k] % LD;
      T s = T(0);
      for (int i = 0; i < h; ++i) s += sA[j * LD + i] * sQi[i * LD + c];
      gP0[lane + 64 * k] = T(0.5) * s;
    }
  if (bad) fill_nan();
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
  PA_REQUIRE(dtype == PA_F32 || dtype == PA_F64, "gaussian_hmm: bad dtype %d", dtype);
  PA_REQUIRE(B >= 0 && T >= 1 && hidden >= 1 && obs >= 1, "gaussian_hmm: bad shape B=%lld T=%lld hidden=%lld obs=%lld",
             (long long)B, (long long)T, (long long)hidden, (long long)obs);
  if (hidden > pa::GH_MAXHIDDEN || obs > pa::GH_MAXOBS)
    return pa::fail(PA_ERR_UNSUPPORTED, "gaussian_hmm: hidden=%lld obs=%lld over the limit of %d / %d",
                    (long long)hidden, (long long)obs, pa::GH_MAXHIDDEN, pa::GH_MAXOBS);
  PA_REQUIRE(B < (int64_t(1) << 31) && T < (int64_t(1) << 31), "gaussian_hmm: shape too large");
  if (B == 0) return PA_OK;
  PA_REQUIRE(m0 && P0 && F && q && Q && H && r && R && x && log_prob, "gaussian_hmm: NULL pointer");
  PA_REQUIRE((filter_mean == nullptr) == (filter_cov == nullptr), "gaussian_hmm: filter mean and covariance go together");
  const int ng = (grad_m0 != nullptr) + (grad_P0 != nullptr) + (grad_F != nullptr) + (grad_q != nullptr) +
                 (grad_Q != nullptr) + (grad_H != nullptr) + (grad_r != nullptr) + (grad_R != nullptr) +
                 (grad_x != nullptr);
  PA_REQUIRE(ng == 0 || ng == 9, "gaussian_hmm: all nine gradient pointers or none");
  PA_REQUIRE(m0_stride_batch >= 0 && P0_stride_batch >= 0 && F_stride_batch >= 0 && F_stride_step >= 0 &&
                 q_stride_batch >= 0 && q_stride_step >= 0 && Q_stride_batch >= 0 && Q_stride_step >= 0 &&
                 H_stride_batch >= 0 && H_stride_step >= 0 && r_stride_batch >= 0 && r_stride_step >= 0 &&
                 R_stride_batch >= 0 && R_stride_step >= 0,
             "gaussian_hmm: negative stride");
  const size_t need = pa_gaussian_hmm_workspace(dtype, B, T, hidden, obs, ng != 0);
  PA_REQUIRE(need == 0 || (workspace && workspace_bytes >= need), "gaussian_hmm: workspace too small");
  pa::GhmmArgs a{{m0, P0, F, q, Q, H, r, R, x,
                  m0_stride_batch, P0_stride_batch, F_stride_batch, F_stride_step, q_stride_batch, q_stride_step,
                  Q_stride_batch, Q_stride_step, H_stride_batch, H_stride_step, r_stride_batch, r_stride_step,
                  R_stride_batch, R_stride_step, (int)T, (int)hidden, (int)obs},
                 ng != 0,
                 log_prob, filter_mean, filter_cov, grad_m0, grad_P0, grad_F, grad_q, grad_Q, grad_H, grad_r, grad_R,
                 grad_x, workspace};
  hipStream_t s = pa::as_stream(stream);
  const bool small = hidden <= 8 && obs <= 8;
#define PA_GH_LAUNCH(T_, MD_) \
  hipLaunchKernelGGL((pa::gaussian_hmm_kernel<T_, MD_>), dim3((unsigned)B), dim3(64), 0, s, a)
  if (dtype == PA_F32) {
    if (small) PA_GH_LAUNCH(float, 8); else PA_GH_LAUNCH(float, 16);
  } else {
    if (small) PA_GH_LAUNCH(double, 8); else PA_GH_LAUNCH(double, 16);
  }
#undef PA_GH_LAUNCH
  return pa::check_launch("gaussian_hmm_kernel");
}

}  // extern "C"
