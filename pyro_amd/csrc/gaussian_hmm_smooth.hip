// gaussian_hmm_smooth.hip -- the smoothed marginals of a linear-Gaussian state-space model given all the data:
// E[z_t | x_1..T], Cov[z_t | x_1..T] and the lag-one Cov[z_t, z_{t+1} | x_1..T] of every step, in ONE launch on the
// caller's stream.
//
// Reference path replaced: there is no method of the reference's GaussianHMM for it; its users differentiate
// log_prob or rebuild the moments from sequential_gaussian_filter_sample (pyro/ops/gaussian.py:600).  Here (row
// vectors, the conventions of gaussian_hmm.hip)
//     z_0 ~ N(m0, P0),   z_t = z_{t-1} F_t + N(q_t, Q_t),   x_t = z_t H_t + N(r_t, R_t),   t = 1..T
// one wave per series runs the Rauch-Tung-Striebel recursion.  Forward: the filter of gaussian_hmm.h (GhFilter, shared
// with gaussian_hmm_kernel and gaussian_hmm_maps_kernel; a non-positive pivot of S marks the series), keeping
// (m_t, P_t) of every step in the workspace.  Backward, with the states as columns: ms_T = m_T, Ps_T = sym(P_T), and
// for t = T..2 from (m_{t-1}, P_{t-1}) and step t's F, q, Q: m^p, P^p as in the forward pass, the gain from
// chol(P^p) and two triangular solves exactly as the maps kernel forms it,
//     G = P_{t-1} F (P^p)^-1,
//     X_{t-1}  = G Ps_t                                   (= Cov(z_{t-1}, z_t | x): the cross output)
//     ms_{t-1} = m_{t-1} + G (ms_t - m^p)
//     Ps_{t-1} = sym(P_{t-1} + (G (Ps_t - P^p)) G^T)
// Ps is in SUBTRACTION form, not the Joseph form of the maps kernel: nothing here is factorised, so the recursion
// does not need Ps to stay positive definite, and in float32 the form is as accurate or better at two matrix
// products instead of six (near-singular Q, hidden 8, T = 33: 3.7e-6 against 2.1e-5).  X is a third product, formed
// only when the caller asks for the cross covariances.  A non-positive pivot of P^p marks the series as one of S
// does, and so does one of the Q of a step the sweep visits (t = 2..T): the convention of gaussian_hmm_kernel's
// backward sweep, a Cholesky sweep over a copy for the pivots alone -- once for a time-homogeneous Q, per step
// otherwise -- since F^T P F + Q is often positive definite where Q is not, and the moments of such a model are not
// a posterior's.  P0 is never checked (the sweep stops at z_1).  A marked series has mean, cov and cross filled with
// NaN, no other series sees it.  No atomics, a fixed order of operations: bit-reproducible.
//
// LDS: the filter's ten matrices and Ps behind them (backward: sP = P_{t-1}, sA = G^T, sB = G (Ps_t - P^p), sC = Ps
// before it is symmetrised), the filter's six vectors and ms.
//
// gfx950 cross-compile (hipcc -O3, -Rpass-analysis=kernel-resource-usage), one wave of 64 lanes per block:
//     instantiation    VGPRs  SGPRs  scratch   LDS bytes   waves / SIMD
//     <float , 8>      73     106    0         3400        6
//     <float , 16>     128    106    0         12424       4
//     <double, 8>      91     106    0         6800        5
//     <double, 16>     176    106    0         24848       2
#include <limits>

#include "common.h"
#include "gaussian_hmm.h"

namespace pa {

struct GhmArgs {
  GhModel m;
  void *ws, *mean, *cov, *cross;
};

template <typename T, int MD>
__global__ __launch_bounds__(64) void gaussian_hmm_smooth_kernel(const GhmArgs a) {
  constexpr int LD = MD + 1, MS = MD * LD, EPL = MD * MD / 64;
  constexpr int NMAT = 11, NVEC = 7;
  __shared__ T sm[NMAT * MS + NVEC * MD + 2];
  const int lane = threadIdx.x;
  const int64_t b = blockIdx.x;
  GhFilter<T, MD> f(a.m, sm, sm + NMAT * MS, sm + NMAT * MS + NVEC * MD, lane, b);
  T *const sP = f.sP, *const sPp = f.sPp, *const sL = f.sL, *const sA = f.sA, *const sB = f.sB, *const sC = f.sC,
    *const vm = f.vm, *const vmp = f.vmp;
  T* const sPs = sC + MS;      // the smoothed covariance Ps_t
  T* const vms = f.vy + MD;    // the smoothed mean ms_t

  const int h = a.m.h, Tn = a.m.T, hh = h * h;
  const T NaN = std::numeric_limits<T>::quiet_NaN();
  const auto& lhh = f.lhh;
  bool& bad = f.bad;
  const bool cross = a.cross != nullptr;
  const int64_t wstep = h + hh;
  T* const wsb = (T*)a.ws + b * (int64_t)Tn * wstep;
  T* const mb = (T*)a.mean + b * (int64_t)Tn * h;
  T* const Vb = (T*)a.cov + b * (int64_t)Tn * hh;
  T* const Xb = cross ? (T*)a.cross + b * (int64_t)(Tn - 1) * hh : nullptr;

  // every output element is written by ONE lane (element e of a matrix by lane e % 64, a vector's by lane e): the NaN
  // fill of a marked series comes after that lane's own stores in program order
  auto fill_nan = [&]() {
    for (int64_t t = 0; t < Tn; ++t) {
      if (lane < h) mb[t * h + lane] = NaN;
#pragma unroll
      for (int k = 0; k < EPL; ++k)
        if (lhh[k] >= 0) {
          Vb[t * hh + lane + 64 * k] = NaN;
          if (cross && t + 1 < Tn) Xb[t * hh + lane + 64 * k] = NaN;
        }
    }
  };

  // ---- forward: the Kalman filter, every step's (m_t, P_t) kept --------------------------------------------------
  f.start();
  for (int t = 0; t < Tn; ++t) f.step(t, wsb + (int64_t)t * wstep);
  __syncthreads();
  if (bad) {
    fill_nan();
    return;
  }

  // ---- backward: Rauch-Tung-Striebel -----------------------------------------------------------------------------
  {                                                                // the last state: ms_T = m_T, Ps_T = sym(P_T)
    const T mv = lane < h ? vm[lane] : T(0);
    if (lane < h) {
      vms[lane] = mv;
      mb[(int64_t)(Tn - 1) * h + lane] = mv;
    }
#pragma unroll
    for (int k = 0; k < EPL; ++k)
      if (lhh[k] >= 0) {
        const int i = lhh[k] / LD, c = lhh[k] % LD;
        const T s = T(0.5) * (sP[i * LD + c] + sP[c * LD + i]);
        sPs[lhh[k]] = s;
        Vb[(int64_t)(Tn - 1) * hh + lane + 64 * k] = s;
      }
  }

  auto load_filtered = [&](int t) {          // (m_t, P_t) of 0-based step t
    const T* w = wsb + (int64_t)t * wstep;
    if (lane < h) f.pm = w[lane];
#pragma unroll
    for (int k = 0; k < EPL; ++k)
      if (lhh[k] >= 0) f.pP[k] = w[h + lane + 64 * k];
  };
  // a pivot check alone, as in gaussian_hmm_kernel: the Cholesky sweep over a copy of Q in sL; ends with a barrier
  auto check_pivots = [&]() {
#pragma unroll
    for (int k = 0; k < EPL; ++k)
      if (lhh[k] >= 0) sL[lhh[k]] = f.sQ[lhh[k]];
    __syncthreads();
    gh_cholesky<T, MD>(sL, h, lane, bad);
    __syncthreads();
  };
  if (Tn > 1 && !a.m.Q_ss) check_pivots();   // (a time-homogeneous Q is in LDS since the filter's first step)
  // (the forward pass wrote the workspace with the lanes that read it back here: same lane, same address)
  if (Tn > 1) {
    f.load_params(Tn - 1, false, false);
    load_filtered(Tn - 2);
  }
  for (int t = Tn - 1; t >= 1; --t) {        // step t's transition, the filtered moments of step t - 1 -> marginal t - 1
    __syncthreads();
    f.commit_params(false, false);
    if (lane < h) vm[lane] = f.pm;
#pragma unroll
    for (int k = 0; k < EPL; ++k)
      if (lhh[k] >= 0) sP[lhh[k]] = f.pP[k];
    if (t > 1) {
      f.load_params(t - 1, false, false);
      load_filtered(t - 2);
    }
    __syncthreads();
    if (a.m.Q_ss) check_pivots();
    f.predict(sL);                                                 // vmp, sPp (= sL), sA = F^T P_{t-1}
    gh_cholesky<T, MD>(sL, h, lane, bad);
    if (lane < h) {                                              // column i of sA <- (P^p)^-1 column: sA[j, i] = G[i, j]
      gh_forward_sub<T, LD>(sL, sA + lane, LD, h);
      gh_backward_sub<T, LD>(sL, sA + lane, LD, h);
    }
    __syncthreads();
    T nm = T(0);
    if (lane < h) {                                              // ms_{t-1} = m_{t-1} + G (ms_t - m^p)
      nm = vm[lane];
      for (int j = 0; j < h; ++j) nm += sA[j * LD + lane] * (vms[j] - vmp[j]);
      mb[(int64_t)(t - 1) * h + lane] = nm;
    }
#pragma unroll
    for (int k = 0; k < EPL; ++k)
      if (lhh[k] >= 0) {                                         // sB = G (Ps_t - P^p), X = G Ps_t
        const int i = lhh[k] / LD, c = lhh[k] % LD;
        T s = T(0);
        for (int j = 0; j < h; ++j) s += sA[j * LD + i] * (sPs[j * LD + c] - sPp[j * LD + c]);
        sB[lhh[k]] = s;
        if (cross) {
          T s2 = T(0);
          for (int j = 0; j < h; ++j) s2 += sA[j * LD + i] * sPs[j * LD + c];
          Xb[(int64_t)(t - 1) * hh + lane + 64 * k] = s2;
        }
      }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < EPL; ++k)
      if (lhh[k] >= 0) {                                         // sC = P_{t-1} + (G (Ps_t - P^p)) G^T
        const int i = lhh[k] / LD, c = lhh[k] % LD;
        T s = sP[lhh[k]];
        for (int j = 0; j < h; ++j) s += sB[i * LD + j] * sA[j * LD + c];
        sC[lhh[k]] = s;
      }
    // (vms was last read before the barrier above)
    if (lane < h) vms[lane] = nm;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < EPL; ++k)
      if (lhh[k] >= 0) {                                         // Ps_{t-1}, symmetrised
        const int i = lhh[k] / LD, c = lhh[k] % LD;
        const T s = T(0.5) * (sC[i * LD + c] + sC[c * LD + i]);
        sPs[lhh[k]] = s;
        Vb[(int64_t)(t - 1) * hh + lane + 64 * k] = s;
      }
  }
  if (bad) fill_nan();
}

}  // namespace pa

extern "C" {

size_t pa_gaussian_hmm_smooth_workspace(int dtype, int64_t B, int64_t T, int64_t hidden, int64_t obs) {
  (void)obs;
  if (B <= 0 || T <= 0 || hidden <= 0) return 0;
  return (size_t)(B * T * (hidden + hidden * hidden)) * (dtype == PA_F32 ? 4 : 8);     // the filtered moments
}

int pa_gaussian_hmm_smooth(int dtype, const void* m0, int64_t m0_stride_batch, const void* P0,
                           int64_t P0_stride_batch, const void* F, int64_t F_stride_batch, int64_t F_stride_step,
                           const void* q, int64_t q_stride_batch, int64_t q_stride_step, const void* Q,
                           int64_t Q_stride_batch, int64_t Q_stride_step, const void* H, int64_t H_stride_batch,
                           int64_t H_stride_step, const void* r, int64_t r_stride_batch, int64_t r_stride_step,
                           const void* R, int64_t R_stride_batch, int64_t R_stride_step, const void* x, int64_t B,
                           int64_t T, int64_t hidden, int64_t obs, void* mean, void* cov, void* cross, void* workspace,
                           size_t workspace_bytes, pa_stream_t stream) {
  PA_REQUIRE(dtype == PA_F32 || dtype == PA_F64, "gaussian_hmm_smooth: bad dtype %d", dtype);
  PA_REQUIRE(B >= 0 && T >= 1 && hidden >= 1 && obs >= 1,
             "gaussian_hmm_smooth: bad shape B=%lld T=%lld hidden=%lld obs=%lld", (long long)B, (long long)T,
             (long long)hidden, (long long)obs);
  if (hidden > pa::GH_MAXHIDDEN || obs > pa::GH_MAXOBS)
    return pa::fail(PA_ERR_UNSUPPORTED, "gaussian_hmm_smooth: hidden=%lld obs=%lld over the limit of %d / %d",
                    (long long)hidden, (long long)obs, pa::GH_MAXHIDDEN, pa::GH_MAXOBS);
  PA_REQUIRE(B < (int64_t(1) << 31) && T < (int64_t(1) << 31), "gaussian_hmm_smooth: shape too large");
  if (B == 0) return PA_OK;
  PA_REQUIRE(m0 && P0 && F && q && Q && H && r && R && x && mean && cov, "gaussian_hmm_smooth: NULL pointer");
  PA_REQUIRE(m0_stride_batch >= 0 && P0_stride_batch >= 0 && F_stride_batch >= 0 && F_stride_step >= 0 &&
                 q_stride_batch >= 0 && q_stride_step >= 0 && Q_stride_batch >= 0 && Q_stride_step >= 0 &&
                 H_stride_batch >= 0 && H_stride_step >= 0 && r_stride_batch >= 0 && r_stride_step >= 0 &&
                 R_stride_batch >= 0 && R_stride_step >= 0,
             "gaussian_hmm_smooth: negative stride");
  const size_t need = pa_gaussian_hmm_smooth_workspace(dtype, B, T, hidden, obs);
  PA_REQUIRE(workspace && workspace_bytes >= need, "gaussian_hmm_smooth: workspace too small");
  if (T == 1) cross = nullptr;                 // (an empty output: nothing to write, and its pointer may be anything)
  pa::GhmArgs a{{m0, P0, F, q, Q, H, r, R, x,
                 m0_stride_batch, P0_stride_batch, F_stride_batch, F_stride_step, q_stride_batch, q_stride_step,
                 Q_stride_batch, Q_stride_step, H_stride_batch, H_stride_step, r_stride_batch, r_stride_step,
                 R_stride_batch, R_stride_step, (int)T, (int)hidden, (int)obs},
                workspace, mean, cov, cross};
  hipStream_t st = pa::as_stream(stream);
  const bool small = hidden <= 8 && obs <= 8;
#define PA_GHM_SMOOTH(T_, MD_) \
  hipLaunchKernelGGL((pa::gaussian_hmm_smooth_kernel<T_, MD_>), dim3((unsigned)B), dim3(64), 0, st, a)
  if (dtype == PA_F32) {
    if (small) PA_GHM_SMOOTH(float, 8); else PA_GHM_SMOOTH(float, 16);
  } else {
    if (small) PA_GHM_SMOOTH(double, 8); else PA_GHM_SMOOTH(double, 16);
  }
#undef PA_GHM_SMOOTH
  return pa::check_launch("gaussian_hmm_smooth_kernel");
}

}  // extern "C"
