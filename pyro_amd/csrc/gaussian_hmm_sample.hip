// gaussian_hmm_sample.hip -- draws of the whole latent path of a linear-Gaussian state-space model given the data:
// forward filter, backward sample, in TWO launches on the caller's stream.
//
// Reference path replaced: GaussianHMM.rsample_posterior (pyro/distributions/hmm.py:596-604) over
// sequential_gaussian_filter_sample (pyro/ops/gaussian.py:600): a parallel-scan forward filter with a tape and
// O(log T) rounds of batched Cholesky-based contractions, then the same number of rounds of conditional draws.
// Here (row vectors, the conventions of gaussian_hmm.hip)
//     z_0 ~ N(m0, P0),   z_t = z_{t-1} F_t + N(q_t, Q_t),   x_t = z_t H_t + N(r_t, R_t),   t = 1..T
// the posterior of the path is the Markov chain, written backward with the states as columns,
//     z_T = c_T + L_T eps_T,     z_{t-1} = c_{t-1} + G_{t-1} z_t + L_{t-1} eps_{t-1},   t = T..2
// whose "maps" (c_t, G_t, L_t) depend on the series only, not on the draw (G_T = 0; z_0 is not drawn).
//
// Maps kernel, one wave per series.  Forward: the filter of gaussian_hmm.h (GhFilter, shared with gaussian_hmm_kernel;
// a non-positive pivot of S marks the series), keeping (m_t, P_t) of every step in the workspace.  Backward:
// L_T = chol(sym(P_T)), c_T = m_T, and for t = T..2 from (m_{t-1}, P_{t-1}) and step t's F, q, Q: m^p, P^p as in the
// forward pass,
//     G = P_{t-1} F (P^p)^-1,   J = I - G F^T,   C = sym(J P_{t-1} J^T + G Q G^T),   L_{t-1} = chol(C),
//     c_{t-1} = m_{t-1} - G m^p.
// C is the conditional covariance in JOSEPH form: a sum of two positive semi-definite terms.  The shorter
// P_{t-1} - G P^p G^T loses positive definiteness in float32 when Q is nearly singular (hidden 8, T = 33, Q scaled
// by 1e-8: the Joseph form keeps a smallest pivot of 9e-5 there).  A non-positive pivot of P^p or C marks the series
// as one of S does; a marked series has c, G and L filled with NaN, no other series sees it.  No atomics, a fixed
// order of operations: bit-reproducible.  L is lower triangular with zeros above the diagonal.
//
// Paths kernel, grid (B, ceil(S / 64)), one wave per block, one lane per draw: z_t lives in MD registers, step t's
// (c, G, L) -- uniform over the wave -- are staged through LDS (two buffers: the next step's are loaded into
// registers while the current step computes, one barrier per step), every lane reads its eps[s, b, t, :] a step
// ahead and writes z[s, b, t, :], both laid out [S, B, T, hidden].
//
// gfx950 cross-compile (hipcc -O3, -Rpass-analysis=kernel-resource-usage), one wave of 64 lanes per block:
//     kernel   instantiation    VGPRs  SGPRs  scratch   LDS bytes   waves / SIMD
//     maps     <float , 8>      71     106    0         3656        7
//     maps     <float , 16>     160    106    0         13448       3
//     maps     <double, 8>      95     106    0         7312        5
//     maps     <double, 16>     204    106    0         26896       2
//     paths    <float , 8>      60     56     0         1088        8
//     paths    <float , 16>     96     96     0         4224        5
//     paths    <double, 8>      95     56     0         2176        5
//     paths    <double, 16>     170    96     0         8448        2
#include <limits>

#include "common.h"
#include "gaussian_hmm.h"

namespace pa {

struct GhsArgs {
  GhModel m;
  void *ws, *c, *G, *L;
};

template <typename T, int MD>
__global__ __launch_bounds__(64) void gaussian_hmm_maps_kernel(const GhsArgs a) {
  constexpr int LD = MD + 1, MS = MD * LD, EPL = MD * MD / 64;
  constexpr int NMAT = 12, NVEC = 6;
  __shared__ T sm[NMAT * MS + NVEC * MD + 2];
  const int lane = threadIdx.x;
  const int64_t b = blockIdx.x;
  GhFilter<T, MD> f(a.m, sm, sm + NMAT * MS, sm + NMAT * MS + NVEC * MD, lane, b);
  // the filter's matrices (backward: sP = P_{t-1}, sA = G^T, sB = G Q, sC = J P_{t-1}) and the sweep's behind them
  T *const sP = f.sP, *const sF = f.sF, *const sQ = f.sQ, *const sL = f.sL, *const sA = f.sA, *const sB = f.sB,
    *const sC = f.sC, *const vm = f.vm, *const vmp = f.vmp;
  T* const sJ = sC + MS;       // I - G F^T
  T* const sD = sJ + MS;       // the conditional covariance before it is symmetrised

  const int h = a.m.h, Tn = a.m.T, hh = h * h;
  const T NaN = std::numeric_limits<T>::quiet_NaN();
  const auto& lhh = f.lhh;
  bool& bad = f.bad;
  const int64_t wstep = h + hh;
  T* const wsb = (T*)a.ws + b * (int64_t)Tn * wstep;
  T* const cb = (T*)a.c + b * (int64_t)Tn * h;
  T* const Gb = (T*)a.G + b * (int64_t)Tn * hh;
  T* const Lb = (T*)a.L + b * (int64_t)Tn * hh;

  // every element of the maps is written by ONE lane (element e of a matrix by lane e % 64, a vector's by lane e):
  // the NaN fill of a marked series comes after that lane's own stores in program order
  auto fill_nan = [&]() {
    for (int64_t t = 0; t < Tn; ++t) {
      if (lane < h) cb[t * h + lane] = NaN;
#pragma unroll
      for (int k = 0; k < EPL; ++k)
        if (lhh[k] >= 0) Gb[t * hh + lane + 64 * k] = Lb[t * hh + lane + 64 * k] = NaN;
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

  // ---- backward: the maps of the chain z_T, z_{T-1} | z_T, ... -----------------------------------------------------
  // step t's map from the factor in sL, the gain (transposed) in sA and this lane's element of c
  auto store_maps = [&](int t, T cv, bool gain) {
    if (lane < h) cb[(int64_t)t * h + lane] = cv;
#pragma unroll
    for (int k = 0; k < EPL; ++k)
      if (lhh[k] >= 0) {
        const int i = lhh[k] / LD, c = lhh[k] % LD;
        Gb[(int64_t)t * hh + lane + 64 * k] = gain ? sA[c * LD + i] : T(0);
        Lb[(int64_t)t * hh + lane + 64 * k] = c <= i ? sL[lhh[k]] : T(0);
      }
  };
#pragma unroll
  for (int k = 0; k < EPL; ++k)
    if (lhh[k] >= 0) {                                           // the last state: L_T = chol(sym(P_T)), c_T = m_T
      const int i = lhh[k] / LD, c = lhh[k] % LD;
      sL[lhh[k]] = T(0.5) * (sP[i * LD + c] + sP[c * LD + i]);
    }
  __syncthreads();
  gh_cholesky<T, MD>(sL, h, lane, bad);
  store_maps(Tn - 1, lane < h ? vm[lane] : T(0), false);

  auto load_filtered = [&](int t) {          // (m_t, P_t) of 0-based step t
    const T* w = wsb + (int64_t)t * wstep;
    if (lane < h) f.pm = w[lane];
#pragma unroll
    for (int k = 0; k < EPL; ++k)
      if (lhh[k] >= 0) f.pP[k] = w[h + lane + 64 * k];
  };
  // (the forward pass wrote the workspace with the lanes that read it back here: same lane, same address)
  if (Tn > 1) {
    f.load_params(Tn - 1, false, false);
    load_filtered(Tn - 2);
  }
  for (int t = Tn - 1; t >= 1; --t) {        // step t's transition, the filtered moments of step t - 1 -> map t - 1
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
    f.predict(sL);                                                 // vmp, sPp (= sL), sA = F^T P_{t-1}
    gh_cholesky<T, MD>(sL, h, lane, bad);
    if (lane < h) {                                              // column i of sA <- (P^p)^-1 column: sA[j, i] = G[i, j]
      gh_forward_sub<T, LD>(sL, sA + lane, LD, h);
      gh_backward_sub<T, LD>(sL, sA + lane, LD, h);
    }
    __syncthreads();
    T cv = T(0);
    if (lane < h) {                                              // c_{t-1} = m_{t-1} - G m^p
      cv = vm[lane];
      for (int j = 0; j < h; ++j) cv -= sA[j * LD + lane] * vmp[j];
    }
#pragma unroll
    for (int k = 0; k < EPL; ++k)
      if (lhh[k] >= 0) {                                         // sJ = I - G F^T, sB = G Q
        const int i = lhh[k] / LD, c = lhh[k] % LD;
        T s = i == c ? T(1) : T(0), s2 = T(0);
        for (int j = 0; j < h; ++j) {
          const T g = sA[j * LD + i];
          s -= g * sF[c * LD + j];
          s2 += g * sQ[j * LD + c];
        }
        sJ[lhh[k]] = s;
        sB[lhh[k]] = s2;
      }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < EPL; ++k)
      if (lhh[k] >= 0) {                                         // sC = J P_{t-1}
        const int i = lhh[k] / LD, c = lhh[k] % LD;
        T s = T(0);
        for (int j = 0; j < h; ++j) s += sJ[i * LD + j] * sP[j * LD + c];
        sC[lhh[k]] = s;
      }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < EPL; ++k)
      if (lhh[k] >= 0) {                                         // sD = J P_{t-1} J^T + G Q G^T
        const int i = lhh[k] / LD, c = lhh[k] % LD;
        T s = T(0), s2 = T(0);
        for (int j = 0; j < h; ++j) {
          s += sC[i * LD + j] * sJ[c * LD + j];
          s2 += sB[i * LD + j] * sA[j * LD + c];
        }
        sD[lhh[k]] = s + s2;
      }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < EPL; ++k)
      if (lhh[k] >= 0) {                                         // C, symmetrised
        const int i = lhh[k] / LD, c = lhh[k] % LD;
        sL[lhh[k]] = T(0.5) * (sD[i * LD + c] + sD[c * LD + i]);
      }
    __syncthreads();
    gh_cholesky<T, MD>(sL, h, lane, bad);
    store_maps(t - 1, cv, true);
  }
  if (bad) fill_nan();
}

// One lane per draw: z_t = c_t + G_t z_{t+1} + L_t eps_t down the chain, the maps staged through LDS.
template <typename T, int MD>
__global__ __launch_bounds__(64) void gaussian_hmm_paths_kernel(const T* __restrict__ mc, const T* __restrict__ mG,
                                                                const T* __restrict__ mL, const T* __restrict__ eps,
                                                                T* __restrict__ z, int64_t B, int Tn, int h,
                                                                int64_t S) {
  constexpr int MM = MD * MD, EPL = MM / 64, STEP = MD + 2 * MM;
  __shared__ T sm[2 * STEP];                 // two buffers of (c [MD], G [MD, MD], L [MD, MD]), zero beyond h
  const int lane = threadIdx.x, hh = h * h;
  const int64_t b = blockIdx.x, s = (int64_t)blockIdx.y * 64 + lane;
  const bool active = s < S;
  int own[EPL];                              // this lane's elements of an [h, h] matrix in the padded image (-1: none)
#pragma unroll
  for (int k = 0; k < EPL; ++k) {
    const int e = lane + 64 * k;
    own[k] = e < hh ? (e / h) * MD + e % h : -1;
  }
  for (int e = lane; e < 2 * STEP; e += 64) sm[e] = T(0);
  const T* cb = mc + b * (int64_t)Tn * h;
  const T* Gb = mG + b * (int64_t)Tn * hh;
  const T* Lb = mL + b * (int64_t)Tn * hh;
  const int64_t row = active ? (s * B + b) * (int64_t)Tn * h : 0;
  const T* eb = eps + row;
  T* zb = z + row;

  T pc = T(0), pG[EPL], pL[EPL], pe[MD], ev[MD], zc[MD];
#pragma unroll
  for (int k = 0; k < EPL; ++k) pG[k] = pL[k] = T(0);
#pragma unroll
  for (int j = 0; j < MD; ++j) pe[j] = ev[j] = zc[j] = T(0);
  auto load = [&](int t) {
    if (lane < h) pc = cb[(int64_t)t * h + lane];
#pragma unroll
    for (int k = 0; k < EPL; ++k)
      if (own[k] >= 0) {
        pG[k] = Gb[(int64_t)t * hh + lane + 64 * k];
        pL[k] = Lb[(int64_t)t * hh + lane + 64 * k];
      }
    if (active) {
#pragma unroll
      for (int j = 0; j < MD; ++j)
        if (j < h) pe[j] = eb[(int64_t)t * h + j];
    }
  };
  auto commit = [&](T* buf) {
    if (lane < h) buf[lane] = pc;
#pragma unroll
    for (int k = 0; k < EPL; ++k)
      if (own[k] >= 0) {
        buf[MD + own[k]] = pG[k];
        buf[MD + MM + own[k]] = pL[k];
      }
#pragma unroll
    for (int j = 0; j < MD; ++j) ev[j] = pe[j];
  };
  __syncthreads();
  load(Tn - 1);
  commit(sm);
  if (Tn > 1) load(Tn - 2);
  __syncthreads();
  for (int t = Tn - 1, n = 0; t >= 0; --t, ++n) {
    const T* cur = sm + (n & 1) * STEP;
    T zn[MD];
#pragma unroll
    for (int i = 0; i < MD; ++i) {
      zn[i] = T(0);
      if (i < h) {
        T acc = cur[i];
#pragma unroll
        for (int j = 0; j < MD; ++j) acc += cur[MD + i * MD + j] * zc[j];
#pragma unroll
        for (int j = 0; j <= i; ++j) acc += cur[MD + MM + i * MD + j] * ev[j];
        zn[i] = acc;
      }
    }
    if (active) {
#pragma unroll
      for (int j = 0; j < MD; ++j)
        if (j < h) zb[(int64_t)t * h + j] = zn[j];
    }
#pragma unroll
    for (int j = 0; j < MD; ++j) zc[j] = zn[j];
    if (t > 0) {
      // (the other buffer was last read in the step before this one, which every lane left through the barrier)
      commit(sm + ((n + 1) & 1) * STEP);
      if (t > 1) load(t - 2);
    }
    __syncthreads();
  }
}

}  // namespace pa

extern "C" {

size_t pa_gaussian_hmm_sample_workspace(int dtype, int64_t B, int64_t T, int64_t hidden, int64_t obs) {
  (void)obs;
  if (B <= 0 || T <= 0 || hidden <= 0) return 0;
  // the filtered moments of every step, and room for the maps of a caller that does not keep them
  return (size_t)(B * T * (2 * hidden + 3 * hidden * hidden)) * (dtype == PA_F32 ? 4 : 8);
}

int pa_gaussian_hmm_sample(int dtype, const void* m0, int64_t m0_stride_batch, const void* P0,
                           int64_t P0_stride_batch, const void* F, int64_t F_stride_batch, int64_t F_stride_step,
                           const void* q, int64_t q_stride_batch, int64_t q_stride_step, const void* Q,
                           int64_t Q_stride_batch, int64_t Q_stride_step, const void* H, int64_t H_stride_batch,
                           int64_t H_stride_step, const void* r, int64_t r_stride_batch, int64_t r_stride_step,
                           const void* R, int64_t R_stride_batch, int64_t R_stride_step, const void* x, int64_t B,
                           int64_t T, int64_t hidden, int64_t obs, int64_t S, const void* eps, void* z, void* maps_c,
                           void* maps_G, void* maps_L, void* workspace, size_t workspace_bytes, pa_stream_t stream) {
  PA_REQUIRE(dtype == PA_F32 || dtype == PA_F64, "gaussian_hmm_sample: bad dtype %d", dtype);
  PA_REQUIRE(B >= 0 && T >= 1 && hidden >= 1 && obs >= 1 && S >= 0,
             "gaussian_hmm_sample: bad shape B=%lld T=%lld hidden=%lld obs=%lld S=%lld", (long long)B, (long long)T,
             (long long)hidden, (long long)obs, (long long)S);
  if (hidden > pa::GH_MAXHIDDEN || obs > pa::GH_MAXOBS)
    return pa::fail(PA_ERR_UNSUPPORTED, "gaussian_hmm_sample: hidden=%lld obs=%lld over the limit of %d / %d",
                    (long long)hidden, (long long)obs, pa::GH_MAXHIDDEN, pa::GH_MAXOBS);
  PA_REQUIRE(B < (int64_t(1) << 31) && T < (int64_t(1) << 31) && S <= int64_t(65535) * 64,
             "gaussian_hmm_sample: shape too large");
  const int nm = (maps_c != nullptr) + (maps_G != nullptr) + (maps_L != nullptr);
  PA_REQUIRE(nm == 0 || nm == 3, "gaussian_hmm_sample: all three maps pointers or none");
  if (B == 0 || (S == 0 && nm == 0)) return PA_OK;
  PA_REQUIRE(m0 && P0 && F && q && Q && H && r && R && x && (S == 0 || (eps && z)),
             "gaussian_hmm_sample: NULL pointer");
  PA_REQUIRE(m0_stride_batch >= 0 && P0_stride_batch >= 0 && F_stride_batch >= 0 && F_stride_step >= 0 &&
                 q_stride_batch >= 0 && q_stride_step >= 0 && Q_stride_batch >= 0 && Q_stride_step >= 0 &&
                 H_stride_batch >= 0 && H_stride_step >= 0 && r_stride_batch >= 0 && r_stride_step >= 0 &&
                 R_stride_batch >= 0 && R_stride_step >= 0,
             "gaussian_hmm_sample: negative stride");
  const size_t need = pa_gaussian_hmm_sample_workspace(dtype, B, T, hidden, obs);
  PA_REQUIRE(workspace && workspace_bytes >= need, "gaussian_hmm_sample: workspace too small");
  const size_t el = dtype == PA_F32 ? 4 : 8;
  const int64_t BT = B * T, hh = hidden * hidden;
  if (nm == 0) {                               // the maps live in the workspace, behind the filtered moments
    char* w = (char*)workspace + (size_t)(BT * (hidden + hh)) * el;
    maps_c = w;
    maps_G = w + (size_t)(BT * hidden) * el;
    maps_L = w + (size_t)(BT * (hidden + hh)) * el;
  }
  pa::GhsArgs a{{m0, P0, F, q, Q, H, r, R, x,
                 m0_stride_batch, P0_stride_batch, F_stride_batch, F_stride_step, q_stride_batch, q_stride_step,
                 Q_stride_batch, Q_stride_step, H_stride_batch, H_stride_step, r_stride_batch, r_stride_step,
                 R_stride_batch, R_stride_step, (int)T, (int)hidden, (int)obs},
                workspace, maps_c, maps_G, maps_L};
  hipStream_t st = pa::as_stream(stream);
  const bool small = hidden <= 8 && obs <= 8;
#define PA_GHS_MAPS(T_, MD_) \
  hipLaunchKernelGGL((pa::gaussian_hmm_maps_kernel<T_, MD_>), dim3((unsigned)B), dim3(64), 0, st, a)
  if (dtype == PA_F32) {
    if (small) PA_GHS_MAPS(float, 8); else PA_GHS_MAPS(float, 16);
  } else {
    if (small) PA_GHS_MAPS(double, 8); else PA_GHS_MAPS(double, 16);
  }
#undef PA_GHS_MAPS
  const int rc = pa::check_launch("gaussian_hmm_maps_kernel");
  if (rc != PA_OK || S == 0) return rc;
  const dim3 grid((unsigned)B, (unsigned)((S + 63) / 64));
  // (the paths kernel pads to the hidden dimension alone)
#define PA_GHS_PATHS(T_, MD_)                                                                                    \
  hipLaunchKernelGGL((pa::gaussian_hmm_paths_kernel<T_, MD_>), grid, dim3(64), 0, st, (const T_*)maps_c,          \
                     (const T_*)maps_G, (const T_*)maps_L, (const T_*)eps, (T_*)z, B, (int)T, (int)hidden, S)
  if (dtype == PA_F32) {
    if (hidden <= 8) PA_GHS_PATHS(float, 8); else PA_GHS_PATHS(float, 16);
  } else {
    if (hidden <= 8) PA_GHS_PATHS(double, 8); else PA_GHS_PATHS(double, 16);
  }
#undef PA_GHS_PATHS
  return pa::check_launch("gaussian_hmm_paths_kernel");
}

}  // extern "C"
