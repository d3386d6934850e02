// gaussian_hmm_draw.hip -- forward draws of a linear-Gaussian state-space model: sample paths of the observations
// (and, when asked for, of the latent states) from the prior, in TWO launches on the caller's stream.
//
// Reference path replaced: GaussianHMM.rsample (pyro/distributions/hmm.py:584-594) over
// sequential_gaussian_filter_sample (pyro/ops/gaussian.py:600) and Gaussian.left_condition(z).rsample(): the
// parallel-scan filter with its tape and O(log T) rounds of conditional draws, then one more batched Cholesky for the
// observation noise.  Here (row vectors, the conventions of gaussian_hmm.h)
//     z_0 = m0 + L_0 e_0,   z_t = z_{t-1} F_t + q_t + L_{Q,t} e_t,   x_t = z_t H_t + r_t + L_{R,t} e'_t,   t = 1..T
// with L L^T the Cholesky factors of P0, Q_t, R_t, each acting on its noise as L e.
//
// Factors kernel, one wave per DISTINCT matrix: P0 per series (once when its batch stride is 0), Q and R per series
// and per step along the axes whose stride is not 0 -- a time-homogeneous parameter shared by the series is factored
// once.  gh_cholesky of gaussian_hmm.h; the factor goes to the workspace as a dense row-major matrix with zeros above
// the diagonal, and the wave stores whether it met a non-positive pivot into a slot of its own.  No atomics.
//
// Draw kernel, grid (B, ceil(S / 64)), one wave per block, one lane per draw: z_t lives in MD registers, step t's
// (F, q, L_Q, H, r, L_R) -- uniform over the wave -- are staged through LDS (two buffers: the next step's are loaded
// into registers while the current step computes, one barrier per step; a time-homogeneous parameter is loaded once
// and written to each buffer once), every lane reads its e_t, e'_t a step ahead and writes x[s, b, t, :] and, when
// asked for, z[s, b, t, :].  Noise and outputs are laid out [S, B, ...]: eps0 [S, B, h], eps_z [S, B, T, h],
// eps_x [S, B, T, o], x [S, B, T, o], z [S, B, T, h].  A series one of whose factors has a recorded bad pivot (its
// own or a shared parameter's) writes NaN for the whole series; no other series sees it.  A draw is a fixed sequence
// of operations on its own noise and its series' parameters: its bits do not depend on S or on the rest of the batch.
//
// gfx950 cross-compile (hipcc -O3, -Rpass-analysis=kernel-resource-usage), one wave of 64 lanes per block:
//     kernel   instantiation    VGPRs  SGPRs  scratch   LDS bytes   waves / SIMD
//     factors  <float , 8>      51     49     0         288         8
//     factors  <float , 16>     51     49     0         1088        8
//     factors  <double, 8>      20     49     0         576         8
//     factors  <double, 16>     24     49     0         2176        8
//     draw     <float , 8>      107    106    0         2432        4
//     draw     <float , 16>     160    106    0         8704        3
//     draw     <double, 8>      193    106    0         4608        2
//     draw     <double, 16>     256    106    0         17152       1       (+ 44 AGPRs: the register file, not scratch)
#include <limits>

#include "common.h"
#include "gaussian_hmm.h"

namespace pa {

struct GhdArgs {
  GhModel m;                                 // (m.x is not used: there is no data)
  const void *eps0, *eps_z, *eps_x;
  void *x, *z;
  void *L0, *LQ, *LR;                        // the factors: [nP0, h, h], [nQb, nQt, h, h], [nRb, nRt, o, o]
  int* flags;                                // one per factor, in that order: 1 = a non-positive pivot
  int64_t B, S, nP0, nQb, nQt, nRb, nRt;
};

// One wave per distinct matrix of P0, Q, R: its Cholesky factor and its flag.
template <typename T, int MD>
__global__ __launch_bounds__(64) void gaussian_hmm_factors_kernel(const GhdArgs a) {
  constexpr int LD = MD + 1;
  __shared__ T sA[MD * LD];
  const int lane = threadIdx.x;
  const int64_t w = blockIdx.x, nQ = a.nQb * a.nQt;
  const T* src;
  T* dst;
  int n;
  if (w < a.nP0) {
    n = a.m.h;
    src = (const T*)a.m.P0 + w * a.m.P0_sb;
    dst = (T*)a.L0 + w * n * n;
  } else if (w < a.nP0 + nQ) {
    const int64_t k = w - a.nP0;
    n = a.m.h;
    src = (const T*)a.m.Q + (k / a.nQt) * a.m.Q_sb + (k % a.nQt) * a.m.Q_ss;
    dst = (T*)a.LQ + k * n * n;
  } else {
    const int64_t k = w - a.nP0 - nQ;
    n = a.m.o;
    src = (const T*)a.m.R + (k / a.nRt) * a.m.R_sb + (k % a.nRt) * a.m.R_ss;
    dst = (T*)a.LR + k * n * n;
  }
  const int nn = n * n;
  for (int e = lane; e < nn; e += 64) sA[(e / n) * LD + e % n] = src[e];
  __syncthreads();
  bool bad = false;
  gh_cholesky<T, MD>(sA, n, lane, bad);
  for (int e = lane; e < nn; e += 64) {
    const int i = e / n, c = e % n;
    dst[e] = c <= i ? sA[i * LD + c] : T(0);
  }
  if (lane == 0) a.flags[w] = bad ? 1 : 0;
}

// One lane per draw: z_t = z_{t-1} F_t + q_t + L_Q e_t and x_t = z_t H_t + r_t + L_R e'_t up the chain, the step's
// parameters staged through LDS.
template <typename T, int MD>
__global__ __launch_bounds__(64) void gaussian_hmm_draw_kernel(const GhdArgs a) {
  constexpr int MM = MD * MD, EPL = MM / 64, STEP = 4 * MM + 2 * MD;
  constexpr int OF = 0, OLQ = MM, OH = 2 * MM, OLR = 3 * MM, Oq = 4 * MM, Or = 4 * MM + MD;
  __shared__ T sm[2 * STEP];                 // two buffers of (F, L_Q, H, L_R [MD, MD], q, r [MD]), zero beyond h / o
  const int lane = threadIdx.x, h = a.m.h, o = a.m.o, Tn = a.m.T, hh = h * h, ho = h * o, oo = o * o;
  const int64_t b = blockIdx.x, s = (int64_t)blockIdx.y * 64 + lane;
  const bool active = s < a.S;
  const int64_t bp = a.m.P0_sb ? b : 0, bq = a.m.Q_sb ? b : 0, br = a.m.R_sb ? b : 0;
  const int64_t sd = active ? s * a.B + b : 0;                   // this lane's draw among the S B
  const T* e0 = (const T*)a.eps0 + sd * h;
  const T* ez = (const T*)a.eps_z + sd * (int64_t)Tn * h;
  const T* ex = (const T*)a.eps_x + sd * (int64_t)Tn * o;
  T* xb = (T*)a.x + sd * (int64_t)Tn * o;
  T* zb = a.z ? (T*)a.z + sd * (int64_t)Tn * h : nullptr;

  // the flags of this series' factors: P0's, then those of every step of Q and R
  int badv = a.flags[bp];
  {
    const int* fq = a.flags + a.nP0 + bq * a.nQt;
    for (int64_t k = lane; k < a.nQt; k += 64) badv |= fq[k];
    const int* fr = a.flags + a.nP0 + a.nQb * a.nQt + br * a.nRt;
    for (int64_t k = lane; k < a.nRt; k += 64) badv |= fr[k];
  }
  if (__syncthreads_or(badv)) {
    const T NaN = std::numeric_limits<T>::quiet_NaN();
    if (active) {
      for (int64_t e = 0; e < (int64_t)Tn * o; ++e) xb[e] = NaN;
      if (zb)
        for (int64_t e = 0; e < (int64_t)Tn * h; ++e) zb[e] = NaN;
    }
    return;
  }

  int ohh[EPL], oho[EPL], ooo[EPL];          // this lane's elements of an [h, h], [h, o], [o, o] matrix in the padded
#pragma unroll                               // image (-1: none)
  for (int k = 0; k < EPL; ++k) {
    const int e = lane + 64 * k;
    ohh[k] = e < hh ? (e / h) * MD + e % h : -1;
    oho[k] = e < ho ? (e / o) * MD + e % o : -1;
    ooo[k] = e < oo ? (e / o) * MD + e % o : -1;
  }
  for (int e = lane; e < 2 * STEP; e += 64) sm[e] = T(0);
  const T* Fb = (const T*)a.m.F + b * a.m.F_sb;
  const T* qb = (const T*)a.m.q + b * a.m.q_sb;
  const T* Hb = (const T*)a.m.H + b * a.m.H_sb;
  const T* rb = (const T*)a.m.r + b * a.m.r_sb;
  const int64_t LQ_ss = a.m.Q_ss ? hh : 0, LR_ss = a.m.R_ss ? oo : 0;
  const T* LQb = (const T*)a.LQ + bq * a.nQt * hh;
  const T* LRb = (const T*)a.LR + br * a.nRt * oo;

  T pF[EPL], pLQ[EPL], pH[EPL], pLR[EPL], pq = T(0), pr = T(0), pez[MD], pex[MD], evz[MD], evx[MD], zc[MD];
#pragma unroll
  for (int k = 0; k < EPL; ++k) pF[k] = pLQ[k] = pH[k] = pLR[k] = T(0);
#pragma unroll
  for (int j = 0; j < MD; ++j) pez[j] = pex[j] = evz[j] = evx[j] = zc[j] = T(0);
  // step t's parameters and noise into the registers (``all``: the time-homogeneous parameters too) ...
  auto load = [&](int t, bool all) {
#pragma unroll
    for (int k = 0; k < EPL; ++k) {
      if ((all || a.m.F_ss) && ohh[k] >= 0) pF[k] = Fb[(int64_t)t * a.m.F_ss + lane + 64 * k];
      if ((all || LQ_ss) && ohh[k] >= 0) pLQ[k] = LQb[(int64_t)t * LQ_ss + lane + 64 * k];
      if ((all || a.m.H_ss) && oho[k] >= 0) pH[k] = Hb[(int64_t)t * a.m.H_ss + lane + 64 * k];
      if ((all || LR_ss) && ooo[k] >= 0) pLR[k] = LRb[(int64_t)t * LR_ss + lane + 64 * k];
    }
    if ((all || a.m.q_ss) && lane < h) pq = qb[(int64_t)t * a.m.q_ss + lane];
    if ((all || a.m.r_ss) && lane < o) pr = rb[(int64_t)t * a.m.r_ss + lane];
    if (active) {
#pragma unroll
      for (int j = 0; j < MD; ++j) {
        if (j < h) pez[j] = ez[(int64_t)t * h + j];
        if (j < o) pex[j] = ex[(int64_t)t * o + j];
      }
    }
  };
  // ... and from there into a buffer (``all``: a buffer's first fill)
  auto commit = [&](T* buf, bool all) {
#pragma unroll
    for (int k = 0; k < EPL; ++k) {
      if ((all || a.m.F_ss) && ohh[k] >= 0) buf[OF + ohh[k]] = pF[k];
      if ((all || LQ_ss) && ohh[k] >= 0) buf[OLQ + ohh[k]] = pLQ[k];
      if ((all || a.m.H_ss) && oho[k] >= 0) buf[OH + oho[k]] = pH[k];
      if ((all || LR_ss) && ooo[k] >= 0) buf[OLR + ooo[k]] = pLR[k];
    }
    if ((all || a.m.q_ss) && lane < h) buf[Oq + lane] = pq;
    if ((all || a.m.r_ss) && lane < o) buf[Or + lane] = pr;
#pragma unroll
    for (int j = 0; j < MD; ++j) {
      evz[j] = pez[j];
      evx[j] = pex[j];
    }
  };

  // the initial state: (m0, L_0) pass through the q and L_Q slots of the second buffer, which step 1 fills anew
  __syncthreads();
  {
    T* const ini = sm + STEP;
    const T* m0b = (const T*)a.m.m0 + b * a.m.m0_sb;
    const T* L0b = (const T*)a.L0 + bp * hh;
    if (lane < h) ini[Oq + lane] = m0b[lane];
#pragma unroll
    for (int k = 0; k < EPL; ++k)
      if (ohh[k] >= 0) ini[OLQ + ohh[k]] = L0b[lane + 64 * k];
    if (active) {
#pragma unroll
      for (int j = 0; j < MD; ++j)
        if (j < h) evz[j] = e0[j];
    }
    load(0, true);
    __syncthreads();
#pragma unroll
    for (int i = 0; i < MD; ++i)
      if (i < h) {
        T acc = ini[Oq + i];
#pragma unroll
        for (int j = 0; j <= i; ++j) acc += ini[OLQ + i * MD + j] * evz[j];
        zc[i] = acc;
      }
  }
  commit(sm, true);
  if (Tn > 1) load(1, false);
  __syncthreads();
  for (int t = 0; t < Tn; ++t) {
    const T* cur = sm + (t & 1) * STEP;
    T zn[MD];
#pragma unroll
    for (int j = 0; j < MD; ++j) {
      zn[j] = T(0);
      if (j < h) {
        T acc = cur[Oq + j];
#pragma unroll
        for (int i = 0; i < MD; ++i) acc += zc[i] * cur[OF + i * MD + j];
#pragma unroll
        for (int k = 0; k <= j; ++k) acc += cur[OLQ + j * MD + k] * evz[k];
        zn[j] = acc;
      }
    }
    if (active && zb) {
#pragma unroll
      for (int j = 0; j < MD; ++j)
        if (j < h) zb[(int64_t)t * h + j] = zn[j];
    }
#pragma unroll
    for (int c = 0; c < MD; ++c)
      if (c < o) {
        T acc = cur[Or + c];
#pragma unroll
        for (int j = 0; j < MD; ++j) acc += zn[j] * cur[OH + j * MD + c];
#pragma unroll
        for (int k = 0; k <= c; ++k) acc += cur[OLR + c * MD + k] * evx[k];
        if (active) xb[(int64_t)t * o + c] = acc;
      }
#pragma unroll
    for (int j = 0; j < MD; ++j) zc[j] = zn[j];
    if (t + 1 < Tn) {
      // (the other buffer was last read in the step before this one, which every lane left through the barrier)
      commit(sm + ((t + 1) & 1) * STEP, t == 0);
      if (t + 2 < Tn) load(t + 2, false);
    }
    __syncthreads();
  }
}

// the factors and flags the strides make distinct
struct GhdCounts {
  int64_t nP0, nQb, nQt, nRb, nRt;
  int64_t factors() const { return nP0 + nQb * nQt + nRb * nRt; }
  size_t bytes(size_t el, int64_t h, int64_t o) const {
    return (size_t)(nP0 * h * h + nQb * nQt * h * h + nRb * nRt * o * o) * el + (size_t)factors() * sizeof(int);
  }
};

}  // namespace pa

extern "C" {

size_t pa_gaussian_hmm_draw_workspace(int dtype, int64_t B, int64_t T, int64_t hidden, int64_t obs) {
  if (B <= 0 || T <= 0 || hidden <= 0 || obs <= 0) return 0;
  const pa::GhdCounts n{B, B, T, B, T};
  return n.bytes(dtype == PA_F32 ? 4 : 8, hidden, obs);
}

int pa_gaussian_hmm_draw(int dtype, const void* m0, int64_t m0_stride_batch, const void* P0, int64_t P0_stride_batch,
                         const void* F, int64_t F_stride_batch, int64_t F_stride_step, const void* q,
                         int64_t q_stride_batch, int64_t q_stride_step, const void* Q, int64_t Q_stride_batch,
                         int64_t Q_stride_step, const void* H, int64_t H_stride_batch, int64_t H_stride_step,
                         const void* r, int64_t r_stride_batch, int64_t r_stride_step, const void* R,
                         int64_t R_stride_batch, int64_t R_stride_step, int64_t B, int64_t T, int64_t hidden,
                         int64_t obs, int64_t S, const void* eps0, const void* eps_z, const void* eps_x, void* x,
                         void* z, void* workspace, size_t workspace_bytes, pa_stream_t stream) {
  PA_REQUIRE(dtype == PA_F32 || dtype == PA_F64, "gaussian_hmm_draw: bad dtype %d", dtype);
  PA_REQUIRE(B >= 0 && T >= 1 && hidden >= 1 && obs >= 1 && S >= 0,
             "gaussian_hmm_draw: bad shape B=%lld T=%lld hidden=%lld obs=%lld S=%lld", (long long)B, (long long)T,
             (long long)hidden, (long long)obs, (long long)S);
  if (hidden > pa::GH_MAXHIDDEN || obs > pa::GH_MAXOBS)
    return pa::fail(PA_ERR_UNSUPPORTED, "gaussian_hmm_draw: hidden=%lld obs=%lld over the limit of %d / %d",
                    (long long)hidden, (long long)obs, pa::GH_MAXHIDDEN, pa::GH_MAXOBS);
  PA_REQUIRE(B < (int64_t(1) << 31) && T < (int64_t(1) << 31) && S <= int64_t(65535) * 64,
             "gaussian_hmm_draw: shape too large");
  if (B == 0 || S == 0) return PA_OK;
  PA_REQUIRE(m0 && P0 && F && q && Q && H && r && R && eps0 && eps_z && eps_x && x,
             "gaussian_hmm_draw: NULL pointer");
  PA_REQUIRE(m0_stride_batch >= 0 && P0_stride_batch >= 0 && F_stride_batch >= 0 && F_stride_step >= 0 &&
                 q_stride_batch >= 0 && q_stride_step >= 0 && Q_stride_batch >= 0 && Q_stride_step >= 0 &&
                 H_stride_batch >= 0 && H_stride_step >= 0 && r_stride_batch >= 0 && r_stride_step >= 0 &&
                 R_stride_batch >= 0 && R_stride_step >= 0,
             "gaussian_hmm_draw: negative stride");
  const pa::GhdCounts n{P0_stride_batch ? B : 1, Q_stride_batch ? B : 1, Q_stride_step ? T : 1,
                        R_stride_batch ? B : 1, R_stride_step ? T : 1};
  const size_t el = dtype == PA_F32 ? 4 : 8;
  PA_REQUIRE(n.factors() < (int64_t(1) << 31), "gaussian_hmm_draw: too many matrices to factor");
  PA_REQUIRE(workspace && workspace_bytes >= n.bytes(el, hidden, obs), "gaussian_hmm_draw: workspace too small");
  const int64_t hh = hidden * hidden;
  char* w = (char*)workspace;
  void* L0 = w;
  void* LQ = w + (size_t)(n.nP0 * hh) * el;
  void* LR = w + (size_t)((n.nP0 + n.nQb * n.nQt) * hh) * el;
  int* flags = (int*)(w + (size_t)((n.nP0 + n.nQb * n.nQt) * hh + n.nRb * n.nRt * obs * obs) * el);
  pa::GhdArgs a{{m0, P0, F, q, Q, H, r, R, nullptr,
                 m0_stride_batch, P0_stride_batch, F_stride_batch, F_stride_step, q_stride_batch, q_stride_step,
                 Q_stride_batch, Q_stride_step, H_stride_batch, H_stride_step, r_stride_batch, r_stride_step,
                 R_stride_batch, R_stride_step, (int)T, (int)hidden, (int)obs},
                eps0, eps_z, eps_x, x, z, L0, LQ, LR, flags, B, S, n.nP0, n.nQb, n.nQt, n.nRb, n.nRt};
  hipStream_t st = pa::as_stream(stream);
  const bool small = hidden <= 8 && obs <= 8;
#define PA_GHD_FACTORS(T_, MD_) \
  hipLaunchKernelGGL((pa::gaussian_hmm_factors_kernel<T_, MD_>), dim3((unsigned)n.factors()), dim3(64), 0, st, a)
  if (dtype == PA_F32) {
    if (small) PA_GHD_FACTORS(float, 8); else PA_GHD_FACTORS(float, 16);
  } else {
    if (small) PA_GHD_FACTORS(double, 8); else PA_GHD_FACTORS(double, 16);
  }
#undef PA_GHD_FACTORS
  const int rc = pa::check_launch("gaussian_hmm_factors_kernel");
  if (rc != PA_OK) return rc;
  const dim3 grid((unsigned)B, (unsigned)((S + 63) / 64));
#define PA_GHD_DRAW(T_, MD_) hipLaunchKernelGGL((pa::gaussian_hmm_draw_kernel<T_, MD_>), grid, dim3(64), 0, st, a)
  if (dtype == PA_F32) {
    if (small) PA_GHD_DRAW(float, 8); else PA_GHD_DRAW(float, 16);
  } else {
    if (small) PA_GHD_DRAW(double, 8); else PA_GHD_DRAW(double, 16);
  }
#undef PA_GHD_DRAW
  return pa::check_launch("gaussian_hmm_draw_kernel");
}

}  // extern "C"
