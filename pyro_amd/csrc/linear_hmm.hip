// linear_hmm.hip -- forward draws of a linear state-space model with ARBITRARY noise: sample paths of the observations
// (and, when asked for, of the latent states) from noise the caller has drawn, in ONE launch on the caller's stream.
//
// Reference path replaced: LinearHMM.rsample (pyro/distributions/hmm.py:1122-1138) over _linear_integrate
// (hmm.py:32-48): a Python loop over T of one small batched matmul, then one more for the observation map.  Here
// (row vectors, the conventions of gaussian_hmm.h)
//     z_0 = init,   z_t = z_{t-1} F_t + e_t,   y_t = z_t H_t + n_t,   t = 1..T
// with init, e_t, n_t draws of the three component distributions, loc and scale already applied: F multiplies init
// at the first step already, as in the reference.
//
// Grid (B, ceil(S / 64)), one wave per block, one lane per draw (the mapping of gaussian_hmm_draw.hip): z_t lives in
// MD registers, step t's (F, H) -- uniform over the wave, so every LDS read is a broadcast -- are staged through LDS
// (two buffers: the next step's are loaded into registers while the current step computes, one barrier per step; a
// time-homogeneous matrix is loaded once and written to each buffer once), every lane reads its e_t, n_t a step ahead
// and writes y[s, b, t, :] and, when asked for, z[s, b, t, :].  Noise and outputs are laid out [S, B, ...]:
// init [S, B, h], e [S, B, T, h], n [S, B, T, o], y [S, B, T, o], z [S, B, T, h].  No factors, no workspace, no flags,
// no atomics.  Non-finite noise is data: it flows into that draw's outputs and nowhere else.  A draw is a fixed
// sequence of operations on its own noise and its series' matrices: its bits do not depend on S or on the rest of
// the batch.
//
// gfx950 cross-compile (hipcc -O3, -Rpass-analysis=kernel-resource-usage), one wave of 64 lanes per block:
//     instantiation    VGPRs  AGPRs  SGPRs  scratch   LDS bytes   waves / SIMD
//     <float , 8>      96     0      106    0         1024        5
//     <float , 16>     141    0      106    0         4096        3
//     <double, 8>      178    0      106    0         2048        2
//     <double, 16>     256    4      106    0         8192        1       (AGPRs: the register file, not scratch)
#include "common.h"
#include "gaussian_hmm.h"

namespace pa {

struct LhdArgs {
  const void *F, *H;                         // [B | 1, T | 1, h, h], [B | 1, T | 1, h, o]
  int64_t F_sb, F_ss, H_sb, H_ss;            // batch and step strides in elements, 0 = shared / time-homogeneous
  const void *init, *e, *n;
  void *y, *z;
  int64_t B, S;
  int T, h, o;
};

// One lane per draw: z_t = z_{t-1} F_t + e_t and y_t = z_t H_t + n_t up the chain, the step's matrices staged through
// LDS.
template <typename T, int MD>
__global__ __launch_bounds__(64) void linear_hmm_draw_kernel(const LhdArgs a) {
  constexpr int MM = MD * MD, EPL = MM / 64, STEP = 2 * MM;
  constexpr int OF = 0, OH = MM;
  __shared__ T sm[2 * STEP];                 // two buffers of (F, H [MD, MD]), zero beyond h / o
  const int lane = threadIdx.x, h = a.h, o = a.o, Tn = a.T, hh = h * h, ho = h * o;
  const int64_t b = blockIdx.x, s = (int64_t)blockIdx.y * 64 + lane;
  const bool active = s < a.S;
  const int64_t sd = active ? s * a.B + b : 0;                   // this lane's draw among the S B
  const T* z0 = (const T*)a.init + sd * h;
  const T* eb = (const T*)a.e + sd * (int64_t)Tn * h;
  const T* nb = (const T*)a.n + sd * (int64_t)Tn * o;
  T* yb = (T*)a.y + sd * (int64_t)Tn * o;
  T* zb = a.z ? (T*)a.z + sd * (int64_t)Tn * h : nullptr;

  int ohh[EPL], oho[EPL];                    // this lane's elements of an [h, h], [h, o] matrix in the padded image
#pragma unroll                               // (-1: none)
  for (int k = 0; k < EPL; ++k) {
    const int el = lane + 64 * k;
    ohh[k] = el < hh ? (el / h) * MD + el % h : -1;
    oho[k] = el < ho ? (el / o) * MD + el % o : -1;
  }
  for (int el = lane; el < 2 * STEP; el += 64) sm[el] = T(0);
  const T* Fb = (const T*)a.F + b * a.F_sb;
  const T* Hb = (const T*)a.H + b * a.H_sb;

  T pF[EPL], pH[EPL], pe[MD], pn[MD], ev[MD], nv[MD], zc[MD];
#pragma unroll
  for (int k = 0; k < EPL; ++k) pF[k] = pH[k] = T(0);
#pragma unroll
  for (int j = 0; j < MD; ++j) pe[j] = pn[j] = ev[j] = nv[j] = zc[j] = T(0);
  // step t's matrices and noise into the registers (``all``: the time-homogeneous matrices too) ...
  auto load = [&](int t, bool all) {
#pragma unroll
    for (int k = 0; k < EPL; ++k) {
      if ((all || a.F_ss) && ohh[k] >= 0) pF[k] = Fb[(int64_t)t * a.F_ss + lane + 64 * k];
      if ((all || a.H_ss) && oho[k] >= 0) pH[k] = Hb[(int64_t)t * a.H_ss + lane + 64 * k];
    }
    if (active) {
#pragma unroll
      for (int j = 0; j < MD; ++j) {
        if (j < h) pe[j] = eb[(int64_t)t * h + j];
        if (j < o) pn[j] = nb[(int64_t)t * o + j];
      }
    }
  };
  // ... and from there into a buffer (``all``: a buffer's first fill)
  auto commit = [&](T* buf, bool all) {
#pragma unroll
    for (int k = 0; k < EPL; ++k) {
      if ((all || a.F_ss) && ohh[k] >= 0) buf[OF + ohh[k]] = pF[k];
      if ((all || a.H_ss) && oho[k] >= 0) buf[OH + oho[k]] = pH[k];
    }
#pragma unroll
    for (int j = 0; j < MD; ++j) {
      ev[j] = pe[j];
      nv[j] = pn[j];
    }
  };

  if (active) {
#pragma unroll
    for (int j = 0; j < MD; ++j)
      if (j < h) zc[j] = z0[j];
  }
  load(0, true);
  __syncthreads();                           // (the zero fill is done)
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
        T acc = ev[j];
#pragma unroll
        for (int i = 0; i < MD; ++i) acc += zc[i] * cur[OF + i * MD + j];
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
        T acc = nv[c];
#pragma unroll
        for (int j = 0; j < MD; ++j) acc += zn[j] * cur[OH + j * MD + c];
        if (active) yb[(int64_t)t * o + c] = acc;
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

}  // namespace pa

extern "C" {

int pa_linear_hmm_draw(int dtype, const void* F, int64_t F_stride_batch, int64_t F_stride_step, const void* H,
                       int64_t H_stride_batch, int64_t H_stride_step, int64_t B, int64_t T, int64_t hidden, int64_t obs,
                       int64_t S, const void* init, const void* e, const void* n, void* y, void* z,
                       pa_stream_t stream) {
  PA_REQUIRE(dtype == PA_F32 || dtype == PA_F64, "linear_hmm_draw: bad dtype %d", dtype);
  PA_REQUIRE(B >= 0 && T >= 1 && hidden >= 1 && obs >= 1 && S >= 0,
             "linear_hmm_draw: bad shape B=%lld T=%lld hidden=%lld obs=%lld S=%lld", (long long)B, (long long)T,
             (long long)hidden, (long long)obs, (long long)S);
  if (hidden > pa::GH_MAXHIDDEN || obs > pa::GH_MAXOBS)
    return pa::fail(PA_ERR_UNSUPPORTED, "linear_hmm_draw: hidden=%lld obs=%lld over the limit of %d / %d",
                    (long long)hidden, (long long)obs, pa::GH_MAXHIDDEN, pa::GH_MAXOBS);
  PA_REQUIRE(B < (int64_t(1) << 31) && T < (int64_t(1) << 31) && S <= int64_t(65535) * 64,
             "linear_hmm_draw: shape too large");
  if (B == 0 || S == 0) return PA_OK;
  PA_REQUIRE(F && H && init && e && n && y, "linear_hmm_draw: NULL pointer");
  PA_REQUIRE(F_stride_batch >= 0 && F_stride_step >= 0 && H_stride_batch >= 0 && H_stride_step >= 0,
             "linear_hmm_draw: negative stride");
  const pa::LhdArgs a{F, H, F_stride_batch, F_stride_step, H_stride_batch, H_stride_step, init, e, n, y, z, B, S,
                      (int)T, (int)hidden, (int)obs};
  hipStream_t st = pa::as_stream(stream);
  const bool small = hidden <= 8 && obs <= 8;
  const dim3 grid((unsigned)B, (unsigned)((S + 63) / 64));
#define PA_LHD_DRAW(T_, MD_) hipLaunchKernelGGL((pa::linear_hmm_draw_kernel<T_, MD_>), grid, dim3(64), 0, st, a)
  if (dtype == PA_F32) {
    if (small) PA_LHD_DRAW(float, 8); else PA_LHD_DRAW(float, 16);
  } else {
    if (small) PA_LHD_DRAW(double, 8); else PA_LHD_DRAW(double, 16);
  }
#undef PA_LHD_DRAW
  return pa::check_launch("linear_hmm_draw_kernel");
}

}  // extern "C"
