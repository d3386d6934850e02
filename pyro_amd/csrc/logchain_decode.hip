// logchain_decode.hip -- a chain of enumerated discrete variables decoded in ONE launch: its most probable path
// (Viterbi) or one joint draw from its posterior (backward messages, forward sampling).
//
// Reference path replaced: infer_discrete on a model written with pyro.markov (pyro/infer/discrete.py
// _sample_posterior_from_trace with the map / sample einsum backends, pyro/ops/einsum/torch_map.py, torch_sample.py):
// every one of the T states is read off a contraction of the whole chain.  The same values have a linear-time form.
// With u = unary [B, T, K], P_t = pairwise[b, t] (row-major [K, K], i = state at t, j = state at t + 1) and (+) = max
// (mode 0) or log-sum-exp (mode 1):
//   backward  m_{T-1} = 0,   m_t[i] = (+)_j (P_t[i, j] + u_{t+1}[j] + m_{t+1}[j])          t = T-2 .. 0
//   forward   s_t[j] = (t ? P_{t-1}[z_{t-1}, j] : 0) + u_t[j] + m_t[j]                       t = 0 .. T-1
//             mode 0: z_t = the smallest j with s_t[j] = max_j s_t[j];
//             mode 1: z_t = the smallest j with c_j > r c_{K-1}, clamped to the largest j with e_j > 0, where
//                     e_j = exp(s_t[j] - max_j s_t[j]), c = the prefix sums of e over the lanes in index order and
//                     r = element b of the Philox uniform stream (seed, offset + t step_blocks): the uniforms that T
//                     reservations of B elements, one per step, hand out (the rule of mixture_assign.hip);
//   log_norm[b] = (+)_j (u_0[j] + m_0[j]): the score of the returned path (mode 0) or log Z (mode 1).
// A step whose scores are all -inf or hold a NaN gets 0 and the chain goes on from state 0.
// One wave per sequence, as logchain.hip: the KP x G register layout with the matrices of the next D steps on their
// way for K <= 32, a lane per state with the matrix in LDS up to 64.  The forward pass is a chain of dependent steps
// -- the row of P to read follows from z_{t-1} --, so no step waits for a load whose address it has just computed:
// the register layout holds the whole P_t, prefetched, and picks the row by a lane exchange; a matrix shared by the
// steps is staged once (registers / LDS); only the lane-per-state kernel with per-step matrices reads the row
// directly, with u_t + m_t already in registers.
#include "common.h"
#include "dist_fam.h"
#include "logchain.h"
#include "mixture_lanes.h"
#include "mixture_assign.h"

namespace pa {

// one step's state from the scores s of its KP lanes (lane k of an aligned group of KP holds state k; -inf on padded
// lanes); every lane of the group returns it.  norm = (+)_k s_k.
template <int MODE, int KP, typename T>
__device__ __forceinline__ int lcd_pick(T s, bool kok, int k, int K, T r, T& norm) {
  const T ninf = lc_neg_inf<T>();
  const T m = mix_allreduce<KP>(s, [](T p, T q) { return mixa_max(p, q); });
  if constexpr (MODE == 0) {
    norm = m;
    const T first = mix_allreduce<KP>((kok && s == m) ? T(k) : T(KP), [](T p, T q) { return mixa_min(p, q); });
    return first < T(K) ? (int)first : 0;            // (a NaN maximum equals no score)
  } else {
    const bool dead = m != m || m == ninf;
    const T e = (dead || !kok) ? T(0) : (s == m ? T(1) : t_exp(s - m));
    T c = e;                                         // inclusive prefix sum over the group, in index order
#pragma unroll
    for (int o = 1; o < KP; o <<= 1) {
      // (lanes below o take nothing: a 0 / 1 factor in a vector register, where a hoisted lane mask per level would
      //  live in scalar registers the whole kernel long; up is a sum of terms in [0, 1], never inf or NaN)
      const T up = __shfl_up(c, o, KP);
      c += up * (k >= o ? T(1) : T(0));
    }
    const T tot = __shfl(c, K - 1, KP);
    norm = (m != m || m == ninf || m == lc_pos_inf<T>()) ? m : m + t_log(tot);
    const T thr = r * tot;
    const T first = mix_allreduce<KP>((kok && c > thr) ? T(k) : T(KP), [](T p, T q) { return mixa_min(p, q); });
    const T last = mix_allreduce<KP>((kok && e > T(0)) ? T(k) : T(-1), [](T p, T q) { return mix_max(p, q); });
    const int zi = (int)mixa_min(first, last);
    return (dead || zi < 0) ? 0 : zi;
  }
}

// ---- K <= 64: a lane per state, the matrix of a step in LDS --------------------------------------------------------
// U[B, T, K]; P[b, t] = P + b * spb + t * spt; msg: workspace [B, T, K]; z [B, T]; norm [B].
template <typename T, int MODE>
__global__ __launch_bounds__(64) void logchain_decode_kernel(const T* __restrict__ U, const T* __restrict__ P,
                                                             int64_t spb, int64_t spt, int Tn, int K, uint64_t seed,
                                                             uint64_t offset,
                                                             const uint64_t* __restrict__ offset_dev,
                                                             uint64_t step_blocks, T* __restrict__ msg,
                                                             int64_t* __restrict__ z_out, T* __restrict__ norm_out) {
  __shared__ T sP[LC_MAXK * LC_MAXK];
  __shared__ T sv[LC_MAXK];
  const int64_t b = blockIdx.x;
  const int j = threadIdx.x;
  const bool act = j < K;
  const int jc = act ? j : 0;
  const T NEG = lc_neg_inf<T>();
  const T* Ub = U + b * (int64_t)Tn * K;
  const T* Pb = P + b * spb;
  T* mb = msg + b * (int64_t)Tn * K;
  int64_t* zb = z_out + b * (int64_t)Tn;
  const bool shared = spt == 0;                       // one matrix for every step: staged once
  if (offset_dev) offset += *offset_dev;
  if (shared && Tn > 1)
    for (int e = j; e < K * K; e += 64) sP[e] = Pb[e];

  // ---- backward messages (lane = i) ---------------------------------------------------------------
  T beta = T(0);
  if (act) mb[(int64_t)(Tn - 1) * K + j] = beta;
  for (int t = Tn - 2; t >= 0; --t) {
    const T w = act ? Ub[(int64_t)(t + 1) * K + j] + beta : NEG;
    __syncthreads();
    if (act) sv[j] = w;
    if (!shared) {
      const T* Pt = Pb + (int64_t)t * spt;
      for (int e = j; e < K * K; e += 64) sP[e] = Pt[e];
    }
    __syncthreads();
    T m = NEG, s = T(0);
    if (act) {
      for (int jj = 0; jj < K; ++jj) {
        const T v = sP[j * K + jj] + sv[jj];
        if constexpr (MODE == 0) m = mixa_max(v, m); else lse_push(v, m, s);
      }
    }
    // (a sum of NaN terms only never raises the running maximum off -inf, where lse_value answers -inf: the NaN is in
    //  s; with a +inf maximum +inf wins, as in lse_value)
    beta = act ? (MODE == 0 ? m : (s != s && m != lc_pos_inf<T>()) ? s : lse_value(m, s)) : T(0);
    if (act) mb[(int64_t)t * K + j] = beta;
  }

  // ---- forward: one state per step (lane = j); a lane reads back the messages it wrote itself -------
  T um = act ? Ub[jc] + beta : NEG;                   // u_0 + m_0
  int z = 0;
  for (int t = 0; t < Tn; ++t) {
    T umn = T(0);
    if (t + 1 < Tn) umn = Ub[(int64_t)(t + 1) * K + jc] + mb[(int64_t)(t + 1) * K + jc];
    T s = um;
    if (t > 0) {
      const T row = shared ? sP[z * K + jc] : Pb[(int64_t)(t - 1) * spt + (int64_t)z * K + jc];
      s = act ? row + um : NEG;
    }
    const T r = MODE == 0 ? T(0) : mixa_uniform(T(0), seed, offset + (uint64_t)t * step_blocks, (uint64_t)b);
    T norm;
    z = __builtin_amdgcn_readfirstlane(lcd_pick<MODE, 64>(s, act, j, K, r, norm));
    if (j == 0) {
      zb[t] = (int64_t)z;
      if (t == 0) norm_out[b] = norm;
    }
    um = act ? umn : NEG;
  }
}

// ---- K <= 32: every lane works ---------------------------------------------------------------------------------
// The wave is a KP x G grid (logchain_lanes_kernel): in the backward pass lane (i, g) holds the NI = KP / G terms
// j = g NI .. of P[i, j] + u_{t+1}[j] + m_{t+1}[j] and reduces them in registers and across the G chunks by
// butterfly steps; in the forward pass lane (j, g) holds the rows i = g NI .. of column j of P_{t-1}, so the whole
// matrix is in the wave before z_{t-1} is known: the row is picked by one select per lane and one lane exchange.
template <typename T, int KP, int D, int MODE>
__global__ __launch_bounds__(64) void logchain_decode_lanes_kernel(const T* __restrict__ U,
                                                                   const T* __restrict__ P, int64_t spb,
                                                                   int64_t spt, int Tn, int K, uint64_t seed,
                                                                   uint64_t offset,
                                                                   const uint64_t* __restrict__ offset_dev,
                                                                   uint64_t step_blocks, T* __restrict__ msg,
                                                                   int64_t* __restrict__ z_out,
                                                                   T* __restrict__ norm_out) {
  constexpr int G = 64 / KP, NI = KP / G;
  const int64_t b = blockIdx.x;
  const int l = threadIdx.x, x = l % KP, g = l / KP;
  const bool xok = x < K, owner = xok && g == 0;
  const int xc = xok ? x : 0;
  const T NEG = lc_neg_inf<T>();
  const T* Ub = U + b * (int64_t)Tn * K;
  const T* Pb = P + b * spb;
  T* mb = msg + b * (int64_t)Tn * K;
  int64_t* zb = z_out + b * (int64_t)Tn;
  const bool shared = spt == 0;                       // one matrix for every step: loaded once, never again
  if (offset_dev) offset += *offset_dev;
  bool cok[NI];                         // is the q-th index of this lane's chunk a state?
  int cc[NI], sc[NI];                   // its index clamped for the loads / the lane its w is read from
#pragma unroll
  for (int q = 0; q < NI; ++q) {
    cok[q] = g * NI + q < K;
    cc[q] = cok[q] ? g * NI + q : 0;
    sc[q] = cok[q] ? g * NI + q : K;    // (a padded term reads lane K, which holds -inf: logchain_lanes_kernel)
  }
  // (+) of the NI terms of every lane of a row, over the G chunks: the same value in all of them
  auto oplus_chunks = [&](const T (&v)[NI]) {
    T m = v[0];
#pragma unroll
    for (int q = 1; q < NI; ++q) m = mixa_max(v[q], m);
#pragma unroll
    for (int o = KP; o < 64; o <<= 1) m = mixa_max(__shfl_xor(m, o, 64), m);
    if constexpr (MODE == 0) return m;
    const T sh = lse_shift(m);
    T s = T(0);
#pragma unroll
    for (int q = 0; q < NI; ++q) s += v[q] == NEG ? T(0) : t_exp(v[q] - sh);
#pragma unroll
    for (int o = KP; o < 64; o <<= 1) s += __shfl_xor(s, o, 64);
    return m == NEG ? NEG : sh + t_log(s);
  };

  // ---- backward messages: lane (i = x, chunk g of j) -----------------------------------------------
  T pre[D][NI], ub[D];
  auto load_row = [&](int t, T (&dst)[NI]) {                  // matrix t, this lane's terms of row x
    const T* Pt = Pb + (int64_t)t * spt;
#pragma unroll
    for (int q = 0; q < NI; ++q) {
      const T p = Pt[xc * K + cc[q]];
      dst[q] = (cok[q] && xok) ? p : NEG;
    }
  };
  T beta = T(0);
  if (owner) mb[(int64_t)(Tn - 1) * K + x] = beta;
#pragma unroll
  for (int d = 0; d < D; ++d)
    if (Tn - 2 - d >= 0) {
      load_row(Tn - 2 - d, pre[d]);
      ub[d] = Ub[(int64_t)(Tn - 1 - d) * K + xc];
    }
  for (int t0 = Tn - 2; t0 >= 0; t0 -= D) {
#pragma unroll
    for (int d = 0; d < D; ++d) {
      const int t = t0 - d;
      if (t >= 0) {                                            // (wave-uniform)
        const T wv = xok ? ub[d] + beta : NEG;                 // w[x] = u_{t+1}[x] + m_{t+1}[x]
        T v[NI];
#pragma unroll
        for (int q = 0; q < NI; ++q) v[q] = pre[d][q] + __shfl(wv, sc[q], 64);     // P[x, j] + w[j]
        if (t - D >= 0) {
          if (!shared) load_row(t - D, pre[d]);
          ub[d] = Ub[(int64_t)(t - D + 1) * K + xc];
        }
        beta = oplus_chunks(v);
        if (!xok) beta = T(0);
        if (owner) mb[(int64_t)t * K + x] = beta;
      }
    }
  }
  // the messages were written by the owners and are read back by every chunk of the column
  __threadfence_block();
  __syncthreads();

  // ---- forward: lane (j = x, chunk g of i) ---------------------------------------------------------
  // (no padding to -inf here: a row past K is never picked, z < K, and a column past K is masked where s is formed)
  auto load_col = [&](int t, T (&dst)[NI]) {                  // matrix t - 1, this lane's rows of column x
    const T* Pt = Pb + (int64_t)(t - 1) * spt;
#pragma unroll
    for (int q = 0; q < NI; ++q) dst[q] = Pt[cc[q] * K + xc];
  };
  auto load_um = [&](int t) { return Ub[(int64_t)t * K + xc] + mb[(int64_t)t * K + xc]; };
#pragma unroll
  for (int d = 0; d < D; ++d)
    if (1 + d < Tn) {
      load_col(1 + d, pre[d]);
      ub[d] = load_um(1 + d);
    }
  T norm;
  const T r0 = MODE == 0 ? T(0) : mixa_uniform(T(0), seed, offset, (uint64_t)b);
  int z = __builtin_amdgcn_readfirstlane(lcd_pick<MODE, KP>(xok ? Ub[xc] + beta : NEG, xok, x, K, r0, norm));
  if (l == 0) {
    zb[0] = (int64_t)z;
    norm_out[b] = norm;
  }
  for (int t0 = 1; t0 < Tn; t0 += D) {
    // the uniforms of the D steps of this round at once: lane d works out step t0 + d's (on the vector unit; D
    // wave-uniform Philox rounds in a row would run on the scalar unit and outgrow its registers)
    const T rv = MODE == 0 ? T(0)
                           : mixa_uniform(T(0), seed, offset + (uint64_t)(t0 + l % D) * step_blocks, (uint64_t)b);
#pragma unroll
    for (int d = 0; d < D; ++d) {
      const int t = t0 + d;
      if (t < Tn) {                                            // (wave-uniform)
        const int zq = z % NI;                                 // (wave-uniform: row z is term zq of chunk z / NI)
        T sel = pre[d][0];
#pragma unroll
        for (int q = 1; q < NI; ++q) sel = zq == q ? pre[d][q] : sel;
        const T row = __shfl(sel, (z / NI) * KP + x, 64);      // P_{t-1}[z, x]
        const T s = xok ? row + ub[d] : NEG;
        if (t + D < Tn) {
          if (!shared) load_col(t + D, pre[d]);
          ub[d] = load_um(t + D);
        }
        const T r = MODE == 0 ? T(0) : __shfl(rv, d, 64);
        z = __builtin_amdgcn_readfirstlane(lcd_pick<MODE, KP>(s, xok, x, K, r, norm));
        if (l == 0) zb[t] = (int64_t)z;
      }
    }
  }
}

template <typename T>
static void logchain_decode_launch(const T* U, const T* P, int64_t spb, int64_t spt, int64_t B, int Tn, int K,
                                   int mode, uint64_t seed, uint64_t offset, const uint64_t* offset_dev,
                                   uint64_t step_blocks, T* msg, int64_t* z, T* norm, hipStream_t s) {
  constexpr int D32 = sizeof(T) == 4 ? 4 : 2;         // the prefetch depths of logchain_lanes_kernel
#define PA_LCD_ARGS dim3((unsigned)B), dim3(64), 0, s, U, P, spb, spt, Tn, K, seed, offset, offset_dev, step_blocks, \
                    msg, z, norm
  if (K <= 16 && Tn > 1) {
    if (mode == 0) hipLaunchKernelGGL((logchain_decode_lanes_kernel<T, 16, 8, 0>), PA_LCD_ARGS);
    else hipLaunchKernelGGL((logchain_decode_lanes_kernel<T, 16, 8, 1>), PA_LCD_ARGS);
  } else if (K <= 32 && Tn > 1) {
    if (mode == 0) hipLaunchKernelGGL((logchain_decode_lanes_kernel<T, 32, D32, 0>), PA_LCD_ARGS);
    else hipLaunchKernelGGL((logchain_decode_lanes_kernel<T, 32, D32, 1>), PA_LCD_ARGS);
  } else {
    if (mode == 0) hipLaunchKernelGGL((logchain_decode_kernel<T, 0>), PA_LCD_ARGS);
    else hipLaunchKernelGGL((logchain_decode_kernel<T, 1>), PA_LCD_ARGS);
  }
#undef PA_LCD_ARGS
}

}  // namespace pa

extern "C" {

size_t pa_logchain_decode_workspace(int dtype, int64_t B, int64_t T, int64_t K) {
  if (B <= 0 || T <= 0 || K <= 0) return 0;
  return (size_t)(B * T * K) * (dtype == PA_F32 ? 4 : 8);
}

int pa_logchain_decode(int dtype, const void* unary, const void* pairwise, int64_t pair_stride_batch,
                       int64_t pair_stride_step, int64_t B, int64_t T, int64_t K, int mode, uint64_t seed,
                       uint64_t offset, const uint64_t* offset_dev, uint64_t step_blocks, int64_t* z_out,
                       void* log_norm, void* workspace, size_t workspace_bytes, pa_stream_t stream) {
  PA_REQUIRE(dtype == PA_F32 || dtype == PA_F64, "logchain_decode: bad dtype %d", dtype);
  PA_REQUIRE(B >= 0 && T >= 1 && K >= 1, "logchain_decode: bad shape B=%lld T=%lld K=%lld", (long long)B,
             (long long)T, (long long)K);
  if (K > pa::LC_MAXK)
    return pa::fail(PA_ERR_UNSUPPORTED, "logchain_decode: K=%lld > %d states", (long long)K, pa::LC_MAXK);
  PA_REQUIRE(mode == 0 || mode == 1, "logchain_decode: mode %d (0: most probable path, 1: a draw)", mode);
  PA_REQUIRE(B < (int64_t(1) << 31) && T < (int64_t(1) << 31), "logchain_decode: shape too large");
  if (B == 0) return PA_OK;
  PA_REQUIRE(unary && z_out && log_norm, "logchain_decode: NULL pointer");
  PA_REQUIRE(T == 1 || pairwise, "logchain_decode: NULL pairwise pointer");
  PA_REQUIRE(pair_stride_batch >= 0 && pair_stride_step >= 0, "logchain_decode: negative stride");
  PA_REQUIRE(workspace && workspace_bytes >= pa_logchain_decode_workspace(dtype, B, T, K),
             "logchain_decode: workspace too small");
  hipStream_t s = pa::as_stream(stream);
  if (dtype == PA_F32)
    pa::logchain_decode_launch<float>((const float*)unary, (const float*)pairwise, pair_stride_batch,
                                      pair_stride_step, B, (int)T, (int)K, mode, seed, offset, offset_dev,
                                      step_blocks, (float*)workspace, z_out, (float*)log_norm, s);
  else
    pa::logchain_decode_launch<double>((const double*)unary, (const double*)pairwise, pair_stride_batch,
                                       pair_stride_step, B, (int)T, (int)K, mode, seed, offset, offset_dev,
                                       step_blocks, (double*)workspace, z_out, (double*)log_norm, s);
  return pa::check_launch("logchain_decode_kernel");
}

}  // extern "C"
