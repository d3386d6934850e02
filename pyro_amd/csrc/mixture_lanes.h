// mixture_lanes.h -- the lane layout the mixture leaves share (mixture.hip, mixture_rows.hip): KP = K rounded up to a
// power of two (<= 64) lanes hold one row's K terms, and a reduction over a row's terms is an all-reduce over KP
// aligned lanes.
#pragma once
#include "common.h"
#include "dist_fam.h"

namespace pa {

constexpr int MIX_THREADS = 256;
constexpr int MIX_MAXK = 64;

template <typename T> __device__ __forceinline__ T mix_max(T a, T b) { return a > b ? a : b; }

// The value of lane (l ^ o) for o < 16 without the LDS crossbar: after quad_perm [1,0,3,2] and [2,3,0,1] every lane
// of a quad has combined the quad's four values; row_half_mirror exchanges the two quads of 8 lanes, row_mirror the
// two halves of 16 -- an all-reduce over 2 / 4 / 8 / 16 lanes in 1..4 DPP moves (ds_bpermute: an LDS instruction
// and its wait each).  64-bit values travel as two halves.
template <int CTRL> __device__ __forceinline__ float mix_dpp(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xf, 0xf, false));
}
template <int CTRL> __device__ __forceinline__ double mix_dpp(double v) {
  const uint64_t u = __builtin_bit_cast(uint64_t, v);
  const uint32_t lo = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)u, CTRL, 0xf, 0xf, false);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)(u >> 32), CTRL, 0xf, 0xf, false);
  return __builtin_bit_cast(double, ((uint64_t)hi << 32) | lo);
}
// all-reduce over the KP lanes (a power of two, aligned) that hold one row's terms
template <int KP, typename T, typename Op> __device__ __forceinline__ T mix_allreduce(T v, Op op) {
  if constexpr (KP >= 2) v = op(v, mix_dpp<0xB1>(v));
  if constexpr (KP >= 4) v = op(v, mix_dpp<0x4E>(v));
  if constexpr (KP >= 8) v = op(v, mix_dpp<0x141>(v));
  if constexpr (KP >= 16) v = op(v, mix_dpp<0x140>(v));
  if constexpr (KP >= 32) v = op(v, __shfl_xor(v, 16, 64));
  if constexpr (KP >= 64) v = op(v, __shfl_xor(v, 32, 64));
  return v;
}

// max that hands on a NaN whichever side it is on (both lanes of a butterfly step agree)
template <typename T> __device__ __forceinline__ T mix_nanmax(T a, T b) { return (a > b || a != a) ? a : b; }

// one row's logsumexp and responsibilities from its KP lanes' terms.  t = -inf on padded lanes.  A row whose every
// term is -inf: lse = -inf, r = 0; a NaN term: lse and every r of the row NaN.
template <int KP, typename T>
__device__ __forceinline__ void mix_row(T t, bool kok, T& lse, T& r) {
  const T ninf = -t_inf<T>();
  const T m = mix_allreduce<KP>(t, [](T p, T q) { return mix_nanmax(p, q); });
  const bool dead = m == ninf;
  const T e = (dead || !kok) ? T(0) : t_exp(t - m);
  const T ssum = mix_allreduce<KP>(e, [](T p, T q) { return p + q; });
  // (ssum >= 1 for a live row: the hardware log / reciprocal of the float path are 1 ulp there)
  lse = dead ? ninf : m + pos_log(dead ? T(1) : ssum);
  r = dead ? T(0) : e * pos_rcp(dead ? T(1) : ssum);
}

}  // namespace pa
