// logchain.h -- the state limit and the log-sum-exp conventions of the chain kernels: shared by logchain.hip (the
// chain summed out) and logchain_decode.hip (the chain decoded).
#pragma once
#include <limits>

#include "common.h"
#include "dist_fam.h"

namespace pa {

constexpr int LC_MAXK = 64;

template <typename T>
__device__ __forceinline__ T lc_neg_inf() { return -std::numeric_limits<T>::infinity(); }
template <typename T>
__device__ __forceinline__ T lc_pos_inf() { return std::numeric_limits<T>::infinity(); }
// +inf potentials follow torch.logsumexp, as lse_fwd_kernel (logsumexp.hip) does: a sum that holds a +inf term
// is +inf -- the shift by the maximum would form exp(inf - inf).  Decided once per sum from its maximum, never
// per term: with a +inf maximum the terms are summed unshifted (lse_shift), so +inf and finite terms give +inf
// and a NaN term still gives NaN.  The online sum of the generic body cannot tell a NaN term from a second
// +inf once its maximum is +inf: there +inf wins (lse_value).
template <typename T>
__device__ __forceinline__ T lse_shift(T m) { return m == lc_pos_inf<T>() ? T(0) : m; }

// online log-sum-exp accumulation of value v into (m, s)
template <typename T>
__device__ __forceinline__ void lse_push(T v, T& m, T& s) {
  if (v == lc_neg_inf<T>()) return;
  if (v > m) {
    s = s * t_exp(m - v) + T(1);
    m = v;
  } else {
    s += t_exp(v - m);
  }
}
template <typename T>
__device__ __forceinline__ T lse_value(T m, T s) {
  return (m == lc_neg_inf<T>() || m == lc_pos_inf<T>()) ? m : m + t_log(s);
}

}  // namespace pa
