// gaussian_hmm.h -- what the Kalman filter / smoother kernel (gaussian_hmm.hip) and the backward-sampling kernels
// (gaussian_hmm_sample.hip) share: the dimension limits (larger dimensions return PA_ERR_UNSUPPORTED; the Python class
// then takes its torch route) and the wave-wide Cholesky and triangular solves on LDS matrices of row stride MD + 1.
#pragma once

#include <hip/hip_runtime.h>

namespace pa {

constexpr int GH_MAXHIDDEN = 16;
constexpr int GH_MAXOBS = 16;

__device__ __forceinline__ float gh_sqrt(float v) { return sqrtf(v); }
__device__ __forceinline__ double gh_sqrt(double v) { return sqrt(v); }
__device__ __forceinline__ float gh_log(float v) { return logf(v); }
__device__ __forceinline__ double gh_log(double v) { return log(v); }

// In-place Cholesky of the n x n matrix A (lower triangle read and written; row stride MD + 1) by the whole wave:
// returns sum log diag L, the same value in every lane.  A pivot that is not positive sets ``bad`` (uniformly:
// every lane reads the same pivot) and is replaced by 1 so that the sweep goes on with finite numbers.
template <typename T, int MD>
__device__ __forceinline__ T gh_cholesky(T* A, int n, int lane, bool& bad) {
  constexpr int LD = MD + 1, EPL = MD * MD / 64, JS = 64 / MD;
  const int i = lane % MD, j0 = lane / MD;
  T logdet = T(0);
  for (int k = 0; k < n; ++k) {
    T p = A[k * LD + k];
    if (!(p > T(0))) {
      bad = true;
      p = T(1);
    }
    const T d = gh_sqrt(p), inv = T(1) / d;
    logdet += gh_log(d);
    if (lane >= k && lane < n) A[lane * LD + k] = lane == k ? d : A[lane * LD + k] * inv;
    __syncthreads();
#pragma unroll
    for (int e = 0; e < EPL; ++e) {
      const int j = j0 + JS * e;
      if (j > k && j <= i && i < n) A[i * LD + j] -= A[i * LD + k] * A[j * LD + k];
    }
    __syncthreads();
  }
  return logdet;
}

// One lane's right-hand side v (element stride sv) against the factor L: v <- L^-1 v, returns |L^-1 v|^2 ...
template <typename T, int LD>
__device__ __forceinline__ T gh_forward_sub(const T* L, T* v, int sv, int n) {
  T quad = T(0);
  for (int i = 0; i < n; ++i) {
    T s = v[i * sv];
    for (int k = 0; k < i; ++k) s -= L[i * LD + k] * v[k * sv];
    s /= L[i * LD + i];
    v[i * sv] = s;
    quad += s * s;
  }
  return quad;
}
// ... and v <- L^-T v
template <typename T, int LD>
__device__ __forceinline__ void gh_backward_sub(const T* L, T* v, int sv, int n) {
  for (int i = n - 1; i >= 0; --i) {
    T s = v[i * sv];
    for (int k = i + 1; k < n; ++k) s -= L[k * LD + i] * v[k * sv];
    v[i * sv] = s / L[i * LD + i];
  }
}

}  // namespace pa
