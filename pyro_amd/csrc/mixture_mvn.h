// mixture_mvn.h -- the full-covariance mixture leaf's limits, staging (mvn_stage) and quadratic form (mvn_quad):
// shared by mixture_mvn.hip (lse and stats launches) and mixture_assign_wide.hip.
#pragma once
#include "common.h"
#include "dist_fam.h"

namespace pa {

constexpr int MVN_THREADS = 256;
constexpr int MVN_MAXK = 64;
constexpr int MVN_MAXD = 64;
constexpr int MVN_LSE_BLOCKS = 2048;    // launch 1: workgroups over all parameter sets (at most, plus B)
constexpr int MVN_STAT_BLOCKS = 1024;   // launch 2: workgroups over all (k, b) (at most, plus K B)

static int mvn_padded_d(int D) { return D <= 8 ? 8 : D <= 16 ? 16 : D <= 32 ? 32 : 64; }
__host__ __device__ inline int64_t mvn_record(int DP) { return 1 + DP + (int64_t)DP * DP; }
static int64_t mvn_lse_blocks_max(int64_t B) { int64_t g = (MVN_LSE_BLOCKS + B - 1) / B; return g < 1 ? 1 : g; }
static int64_t mvn_chunks_max(int K, int64_t B) {
  const int64_t kb = (int64_t)K * B;
  int64_t c = (MVN_STAT_BLOCKS + kb - 1) / kb;
  return c < 1 ? 1 : c;
}

// Stage component k of the current set: W_k (lower triangle, zero past D) in Ws[DP][DP], mu_k in mus, and the
// constant a_k + sum_i log W_ii - D/2 log 2 pi in ck[0].  Every thread of the workgroup calls it.
template <typename T, int DP>
__device__ __forceinline__ void mvn_stage(T* Ws, T* mus, T* ck, const T* __restrict__ a, const T* __restrict__ loc,
                                          int64_t l_sk, const T* __restrict__ w, int64_t w_sk, int D, int k) {
  const int tid = threadIdx.x;
  __syncthreads();                                  // (the previous component's readers are done)
  const T* wk = w + (int64_t)k * w_sk;
  for (int e = tid; e < DP * DP; e += MVN_THREADS) {
    const int i = e / DP, j = e % DP;
    Ws[e] = (i < D && j <= i) ? wk[i * D + j] : T(0);
  }
  if (tid < DP) mus[tid] = tid < D ? loc[(int64_t)k * l_sk + tid] : T(0);
  if (tid < 64) {                                   // (DP <= 64: wave 0)
    T v = tid < D ? t_log(wk[tid * D + tid]) : T(0);
    v = wave_sum(v);
    if (tid == 0) ck[0] = a[k] + v - T(D) * Consts<T>::half_log_2pi;
  }
  __syncthreads();
}

// |W d|^2 over the rows i < D of the staged triangle (d and W are zero past D)
template <typename T, int DP>
__device__ __forceinline__ T mvn_quad(const T* Ws, const T (&d)[DP], int D) {
  T q = T(0);
#pragma unroll
  for (int i = 0; i < DP; ++i) {
    if (i < D) {
      T z = T(0);
#pragma unroll
      for (int j = 0; j <= i; ++j) z += Ws[i * DP + j] * d[j];
      q += z * z;
    }
  }
  return q;
}

}  // namespace pa
