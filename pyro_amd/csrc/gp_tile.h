// gp_tile.h -- what the tiled covariance kernels share (gp_kernel.hip, gp_periodic.hip): the 4-wide vector, the
// exponential of a float64 argument, the staging of a 64-row tile, the load of a thread's 4 x 4 entries of the incoming
// gradient and the sum over the 16 lanes of a row.  Geometry: gp_kernel_plan.h.
#pragma once
#include "common.h"
#include "gp_kernel_plan.h"

namespace pa {

template <typename T>
struct alignas(4 * sizeof(T)) Vec4 {
  T v[4];
};

// exp(a) for an argument held in float64.  In float32 the argument is split into its rounded value and the remainder,
// exp(hi + lo) = exp(hi) (1 + lo): rounding a = -r2 / 2 to float32 alone would cost |a| 2^-24 relative (4e-6 at r2 = 130).
template <typename T>
__device__ __forceinline__ T gp_exp_of(double a) {
  if constexpr (sizeof(T) == 8) {
    return exp(a);
  } else {
    const float hi = (float)a, lo = (float)(a - (double)hi);
    return expf(hi) * (1.0f + lo);
  }
}

// ---- staging: rows [first, first + 64) of p [n, D] into tile [64, stride], zeros past the end ----------------------
template <typename T>
__device__ __forceinline__ void gp_stage(const T* __restrict__ p, int64_t first, int64_t n, int D, int stride, T* tile) {
  const int total = GPK_TILE * D;
  for (int e = threadIdx.x; e < total; e += GPK_THREADS) {
    const int row = e / D, k = e - row * D;
    const int64_t i = first + row;
    tile[row * stride + k] = i < n ? p[i * D + k] : T(0);
  }
}

// sum over the 16 lanes of a DPP row (the lanes that share ty); every lane of the wave must be active
template <typename T>
__device__ __forceinline__ T gp_row16_sum(T v) {
  v += dpp_get<0xB1>(v);
  v += dpp_get<0x4E>(v);
  v += dpp_get<0x141>(v);
  v += dpp_get<0x140>(v);
  return v;
}

// ``a`` carries G, R and C: G(i, j) at i * sr + j * sc for the thread's 4 x 4 entries, zero outside [R, C]
template <typename T, template <typename> class ARGS>
__device__ __forceinline__ void gp_load_g(const ARGS<T>& a, int64_t sr, int64_t sc, int64_t i0, int64_t j0, int ty,
                                          int tx, T (&g)[4][4]) {
  const int64_t i = i0 + 4 * ty, j = j0 + 4 * tx;
  const bool inside = i + 3 < a.R && j + 3 < a.C && (uintptr_t)a.G % sizeof(Vec4<T>) == 0;
  if (sc == 1 && inside && (sr & 3) == 0) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const Vec4<T> v = *reinterpret_cast<const Vec4<T>*>(a.G + (i + r) * sr + j);
#pragma unroll
      for (int c = 0; c < 4; ++c) g[r][c] = v.v[c];
    }
  } else if (sr == 1 && inside && (sc & 3) == 0) {
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const Vec4<T> v = *reinterpret_cast<const Vec4<T>*>(a.G + (j + c) * sc + i);
#pragma unroll
      for (int r = 0; r < 4; ++r) g[r][c] = v.v[r];
    }
  } else {
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int c = 0; c < 4; ++c) g[r][c] = (i + r < a.R && j + c < a.C) ? a.G[(i + r) * sr + (j + c) * sc] : T(0);
  }
}

}  // namespace pa
