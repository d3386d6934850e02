// gp_tile.h -- the frame that the kernels on the 64 x 64 tile share (gp_kernel.hip, gp_wrap.hip, gp_periodic.hip,
// gp_compose.hip; gp_dot.hip takes the row-record copy and the sum over the splits): the 4-wide vector, the staging of
// a 64-row tile, the float64 r2 of a thread's entries (gp_kernel.hip and gp_wrap.hip), the load of a thread's 4 x 4
// entries of the incoming gradient, the adds into the one-writer float64
// accumulators, the four-wave fold, the row-record copy and the finalize's sum over the splits.  (Two pieces of the
// frame stay spelt out in the kernels, because as functions they changed the compiler's instruction schedule: the
// vectorised-or-masked store of K in the three forward kernels, and the decode of blockIdx.x into row block and split
// with the split's column-tile range in the four backward kernels.)  Each is the text that those kernels
// spelt out before, so the float64 summation orders -- and with them the bit-reproducibility that the kernels' file
// heads promise -- are in one place.  Geometry: gp_kernel_plan.h.
#pragma once
#include "common.h"
#include "gp_kernel_plan.h"

namespace pa {

template <typename T>
struct alignas(4 * sizeof(T)) Vec4 {
  T v[4];
};

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

// ---- 1 / lengthscale [D] in float64, and r2 of a thread's entries (the kernels of the stationary families) --------------
template <typename T>
__device__ __forceinline__ void gp_inverse_lengthscale(const T* __restrict__ ls, int n_ls, int D, double* inv_l) {
  for (int k = threadIdx.x; k < D; k += GPK_THREADS) inv_l[k] = 1.0 / (double)ls[n_ls == 1 ? 0 : k];
}

// r2 of the thread's 4 x 4 entries, in float64 for both dtypes: the difference, its scaling by 1 / l and the sum over
// the features.  f(r2) = exp(-r2 / 2) magnifies a relative error of r2 by r2 / 2: in float32 the two roundings of
// d = (x - z) / l and a sequential sum of 64 squares are 3e-5 relative in f at r2 = 130, as much as or more than the
// float32 restatement on the CPU carries.  The float32 inputs are exact in float64, so r2 is that of the inputs
// as given, to float64 rounding, and stays in float64 up to the exponential (gp_exp_of).
template <typename T>
__device__ __forceinline__ void gp_r2_tile(const T* xs, const T* zs, const double* inv_l, int D, int stride, int ty,
                                           int tx, double (&acc)[4][4]) {
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[r][c] = 0.0;
  for (int k = 0; k < D; ++k) {
    const double il = inv_l[k];
    double xv[4], zv[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) xv[r] = (double)xs[(4 * ty + r) * stride + k];
#pragma unroll
    for (int c = 0; c < 4; ++c) zv[c] = (double)zs[(4 * tx + c) * stride + k];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const double d = (xv[r] - zv[c]) * il;
        acc[r][c] = fma(d, d, acc[r][c]);
      }
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

// ---- the float64 accumulators in LDS, one writer per entry ------------------------------------------------------------
// a thread's sum p over its 4 columns of one row and feature: the 16 lanes of the row add theirs on DPP and lane
// tx = 0, the only writer of that row, adds the result to acc[entry] of the row accumulator
template <typename T>
__device__ __forceinline__ void gp_row_add(T p, double* acc, int entry, int tx) {
  const T total = gp_row16_sum(p);
  if (tx == 0) acc[entry] += (double)total;
}
// the same with the sum scaled first (gp_compose.hip: the scale differs from factor to factor)
template <typename T>
__device__ __forceinline__ void gp_row_add(T p, double scale, double* acc, int entry, int tx) {
  const T total = gp_row16_sum(p);
  if (tx == 0) acc[entry] += scale * (double)total;
}
// the wave's sum of q to acc[entry], an entry of the wave's own
template <typename T>
__device__ __forceinline__ void gp_wave_add(T q, double* acc, int entry, int lane) {
  const T total = wave_sum(q);
  if (lane == 0) acc[entry] += (double)total;
}
// entry k of the four waves' accumulators a [4, step], in the fixed order (a0 + a1) + (a2 + a3)
__device__ __forceinline__ double gp_fold_waves(const double* a, int k, int step) {
  return (a[k] + a[step + k]) + (a[2 * step + k] + a[3 * step + k]);
}

// ---- records ------------------------------------------------------------------------------------------------------------
// the row block's accumulator [64, width] to slot ``split`` of the row records [splits, R, width]
__device__ __forceinline__ void gp_copy_row_record(const double* acc, double* row_rec, int split, int64_t R, int64_t i0,
                                                   int width) {
  const int64_t rows_here = R - i0 < GPK_TILE ? R - i0 : GPK_TILE;
  double* rec = row_rec + ((int64_t)split * R + i0) * width;
  for (int64_t e = threadIdx.x; e < rows_here * width; e += GPK_THREADS) rec[e] = acc[e];
}
// the finalize's sum over the splits for entry e of the ``total`` entries of a row record, in split order
__device__ __forceinline__ double gp_sum_splits(const double* row_rec, int splits, int64_t total, int64_t e) {
  double s = 0.0;
  for (int sp = 0; sp < splits; ++sp) s += row_rec[(int64_t)sp * total + e];
  return s;
}

}  // namespace pa
