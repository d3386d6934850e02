// gp_sparse_dev.h -- the device helpers that the streamed sparse-GP kernels share (gp_sgpr.hip, gp_cond.hip): a wave's
// 32 x 32 block in the register layout of v_mfma_f32_32x32x2_f32, its row map, the staging of rows into LDS and r2 of a
// pair of points.  The matrix primitives differ (gps_mac, gpc_mac) and stay in their files.  Geometry: gp_sgpr_plan.h.
#pragma once
#include "common.h"
#include "gp_sgpr_plan.h"

namespace pa {

// ---- the 32 x 32 block of one wave ----------------------------------------------------------------------------------
typedef float gps_f32x16 __attribute__((ext_vector_type(16)));
template <typename T>
struct GpsAcc;
template <>
struct GpsAcc<float> {
  gps_f32x16 c;
};
template <>
struct GpsAcc<double> {
  double c[16];
};
template <typename T>
__device__ __forceinline__ void gps_clear(GpsAcc<T>& a) {
#pragma unroll
  for (int v = 0; v < 16; ++v) a.c[v] = T(0);
}
// the row of the block that register v of lane ``lane`` holds (its column is lane % 32)
__device__ __forceinline__ int gps_row(int v, int lane) { return 8 * (v >> 2) + 4 * (lane >> 5) + (v & 3); }

// rows [first, first + rows) of p [n, D] into tile [rows, stride], zeros past the end
template <typename T>
__device__ __forceinline__ void gps_stage(const T* __restrict__ p, int64_t first, int64_t n, int rows, int D, int stride,
                                          T* tile) {
  for (int e = threadIdx.x; e < rows * D; e += GPS_THREADS) {
    const int row = e / D, k = e - row * D;
    const int64_t i = first + row;
    tile[row * stride + k] = i < n ? p[i * D + k] : T(0);
  }
}

// r2 of (u, x) in float64: the difference first, then 1 / l (gp_kernel.hip: gp_r2_tile)
template <typename T>
__device__ __forceinline__ double gps_r2(const T* u, const T* x, const double* inv_l, int D) {
  double s = 0.0;
  for (int k = 0; k < D; ++k) {
    const double d = ((double)u[k] - (double)x[k]) * inv_l[k];
    s = fma(d, d, s);
  }
  return s;
}

}  // namespace pa
