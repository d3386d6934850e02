// mixture_assign.h -- the NaN-carrying max / min and the per-row Philox uniform of the assignment kernels: shared by
// mixture_assign.hip and mixture_assign_wide.hip.
#pragma once
#include "common.h"
#include "dist_fam.h"

namespace pa {

// max that hands on a NaN whichever side it is on (both lanes of a butterfly step agree)
template <typename T> __device__ __forceinline__ T mixa_max(T a, T b) { return (a > b || a != a) ? a : b; }
template <typename T> __device__ __forceinline__ T mixa_min(T a, T b) { return a < b ? a : b; }

__device__ __forceinline__ float mixa_uniform(float, uint64_t seed, uint64_t offset, uint64_t i) {
  const u32x4 b = philox4x32_10(seed, offset + (i >> 2), 0);
  const uint32_t l = (uint32_t)(i & 3);
  return u32_to_unit_f32(l == 0 ? b.x : l == 1 ? b.y : l == 2 ? b.z : b.w);
}
__device__ __forceinline__ double mixa_uniform(double, uint64_t seed, uint64_t offset, uint64_t i) {
  const u32x4 b = philox4x32_10(seed, offset + (i >> 1), 0);
  return (i & 1) ? u32x2_to_unit_f64(b.z, b.w) : u32x2_to_unit_f64(b.x, b.y);
}

}  // namespace pa
