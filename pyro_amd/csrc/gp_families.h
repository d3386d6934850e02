// gp_families.h -- the five stationary families as device evaluators, shared by the leaf kernel (gp_kernel.hip) and the
// composite kernel (gp_compose.hip): f(r2) and f'(r2) = df / d(r2), the reference's guard r = sqrt(r2 + 1e-12) inside.
#pragma once
#include "gp_tile.h"

namespace pa {

// ---- the families: f(r2) and f'(r2) = df / d(r2), the guard inside --------------------------------------------------
template <typename T>
__device__ __forceinline__ T gp_exp(T v) {
  if constexpr (sizeof(T) == 4) return expf(v);
  else return exp(v);
}
template <typename T>
__device__ __forceinline__ T gp_sqrt(T v) {
  if constexpr (sizeof(T) == 4) return sqrtf(v);
  else return sqrt(v);
}
template <typename T>
__device__ __forceinline__ T gp_log1p(T v) {
  if constexpr (sizeof(T) == 4) return log1pf(v);
  else return log1p(v);
}

// eval(r2 in float64, alpha) -> f, df = df / d(r2), da = df / d(alpha)
template <typename T>
struct GpRbf {
  __device__ __forceinline__ static void eval(double r2, T, T& f, T& df, T& da) {
    f = gp_exp_of<T>(-0.5 * r2);
    df = T(-0.5) * f;
    da = T(0);
  }
};
template <typename T>
struct GpRq {
  __device__ __forceinline__ static void eval(double r2d, T alpha, T& f, T& df, T& da) {
    const T u = (T)r2d / (T(2) * alpha), l1 = gp_log1p(u);
    f = gp_exp(-alpha * l1);
    df = T(-0.5) * f / (T(1) + u);
    da = f * (u / (T(1) + u) - l1);
  }
};
template <typename T>
struct GpExponential {
  __device__ __forceinline__ static void eval(double r2, T, T& f, T& df, T& da) {
    const double r = sqrt(r2 + 1e-12);
    f = gp_exp_of<T>(-r);
    df = T(-0.5) * f / (T)r;
    da = T(0);
  }
};
template <typename T>
struct GpMatern32 {
  __device__ __forceinline__ static void eval(double r2, T, T& f, T& df, T& da) {
    const double sr = 1.7320508075688772935 * sqrt(r2 + 1e-12);
    const T e = gp_exp_of<T>(-sr);
    f = (T(1) + (T)sr) * e;
    df = T(-1.5) * e;
    da = T(0);
  }
};
template <typename T>
struct GpMatern52 {
  __device__ __forceinline__ static void eval(double r2, T, T& f, T& df, T& da) {
    const double r = sqrt(r2 + 1e-12), sr = 2.2360679774997896964 * r;
    const T e = gp_exp_of<T>(-sr);
    f = (T(1) + (T)sr + T(5.0 / 3.0) * (T)r2) * e;
    df = e * (T(-5.0 / 6.0) - T(5.0 * 2.2360679774997896964 / 6.0) * (T)(r2 / r));
    da = T(0);
  }
};

}  // namespace pa
