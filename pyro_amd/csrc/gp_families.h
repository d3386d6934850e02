// gp_families.h -- the five stationary families (and the cosine, which gp_wrap.hip alone dispatches) as device
// evaluators, the ONE copy that every Gaussian-process kernel evaluates (gp_kernel.hip, gp_wrap.hip, gp_compose.hip,
// gp_sgpr.hip, gp_cond.hip): f(r2) and f'(r2) = df / d(r2), the reference's
// guard r = sqrt(r2 + 1e-12) inside, the exponential of a float64 argument (gp_exp_of, which gp_periodic.hip takes as
// well) and the switch over the family.  The guard and the hi / lo exponential are numerics that the tests' bounds were
// derived with: they live here and nowhere else.  Stands on common.h alone, no tile geometry.
#pragma once
#include "common.h"

namespace pa {

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

// sin(a) and cos(a) for an argument held in float64.  In float32 the argument is split as in gp_exp_of,
// cos(hi + lo) = cos(hi) - lo sin(hi): rounding a = r to float32 alone would cost r 2^-24 ABSOLUTE in cos(r).
template <typename T>
__device__ __forceinline__ void gp_sincos_of(double a, T& s, T& c) {
  if constexpr (sizeof(T) == 8) {
    s = sin(a), c = cos(a);
  } else {
    const float hi = (float)a, lo = (float)(a - (double)hi);
    const float sh = sinf(hi), ch = cosf(hi);
    s = fmaf(lo, ch, sh), c = fmaf(-lo, sh, ch);
  }
}
// cos(r), PA_GP_COSINE: dispatched by gp_wrap.hip alone (GP_FAMILY_DISPATCH below is the five families of the others)
template <typename T>
struct GpCosine {
  __device__ __forceinline__ static void eval(double r2, T, T& f, T& df, T& da) {
    const double r = sqrt(r2 + 1e-12);
    T s;
    gp_sincos_of<T>(r, s, f);
    df = T(-0.5) * s / (T)r;
    da = T(0);
  }
};

// CALL<T, family>(...) under the switch over ``family`` (PA_GP_RBF .. PA_GP_MATERN52, checked by the caller)
#define GP_FAMILY_DISPATCH(CALL, ...)                                                 \
  switch (family) {                                                                   \
    case PA_GP_RBF: return CALL<T, GpRbf>(__VA_ARGS__);                               \
    case PA_GP_RATIONAL_QUADRATIC: return CALL<T, GpRq>(__VA_ARGS__);                 \
    case PA_GP_EXPONENTIAL: return CALL<T, GpExponential>(__VA_ARGS__);               \
    case PA_GP_MATERN32: return CALL<T, GpMatern32>(__VA_ARGS__);                     \
    default: return CALL<T, GpMatern52>(__VA_ARGS__);                                 \
  }

}  // namespace pa
