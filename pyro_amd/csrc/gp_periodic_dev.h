// gp_periodic_dev.h -- the sines of the periodic covariance, shared by the leaf kernel (gp_periodic.hip) and the
// composite kernel (gp_compose.hip).
#pragma once
#include "gp_tile.h"

namespace pa {

// sin(pi t) of the reduced argument for the EXPONENT, in float64.  exp magnifies a relative error of s^2 by the exponent
// itself: sinpif's one or two float32 units per feature are 50 * 2^-23 in K at an exponent of 50, over the float32
// bound of the reduced gradients where every K is that small (D = 64).  So the float32 kernels take t * P(t^2) in
// float64, P the Chebyshev interpolant of sin(pi t) / t of degree 5 on t^2 in [0, 1/4] (relative error 2.7e-11, the
// zero at t = 0 exact): seven float64 instructions, no more than sinpif's float32 ones at the same issue rate.
template <typename T>
__device__ __forceinline__ double gpp_sinpi_reduced(double t) {
  if constexpr (sizeof(T) == 8) {
    return sinpi(t);
  } else {
    const double w = t * t;
    double p = -0.007028303652380903;
    p = fma(p, w, 0.08205035003144681);
    p = fma(p, w, -0.5992521864819006);
    p = fma(p, w, 2.5501633179323684);
    p = fma(p, w, -5.167712764592721);
    p = fma(p, w, 3.141592653536129);
    return t * p;
  }
}
template <typename T>
__device__ __forceinline__ void gpp_sincospi(T t, T& s, T& c) {
  if constexpr (sizeof(T) == 4) sincospif(t, &s, &c);
  else sincospi(t, &s, &c);
}

}  // namespace pa
