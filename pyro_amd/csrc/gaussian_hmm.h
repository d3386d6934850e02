// gaussian_hmm.h -- what the Kalman filter / smoother kernel (gaussian_hmm.hip) and the backward-sampling kernels
// (gaussian_hmm_sample.hip) share: the dimension limits (larger dimensions return PA_ERR_UNSUPPORTED; the Python class
// then takes its torch route), the wave-wide Cholesky and triangular solves on LDS matrices of row stride MD + 1, the
// model's arguments (GhModel) and the Kalman filter itself (GhFilter).
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

// The model as both entry points receive it: nine arrays, their batch (_sb) and step (_ss) strides in elements (a
// step stride of 0: the parameter is time-homogeneous), the number of steps and the two dimensions.
struct GhModel {
  const void *m0, *P0, *F, *q, *Q, *H, *r, *R, *x;
  int64_t m0_sb, P0_sb, F_sb, F_ss, q_sb, q_ss, Q_sb, Q_ss, H_sb, H_ss, r_sb, r_ss, R_sb, R_ss;
  int T, h, o;
};

// The Kalman filter of one series, run by one wave: the state both kernels keep and the one forward step they share.
// Per step (row vectors):  m^p = m F + q,  P^p = sym(F^T P F + Q),  y = x - m^p H - r,  S = H^T P^p H + R = L L^T,
//     U = P^p H L^-T,  v = L^-1 y,  m = m^p + U v,  P = P^p - U U^T.
// Symmetry: P^p is SYMMETRISED ((A + A^T) / 2 after the two products, F^T P first, then (F^T P) F) and the update
// subtracts U U^T, which is symmetric by construction; there is no Joseph form.  A non-positive (or NaN) pivot of S
// sets ``bad`` and the step goes on with finite numbers; what a marked series returns is the kernel's business.
//
// LDS: ten matrices of MD * (MD + 1) elements at ``mats``, six vectors of MD at ``vecs`` and the scalar slot ``sc``;
// a lane owns MD^2 / 64 elements of every matrix (lhh / lho / loo: their LDS offsets in an [h, h], [h, o] and [o, o]
// matrix, -1: none).  One step's inputs wait in registers: loaded a step ahead, written to LDS at the top of their
// step.  The backward sweeps of the kernels reuse the tables, the base pointers, the registers and ``predict``.
template <typename T, int MD>
struct GhFilter {
  static constexpr int LD = MD + 1, MS = MD * LD, EPL = MD * MD / 64;
  const GhModel& a;
  const int lane, h, o;
  T* const sP;                 // filtered covariance P_t (backward: P_{t-1})
  T *const sF, *const sQ, *const sH, *const sR;
  T* const sPp;                // predicted covariance
  T* const sL;                 // Cholesky factors
  T* const sA;                 // F^T P
  T* const sB;                 // P^p H -> U
  T* const sC;
  T* const vm;                 // filtered mean
  T *const vq, *const vr, *const vx;
  T* const vmp;                // predicted mean
  T* const vy;                 // innovation -> L^-1 y
  T* const sc;                 // scalars
  int lhh[EPL], lho[EPL], loo[EPL];
  const T *m0b, *P0b, *Fb, *qb, *Qb, *Hb, *rb, *Rb, *xb;
  T pF[EPL], pQ[EPL], pH[EPL], pR[EPL], pP[EPL], pq = T(0), pr = T(0), px = T(0), pm = T(0);
  bool bad = false;

  __device__ __forceinline__ GhFilter(const GhModel& a_, T* mats, T* vecs, T* sc_, int lane_, int64_t b)
      : a(a_), lane(lane_), h(a_.h), o(a_.o),
        sP(mats), sF(mats + MS), sQ(mats + 2 * MS), sH(mats + 3 * MS), sR(mats + 4 * MS), sPp(mats + 5 * MS),
        sL(mats + 6 * MS), sA(mats + 7 * MS), sB(mats + 8 * MS), sC(mats + 9 * MS),
        vm(vecs), vq(vecs + MD), vr(vecs + 2 * MD), vx(vecs + 3 * MD), vmp(vecs + 4 * MD), vy(vecs + 5 * MD), sc(sc_),
        m0b((const T*)a_.m0 + b * a_.m0_sb), P0b((const T*)a_.P0 + b * a_.P0_sb), Fb((const T*)a_.F + b * a_.F_sb),
        qb((const T*)a_.q + b * a_.q_sb), Qb((const T*)a_.Q + b * a_.Q_sb), Hb((const T*)a_.H + b * a_.H_sb),
        rb((const T*)a_.r + b * a_.r_sb), Rb((const T*)a_.R + b * a_.R_sb),
        xb((const T*)a_.x + b * (int64_t)a_.T * a_.o) {
    const int hh = h * h, ho = h * o, oo = o * o;
#pragma unroll
    for (int k = 0; k < EPL; ++k) {
      const int e = lane + 64 * k;
      lhh[k] = e < hh ? (e / h) * LD + e % h : -1;
      lho[k] = e < ho ? (e / o) * LD + e % o : -1;
      loo[k] = e < oo ? (e / o) * LD + e % o : -1;
      pF[k] = pQ[k] = pH[k] = pR[k] = pP[k] = T(0);
    }
  }

  // (``obs``: the observation side and the data too; a sweep that reads F, q, Q only passes false)
  __device__ __forceinline__ void load_params(int t, bool first, bool obs) {
    if (first || a.F_ss) {
      const T* p = Fb + (int64_t)t * a.F_ss;
#pragma unroll
      for (int k = 0; k < EPL; ++k)
        if (lhh[k] >= 0) pF[k] = p[lane + 64 * k];
    }
    if (first || a.Q_ss) {
      const T* p = Qb + (int64_t)t * a.Q_ss;
#pragma unroll
      for (int k = 0; k < EPL; ++k)
        if (lhh[k] >= 0) pQ[k] = p[lane + 64 * k];
    }
    if ((first || a.q_ss) && lane < h) pq = qb[(int64_t)t * a.q_ss + lane];
    if (!obs) return;
    if (first || a.H_ss) {
      const T* p = Hb + (int64_t)t * a.H_ss;
#pragma unroll
      for (int k = 0; k < EPL; ++k)
        if (lho[k] >= 0) pH[k] = p[lane + 64 * k];
    }
    if (first || a.R_ss) {
      const T* p = Rb + (int64_t)t * a.R_ss;
#pragma unroll
      for (int k = 0; k < EPL; ++k)
        if (loo[k] >= 0) pR[k] = p[lane + 64 * k];
    }
    if ((first || a.r_ss) && lane < o) pr = rb[(int64_t)t * a.r_ss + lane];
    if (lane < o) px = xb[(int64_t)t * o + lane];
  }
  __device__ __forceinline__ void commit_params(bool first, bool obs) {
#pragma unroll
    for (int k = 0; k < EPL; ++k) {
      if ((first || a.F_ss) && lhh[k] >= 0) sF[lhh[k]] = pF[k];
      if ((first || a.Q_ss) && lhh[k] >= 0) sQ[lhh[k]] = pQ[k];
      if (obs && (first || a.H_ss) && lho[k] >= 0) sH[lho[k]] = pH[k];
      if (obs && (first || a.R_ss) && loo[k] >= 0) sR[loo[k]] = pR[k];
    }
    if ((first || a.q_ss) && lane < h) vq[lane] = pq;
    if (obs && (first || a.r_ss) && lane < o) vr[lane] = pr;
    if (obs && lane < o) vx[lane] = px;
  }
  // predicted moments from (vm, sP) and the step's parameters: vmp, sPp (symmetrised); leaves F^T P in sA and a
  // copy of sPp in ``copy`` when given.  Ends with a barrier.
  __device__ __forceinline__ void predict(T* copy) {
    if (lane < h) {
      T s = vq[lane];
      for (int i = 0; i < h; ++i) s += vm[i] * sF[i * LD + lane];
      vmp[lane] = s;
    }
#pragma unroll
    for (int k = 0; k < EPL; ++k)
      if (lhh[k] >= 0) {
        const int j = lhh[k] / LD, c = lhh[k] % LD;
        T s = T(0);
        for (int i = 0; i < h; ++i) s += sF[i * LD + j] * sP[i * LD + c];
        sA[lhh[k]] = s;
      }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < EPL; ++k)
      if (lhh[k] >= 0) {
        const int j = lhh[k] / LD, c = lhh[k] % LD;
        T s = sQ[lhh[k]];
        for (int i = 0; i < h; ++i) s += sA[j * LD + i] * sF[i * LD + c];
        sC[lhh[k]] = s;
      }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < EPL; ++k)
      if (lhh[k] >= 0) {
        const int j = lhh[k] / LD, c = lhh[k] % LD;
        const T s = T(0.5) * (sC[j * LD + c] + sC[c * LD + j]);
        sPp[lhh[k]] = s;
        if (copy) copy[lhh[k]] = s;
      }
    __syncthreads();
  }

  // (m0, P0) into (vm, sP), step 0's inputs into the registers
  __device__ __forceinline__ void start() {
#pragma unroll
    for (int k = 0; k < EPL; ++k)
      if (lhh[k] >= 0) sP[lhh[k]] = P0b[lane + 64 * k];
    if (lane < h) vm[lane] = m0b[lane];
    load_params(0, true, true);
  }

  // Step t (0-based) of the filter: (vm, sP) <- (m_t, P_t), stored to ``w`` as well (h, then h^2 elements) when it
  // is not null.  Returns sum log diag L and leaves |v|^2 in sc[0], which the next step does not write before its
  // Cholesky.  Begins with a barrier and ends without one.
  __device__ __forceinline__ T step(int t, T* w) {
    __syncthreads();
    commit_params(t == 0, true);
    if (t + 1 < a.T) load_params(t + 1, false, true);
    __syncthreads();
    predict(nullptr);
    if (lane < o) {                                             // innovation
      T s = vx[lane] - vr[lane];
      for (int j = 0; j < h; ++j) s -= vmp[j] * sH[j * LD + lane];
      vy[lane] = s;
    }
#pragma unroll
    for (int k = 0; k < EPL; ++k)                               // sB = P^p H
      if (lho[k] >= 0) {
        const int j = lho[k] / LD, c = lho[k] % LD;
        T s = T(0);
        for (int i = 0; i < h; ++i) s += sPp[j * LD + i] * sH[i * LD + c];
        sB[lho[k]] = s;
      }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < EPL; ++k)                               // S = H^T P^p H + R
      if (loo[k] >= 0) {
        const int r_ = loo[k] / LD, c = loo[k] % LD;
        T s = sR[loo[k]];
        for (int j = 0; j < h; ++j) s += sH[j * LD + r_] * sB[j * LD + c];
        sL[loo[k]] = s;
      }
    __syncthreads();
    const T logdet = gh_cholesky<T, MD>(sL, o, lane, bad);
    if (lane < h) gh_forward_sub<T, LD>(sL, sB + lane * LD, 1, o);          // row j of U = P^p H L^-T
    if (lane == h) sc[0] = gh_forward_sub<T, LD>(sL, vy, 1, o);             // v = L^-1 y, |v|^2
    __syncthreads();
    T nm = T(0);
    if (lane < h) {
      nm = vmp[lane];
      for (int c = 0; c < o; ++c) nm += sB[lane * LD + c] * vy[c];
    }
    T nP[EPL];
#pragma unroll
    for (int k = 0; k < EPL; ++k) {
      nP[k] = T(0);
      if (lhh[k] >= 0) {
        const int j = lhh[k] / LD, c = lhh[k] % LD;
        T s = sPp[lhh[k]];
        for (int i = 0; i < o; ++i) s -= sB[j * LD + i] * sB[c * LD + i];
        nP[k] = s;
      }
    }
    // (vm and sP are read by this phase only through vmp / sPp: no barrier before they are overwritten)
    if (lane < h) vm[lane] = nm;
#pragma unroll
    for (int k = 0; k < EPL; ++k)
      if (lhh[k] >= 0) sP[lhh[k]] = nP[k];
    if (w) {
      if (lane < h) w[lane] = nm;
#pragma unroll
      for (int k = 0; k < EPL; ++k)
        if (lhh[k] >= 0) w[h + lane + 64 * k] = nP[k];
    }
    return logdet;
  }
};

}  // namespace pa
