// time_transform.hip -- the four orthonormal transforms along the time axis that a time reparameteriser runs in every
// evaluation of a model, ONE launch each on the caller's stream: the type-II DCT and its inverse, the Haar wavelet
// transform (the layout of the reference's recursion) and its inverse, over x [outer, N, inner] contiguous -> y of
// the same shape.  The transforms are orthonormal, so the adjoint of each is its inverse: the same four kernels are
// the backward passes.
//
// Reference path replaced: pyro/ops/tensor_utils.py dct / idct (about fifteen torch operators around an rfft each) and
// haar_transform / inverse_haar_transform (a Python recursion of log2 N rounds of slicing, stack and cat), doubled
// by autograd.
//
// Columns.  The outer * inner series are numbered col = o * inner + i; a workgroup of 256 threads takes a strip of W
// adjacent ones (W = 4; 2 for f64 with N > 1024), so a small inner packs several outer indices into one strip.
// Element n of series col sits at (o * N + n) * inner + i; the W bases are worked out once, by W threads, into LDS.
//
// DCT / IDCT: direct sums, y_k = s_k sum_n x_n cos(pi (2n + 1) k / 2N) and x_n = sum_k s_k X_k cos(same), with
// s_0 = sqrt(1/N), s_k = sqrt(2/N).  The strip [N, W] is staged in LDS beside a QUARTER-WAVE table
// tab[j] = cos(pi j / 2N), j = 0..N (rounded once from float64 cospi; tab[N] = 0).  A thread owns one output index
// and all W columns of the strip in registers; the table index ((2n + 1) k) mod 4N is stepped by integer addition
// (start k, step 2k for the DCT; start 0, step 2n + 1 for the IDCT) and folded onto the quarter wave by two
// comparisons and a sign, so no cosine of a large argument and no [N, N] matrix exists anywhere.  Every thread of a
// wave reads the same x[n, 0..W) (an LDS broadcast) and its own table entry.  Accumulation is fma in the tensor's
// dtype into TT_CHAINS interleaved partial sums (terms n = u mod 8, each with its own index chain, so that eight
// table reads are in flight instead of one: a single chain ran at the latency of its read, 49 ns per term), added
// in a fixed order; the scale is applied once to the sum (the IDCT stages X_0 / sqrt 2 and scales by sqrt(2/N)).
// The O(N^2) work of a strip is split over gridDim.y = ceil(N / 256) workgroups, each of which stages the strip.
//
// Haar: level l pairs the current low band (length len): lo = (even + odd) / sqrt 2 goes to an LDS buffer, hi =
// (even - odd) / sqrt 2 and the tail of an odd length are FINAL and go straight to y at [n, 2n) and 2n; level 0 reads
// x from global memory, so the forward transform keeps only the low bands in LDS: two ping-pong buffers of N/2 and
// N/4 rows, one barrier per level, ceil(log2 N) levels.  The inverse stages X [N, W] in LDS, runs the levels from the
// deepest up through the same two buffers (lo from the level below, hi and the tail from the staged X) and writes the
// last level to y.
//
// One launch, no atomics, no workspace: bit-reproducible.  A NaN stays inside its own column.
//
// gfx950 cross-compile (hipcc -O3, -Rpass-analysis=kernel-resource-usage); LDS is dynamic, the bytes are those of
// N = 2048 (f64 W = 4: N = 1024) plus 8 W for the strip's bases; no scratch, no AGPRs; waves / SIMD by registers: 8 for
// the Haar kernels, 7 / 4 / 7 for the DCT ones (a workgroup is 4 waves, one per SIMD, and LDS admits 3 workgroups per CU):
//     instantiation <T, W>     dct / idct: VGPRs  SGPRs  LDS bytes     haar / inverse: VGPRs  SGPRs  LDS bytes
//     <float , 4>              67 / 67            32 / 31  40996         28 / 22                34 / 31  24640 / 57408
//     <double, 4>              103 / 103          32 / 31  41000         32 / 24                36 / 33  24672 / 57440
//     <double, 2>              69 / 68            32 / 31  49176         32 / 24                36 / 33  24624 / 57392
#include "common.h"

namespace pa {

constexpr int TT_MAX_STEPS = 2048;
constexpr int TT_THREADS = 256;
constexpr int TT_WIDE_F64 = 1024;            // f64 and N over this: strips of 2 columns, else 4
constexpr int TT_CHAINS = 8;                 // interleaved partial sums of a DCT output

struct TtArgs {
  const void* x;
  void* y;
  int64_t cols, inner;                       // cols = outer * inner
  int n;
  double s0, s1;                             // DCT: the scales of k = 0 and k > 0; IDCT: sqrt(1/2) and sqrt(2/N)
};

// the W series of a strip: base[c] = offset of element 0 of series col0 + c, or -1 past the last series
template <int W>
__device__ __forceinline__ void tt_bases(const TtArgs& a, int64_t* base) {
  const int tid = threadIdx.x;
  if (tid < W) {
    const int64_t col = (int64_t)blockIdx.x * W + tid;
    int64_t b = -1;
    if (col < a.cols) {
      const int64_t o = col / a.inner, i = col - o * a.inner;
      b = o * a.n * a.inner + i;
    }
    base[tid] = b;
  }
  __syncthreads();
}

template <typename T, int W, bool INV>
__global__ __launch_bounds__(TT_THREADS) void tt_dct_kernel(const TtArgs a) {
  static_assert(TT_THREADS % W == 0, "a thread stages one column of the strip");
  extern __shared__ __attribute__((aligned(16))) unsigned char tt_lds[];
  __shared__ int64_t base[W];
  const int N = a.n, tid = threadIdx.x;
  T* tile = reinterpret_cast<T*>(tt_lds);    // [N][W]
  T* tab = tile + (size_t)N * W;             // [N + 1]
  const T* x = (const T*)a.x;
  T* y = (T*)a.y;
  tt_bases<W>(a, base);

  {
    const int c = tid % W;
    const int64_t b = base[c];
    for (int n = tid / W; n < N; n += TT_THREADS / W) {
      T v = T(0);
      if (b >= 0) v = x[b + (int64_t)n * a.inner];
      if (INV && n == 0) v *= (T)a.s0;
      tile[n * W + c] = v;
    }
    const double step = 1.0 / (2.0 * (double)N);
    for (int j = tid; j <= N; j += TT_THREADS) tab[j] = j == N ? T(0) : (T)cospi((double)j * step);
  }
  __syncthreads();

  const int k = blockIdx.y * TT_THREADS + tid;          // the output index: a frequency (DCT) or a step (IDCT)
  if (k >= N) return;
  const int twoN = 2 * N, fourN = 4 * N;
  const int step = INV ? 2 * k + 1 : 2 * k;
  // U interleaved partial sums (terms n = u mod U), each with its own index chain stepped by U * step: one chain is
  // bound by the latency of its table read (measured: 49 ns per term), U of them keep U reads in flight
  constexpr int U = TT_CHAINS;
  const int stepU = (U * step) % fourN;
  int idx[U];
  T acc[U][W];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    idx[u] = ((INV ? 0 : k) + u * step) % fourN;
#pragma unroll
    for (int c = 0; c < W; ++c) acc[u][c] = T(0);
  }
  auto term = [&](int n, int u) {
    int j = idx[u] > twoN ? fourN - idx[u] : idx[u];     // cos(2 pi - t) = cos t
    const bool neg = j > N;                              // cos(pi - t) = -cos t
    j = neg ? twoN - j : j;
    const T t = tab[j];
    const T cv = neg ? -t : t;
#pragma unroll
    for (int c = 0; c < W; ++c) acc[u][c] = fma(tile[n * W + c], cv, acc[u][c]);
    idx[u] += stepU;
    idx[u] = idx[u] >= fourN ? idx[u] - fourN : idx[u];
  };
  int n0 = 0;
  for (; n0 + U <= N; n0 += U) {
#pragma unroll
    for (int u = 0; u < U; ++u) term(n0 + u, u);
  }
#pragma unroll
  for (int u = 0; u < U - 1; ++u)
    if (n0 + u < N) term(n0 + u, u);
  const T scale = (INV || k > 0) ? (T)a.s1 : (T)a.s0;
#pragma unroll
  for (int c = 0; c < W; ++c) {
    T sum = acc[0][c];
#pragma unroll
    for (int u = 1; u < U; ++u) sum += acc[u][c];        // (a fixed order: bit-reproducible)
    const int64_t b = base[c];
    if (b >= 0) y[b + (int64_t)k * a.inner] = sum * scale;
  }
}

template <typename T, int W, bool INV>
__global__ __launch_bounds__(TT_THREADS) void tt_haar_kernel(const TtArgs a) {
  static_assert(TT_THREADS % W == 0, "a thread keeps to one column of the strip");
  extern __shared__ __attribute__((aligned(16))) unsigned char tt_lds[];
  __shared__ int64_t base[W];
  const int N = a.n, tid = threadIdx.x;
  const int c = tid % W, p0 = tid / W;
  constexpr int PS = TT_THREADS / W;
  T* bufA = reinterpret_cast<T*>(tt_lds);    // [N / 2 + 1][W]: the low band of the odd levels
  T* bufB = bufA + (size_t)(N / 2 + 1) * W;  // [N / 4 + 1][W]: of the even ones
  const T* x = (const T*)a.x;
  T* y = (T*)a.y;
  const T r = (T)0.70710678118654752440;
  tt_bases<W>(a, base);
  const int64_t b = base[c], inner = a.inner;
  const bool live = b >= 0;

  if constexpr (!INV) {
    int len = N;
    for (int level = 0;; ++level) {
      const int n = len >> 1;
      const T* src = (level & 1) ? bufA : bufB;          // (level 0 reads x)
      T* dst = (level & 1) ? bufB : bufA;
      for (int p = p0; p < n; p += PS) {
        T e = T(0), o = T(0);
        if (level == 0) {
          if (live) {
            e = x[b + (int64_t)(2 * p) * inner];
            o = x[b + (int64_t)(2 * p + 1) * inner];
          }
        } else {
          e = src[(2 * p) * W + c];
          o = src[(2 * p + 1) * W + c];
        }
        const T hi = (e - o) * r, lo = (e + o) * r;
        if (live) y[b + (int64_t)(n + p) * inner] = hi;
        if (n >= 2) dst[p * W + c] = lo;
        else if (live) y[b + (int64_t)p * inner] = lo;
      }
      if ((len & 1) && p0 == 0 && live)                  // the tail of an odd length stays where it is
        y[b + (int64_t)(2 * n) * inner] = level == 0 ? x[b + (int64_t)(2 * n) * inner] : src[(2 * n) * W + c];
      if (n < 2) break;
      __syncthreads();
      len = n;
    }
  } else {
    T* tile = bufB + (size_t)(N / 4 + 1) * W;            // [N][W]: the coefficients
    for (int n = p0; n < N; n += PS) tile[n * W + c] = live ? x[b + (int64_t)n * inner] : T(0);
    int deepest = 0;
    while (((N >> deepest) >> 1) >= 2) ++deepest;
    __syncthreads();
    for (int level = deepest; level >= 0; --level) {
      const int len = N >> level, n = len >> 1;
      const T* lo_src = level == deepest ? tile : ((level & 1) ? bufB : bufA);      // (the buffer of level + 1)
      T* dst = (level & 1) ? bufA : bufB;                                            // (level 0 writes y)
      for (int p = p0; p < n; p += PS) {
        const T lo = lo_src[p * W + c], hi = tile[(n + p) * W + c];
        const T e = (lo + hi) * r, o = (lo - hi) * r;
        if (level == 0) {
          if (live) {
            y[b + (int64_t)(2 * p) * inner] = e;
            y[b + (int64_t)(2 * p + 1) * inner] = o;
          }
        } else {
          dst[(2 * p) * W + c] = e;
          dst[(2 * p + 1) * W + c] = o;
        }
      }
      if ((len & 1) && p0 == 0) {
        const T end = tile[(2 * n) * W + c];
        if (level == 0) {
          if (live) y[b + (int64_t)(2 * n) * inner] = end;
        } else {
          dst[(2 * n) * W + c] = end;
        }
      }
      if (level > 0) __syncthreads();
    }
  }
}

}  // namespace pa

extern "C" {

int pa_time_transform(int dtype, int op, const void* x, void* y, int64_t outer, int64_t n, int64_t inner,
                      pa_stream_t stream) {
  PA_REQUIRE(dtype == PA_F32 || dtype == PA_F64, "time_transform: bad dtype %d", dtype);
  PA_REQUIRE(op >= 0 && op <= 3, "time_transform: bad op %d (0 dct, 1 idct, 2 haar, 3 inverse haar)", op);
  PA_REQUIRE(outer >= 0 && n >= 0 && inner >= 0, "time_transform: bad shape [%lld, %lld, %lld]", (long long)outer,
             (long long)n, (long long)inner);
  if (n > pa::TT_MAX_STEPS)
    return pa::fail(PA_ERR_UNSUPPORTED, "time_transform: N=%lld over the limit of %d", (long long)n,
                    pa::TT_MAX_STEPS);
  if (outer == 0 || n == 0 || inner == 0) return PA_OK;
  PA_REQUIRE(outer <= (int64_t(1) << 31) && inner <= (int64_t(1) << 31) && outer * inner <= (int64_t(1) << 31),
             "time_transform: shape too large");
  PA_REQUIRE(x && y && x != y, "time_transform: x and y distinct and not NULL");
  const int N = (int)n;
  const size_t es = dtype == PA_F32 ? 4 : 8;
  const int W = (dtype == PA_F64 && N > pa::TT_WIDE_F64) ? 2 : 4;
  const int64_t cols = outer * inner;
  const bool inv = op == 1 || op == 3, haar = op >= 2;
  pa::TtArgs a{x, y, cols, inner, N, 0.0, 0.0};
  if (op == 0) {
    a.s0 = sqrt(1.0 / (double)N);
    a.s1 = sqrt(2.0 / (double)N);
  } else if (op == 1) {
    a.s0 = sqrt(0.5);
    a.s1 = sqrt(2.0 / (double)N);
  }
  size_t lds;
  if (!haar) lds = ((size_t)N * W + N + 1) * es;
  else lds = ((size_t)(N / 2 + 1) * W + (size_t)(N / 4 + 1) * W + (inv ? (size_t)N * W : 0)) * es;
  PA_REQUIRE(lds <= 65536, "time_transform: %zu bytes of LDS", lds);
  const dim3 grid((unsigned)((cols + W - 1) / W), haar ? 1u : (unsigned)((N + pa::TT_THREADS - 1) / pa::TT_THREADS));
  hipStream_t st = pa::as_stream(stream);
#define PA_TT_LAUNCH(K_, T_, W_, INV_) \
  hipLaunchKernelGGL((pa::K_<T_, W_, INV_>), grid, dim3(pa::TT_THREADS), lds, st, a)
#define PA_TT_PICK(K_, T_, W_) \
  do { if (inv) PA_TT_LAUNCH(K_, T_, W_, true); else PA_TT_LAUNCH(K_, T_, W_, false); } while (0)
  if (dtype == PA_F32) {
    if (haar) PA_TT_PICK(tt_haar_kernel, float, 4); else PA_TT_PICK(tt_dct_kernel, float, 4);
  } else if (W == 4) {
    if (haar) PA_TT_PICK(tt_haar_kernel, double, 4); else PA_TT_PICK(tt_dct_kernel, double, 4);
  } else {
    if (haar) PA_TT_PICK(tt_haar_kernel, double, 2); else PA_TT_PICK(tt_dct_kernel, double, 2);
  }
#undef PA_TT_PICK
#undef PA_TT_LAUNCH
  return pa::check_launch("time_transform_kernel");
}

}  // extern "C"
