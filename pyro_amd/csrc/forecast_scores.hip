// forecast_scores.hip -- the three scores of a sample forecast in ONE pass over the samples: per column of
// pred [S, M] against truth [M], the sample mean, the lower median and the CRPS, in one launch on the caller's stream.
//
// Reference path replaced: pyro/ops/stats.py crps_empirical (a sort of [S, M] along the strided sample axis --
// values and int64 indices --, differences, weights, two reductions), pyro/contrib/forecast/evaluate.py eval_mae
// (a second selection for median(0)) and eval_rmse (a third pass for mean(0)).  Here pred is read exactly once.
//
// A workgroup takes a strip of C adjacent columns and stages all S samples of the strip in LDS (a row of the strip
// is C contiguous elements of pred), padded with +inf to NP, the next power of two.  Every column is sorted in place
// by a bitonic network.  A thread holds 2^nb elements (nb <= 3) of one column whose rows differ in nb adjacent bits
// and runs nb stages of the network on them in registers, so a merge of 2^L elements costs ceil(L / 3) trips
// through LDS instead of L: 22 instead of 55 at NP = 1024.  Adjacent lanes hold adjacent columns.  With C = 32 a
// group of 32 lanes reads one row of the strip: every bank once.  With C = 16 it reads two rows that differ in
// exactly one bit of the row number (the lane groups are aligned), and rows are laid out in pairs, the half of the
// 32-wide line picked by the parity of the row number: again every bank once (fs_addr).
//
// Read-out: NT / C threads per column sum |p_i - y|, p_i and (p_(i+1) - p_(i)) i (S - i) over interleaved rows in
// float64 (f32 samples too: the sums then carry one rounding each), the partial sums go through LDS (the tile's
// memory, which is dead by then) and one thread per column adds them in a fixed order:
//     mean   = sum p_i / S
//     median = p_((S - 1) / 2)                    (the lower median of torch's median(0).values)
//     crps   = sum |p_i - y| / S  -  sum_{i=1..S-1} (p_(i+1) - p_(i)) i (S - i) / S^2
// S = 1 gives |p - y|.  A NaN sample is noted while the strip is staged (a plain LDS store of 1 by whoever sees one);
// its column, and a column whose truth is NaN, is NaN in all three outputs, and no other.  +-inf samples follow IEEE
// through the formula above as they do through torch's.  No atomics, no workspace, bit-reproducible.
//
// Buckets (strip width per S so that the tile stays within the CU's 160 KiB of LDS and more than one workgroup fits
// where it can):
//     S <= 128 :  C = 32, 256 threads   (f32 16 KiB, f64 32 KiB)
//     S <= 1024:  C = 16, 512 threads   (f32 64 KiB: two workgroups per CU; f64 128 KiB: one)
//
// gfx950 cross-compile (hipcc -O3, -Rpass-analysis=kernel-resource-usage):
//     instantiation <T, C, NPMAX, NT>   VGPRs  AGPRs  SGPRs  scratch   LDS bytes   waves / SIMD   (workgroups / CU by LDS)
//     <float , 32,  128, 256>           35     0      57     0         16512       8              (8 by waves; LDS 9)
//     <float , 16, 1024, 512>           35     0      57     0         65600       4              (2)
//     <double, 32,  128, 256>           48     0      57     0         32896       4              (4)
//     <double, 16, 1024, 512>           136    0      57     0         131136      2              (1)
#include "common.h"

#include <limits>

namespace pa {

constexpr int FS_MAX_SAMPLES = 1024;
constexpr int FS_SMALL = 128;                // S <= FS_SMALL: the wide strip

struct FsArgs {
  const void *pred, *truth;                  // [S, M] contiguous, [M]
  void *mean, *median, *crps;                // [M] each
  int64_t M;
  int S, NP, LOGN;                           // NP = 2^LOGN >= S
};

// element (row, c) of the strip's tile
template <int C>
__device__ __forceinline__ int fs_addr(int row, int c) {
  if constexpr (C == 32) {
    return row * 32 + c;
  } else {
    static_assert(C == 16, "strip widths: 16 and 32");
    return (row >> 1) * 32 + ((__popc(row) & 1) << 4) + c;      // rows 2a, 2a + 1 share a line, halves by parity
  }
}

// NB stages of the merge into sorted runs of k elements, partner distances 2^(b + NB - 1) .. 2^b
template <typename T, int C, int NB, int NT>
__device__ __forceinline__ void fs_pass(T* tile, int NP, int k, int b, int tid) {
  constexpr int G = 1 << NB;
  const int items = (NP >> NB) * C;
  for (int item = tid; item < items; item += NT) {
    const int c = item % C, g = item / C;
    const int base = ((g >> b) << (b + NB)) | (g & ((1 << b) - 1));
    const bool up = (base & k) == 0;
    T v[G];
#pragma unroll
    for (int e = 0; e < G; ++e) v[e] = tile[fs_addr<C>(base | (e << b), c)];
#pragma unroll
    for (int t = NB - 1; t >= 0; --t) {
#pragma unroll
      for (int e = 0; e < G; ++e) {
        if (e & (1 << t)) continue;
        const T lo = v[e], hi = v[e | (1 << t)];
        const bool sw = hi < lo;
        const T mn = sw ? hi : lo, mx = sw ? lo : hi;
        v[e] = up ? mn : mx;
        v[e | (1 << t)] = up ? mx : mn;
      }
    }
#pragma unroll
    for (int e = 0; e < G; ++e) tile[fs_addr<C>(base | (e << b), c)] = v[e];
  }
}

template <typename T, int C, int NPMAX, int NT>
__global__ __launch_bounds__(NT) void forecast_scores_kernel(const FsArgs a) {
  constexpr int TPC = NT / C;                // threads per column in the read-out
  static_assert(NT % C == 0 && (size_t)NPMAX * C * sizeof(T) >= (size_t)3 * NT * sizeof(double), "tile holds the partials");
  __shared__ __attribute__((aligned(16))) unsigned char raw[(size_t)NPMAX * C * sizeof(T)];
  __shared__ int has_nan[C];
  T* tile = reinterpret_cast<T*>(raw);
  double* part = reinterpret_cast<double*>(raw);
  const int tid = threadIdx.x, S = a.S, NP = a.NP;
  const int64_t m0 = (int64_t)blockIdx.x * C, M = a.M;
  const T* pred = (const T*)a.pred;

  if (tid < C) has_nan[tid] = 0;
  __syncthreads();
  for (int item = tid; item < NP * C; item += NT) {
    const int c = item % C, s = item / C;
    T v = std::numeric_limits<T>::infinity();
    if (s < S && m0 + c < M) {
      v = pred[(int64_t)s * M + m0 + c];
      if (v != v) has_nan[c] = 1;
    }
    tile[fs_addr<C>(s, c)] = v;
  }
  __syncthreads();
  for (int L = 1; L <= a.LOGN; ++L) {
    const int k = 1 << L;
    for (int rem = L; rem > 0;) {
      const int nb = rem >= 3 ? 3 : rem, b = rem - nb;
      if (nb == 3) fs_pass<T, C, 3, NT>(tile, NP, k, b, tid);
      else if (nb == 2) fs_pass<T, C, 2, NT>(tile, NP, k, b, tid);
      else fs_pass<T, C, 1, NT>(tile, NP, k, b, tid);
      rem = b;
      __syncthreads();
    }
  }

  const int c = tid % C, q = tid / C;
  const int64_t m = m0 + c;
  const bool live = m < M;
  const T y = live ? ((const T*)a.truth)[m] : T(0);
  double sa = 0.0, sm = 0.0, sw = 0.0;
  for (int i = q; i < S; i += TPC) {
    const T p = tile[fs_addr<C>(i, c)];
    sa += (double)fabs(p - y);
    sm += (double)p;
    if (i + 1 < S) {
      const T d = tile[fs_addr<C>(i + 1, c)] - p;
      sw += (double)d * (double)((int64_t)(i + 1) * (S - 1 - i));
    }
  }
  const T med = tile[fs_addr<C>((S - 1) >> 1, c)];
  const bool bad = has_nan[c] != 0 || y != y;
  __syncthreads();                           // (the tile is dead: its memory takes the partial sums)
  part[tid] = sa;
  part[NT + tid] = sm;
  part[2 * NT + tid] = sw;
  __syncthreads();
  if (q == 0 && live) {
    double ta = 0.0, tm = 0.0, tw = 0.0;
    for (int j = 0; j < TPC; ++j) {
      ta += part[j * C + c];
      tm += part[NT + j * C + c];
      tw += part[2 * NT + j * C + c];
    }
    const double n = (double)S;
    const T nan = std::numeric_limits<T>::quiet_NaN();
    ((T*)a.mean)[m] = bad ? nan : (T)(tm / n);
    ((T*)a.median)[m] = bad ? nan : med;
    ((T*)a.crps)[m] = bad ? nan : (T)(ta / n - tw / (n * n));
  }
}

}  // namespace pa

extern "C" {

int pa_forecast_scores(int dtype, const void* pred, const void* truth, int64_t S, int64_t M, void* mean, void* median,
                       void* crps, pa_stream_t stream) {
  PA_REQUIRE(dtype == PA_F32 || dtype == PA_F64, "forecast_scores: bad dtype %d", dtype);
  PA_REQUIRE(S >= 1 && M >= 0, "forecast_scores: bad shape S=%lld M=%lld", (long long)S, (long long)M);
  if (S > pa::FS_MAX_SAMPLES)
    return pa::fail(PA_ERR_UNSUPPORTED, "forecast_scores: S=%lld over the limit of %d", (long long)S,
                    pa::FS_MAX_SAMPLES);
  PA_REQUIRE(M <= (int64_t(1) << 34), "forecast_scores: shape too large");
  if (M == 0) return PA_OK;
  PA_REQUIRE(pred && truth && mean && median && crps, "forecast_scores: NULL pointer");
  int logn = 0;
  while ((int64_t(1) << logn) < S) ++logn;
  const pa::FsArgs a{pred, truth, mean, median, crps, M, (int)S, 1 << logn, logn};
  hipStream_t st = pa::as_stream(stream);
#define PA_FS_LAUNCH(T_, C_, NP_, NT_)                                                                       \
  hipLaunchKernelGGL((pa::forecast_scores_kernel<T_, C_, NP_, NT_>), dim3((unsigned)((M + C_ - 1) / C_)), \
                     dim3(NT_), 0, st, a)
  if (dtype == PA_F32) {
    if (S <= pa::FS_SMALL) PA_FS_LAUNCH(float, 32, 128, 256); else PA_FS_LAUNCH(float, 16, 1024, 512);
  } else {
    if (S <= pa::FS_SMALL) PA_FS_LAUNCH(double, 32, 128, 256); else PA_FS_LAUNCH(double, 16, 1024, 512);
  }
#undef PA_FS_LAUNCH
  return pa::check_launch("forecast_scores_kernel");
}

}  // extern "C"
