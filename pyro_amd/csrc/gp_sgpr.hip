// gp_sgpr.hip -- the statistics of a sparse Gaussian-process regression (DTC / VFE) streamed over the data, so that
// Kuf [M, N] is never formed:  A = Kuf Kuf^T [M, M],  b = Kuf r [M, Q],  Kuf[i, n] = variance f(r2(xu_i, x_n)), and
// their gradient given gA, gb, where G = dL/dKuf = (gA + gA^T) Kuf + gb r^T exists one [rows, 32] block at a time in
// registers.  f32 and f64, the five stationary families of gp_kernel.hip, 1 <= D <= 64, 1 <= Q <= 16, M <= 512 (f32) /
// 256 (f64).  No float atomics: partial records in float64, summed in a fixed order; bit-reproducible.
//
// Reference path replaced: pyro/contrib/gp/models/sgpr.py forms Kuf, solves Luu^-1 Kuf and hands W [N, M] to
// LowRankMultivariateNormal (W^T D^-1 W, W^T r, W.pow(2).sum()), all of them [M, N] and all kept by autograd.
//
// r2 is gp_kernel.hip's: the difference first, (xu - x) * (1 / l), its square summed in float64 for both dtypes and
// kept in float64 up to the exponential.  The family functions are gp_families.h's, the ones that file evaluates; the
// wave's block, the staging and r2 are gp_sparse_dev.h's, shared with gp_cond.hip.
//
// Matrix cores.  One primitive, gps_mac: C [32, 32] += A [32, K] B [K, 32] for one wave, the result in the register
// layout of v_mfma_f32_32x32x2_f32 (lane l holds column l % 32 and rows 8 (v / 4) + 4 (l / 32) + v % 4, v < 16).  In
// f32 it IS that instruction (exact f32 products); in f64 the same layout is filled by VALU FMAs (the f64 matrix
// instruction is not used; see the README entry).  r2 is NOT formed there: the expansion x2 - 2 x z + z2 that a matrix
// product would need is the cancellation the direct differences exist to avoid.
//
// Forward.  Workgroup (block pair I <= J of T_M = 128 (f32) / 64 (f64) rows of A, split of N).  Per step of T_N = 32
// points: x and r rows into LDS, Kuf_I and Kuf_J [T_M, 32] generated into LDS (row stride 33: the 32 rows a wave
// reads as an operand fall into 32 banks), then every wave adds its 32 x 32 blocks of Kuf_I Kuf_J^T.  On the diagonal
// (I = J) only one tile is generated and b rides along on the VALU from the same tile.  Every GPS_FLUSH = 4096 points
// the accumulators are added to the workgroup's own float64 record and cleared.  The finalize kernel sums the records
// of the splits in order, takes both triangles from the upper one (exactly symmetric), rounds once.
//
// Backward.  Workgroup (chunk of 128 inducing rows, split of N) walks its steps.  Per step: Kuf[:, step] [M, 32] into
// LDS (all M rows: they are the inner dimension of S Kuf); wave w forms G^T [32 points, 32 rows] for rows
// 32 w .. 32 w + 31 of the chunk: S is read as its own transpose (it is symmetric), 32 consecutive words per operand,
// through L2; gb r^T follows as Q more inner steps.  In that layout a lane owns ONE inducing row and 16 points, so the
// sum over points that the gradient of Xu needs is in-lane plus one exchange between the half-waves.  r2, f, f' are
// recomputed for the lane's 16 entries, w = G f', and the float64 accumulators [128, D] in LDS have one writer per
// entry.  gr is written directly by chunk 0 from the staged tile; gx leaves one partial per chunk (w goes through LDS
// once, then one thread per (point, feature)).  The finalize kernel sums records and applies 2 variance / l_k.
#include "gp_families.h"
#include "gp_host.h"
#include "gp_sparse_dev.h"

namespace pa {

// C += A B.  A(i, k) = A[i * a_si + k * a_sk], i < 32 (always readable); B(k, j) = B[k * b_sk + j * b_sj], read only
// where b_ok (the lane's column j = lane % 32 exists), zero otherwise; k < K
template <typename T>
__device__ __forceinline__ void gps_mac(GpsAcc<T>& acc, const T* A, int a_si, int a_sk, const T* B, int b_sk, int b_sj,
                                        int K, bool b_ok, int lane) {
  const int col = lane & 31, half = lane >> 5;
  if constexpr (sizeof(T) == 4) {
#pragma unroll 4
    for (int k0 = 0; k0 < K; k0 += 2) {
      const int k = k0 + half;
      const bool in = k < K;
      const float av = in ? A[col * a_si + k * a_sk] : 0.0f;
      const float bv = (in && b_ok) ? B[k * b_sk + col * b_sj] : 0.0f;
      acc.c = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc.c, 0, 0, 0);
    }
  } else {
#pragma unroll 2
    for (int k = 0; k < K; ++k) {
      const double bv = b_ok ? B[k * b_sk + col * b_sj] : 0.0;
#pragma unroll
      for (int v = 0; v < 16; ++v) acc.c[v] = fma(A[gps_row(v, lane) * a_si + k * a_sk], bv, acc.c[v]);
    }
  }
}

// ---- forward ---------------------------------------------------------------------------------------------------------
template <typename T>
struct GpsFwdArgs {
  const T *x, *xu, *r, *ls, *variance, *alpha;
  int n_ls, D, Q, blocks, splits, rec_dim;
  int64_t N, M, steps, steps_per_split;
  double *a_rec, *b_rec;      // [pairs, splits, rec_dim, rec_dim], [blocks, splits, rec_dim, Q]
};

template <typename T, template <typename> class FAM, int TM>
__global__ __launch_bounds__(GPS_THREADS) void gp_sgpr_fwd_kernel(const GpsFwdArgs<T> a) {
  constexpr int NB = TM / GPS_SUB, NT = NB * NB / 4, QG = GPS_THREADS / TM, NQ = GPS_MAX_Q / QG;
  extern __shared__ __attribute__((aligned(16))) unsigned char gps_lds[];
  const int D = a.D, Q = a.Q, stride = gps_lds_stride(D);
  double* inv_l = reinterpret_cast<double*>(gps_lds);      // [D]
  T* xui = reinterpret_cast<T*>(inv_l + D);                // [TM, stride]
  T* xuj = xui + TM * stride;                              // [TM, stride]
  T* xs = xuj + TM * stride;                               // [TN, stride]
  T* ksi = xs + GPS_TN * stride;                           // [TM, KS]
  T* ksj = ksi + TM * GPS_KS;                              // [TM, KS]
  T* rs = ksj + TM * GPS_KS;                               // [TN, Q]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int pair = (int)(blockIdx.x / a.splits), split = (int)(blockIdx.x - (unsigned)pair * a.splits);
  int I = 0, rem = pair;
  while (rem >= a.blocks - I) rem -= a.blocks - I, ++I;
  const int J = I + rem;
  const bool diag = I == J;
  gps_stage(a.xu, (int64_t)I * TM, a.M, TM, D, stride, xui);
  if (!diag) gps_stage(a.xu, (int64_t)J * TM, a.M, TM, D, stride, xuj);
  for (int k = tid; k < D; k += GPS_THREADS) inv_l[k] = 1.0 / (double)a.ls[a.n_ls == 1 ? 0 : k];
  const T var = a.variance[0], alpha = a.alpha ? a.alpha[0] : T(1);
  GpsAcc<T> acc[NT];
#pragma unroll
  for (int u = 0; u < NT; ++u) gps_clear(acc[u]);
  double bacc[NQ];
#pragma unroll
  for (int u = 0; u < NQ; ++u) bacc[u] = 0.0;
  const int rd = a.rec_dim;
  double* rec = a.a_rec + ((int64_t)pair * a.splits + split) * rd * rd;
  bool flushed = false;
  auto flush = [&]() {
#pragma unroll
    for (int u = 0; u < NT; ++u) {
      const int t = wave * NT + u, rb = t / NB, cb = t - rb * NB;
#pragma unroll
      for (int v = 0; v < 16; ++v) {
        const int li = rb * GPS_SUB + gps_row(v, lane), lj = cb * GPS_SUB + (lane & 31);
        if (li < rd && lj < rd) rec[li * rd + lj] = (flushed ? rec[li * rd + lj] : 0.0) + (double)acc[u].c[v];
      }
      gps_clear(acc[u]);
    }
    flushed = true;
  };
  const int p = tid & 31, row0 = tid >> 5;      // generation: point p, rows row0 + 8 e
  const int brow = tid % TM, bq0 = tid / TM;    // b: row brow, columns bq0 + QG u
  int64_t s_end = (int64_t)(split + 1) * a.steps_per_split;
  if (s_end > a.steps) s_end = a.steps;
  int since = 0;
  for (int64_t s = (int64_t)split * a.steps_per_split; s < s_end; ++s) {
    const int64_t n0 = s * GPS_TN;
    __syncthreads();      // the previous step's reads of xs, rs and the Kuf tiles are over
    gps_stage(a.x, n0, a.N, GPS_TN, D, stride, xs);
    if (diag) gps_stage(a.r, n0, a.N, GPS_TN, Q, Q, rs);
    __syncthreads();
    const bool p_in = n0 + p < a.N;
    for (int e = 0; e < TM / 8; ++e) {
      const int row = row0 + 8 * e;
      T ki = T(0), kj = T(0), df, da;
      if (p_in && (int64_t)I * TM + row < a.M) {
        FAM<T>::eval(gps_r2(xui + row * stride, xs + p * stride, inv_l, D), alpha, ki, df, da);
        ki *= var;
      }
      ksi[row * GPS_KS + p] = ki;
      if (!diag) {
        if (p_in && (int64_t)J * TM + row < a.M) {
          FAM<T>::eval(gps_r2(xuj + row * stride, xs + p * stride, inv_l, D), alpha, kj, df, da);
          kj *= var;
        }
        ksj[row * GPS_KS + p] = kj;
      }
    }
    __syncthreads();
    const T* kcol = diag ? ksi : ksj;
#pragma unroll
    for (int u = 0; u < NT; ++u) {
      const int t = wave * NT + u, rb = t / NB, cb = t - rb * NB;
      if ((int64_t)I * TM + rb * GPS_SUB >= a.M || (int64_t)J * TM + cb * GPS_SUB >= a.M) continue;      // (wave-uniform)
      gps_mac<T>(acc[u], ksi + rb * GPS_SUB * GPS_KS, GPS_KS, 1, kcol + cb * GPS_SUB * GPS_KS, 1, GPS_KS, GPS_TN, true, lane);
    }
    if (diag) {
#pragma unroll
      for (int u = 0; u < NQ; ++u) {
        const int q = bq0 + QG * u;
        if (q >= Q) continue;
        T sum = T(0);      // 32 products in the tensor's dtype, then float64
        for (int pp = 0; pp < GPS_TN; ++pp) sum += ksi[brow * GPS_KS + pp] * rs[pp * Q + q];
        bacc[u] += (double)sum;
      }
    }
    since += GPS_TN;
    if (since >= GPS_FLUSH && s + 1 < s_end) flush(), since = 0;
  }
  flush();
  if (diag && brow < rd) {
    double* brec = a.b_rec + ((int64_t)I * a.splits + split) * rd * Q;
#pragma unroll
    for (int u = 0; u < NQ; ++u) {
      const int q = bq0 + QG * u;
      if (q < Q) brec[brow * Q + q] = bacc[u];
    }
  }
}

// records -> A (both triangles from the upper one) and b, float64 sums over the splits in order
template <typename T>
__global__ __launch_bounds__(GPS_THREADS) void gp_sgpr_fwd_fin_kernel(const double* __restrict__ a_rec,
                                                                      const double* __restrict__ b_rec, T* __restrict__ A,
                                                                      T* __restrict__ b, int M, int Q, int tm, int blocks,
                                                                      int splits, int rd, int a_blocks) {
  if ((int)blockIdx.x < a_blocks) {
    const int e = blockIdx.x * GPS_THREADS + threadIdx.x;
    if (e >= M * M) return;
    int i = e / M, j = e - i * M;
    if (i > j) {
      const int t = i;
      i = j, j = t;
    }
    const int I = i / tm, J = j / tm;
    const int pair = I * blocks - I * (I - 1) / 2 + (J - I);
    const double* rec = a_rec + (int64_t)pair * splits * rd * rd + (i - I * tm) * rd + (j - J * tm);
    double s = 0.0;
    for (int sp = 0; sp < splits; ++sp) s += rec[(int64_t)sp * rd * rd];
    A[e] = (T)s;
    return;
  }
  const int e = ((int)blockIdx.x - a_blocks) * GPS_THREADS + threadIdx.x;
  if (e >= M * Q) return;
  const int i = e / Q, q = e - i * Q, I = i / tm;
  const double* rec = b_rec + (int64_t)I * splits * rd * Q + (i - I * tm) * Q + q;
  double s = 0.0;
  for (int sp = 0; sp < splits; ++sp) s += rec[(int64_t)sp * rd * Q];
  b[e] = (T)s;
}

// ---- backward --------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(GPS_THREADS) void gp_sgpr_sym_kernel(const T* __restrict__ gA, T* __restrict__ S, int M) {
  const int e = blockIdx.x * GPS_THREADS + threadIdx.x;
  if (e >= M * M) return;
  const int i = e / M, j = e - i * M;
  S[e] = gA[e] + gA[j * M + i];
}

template <typename T>
struct GpsBwdArgs {
  const T *x, *xu, *r, *ls, *variance, *alpha, *S, *gb;
  int n_ls, D, Q, M, splits;
  int want_rows, want_ls, want_scalars, want_gx;
  int64_t N, steps, steps_per_split;
  double *row_rec, *sc_rec, *gx_rec;      // [splits, M, D], [workgroups, SCALARS + D], [chunks, N, D]
  T* gr;                                  // [N, Q] or null
};

template <typename T, template <typename> class FAM>
__global__ __launch_bounds__(GPS_THREADS) void gp_sgpr_bwd_kernel(const GpsBwdArgs<T> a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char gps_lds[];
  __shared__ double red[GPS_THREADS / 64];
  const int D = a.D, Q = a.Q, M = a.M, stride = gps_lds_stride(D);
  const int ks_rows = (M > GPS_BWD_ROWS ? M : GPS_BWD_ROWS) + 1;
  double* inv_l = reinterpret_cast<double*>(gps_lds);      // [D]
  double* acc = inv_l + D;                                 // [BWD_ROWS, D]
  double* ls_acc = acc + GPS_BWD_ROWS * D;                 // [waves, D]
  T* ks = reinterpret_cast<T*>(ls_acc + (GPS_THREADS / 64) * D);      // [ks_rows, KS]: Kuf[:, step], later w of the chunk
  T* xs = ks + ks_rows * GPS_KS;                           // [TN, stride]
  T* rs = xs + GPS_TN * stride;                            // [TN, Q]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, col = lane & 31;
  const int chunk = (int)(blockIdx.x / a.splits), split = (int)(blockIdx.x - (unsigned)chunk * a.splits);
  const int c0 = chunk * GPS_BWD_ROWS, i0 = c0 + wave * GPS_SUB, i = i0 + col;
  const bool wave_on = i0 < M, row_ok = i < M;
  const int rows_here = M - c0 < GPS_BWD_ROWS ? M - c0 : GPS_BWD_ROWS;
  const T* xu_i = a.xu + (int64_t)(row_ok ? i : M - 1) * D;
  for (int k = tid; k < D; k += GPS_THREADS) inv_l[k] = 1.0 / (double)a.ls[a.n_ls == 1 ? 0 : k];
  for (int e = tid; e < GPS_BWD_ROWS * D + (GPS_THREADS / 64) * D; e += GPS_THREADS) acc[e] = 0.0;
  const T var = a.variance[0], alpha = a.alpha ? a.alpha[0] : T(1);
  const bool ard = a.want_ls && a.n_ls != 1;
  const int p = tid & 31, g8 = tid >> 5;
  double s_var = 0.0, s_alpha = 0.0, s_ls = 0.0;
  int64_t s_end = (int64_t)(split + 1) * a.steps_per_split;
  if (s_end > a.steps) s_end = a.steps;
  for (int64_t s = (int64_t)split * a.steps_per_split; s < s_end; ++s) {
    const int64_t n0 = s * GPS_TN;
    __syncthreads();      // the previous step's reads of ks, xs, rs are over
    gps_stage(a.x, n0, a.N, GPS_TN, D, stride, xs);
    gps_stage(a.r, n0, a.N, GPS_TN, Q, Q, rs);
    __syncthreads();
    const bool p_in = n0 + p < a.N;
    for (int j = g8; j < M; j += 8) {
      T f = T(0), df, da;
      if (p_in) {
        FAM<T>::eval(gps_r2(a.xu + (int64_t)j * D, xs + p * stride, inv_l, D), alpha, f, df, da);
        f *= var;
      }
      ks[j * GPS_KS + p] = f;
    }
    __syncthreads();
    T w[16];
    if (wave_on) {
      // G^T [32 points, 32 rows] = Kuf[:, step]^T S[:, rows] + r[step] gb[rows]^T
      GpsAcc<T> g;
      gps_clear(g);
      gps_mac<T>(g, ks, 1, GPS_KS, a.S + i0, M, 1, M, row_ok, lane);
      gps_mac<T>(g, rs, Q, 1, a.gb + (int64_t)i0 * Q, 1, Q, Q, row_ok, lane);
      T t_var = T(0), t_alpha = T(0), t_ls = T(0);
#pragma unroll
      for (int v = 0; v < 16; ++v) {
        const int pv = gps_row(v, lane);
        const T gv = (row_ok && n0 + pv < a.N) ? g.c[v] : T(0);      // padded entries weigh nothing
        const double r2 = gps_r2(xu_i, xs + pv * stride, inv_l, D);
        T f, df, da;
        FAM<T>::eval(r2, alpha, f, df, da);
        w[v] = gv * var * df;
        t_var += gv * f;
        t_alpha += gv * da;
        t_ls += w[v] * (T)r2;
      }
      s_var += (double)t_var, s_alpha += (double)t_alpha, s_ls += (double)t_ls;
      if (a.want_rows || ard) {
        for (int k = 0; k < D; ++k) {
          const T il = (T)inv_l[k], xi = xu_i[k];
          T sum = T(0), q2 = T(0);
#pragma unroll
          for (int v = 0; v < 16; ++v) {
            const T d = (xi - xs[gps_row(v, lane) * stride + k]) * il;
            sum += w[v] * d;
            q2 += w[v] * d * d;
          }
          if (a.want_rows) {
            sum += __shfl_xor(sum, 32);
            if (lane < 32 && row_ok) acc[(i - c0) * D + k] += (double)sum;      // one writer per entry
          }
          if (ard) {
            const T total = wave_sum(q2);
            if (lane == 0) ls_acc[wave * D + k] += (double)total;
          }
        }
      }
    } else {
#pragma unroll
      for (int v = 0; v < 16; ++v) w[v] = T(0);
    }
    if (a.gr != nullptr && chunk == 0 && p_in) {
      for (int q = g8; q < Q; q += 8) {
        double sum = 0.0;
        for (int j = 0; j < M; ++j) sum += (double)(ks[j * GPS_KS + p] * a.gb[j * Q + q]);
        a.gr[(n0 + p) * Q + q] = (T)sum;
      }
    }
    if (a.want_gx) {      // (uniform over the workgroup)
      __syncthreads();    // every read of Kuf[:, step] is over: the tile now carries w of the chunk's rows
#pragma unroll
      for (int v = 0; v < 16; ++v) ks[(wave * GPS_SUB + col) * GPS_KS + gps_row(v, lane)] = w[v];
      __syncthreads();
      if (p_in) {
        for (int k = g8; k < D; k += 8) {
          const double il = inv_l[k];
          const T xv = xs[p * stride + k];
          double sum = 0.0;
          for (int li = 0; li < rows_here; ++li)
            sum += (double)(ks[li * GPS_KS + p] * ((a.xu[(int64_t)(c0 + li) * D + k] - xv) * (T)il));
          a.gx_rec[((int64_t)chunk * a.N + n0 + p) * D + k] = sum;
        }
      }
    }
  }
  __syncthreads();
  if (a.want_rows) {
    double* rec = a.row_rec + ((int64_t)split * M + c0) * D;
    for (int e = tid; e < rows_here * D; e += GPS_THREADS) rec[e] = acc[e];
  }
  if (a.want_scalars) {
    double* sc = a.sc_rec + (int64_t)blockIdx.x * (GPS_SCALARS + D);
    const double v0 = block_sum_f64_waves(s_var, red, GPS_THREADS / 64);
    const double v1 = block_sum_f64_waves(s_alpha, red, GPS_THREADS / 64);
    const double v2 = block_sum_f64_waves(s_ls, red, GPS_THREADS / 64);
    if (tid == 0) sc[0] = v0, sc[1] = v1, sc[2] = v2;
    if (ard)
      for (int k = tid; k < D; k += GPS_THREADS)
        sc[GPS_SCALARS + k] = (ls_acc[k] + ls_acc[D + k]) + (ls_acc[2 * D + k] + ls_acc[3 * D + k]);
  }
}

// records -> gradients, float64 sums in a fixed order.  Blocks [0, xu_blocks): gxu[i, k] = (2 variance / l_k) sum over
// the splits; [.., + x_blocks): gx[n, k] = -(2 variance / l_k) sum over the chunks; then one block per reduced output:
// lengthscale (n_ls of them), variance, alpha.  w carries the variance already (w = G variance f').
template <typename T>
struct GpsFinArgs {
  const double *row_rec, *sc_rec, *gx_rec;
  const T *ls, *variance;
  int n_ls, D, M, splits, chunks;
  int64_t N, workgroups, xu_blocks, x_blocks;
  T *gxu, *gx, *g_ls, *g_var, *g_alpha;
};

template <typename T>
__global__ __launch_bounds__(GPS_THREADS) void gp_sgpr_bwd_fin_kernel(const GpsFinArgs<T> a) {
  __shared__ double red[GPS_THREADS / 64];
  const int64_t blk = blockIdx.x;
  if (blk < a.xu_blocks) {
    const int64_t e = blk * GPS_THREADS + threadIdx.x, total = (int64_t)a.M * a.D;
    if (e >= total) return;
    double s = 0.0;
    for (int sp = 0; sp < a.splits; ++sp) s += a.row_rec[(int64_t)sp * total + e];
    a.gxu[e] = (T)(2.0 / (double)a.ls[a.n_ls == 1 ? 0 : (int)(e % a.D)] * s);
    return;
  }
  if (blk < a.xu_blocks + a.x_blocks) {
    const int64_t e = (blk - a.xu_blocks) * GPS_THREADS + threadIdx.x, total = a.N * a.D;
    if (e >= total) return;
    double s = 0.0;
    for (int c = 0; c < a.chunks; ++c) s += a.gx_rec[(int64_t)c * total + e];
    a.gx[e] = (T)(-2.0 / (double)a.ls[a.n_ls == 1 ? 0 : (int)(e % a.D)] * s);
    return;
  }
  const int which = (int)(blk - a.xu_blocks - a.x_blocks);      // 0 .. n_ls - 1: lengthscale; then variance, alpha
  int slot;
  T* out;
  if (which < a.n_ls) slot = a.n_ls == 1 ? 2 : GPS_SCALARS + which, out = a.g_ls ? a.g_ls + which : nullptr;
  else if (which == a.n_ls) slot = 0, out = a.g_var;
  else slot = 1, out = a.g_alpha;
  if (out == nullptr) return;      // (uniform over the block)
  double s = 0.0;
  for (int64_t wg = threadIdx.x; wg < a.workgroups; wg += GPS_THREADS) s += a.sc_rec[wg * (GPS_SCALARS + a.D) + slot];
  s = block_sum_f64_waves(s, red, GPS_THREADS / 64);
  if (threadIdx.x == 0) {
    if (which < a.n_ls) s *= -2.0 / (double)a.ls[which];
    else if (which > a.n_ls) s *= (double)a.variance[0];
    *out = (T)s;
  }
}

// ---- launchers -------------------------------------------------------------------------------------------------------
template <typename T, template <typename> class FAM>
static int gps_fwd_launch(const GpsFwdPlan& pl, const void* x, const void* xu, const void* r, const void* ls, int n_ls,
                          const void* variance, const void* alpha, void* A, void* b, int64_t N, int64_t M, void* workspace,
                          hipStream_t st) {
  GpsFwdArgs<T> a;
  a.x = (const T*)x, a.xu = (const T*)xu, a.r = (const T*)r, a.ls = (const T*)ls, a.variance = (const T*)variance;
  a.alpha = (const T*)alpha, a.n_ls = n_ls, a.D = pl.D, a.Q = pl.Q, a.blocks = pl.blocks, a.splits = pl.splits;
  a.rec_dim = pl.rec_dim, a.N = N, a.M = M, a.steps = pl.steps, a.steps_per_split = pl.steps_per_split;
  a.a_rec = (double*)workspace, a.b_rec = a.a_rec + pl.a_doubles;
  constexpr int TM = sizeof(T) == 4 ? 128 : 64;
  int rc = gp_launch("gp_sgpr_fwd_kernel", gp_sgpr_fwd_kernel<T, FAM, TM>, pl.workgroups, GPS_THREADS, pl.lds_bytes, st, a);
  if (rc != PA_OK) return rc;
  const int a_blocks = (int)gps_div_up(M * M, GPS_THREADS), b_blocks = (int)gps_div_up(M * pl.Q, GPS_THREADS);
  hipLaunchKernelGGL(gp_sgpr_fwd_fin_kernel<T>, dim3((unsigned)(a_blocks + b_blocks)), dim3(GPS_THREADS), 0, st, a.a_rec,
                     a.b_rec, (T*)A, (T*)b, (int)M, pl.Q, pl.tm, pl.blocks, pl.splits, pl.rec_dim, a_blocks);
  return check_launch("gp_sgpr_fwd_fin_kernel");
}

struct GpsBwdOut {
  void *gx, *gxu, *g_ls, *g_var, *g_alpha, *gr;
};

template <typename T, template <typename> class FAM>
static int gps_bwd_launch(const GpsBwdPlan& pl, const void* x, const void* xu, const void* r, const void* ls, int n_ls,
                          const void* variance, const void* alpha, const void* gA, const void* gb, int64_t N, int64_t M,
                          const GpsBwdOut& o, void* workspace, hipStream_t st) {
  double* ws = (double*)workspace;
  T* S = (T*)ws;
  hipLaunchKernelGGL(gp_sgpr_sym_kernel<T>, dim3((unsigned)gps_div_up(M * M, GPS_THREADS)), dim3(GPS_THREADS), 0, st,
                     (const T*)gA, S, (int)M);
  int rc = check_launch("gp_sgpr_sym_kernel");
  if (rc != PA_OK) return rc;
  const bool scalars = o.g_ls || o.g_var || o.g_alpha;
  GpsBwdArgs<T> a;
  a.x = (const T*)x, a.xu = (const T*)xu, a.r = (const T*)r, a.ls = (const T*)ls, a.variance = (const T*)variance;
  a.alpha = (const T*)alpha, a.S = S, a.gb = (const T*)gb, a.n_ls = n_ls, a.D = pl.D, a.Q = pl.Q, a.M = (int)M;
  a.splits = pl.splits, a.want_rows = pl.want_gxu ? 1 : 0, a.want_ls = o.g_ls ? 1 : 0, a.want_scalars = scalars ? 1 : 0;
  a.want_gx = pl.want_gx ? 1 : 0, a.N = N, a.steps = pl.steps, a.steps_per_split = pl.steps_per_split;
  a.row_rec = ws + pl.s_doubles, a.sc_rec = a.row_rec + pl.row_doubles, a.gx_rec = a.sc_rec + pl.scalar_doubles;
  a.gr = (T*)o.gr;
  rc = gp_launch("gp_sgpr_bwd_kernel", gp_sgpr_bwd_kernel<T, FAM>, pl.workgroups, GPS_THREADS, pl.lds_bytes, st, a);
  if (rc != PA_OK) return rc;
  GpsFinArgs<T> f;
  f.row_rec = a.row_rec, f.sc_rec = a.sc_rec, f.gx_rec = a.gx_rec, f.ls = a.ls, f.variance = a.variance, f.n_ls = n_ls;
  f.D = pl.D, f.M = (int)M, f.splits = pl.splits, f.chunks = pl.chunks, f.N = N, f.workgroups = pl.workgroups;
  f.xu_blocks = pl.want_gxu ? gps_div_up(M * pl.D, GPS_THREADS) : 0;
  f.x_blocks = pl.want_gx ? gps_div_up(N * pl.D, GPS_THREADS) : 0;
  f.gxu = (T*)o.gxu, f.gx = (T*)o.gx, f.g_ls = (T*)o.g_ls, f.g_var = (T*)o.g_var, f.g_alpha = (T*)o.g_alpha;
  const int64_t blocks = f.xu_blocks + f.x_blocks + (scalars ? n_ls + 2 : 0);
  if (blocks == 0) return PA_OK;
  PA_REQUIRE(blocks <= GPS_MAX_WORKGROUPS, "pa_gp_sgpr_bwd: finalize grid of %lld blocks", (long long)blocks);
  hipLaunchKernelGGL(gp_sgpr_bwd_fin_kernel<T>, dim3((unsigned)blocks), dim3(GPS_THREADS), 0, st, f);
  return check_launch("gp_sgpr_bwd_fin_kernel");
}

template <typename T>
static int gps_fwd_family(int family, const GpsFwdPlan& pl, const void* x, const void* xu, const void* r, const void* ls,
                          int n_ls, const void* variance, const void* alpha, void* A, void* b, int64_t N, int64_t M,
                          void* workspace, hipStream_t st) {
  GP_FAMILY_DISPATCH(gps_fwd_launch, pl, x, xu, r, ls, n_ls, variance, alpha, A, b, N, M, workspace, st)
}
template <typename T>
static int gps_bwd_family(int family, const GpsBwdPlan& pl, const void* x, const void* xu, const void* r, const void* ls,
                          int n_ls, const void* variance, const void* alpha, const void* gA, const void* gb, int64_t N,
                          int64_t M, const GpsBwdOut& o, void* workspace, hipStream_t st) {
  GP_FAMILY_DISPATCH(gps_bwd_launch, pl, x, xu, r, ls, n_ls, variance, alpha, gA, gb, N, M, o, workspace, st)
}

static int gps_check(const char* who, int dtype, int family, const void* x, const void* xu, const void* r, const void* ls,
                     int n_ls, const void* variance, const void* alpha, int64_t N, int64_t M, int64_t D, int64_t Q) {
  PA_REQUIRE(dtype == PA_F32 || dtype == PA_F64, "%s: dtype %d", who, dtype);
  const size_t elem = dtype == PA_F32 ? 4 : 8;
  PA_REQUIRE(family >= 0 && family < GPS_FAMILIES && N >= 0 && M >= 0 && N < GPS_MAX_POINTS && (n_ls == 1 || n_ls == D),
             "%s: family=%d N=%lld M=%lld n_ls=%d", who, family, (long long)N, (long long)M, n_ls);
  if (!gps_shape_ok(family, N, M, D, Q, n_ls, elem))
    return fail(PA_ERR_UNSUPPORTED, "%s: M=%lld D=%lld Q=%lld outside M <= %d, 1 <= D <= %d, 1 <= Q <= %d", who,
                (long long)M, (long long)D, (long long)Q, gps_max_m(elem), GPS_MAX_D, GPS_MAX_Q);
  PA_REQUIRE(ls != nullptr && variance != nullptr && (N == 0 || (x != nullptr && r != nullptr)) &&
                 (M == 0 || xu != nullptr),
             "%s: null input", who);
  PA_REQUIRE(family != PA_GP_RATIONAL_QUADRATIC || alpha != nullptr, "%s: RationalQuadratic needs scale_mixture", who);
  return PA_OK;
}

}  // namespace pa

extern "C" {

size_t pa_gp_sgpr_workspace(int dtype, int64_t N, int64_t M, int64_t D, int64_t Q, int backward, int want_gx,
                            int want_gxu, int forced_splits) {
  const size_t elem = dtype == PA_F32 ? 4 : 8;
  if (!pa::gps_shape_ok(0, N, M, D, Q, 1, elem) || N == 0 || M == 0) return 0;
  if (backward)
    return pa::gps_bwd_plan(N, M, (int)D, (int)Q, elem, want_gx != 0, want_gxu != 0, pa::cu_count(), forced_splits).bytes;
  return pa::gps_fwd_plan(N, M, (int)D, (int)Q, elem, pa::cu_count(), forced_splits).bytes;
}

int pa_gp_sgpr_fwd(int dtype, int family, const void* x, const void* xu, const void* r, const void* lengthscale, int n_ls,
                   const void* variance, const void* alpha, void* A, void* b, int64_t N, int64_t M, int64_t D, int64_t Q,
                   int forced_splits, void* workspace, size_t workspace_bytes, pa_stream_t stream) {
  int rc = pa::gps_check("pa_gp_sgpr_fwd", dtype, family, x, xu, r, lengthscale, n_ls, variance, alpha, N, M, D, Q);
  if (rc != PA_OK) return rc;
  PA_REQUIRE(forced_splits >= 0, "pa_gp_sgpr_fwd: forced_splits=%d", forced_splits);
  if (N == 0 || M == 0) return PA_OK;      // (no launch: the caller fills the zeros)
  PA_REQUIRE(A != nullptr && b != nullptr, "pa_gp_sgpr_fwd: null output");
  const size_t elem = dtype == PA_F32 ? 4 : 8;
  const pa::GpsFwdPlan pl = pa::gps_fwd_plan(N, M, (int)D, (int)Q, elem, pa::cu_count(), forced_splits);
  rc = pa::gp_workspace_check("pa_gp_sgpr_fwd", workspace, workspace_bytes, pl.bytes);
  if (rc != PA_OK) return rc;
  PA_REQUIRE(pl.workgroups <= pa::GPS_MAX_WORKGROUPS && (pl.a_doubles + pl.b_doubles) * sizeof(double) == pl.bytes,
             "pa_gp_sgpr_fwd: inconsistent plan");
  hipStream_t st = pa::as_stream(stream);
  if (dtype == PA_F32)
    return pa::gps_fwd_family<float>(family, pl, x, xu, r, lengthscale, n_ls, variance, alpha, A, b, N, M, workspace, st);
  return pa::gps_fwd_family<double>(family, pl, x, xu, r, lengthscale, n_ls, variance, alpha, A, b, N, M, workspace, st);
}

int pa_gp_sgpr_bwd(int dtype, int family, const void* x, const void* xu, const void* r, const void* lengthscale, int n_ls,
                   const void* variance, const void* alpha, const void* gA, const void* gb, int64_t N, int64_t M, int64_t D,
                   int64_t Q, void* gx, void* gxu, void* g_lengthscale, void* g_variance, void* g_alpha, void* gr,
                   int forced_splits, void* workspace, size_t workspace_bytes, pa_stream_t stream) {
  int rc = pa::gps_check("pa_gp_sgpr_bwd", dtype, family, x, xu, r, lengthscale, n_ls, variance, alpha, N, M, D, Q);
  if (rc != PA_OK) return rc;
  PA_REQUIRE(g_alpha == nullptr || family == PA_GP_RATIONAL_QUADRATIC, "pa_gp_sgpr_bwd: g_alpha for family %d", family);
  PA_REQUIRE(forced_splits >= 0, "pa_gp_sgpr_bwd: forced_splits=%d", forced_splits);
  if (!(gx || gxu || g_lengthscale || g_variance || g_alpha || gr)) return PA_OK;
  if (N == 0 || M == 0) return PA_OK;      // (no launch: the caller fills the zeros)
  PA_REQUIRE(gA != nullptr && gb != nullptr, "pa_gp_sgpr_bwd: null gA or gb");
  const size_t elem = dtype == PA_F32 ? 4 : 8;
  const pa::GpsBwdPlan pl =
      pa::gps_bwd_plan(N, M, (int)D, (int)Q, elem, gx != nullptr, gxu != nullptr, pa::cu_count(), forced_splits);
  rc = pa::gp_workspace_check("pa_gp_sgpr_bwd", workspace, workspace_bytes, pl.bytes);
  if (rc != PA_OK) return rc;
  PA_REQUIRE(pl.workgroups <= pa::GPS_MAX_WORKGROUPS &&
                 (pl.s_doubles + pl.row_doubles + pl.scalar_doubles + pl.gx_doubles) * sizeof(double) == pl.bytes,
             "pa_gp_sgpr_bwd: inconsistent plan");
  const pa::GpsBwdOut o = {gx, gxu, g_lengthscale, g_variance, g_alpha, gr};
  hipStream_t st = pa::as_stream(stream);
  if (dtype == PA_F32)
    return pa::gps_bwd_family<float>(family, pl, x, xu, r, lengthscale, n_ls, variance, alpha, gA, gb, N, M, o, workspace,
                                     st);
  return pa::gps_bwd_family<double>(family, pl, x, xu, r, lengthscale, n_ls, variance, alpha, gA, gb, N, M, o, workspace,
                                    st);
}

}  // extern "C"
