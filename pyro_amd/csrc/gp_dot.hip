// gp_dot.hip -- the dot-product covariance matrix of a Gaussian-process model and its gradient ON MATRIX CORES:
//   K[i, j] = variance * (bias + sum_k x_ik z_jk)^degree,
// x [N, D], z [M, D] or z = x, 1 <= D <= 64, 1 <= degree <= 16, f32 and f64; bias = NULL means 0 and variance = NULL
// means 1.  gp.kernels.Polynomial is this function; gp.kernels.Coregionalize is its degree 1 without bias and variance
// on the features [X C, X sqrt(d)].  The forward is ONE launch that writes K once; the backward is ONE pass over the
// incoming gradient G for every wanted gradient, plus a fixed-order float64 finalize.  No float atomics:
// bit-reproducible from call to call.
//
// Reference path replaced: pyro/contrib/gp/kernels/dot_product.py makes four passes over [N, M] (matmul, + bias,
// ** degree, * variance), two of which autograd keeps; coregionalize.py two [N, M] products and an add.
//
// A dot product does not cancel the way x2 - 2 x z + z2 does (gp_kernel.hip, gp_periodic.hip: VALU work for that
// reason), so here s = x z^T is formed where it belongs.  A workgroup of 4 waves owns a 64 x 64 tile (gp_kernel_plan.h),
// a wave one 32 x 32 block of it, held as 16 values per lane (GpdFrag):
//   f32  one accumulator of v_mfma_f32_32x32x2_f32 (exact f32 products): lane l holds column l % 32 and rows
//        8 (v / 4) + 4 (l / 32) + v % 4 (the layout of gp_sgpr.hip)
//   f64  2 x 2 accumulators of v_mfma_f64_16x16x4_f64: in block (rb, cb), lane l holds column 16 cb + l % 16 and rows
//        16 rb + 4 r + l / 16, r < 4
// Both row blocks are staged once in LDS at the tree's odd row stride over the PADDED width (2 features per f32
// instruction, 4 per f64 one: gp_dot_plan.h); the pad is zeros in LDS, the inner loop has no branch.  Edge tiles are
// masked at the store.  The epilogue is in registers: t = bias + s, t^degree by repeated multiplication (degree is
// uniform), times variance; a lane's stores run along the row (32 lanes x 4 bytes, 16 lanes x 8 bytes).
//
// Backward.  K is recomputed, never saved (the models add noise to its diagonal in place).  Workgroup (row block,
// column split: the split rule of gp_kernel_plan.h) walks its column tiles; per tile and wave
//   s by the matrix instruction as above;  W = G variance degree t^(degree - 1), zero outside [N, M]
//   g_variance += sum G t^degree,  g_bias += sum W            16 terms in the tensor's dtype, then float64
//   cols:  W^T X [32 columns, D].  W already IS an A operand of that product: a lane owns one column of W and 16 rows,
//          and register v of the two half-waves (f32; the four quarter-waves in f64) are exactly the consecutive inner
//          indices of one instruction -- if X's rows are read from LDS in that same permuted order.  No LDS trip.  The
//          result leaves as one float64 record [columns, D] per HALF row block (no sum across waves is needed).
//   rows:  W Z [32 rows, D] needs W by rows: one transposition of the block through the wave's own LDS buffer at
//          stride 33, then the matrix instruction into accumulators that live across the tiles (D <= 64: two blocks per
//          wave).  Every GPD_FLUSH columns they are added to the float64 rows [64, D] in LDS (the two waves of a row
//          in turn: one writer per entry at a time) and cleared; the workgroup leaves one row record in slot ``split``.
// gX is the rows part and gZ the cols part.  With z = x both parts run on the same G, read ONCE, and the finalize adds
// them: gX = (W + W^T) X.  A part that no wanted gradient needs is not computed.  The finalize kernel adds the records
// in a fixed order in float64 and rounds once (the row-record copy and the sum over the splits are
// gp_tile.h's, as in the direct-difference kernels).  The cols records cost ceil(N / 32) M D float64 words: for
// N >> M give the long side the role of z.
//
// gfx950 cross-compile (hipcc -O3, -Rpass-analysis=kernel-resource-usage): no instantiation uses scratch; LDS is
// dynamic; the register table is in the README entry "Gaussian processes".
#include "gp_dot_plan.h"
#include "gp_host.h"
#include "gp_tile.h"

namespace pa {

typedef float gpd_f32x16 __attribute__((ext_vector_type(16)));
typedef double gpd_f64x4 __attribute__((ext_vector_type(4)));

// ---- a wave's 32 x 32 block: 16 values per lane -----------------------------------------------------------------------
template <typename T>
struct GpdFrag;
template <>
struct GpdFrag<float> {
  gpd_f32x16 c;
  __device__ __forceinline__ float get(int v) const { return c[v]; }
  __device__ __forceinline__ void clear() {
#pragma unroll
    for (int v = 0; v < 16; ++v) c[v] = 0.0f;
  }
  __device__ __forceinline__ static int row(int v, int lane) { return 8 * (v >> 2) + 4 * (lane >> 5) + (v & 3); }
  __device__ __forceinline__ static int col(int, int lane) { return lane & 31; }
};
template <>
struct GpdFrag<double> {
  gpd_f64x4 b[4];      // block (rb, cb) is b[2 rb + cb]; value v is b[v / 4][v % 4]
  __device__ __forceinline__ double get(int v) const { return b[v >> 2][v & 3]; }
  __device__ __forceinline__ void clear() {
#pragma unroll
    for (int u = 0; u < 4; ++u) b[u] = gpd_f64x4{0.0, 0.0, 0.0, 0.0};
  }
  __device__ __forceinline__ static int row(int v, int lane) { return 16 * (v >> 3) + 4 * (v & 3) + (lane >> 4); }
  __device__ __forceinline__ static int col(int v, int lane) { return 16 * ((v >> 2) & 1) + (lane & 15); }
};

// acc += A B^T: A [32, kp] and B [32, kp] row-major in LDS at ``stride``, kp the padded width (zeros past D)
__device__ __forceinline__ void gpd_mac_nt(GpdFrag<float>& acc, const float* A, const float* B, int stride, int kp,
                                           int lane) {
  const float* a = A + (lane & 31) * stride + (lane >> 5);
  const float* b = B + (lane & 31) * stride + (lane >> 5);
  for (int k = 0; k < kp; k += 2) acc.c = __builtin_amdgcn_mfma_f32_32x32x2f32(a[k], b[k], acc.c, 0, 0, 0);
}
__device__ __forceinline__ void gpd_mac_nt(GpdFrag<double>& acc, const double* A, const double* B, int stride, int kp,
                                           int lane) {
  const double* a = A + (lane & 15) * stride + (lane >> 4);
  const double* b = B + (lane & 15) * stride + (lane >> 4);
  for (int k = 0; k < kp; k += 4) {
    const double a0 = a[k], a1 = a[16 * stride + k], b0 = b[k], b1 = b[16 * stride + k];
    acc.b[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc.b[0], 0, 0, 0);
    acc.b[1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc.b[1], 0, 0, 0);
    acc.b[2] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc.b[2], 0, 0, 0);
    acc.b[3] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc.b[3], 0, 0, 0);
  }
}

// out [32 columns of W, features d0 .. d0 + 31] += W^T X: W in the block layout IS the A operand; X [32, stride] are
// the block's rows in LDS, read in the order in which the lanes hold W's rows.  Features past D read as zero.
__device__ __forceinline__ void gpd_mac_tn(GpdFrag<float>& out, const float (&w)[16], const float* X, int stride, int d0,
                                           int D, int lane) {
  const int d = d0 + (lane & 31);
  const bool ok = d < D;
#pragma unroll
  for (int v = 0; v < 16; ++v) {
    const float xv = ok ? X[GpdFrag<float>::row(v, lane) * stride + d] : 0.0f;
    out.c = __builtin_amdgcn_mfma_f32_32x32x2f32(w[v], xv, out.c, 0, 0, 0);
  }
}
__device__ __forceinline__ void gpd_mac_tn(GpdFrag<double>& out, const double (&w)[16], const double* X, int stride,
                                           int d0, int D, int lane) {
  const int da = d0 + (lane & 15), db = da + 16;
  const bool ok_a = da < D, ok_b = db < D;
#pragma unroll
  for (int v = 0; v < 16; ++v) {      // v = 8 rb + 4 cb + r: W's block (rb, cb) adds to out's blocks (cb, 0) and (cb, 1)
    const double* xr = X + GpdFrag<double>::row(v, lane) * stride;
    const double xa = ok_a ? xr[da] : 0.0, xb = ok_b ? xr[db] : 0.0;
    const int cb = (v >> 2) & 1;
    out.b[2 * cb] = __builtin_amdgcn_mfma_f64_16x16x4f64(w[v], xa, out.b[2 * cb], 0, 0, 0);
    out.b[2 * cb + 1] = __builtin_amdgcn_mfma_f64_16x16x4f64(w[v], xb, out.b[2 * cb + 1], 0, 0, 0);
  }
}

// acc [32 rows of W, features d0 .. d0 + 31] += W Z: W [32, 32] by rows in the wave's buffer at stride GPD_WT, Z [32,
// stride] the block's columns in LDS.  Features past D read as zero.
__device__ __forceinline__ void gpd_mac_nn(GpdFrag<float>& acc, const float* W, const float* Z, int stride, int d0, int D,
                                           int lane) {
  const int d = d0 + (lane & 31);
  const bool ok = d < D;
  const float* a = W + (lane & 31) * GPD_WT + (lane >> 5);
  const float* b = Z + (lane >> 5) * stride + d;
#pragma unroll 4
  for (int k = 0; k < GPD_SUB; k += 2)
    acc.c = __builtin_amdgcn_mfma_f32_32x32x2f32(a[k], ok ? b[k * stride] : 0.0f, acc.c, 0, 0, 0);
}
__device__ __forceinline__ void gpd_mac_nn(GpdFrag<double>& acc, const double* W, const double* Z, int stride, int d0,
                                           int D, int lane) {
  const int da = d0 + (lane & 15), db = da + 16;
  const bool ok_a = da < D, ok_b = db < D;
  const double* a = W + (lane & 15) * GPD_WT + (lane >> 4);
  const double* b = Z + (lane >> 4) * stride;
#pragma unroll 2
  for (int k = 0; k < GPD_SUB; k += 4) {
    const double a0 = a[k], a1 = a[16 * GPD_WT + k];
    const double b0 = ok_a ? b[k * stride + da] : 0.0, b1 = ok_b ? b[k * stride + db] : 0.0;
    acc.b[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc.b[0], 0, 0, 0);
    acc.b[1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc.b[1], 0, 0, 0);
    acc.b[2] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc.b[2], 0, 0, 0);
    acc.b[3] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc.b[3], 0, 0, 0);
  }
}

// rows [first, first + 64) of p [n, D] into tile [64, stride], zeros past the end and in the pad [D, stride)
template <typename T>
__device__ __forceinline__ void gpd_stage(const T* __restrict__ p, int64_t first, int64_t n, int D, int stride, T* tile) {
  for (int e = threadIdx.x; e < GPK_TILE * stride; e += GPD_THREADS) {
    const int row = e / stride, k = e - row * stride;
    const int64_t i = first + row;
    tile[e] = (i < n && k < D) ? p[i * D + k] : T(0);
  }
}

// ---- forward ---------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(GPD_THREADS) void gp_dot_fwd_kernel(const T* __restrict__ x, const T* __restrict__ z,
                                                                 const T* __restrict__ variance, const T* __restrict__ bias,
                                                                 int degree, T* __restrict__ K, int64_t N, int64_t M, int D,
                                                                 int64_t col_tiles) {
  extern __shared__ __attribute__((aligned(16))) unsigned char gpd_lds[];
  const int stride = gpd_lds_stride(D, sizeof(T)), kp = gpd_padded_d(D, sizeof(T));
  T* xs = reinterpret_cast<T*>(gpd_lds);
  T* zs = xs + GPK_TILE * stride;
  const int64_t rt = (int64_t)blockIdx.x / col_tiles, ct = (int64_t)blockIdx.x - rt * col_tiles;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, wr = wave >> 1, wc = wave & 1;
  const int64_t i0 = rt * GPK_TILE + wr * GPD_SUB, j0 = ct * GPK_TILE + wc * GPD_SUB;
  gpd_stage(x, rt * GPK_TILE, N, D, stride, xs);
  gpd_stage(z, ct * GPK_TILE, M, D, stride, zs);
  __syncthreads();
  GpdFrag<T> s;
  s.clear();
  gpd_mac_nt(s, xs + wr * GPD_SUB * stride, zs + wc * GPD_SUB * stride, stride, kp, lane);
  const T var = variance ? variance[0] : T(1), b = bias ? bias[0] : T(0);
  T t[16], p[16];
#pragma unroll
  for (int v = 0; v < 16; ++v) p[v] = t[v] = b + s.get(v);
  for (int e = 1; e < degree; ++e)
#pragma unroll
    for (int v = 0; v < 16; ++v) p[v] *= t[v];
#pragma unroll
  for (int v = 0; v < 16; ++v) {
    const int64_t i = i0 + GpdFrag<T>::row(v, lane), j = j0 + GpdFrag<T>::col(v, lane);
    if (i < N && j < M) K[i * M + j] = var * p[v];
  }
}

// ---- backward --------------------------------------------------------------------------------------------------------
template <typename T>
struct GpdBwdArgs {
  const T *x, *z, *G, *variance, *bias;      // x [R, D] the rows, z [C, D] the columns (z = x with sym), G [R, C]
  int degree, D, splits, rows_part, cols_part, want_scalars;
  int64_t R, C, tiles_per_split, col_tiles, half_blocks;
  double *row_rec, *col_rec, *sc_rec;        // [splits, R, D], [half_blocks, C, D], [workgroups, GPD_SCALARS]
};

template <typename T>
__global__ __launch_bounds__(GPD_THREADS) void gp_dot_bwd_kernel(const GpdBwdArgs<T> a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char gpd_lds[];
  __shared__ double red[GPK_WAVES];
  const int D = a.D, stride = gpd_lds_stride(D, sizeof(T)), kp = gpd_padded_d(D, sizeof(T));
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wr = wave >> 1, wc = wave & 1;
  T* xs = reinterpret_cast<T*>(gpd_lds);
  T* zs = xs + GPK_TILE * stride;
  T* wt = zs + GPK_TILE * stride + wave * GPD_SUB * GPD_WT;                        // the wave's own [32, 33]
  double* acc = reinterpret_cast<double*>(gpd_lds + gpd_bwd_acc_offset(D, sizeof(T)));      // [64, D]
  const int64_t rb = (int64_t)blockIdx.x / a.splits;
  const int split = (int)((int64_t)blockIdx.x - rb * a.splits);
  const int64_t i0 = rb * GPK_TILE + wr * GPD_SUB, hb = 2 * rb + wr;
  const T* xw = xs + wr * GPD_SUB * stride;      // the wave's rows
  const T* zw = zs + wc * GPD_SUB * stride;      // the wave's columns
  gpd_stage(a.x, rb * GPK_TILE, a.R, D, stride, xs);
  if (a.rows_part)
    for (int e = tid; e < GPK_TILE * D; e += GPD_THREADS) acc[e] = 0.0;
  const T b = a.bias ? a.bias[0] : T(0);
  const T scale = (a.variance ? a.variance[0] : T(1)) * (T)a.degree;
  GpdFrag<T> gx0, gx1;      // gX of the wave's rows: features [0, 32) and [32, 64)
  gx0.clear(), gx1.clear();
  auto flush = [&]() {      // (uniform over the workgroup)
#pragma unroll
    for (int turn = 0; turn < 2; ++turn) {
      if (wc == turn) {
#pragma unroll
        for (int v = 0; v < 16; ++v) {
          const int r = wr * GPD_SUB + GpdFrag<T>::row(v, lane), d = GpdFrag<T>::col(v, lane);
          if (d < D) acc[r * D + d] += (double)gx0.get(v);
          if (d + GPD_SUB < D) acc[r * D + d + GPD_SUB] += (double)gx1.get(v);
        }
      }
      __syncthreads();
    }
    gx0.clear(), gx1.clear();
  };
  double s_var = 0.0, s_bias = 0.0;
  int since = 0;
  int64_t ct_end = (int64_t)(split + 1) * a.tiles_per_split;
  if (ct_end > a.col_tiles) ct_end = a.col_tiles;
  for (int64_t ct = (int64_t)split * a.tiles_per_split; ct < ct_end; ++ct) {
    const int64_t j0 = ct * GPK_TILE + wc * GPD_SUB;
    __syncthreads();      // the previous tile's reads of zs are over
    gpd_stage(a.z, ct * GPK_TILE, a.C, D, stride, zs);
    __syncthreads();
    GpdFrag<T> s;
    s.clear();
    gpd_mac_nt(s, xw, zw, stride, kp, lane);
    T w[16], t[16], q[16], t_var = T(0), t_bias = T(0);
#pragma unroll
    for (int v = 0; v < 16; ++v) t[v] = b + s.get(v), q[v] = T(1);
    for (int e = 1; e < a.degree; ++e)      // t^(degree - 1)
#pragma unroll
      for (int v = 0; v < 16; ++v) q[v] *= t[v];
#pragma unroll
    for (int v = 0; v < 16; ++v) {
      const int64_t i = i0 + GpdFrag<T>::row(v, lane), j = j0 + GpdFrag<T>::col(v, lane);
      const T g = (i < a.R && j < a.C) ? a.G[i * a.C + j] : T(0);      // padded entries weigh nothing
      w[v] = g * scale * q[v];
      t_var += g * (q[v] * t[v]);
      t_bias += w[v];
    }
    s_var += (double)t_var, s_bias += (double)t_bias;
    if (a.cols_part && hb < a.half_blocks) {      // (wave-uniform)
      double* rec = a.col_rec + hb * a.C * D;
#pragma unroll
      for (int half = 0; half < 2; ++half) {
        const int d0 = half * GPD_SUB;
        if (d0 >= D) break;
        GpdFrag<T> out;
        out.clear();
        gpd_mac_tn(out, w, xw, stride, d0, D, lane);
#pragma unroll
        for (int v = 0; v < 16; ++v) {
          const int64_t c = j0 + GpdFrag<T>::row(v, lane);
          const int d = d0 + GpdFrag<T>::col(v, lane);
          if (c < a.C && d < D) rec[c * D + d] = (double)out.get(v);
        }
      }
    }
    if (a.rows_part) {      // (uniform over the workgroup)
#pragma unroll
      for (int v = 0; v < 16; ++v) wt[GpdFrag<T>::row(v, lane) * GPD_WT + GpdFrag<T>::col(v, lane)] = w[v];
      __syncthreads();
      gpd_mac_nn(gx0, wt, zw, stride, 0, D, lane);
      if (D > GPD_SUB) gpd_mac_nn(gx1, wt, zw, stride, GPD_SUB, D, lane);
      since += GPK_TILE;
      if (since >= GPD_FLUSH && ct + 1 < ct_end) flush(), since = 0;
    }
  }
  if (a.rows_part) {
    __syncthreads();      // the zeros of acc are in place even where no tile was walked
    flush();
    gp_copy_row_record(acc, a.row_rec, split, a.R, rb * GPK_TILE, D);
  }
  if (a.want_scalars) {
    double* sc = a.sc_rec + (int64_t)blockIdx.x * GPD_SCALARS;
    const double v0 = block_sum_f64_waves(s_var, red, GPK_WAVES);
    const double v1 = block_sum_f64_waves(s_bias, red, GPK_WAVES);
    if (tid == 0) sc[0] = v0, sc[1] = v1;
  }
}

// records -> gradients, float64 sums in a fixed order.  Blocks [0, x_blocks): gx[e] = sum over the splits of the row
// records (+ with z = x the sum over the half row blocks of the cols records); [.., + z_blocks): gz[e] = sum over the
// half row blocks; then one block each for g_variance and g_bias.
template <typename T>
struct GpdFinArgs {
  const double *row_rec, *col_rec, *sc_rec;
  int D, splits, rows_part, sym;
  int64_t R, C, half_blocks, workgroups, x_blocks, z_blocks;
  T *gx, *gz, *g_var, *g_bias;
};

template <typename T>
__global__ __launch_bounds__(GPD_THREADS) void gp_dot_fin_kernel(const GpdFinArgs<T> a) {
  __shared__ double red[GPK_WAVES];
  const int64_t blk = blockIdx.x;
  if (blk < a.x_blocks) {
    const int64_t e = blk * GPD_THREADS + threadIdx.x, total = a.R * a.D;
    if (e >= total) return;
    double s = 0.0;
    if (a.rows_part) s = gp_sum_splits(a.row_rec, a.splits, total, e);
    if (a.sym)
      for (int64_t h = 0; h < a.half_blocks; ++h) s += a.col_rec[h * total + e];
    a.gx[e] = (T)s;
    return;
  }
  if (blk < a.x_blocks + a.z_blocks) {
    const int64_t e = (blk - a.x_blocks) * GPD_THREADS + threadIdx.x, total = a.C * a.D;
    if (e >= total) return;
    double s = 0.0;
    for (int64_t h = 0; h < a.half_blocks; ++h) s += a.col_rec[h * total + e];
    a.gz[e] = (T)s;
    return;
  }
  const int slot = (int)(blk - a.x_blocks - a.z_blocks);      // variance, bias
  T* out = slot == 0 ? a.g_var : a.g_bias;
  if (out == nullptr) return;      // (uniform over the block)
  double s = 0.0;
  for (int64_t w = threadIdx.x; w < a.workgroups; w += GPD_THREADS) s += a.sc_rec[w * GPD_SCALARS + slot];
  s = block_sum_f64_waves(s, red, GPK_WAVES);
  if (threadIdx.x == 0) *out = (T)s;
}

// ---- launchers -------------------------------------------------------------------------------------------------------
template <typename T>
static int gpd_fwd_launch(const void* x, const void* z, const void* variance, const void* bias, int degree, void* K,
                          int64_t N, int64_t M, int D, hipStream_t st) {
  const int64_t col_tiles = gpk_tiles(M), tiles = gpk_tiles(N) * col_tiles;
  PA_REQUIRE(tiles <= GPK_MAX_WORKGROUPS, "pa_gp_dot_fwd: %lld tiles over the grid limit", (long long)tiles);
  return gp_launch("gp_dot_fwd_kernel", gp_dot_fwd_kernel<T>, tiles, GPD_THREADS, gpd_fwd_lds_bytes(D, sizeof(T)), st,
                   (const T*)x, (const T*)(z ? z : x), (const T*)variance, (const T*)bias, degree, (T*)K, N, M, D, col_tiles);
}

struct GpdOut {
  void *gx, *gz, *g_var, *g_bias;
};

template <typename T>
static int gpd_bwd_launch(const GpdPlan& pl, const void* x, const void* z, const void* variance, const void* bias,
                          int degree, const void* G, const GpdOut& o, void* workspace, hipStream_t st) {
  const GpkLaunchPlan& g = pl.grid;
  PA_REQUIRE(g.workgroups <= GPK_MAX_WORKGROUPS, "pa_gp_dot_bwd: %lld workgroups over the grid limit",
             (long long)g.workgroups);
  const bool scalars = o.g_var || o.g_bias;
  GpdBwdArgs<T> a;
  a.x = (const T*)x, a.z = (const T*)(z ? z : x), a.G = (const T*)G, a.variance = (const T*)variance;
  a.bias = (const T*)bias, a.degree = degree, a.D = g.D, a.splits = g.splits, a.rows_part = pl.rows_part ? 1 : 0;
  a.cols_part = pl.cols_part ? 1 : 0, a.want_scalars = scalars ? 1 : 0, a.R = g.rows, a.C = g.cols;
  a.tiles_per_split = g.tiles_per_split, a.col_tiles = g.col_tiles, a.half_blocks = pl.half_blocks;
  a.row_rec = (double*)workspace, a.col_rec = a.row_rec + pl.row_doubles, a.sc_rec = a.col_rec + pl.col_doubles;
  int rc = gp_launch("gp_dot_bwd_kernel", gp_dot_bwd_kernel<T>, g.workgroups, GPD_THREADS, gpd_bwd_lds_bytes(g.D, sizeof(T)),
                     st, a);
  if (rc != PA_OK) return rc;
  GpdFinArgs<T> f;
  f.row_rec = a.row_rec, f.col_rec = a.col_rec, f.sc_rec = a.sc_rec, f.D = g.D, f.splits = g.splits;
  f.rows_part = a.rows_part, f.sym = pl.sym ? 1 : 0, f.R = g.rows, f.C = g.cols, f.half_blocks = pl.half_blocks;
  f.workgroups = g.workgroups;
  f.x_blocks = o.gx ? (g.rows * g.D + GPD_THREADS - 1) / GPD_THREADS : 0;
  f.z_blocks = o.gz ? (g.cols * g.D + GPD_THREADS - 1) / GPD_THREADS : 0;
  f.gx = (T*)o.gx, f.gz = (T*)o.gz, f.g_var = (T*)o.g_var, f.g_bias = (T*)o.g_bias;
  const int64_t blocks = f.x_blocks + f.z_blocks + (scalars ? GPD_SCALARS : 0);
  PA_REQUIRE(blocks <= GPK_MAX_WORKGROUPS, "pa_gp_dot_bwd: finalize grid of %lld blocks", (long long)blocks);
  return gp_launch("gp_dot_fin_kernel", gp_dot_fin_kernel<T>, blocks, GPD_THREADS, 0, st, f);
}

static int gpd_check(const char* who, int dtype, const void* x, const void* z, int degree, int64_t N, int64_t M,
                     int64_t D) {
  PA_REQUIRE(dtype == PA_F32 || dtype == PA_F64, "%s: dtype %d", who, dtype);
  if (!(D >= 1 && D <= GPK_MAX_D && degree >= 1 && degree <= GPD_MAX_DEGREE))
    return fail(PA_ERR_UNSUPPORTED, "%s: D=%lld outside [1, %d] or degree=%d outside [1, %d]", who, (long long)D, GPK_MAX_D,
                degree, GPD_MAX_DEGREE);
  PA_REQUIRE(gpd_shape_ok(N, M, D, degree), "%s: N=%lld M=%lld D=%lld", who, (long long)N, (long long)M, (long long)D);
  PA_REQUIRE(z != nullptr || N == M, "%s: z = x needs M = N, got N=%lld M=%lld", who, (long long)N, (long long)M);
  PA_REQUIRE(N == 0 || x != nullptr, "%s: null input", who);
  return PA_OK;
}

}  // namespace pa

extern "C" {

int pa_gp_dot_fwd(int dtype, const void* x, const void* z, const void* variance, const void* bias, int degree, void* K,
                  int64_t N, int64_t M, int64_t D, pa_stream_t stream) {
  int rc = pa::gpd_check("pa_gp_dot_fwd", dtype, x, z, degree, N, M, D);
  if (rc != PA_OK) return rc;
  if (N == 0 || M == 0) return PA_OK;
  PA_REQUIRE(K != nullptr, "pa_gp_dot_fwd: null output");
  hipStream_t st = pa::as_stream(stream);
  if (dtype == PA_F32) return pa::gpd_fwd_launch<float>(x, z, variance, bias, degree, K, N, M, (int)D, st);
  return pa::gpd_fwd_launch<double>(x, z, variance, bias, degree, K, N, M, (int)D, st);
}

size_t pa_gp_dot_bwd_workspace(int64_t N, int64_t M, int64_t D, int z_null, int want_gx, int want_gz, int forced_splits) {
  if (!pa::gpd_shape_ok(N, M, D, 1) || N == 0 || M == 0) return 0;
  return pa::gpd_plan(N, M, (int)D, z_null != 0, want_gx != 0, want_gz != 0, pa::cu_count(), forced_splits).bytes;
}

int pa_gp_dot_bwd(int dtype, const void* x, const void* z, const void* variance, const void* bias, int degree,
                  const void* G, int64_t N, int64_t M, int64_t D, void* gx, void* gz, void* g_variance, void* g_bias,
                  int forced_splits, void* workspace, size_t workspace_bytes, pa_stream_t stream) {
  int rc = pa::gpd_check("pa_gp_dot_bwd", dtype, x, z, degree, N, M, D);
  if (rc != PA_OK) return rc;
  PA_REQUIRE((g_variance == nullptr || variance != nullptr) && (g_bias == nullptr || bias != nullptr),
             "pa_gp_dot_bwd: a gradient for a parameter that was not given");
  bool launch;
  rc = pa::gp_bwd_preamble("pa_gp_dot_bwd", z, gz, forced_splits, gx || gz || g_variance || g_bias, N, M, G, &launch);
  if (rc != PA_OK || !launch) return rc;
  const pa::GpdPlan pl = pa::gpd_plan(N, M, (int)D, z == nullptr, gx != nullptr, gz != nullptr, pa::cu_count(), forced_splits);
  rc = pa::gp_workspace_check("pa_gp_dot_bwd", workspace, workspace_bytes, pl.bytes);
  if (rc != PA_OK) return rc;
  PA_REQUIRE((pl.row_doubles + pl.col_doubles + pl.scalar_doubles) * sizeof(double) == pl.bytes &&
                 pl.half_blocks * pa::GPD_SUB >= N && pl.grid.row_blocks * 2 >= pl.half_blocks,
             "pa_gp_dot_bwd: inconsistent plan");
  const pa::GpdOut o = {gx, gz, g_variance, g_bias};
  hipStream_t st = pa::as_stream(stream);
  if (dtype == PA_F32) return pa::gpd_bwd_launch<float>(pl, x, z, variance, bias, degree, G, o, workspace, st);
  return pa::gpd_bwd_launch<double>(pl, x, z, variance, bias, degree, G, o, workspace, st);
}

}  // extern "C"
