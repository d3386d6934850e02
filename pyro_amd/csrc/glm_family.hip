// glm_family.hip -- fused plated regression sites beyond Bernoulli: Normal, StudentT, Poisson (log link) and
// Binomial (logit link) likelihoods of a linear predictor, forward + gradient in one pass over X.
//
// Reference path replaced (per ELBO-gradient step, P vectorised particles, plate size N):
//   eta = w @ X^T + b                                      (user model, torch matmul)
//   Normal(eta, sigma) / StudentT(nu, eta, sigma) / Poisson(exp(eta)) / Binomial(n, logits=eta) .log_prob(y)
//   scale_and_mask, .sum()                                 (pyro/poutine/trace_struct.py:264-278)
//   backward of all of them                                (pyro/infer/trace_elbo.py:153-157)
// which materialises [P,N] predictors / log-probs / grads several times.  Here X, y (and the Binomial counts) are
// read ONCE; nothing of size P*N ever reaches HBM.
//
// The frame is the exact-f32 kernel of glm.hip (glm_bernoulli_kernel, ungrouped), copied: one wavefront owns a
// 32-row tile of X in its private LDS slice (row stride DP + 3: the three spare columns hold y, the mask and the
// Binomial count of the row), GEMM1 is v_mfma_f32_32x32x2_f32 with the W fragments in registers, the family's
// element-wise step runs on the accumulator registers, GEMM2 reads those registers as its A operand, per-workgroup
// partial records are reduced by an fp64 finalize (no float atomics: bit-reproducible).
//
// What the family supplies is GlmFam<FAM>::elem: from (y, n, eta, k_p) the value g' that GEMM2 contracts with X and
// up to two scalars (S0, S1) that are summed per particle.  Every factor that depends on the particle only is kept
// OUT of the f32 loop and applied once, in fp64, by the finalize (GlmFam<FAM>::post):
//   Normal    g' = r = y - eta, S0 = r^2:          s = -S0 / (2 sigma^2), d/d eta = g' / sigma^2, d/d sigma = S0 / sigma^3
//   StudentT  u = r^2 k, k = 1 / (nu sigma^2), g' = r / (1 + u), S0 = log1p(u), S1 = u / (1 + u):
//             s = -(nu + 1)/2 S0, d/d eta = (nu + 1) k g', d/d sigma = (nu + 1) S1 / sigma,
//             d/d nu = -S0 / 2 + (nu + 1) S1 / (2 nu)
//   Poisson   S0 = y eta - exp(eta), g' = y - exp(eta)
//   Binomial  S0 = y eta - n softplus(eta), g' = y - n sigmoid(eta)   (the arithmetic of glm_bernoulli_kernel)
// so a rounded 1 / sigma never multiplies every term of a sum the same way.  The lgamma terms of Poisson / Binomial
// depend on the row only: they are evaluated once per row where y is staged (first particle pass only), summed in
// fp64, and added to every particle's s by the finalize.
#include "common.h"
#include "dist_fam.h"
#include "glm_family_plan.h"

namespace pa {

typedef float glmf_f32x16 __attribute__((ext_vector_type(16)));

template <int DT>
struct GlmFamCfg {
  static constexpr int DP = 32 * DT;      // padded feature count
  static constexpr int S = DP + 3;        // LDS row stride in floats (odd)
  static constexpr int TILE_F = 32 * S;   // floats per wave tile
};

// ---- the families ----------------------------------------------------------------------------------------------
// A: aux columns.  COUNT: the row carries a trial count.  ROW_TERM: the row has a particle-independent term.
// prep(aux_p) -> k_p (f32, rounded once from fp64);  elem(...) -> g', S0, S1 of an UNMASKED element;
// post(aux_p, S0, S1) -> s, the factor of gw / gb, and d s / d aux  (fp64).
template <int FAM> struct GlmFam;

template <> struct GlmFam<PA_GLM_NORMAL> {
  static constexpr int A = 1;
  static constexpr bool COUNT = false, ROW_TERM = false, TWO_SUMS = false;
  static __device__ __forceinline__ float prep(const float*) { return 1.0f; }
  static __device__ __forceinline__ float elem(float y, float, float eta, float, float& s0, float&) {
    const float r = y - eta;
    s0 = r * r;
    return r;
  }
  static __device__ __forceinline__ float row_term(float, float) { return 0.0f; }
  static __device__ __forceinline__ void post(const float* a, double S0, double, double& s, double& fg,
                                              double* ga) {
    const double sg = (double)a[0], is2 = 1.0 / (sg * sg);
    s = -0.5 * S0 * is2;
    fg = is2;
    ga[0] = S0 * is2 / sg;
  }
};

template <> struct GlmFam<PA_GLM_STUDENT_T> {
  static constexpr int A = 2;
  static constexpr bool COUNT = false, ROW_TERM = false, TWO_SUMS = true;
  static __device__ __forceinline__ float prep(const float* a) {
    return (float)(1.0 / ((double)a[0] * (double)a[1] * (double)a[1]));
  }
  static __device__ __forceinline__ float elem(float y, float, float eta, float k, float& s0, float& s1) {
    const float r = y - eta;
    const float u = r * r * k;            // z^2 / nu
    const float iw = 1.0f / (1.0f + u);
    s0 = log1pf(u);
    s1 = u * iw;
    return r * iw;
  }
  static __device__ __forceinline__ float row_term(float, float) { return 0.0f; }
  static __device__ __forceinline__ void post(const float* a, double S0, double S1, double& s, double& fg,
                                              double* ga) {
    const double nu = (double)a[0], sg = (double)a[1];
    s = -0.5 * (nu + 1.0) * S0;
    fg = (nu + 1.0) / (nu * sg * sg);
    ga[0] = -0.5 * S0 + (nu + 1.0) * S1 / (2.0 * nu);
    ga[1] = (nu + 1.0) * S1 / sg;
  }
};

template <> struct GlmFam<PA_GLM_POISSON_LOG> {
  static constexpr int A = 0;
  static constexpr bool COUNT = false, ROW_TERM = true, TWO_SUMS = false;
  static __device__ __forceinline__ float prep(const float*) { return 1.0f; }
  static __device__ __forceinline__ float elem(float y, float, float eta, float, float& s0, float&) {
    const float e = expf(eta);
    s0 = y * eta - e;
    return y - e;
  }
  static __device__ __forceinline__ float row_term(float y, float) { return -t_lgamma(y + 1.0f); }
  static __device__ __forceinline__ void post(const float*, double S0, double, double& s, double& fg, double*) {
    s = S0;
    fg = 1.0;
  }
};

template <> struct GlmFam<PA_GLM_BINOMIAL_LOGITS> {
  static constexpr int A = 0;
  static constexpr bool COUNT = true, ROW_TERM = true, TWO_SUMS = false;
  static __device__ __forceinline__ float prep(const float*) { return 1.0f; }
  static __device__ __forceinline__ float elem(float y, float n, float l, float, float& s0, float&) {
    // the element-wise step of glm_bernoulli_kernel with n in the place of the mask's 1
    const float e = __builtin_amdgcn_exp2f(-1.44269504088896340736f * fabsf(l));
    const float t = 1.0f + e;
    const float lg = 0.69314718055994530942f * __builtin_amdgcn_logf(t);
    const float sp = fmaxf(l, 0.0f) + lg;          // softplus(l)
    const float inv = __builtin_amdgcn_rcpf(t);
    const float sig = l >= 0.0f ? inv : e * inv;   // sigmoid(l)
    s0 = y * l - n * sp;
    return y - n * sig;
  }
  static __device__ __forceinline__ float row_term(float y, float n) {
    return t_lgamma(n + 1.0f) - t_lgamma(y + 1.0f) - t_lgamma(n - y + 1.0f);
  }
  static __device__ __forceinline__ void post(const float*, double S0, double, double& s, double& fg, double*) {
    s = S0;
    fg = 1.0;
  }
};

template <int FAM, int DT, int PT, bool VEC4>
__global__ __launch_bounds__(64 * GLMF_WAVES, DT == 4 ? 1 : 2) void glm_family_kernel(
    const float* __restrict__ X, const float* __restrict__ y, const float* __restrict__ w,
    const float* __restrict__ b, const float* __restrict__ aux, const float* __restrict__ count,
    float count_scalar, const uint8_t* __restrict__ mask, int64_t N, int D, int P, int64_t iters,
    float* __restrict__ part) {
  using C = GlmFamCfg<DT>;
  using F = GlmFam<FAM>;
  constexpr int DP = C::DP, S = C::S, TILE_F = C::TILE_F;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int l31 = lane & 31, h = lane >> 5;
  float* Xs = lds + wave * TILE_F;

  for (int i = threadIdx.x; i < GLMF_WAVES * TILE_F; i += 64 * GLMF_WAVES) lds[i] = 0.0f;

  // ---- W fragments (B operand of GEMM1), bias and the family's per-particle constant: registers -------------
  const int pbase = blockIdx.y * 32 * PT;
  float wf[PT][DP / 2];
  float bias[PT], kc[PT];
#pragma unroll
  for (int pt = 0; pt < PT; ++pt) {
    const int p = pbase + pt * 32 + l31;
#pragma unroll
    for (int kk = 0; kk < DP / 2; ++kk) {
      const int d = 2 * kk + h;
      wf[pt][kk] = (p < P && d < D) ? w[(int64_t)p * D + d] : 0.0f;
    }
    bias[pt] = (p < P && b != nullptr) ? b[p] : 0.0f;
    kc[pt] = (p < P && F::A > 0) ? F::prep(aux + (int64_t)p * F::A) : 1.0f;
  }

  glmf_f32x16 gwacc[PT][DT];
  float s0_acc[PT], s1_acc[PT], gb_acc[PT];
#pragma unroll
  for (int pt = 0; pt < PT; ++pt) {
    s0_acc[pt] = 0.0f;
    s1_acc[pt] = 0.0f;
    gb_acc[pt] = 0.0f;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
      for (int r = 0; r < 16; ++r) gwacc[pt][dt][r] = 0.0f;
  }
  double lg_acc = 0.0, cnt_acc = 0.0;   // row terms and unmasked rows (first particle pass, lanes 0..31)

  // ---- staging registers: the next tile travels global -> VGPR while this one computes (X % 4 == 0 layouts;
  //      the scalar-load layouts would need 16 * DT staging registers per lane and spill: they load in
  //      write_stage itself, with the y / mask / count of the row still prefetched) ----
  constexpr int NLD = VEC4 ? 4 * DT : 16 * DT;  // loads per lane per tile
  constexpr int EPL = VEC4 ? 4 : 1;             // floats per load
  float stage[VEC4 ? NLD * EPL : 1];
  static_assert(NLD <= 64, "one mask bit per staged load");
  uint64_t stage_m = 0;        // bit j: the row of the j-th staged load is unmasked (all set without a mask)
  float st_y = 0.0f, st_m = 0.0f, st_c = 0.0f;
  const int step_e = 64 * EPL;                   // flat-element stride between a lane's loads
  const int q0 = step_e / D, r0 = step_e % D;    // (row, col) increment per load
  const int e0 = lane * EPL;
  const int n_first = e0 / D, d_first = e0 % D;
  const int64_t total_e = N * (int64_t)D;

  // Loads use CLAMPED addresses and are consumed raw; validity is applied in write_stage(), one tile of compute
  // later (a select next to the load makes the compiler wait for it right there).
  auto issue_loads = [&](int64_t tile) {
    if constexpr (VEC4) {
      const int64_t base = tile * 32 * (int64_t)D;  // flat offset of the tile's first element
      int ln = n_first, ld = d_first;               // tile-local (row, col) of the j-th load
      stage_m = 0;
#pragma unroll
      for (int j = 0; j < NLD; ++j) {
        const int64_t e = base + e0 + (int64_t)j * step_e;
        const bool ok = ((e0 + j * step_e) < 32 * D) && (e < total_e);
        const int64_t ec = ok ? e : 0;
        const float4 v = *reinterpret_cast<const float4*>(X + ec);
        stage[4 * j + 0] = v.x; stage[4 * j + 1] = v.y;
        stage[4 * j + 2] = v.z; stage[4 * j + 3] = v.w;
        // a masked row must contribute nothing whatever it holds (where(mask, x, 0),
        // pyro/distributions/util.py:326): its X values are dropped at staging
        const bool keep = (mask != nullptr && ok) ? mask[tile * 32 + ln] != 0 : true;
        stage_m |= (uint64_t)(keep ? 1 : 0) << j;
        ln += q0;
        ld += r0;
        if (ld >= D) { ld -= D; ln += 1; }
      }
    }
    const int64_t n = tile * 32 + l31;
    const int64_t nc = n < N ? n : 0;
    st_y = y[nc];
    st_m = mask == nullptr ? 1.0f : (mask[nc] != 0 ? 1.0f : 0.0f);
    if constexpr (F::COUNT) st_c = count != nullptr ? count[nc] : count_scalar;
  };
  auto write_stage = [&](int64_t tile) {
    const int64_t base = tile * 32 * (int64_t)D;
    int n = n_first, d = d_first;
    if constexpr (VEC4) {
#pragma unroll
      for (int j = 0; j < NLD; ++j) {
        if (e0 + j * step_e < 32 * D) {
          const bool ok = (base + e0 + (int64_t)j * step_e < total_e) && ((stage_m >> j) & 1) != 0;
#pragma unroll
          for (int k = 0; k < EPL; ++k) Xs[n * S + d + k] = ok ? stage[EPL * j + k] : 0.0f;
        }
        n += q0;
        d += r0;
        if (d >= D) { d -= D; n += 1; }
      }
    } else {
#pragma unroll 8
      for (int j = 0; j < NLD; ++j) {
        if (e0 + j * step_e < 32 * D) {
          const int64_t e = base + e0 + (int64_t)j * step_e;
          const bool in = e < total_e;
          const float v = X[in ? e : 0];
          const bool ok = in && (mask == nullptr || mask[tile * 32 + n] != 0);
          Xs[n * S + d] = ok ? v : 0.0f;
        }
        n += q0;
        d += r0;
        if (d >= D) { d -= D; n += 1; }
      }
    }
    if (h == 0) {
      // y and the count of a masked-out (or out-of-range) row are SELECTED away, never multiplied: NaN / inf
      // there contribute exactly 0
      const bool on = (tile * 32 + l31 < N) && st_m != 0.0f;
      Xs[l31 * S + DP] = on ? st_y : 0.0f;
      Xs[l31 * S + DP + 1] = on ? 1.0f : 0.0f;
      if constexpr (F::COUNT) Xs[l31 * S + DP + 2] = on ? st_c : 0.0f;
      if (blockIdx.y == 0) {
        cnt_acc += on ? 1.0 : 0.0;
        if constexpr (F::ROW_TERM) {
          const float rt = F::row_term(st_y, st_c);
          lg_acc += on ? (double)rt : 0.0;
        }
      }
    }
  };

  const int64_t ntiles = (N + 31) / 32;
  int64_t tile = (int64_t)blockIdx.x * GLMF_WAVES + wave;
  const int64_t tile_stride = (int64_t)gridDim.x * GLMF_WAVES;

  // (a tile index at or beyond ntiles: every address is clamped to element 0, every row is off)
  issue_loads(tile);
  __syncthreads();  // LDS zero-fill complete
  write_stage(tile);
  __syncthreads();

  for (int64_t it = 0; it < iters; ++it) {
    const int64_t next = tile + tile_stride;
    if (it + 1 < iters) issue_loads(next);

    if (tile < ntiles) {
      glmf_f32x16 acc[PT];
#pragma unroll
      for (int pt = 0; pt < PT; ++pt)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[pt][r] = 0.0f;

      auto gemm1_step = [&](int pt, int kk) {
        const float a = Xs[l31 * S + 2 * kk + h];
        acc[pt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, wf[pt][kk], acc[pt], 0, 0, 0);
      };
      // element-wise on accumulator register r of particle tile pt (rows nr / nr+4 by lane half)
      auto elementwise = [&](int pt, int r) {
        const int nr = (r & 3) + 8 * (r >> 2) + 4 * h;
        const float yy = Xs[nr * S + DP];
        const bool on = Xs[nr * S + DP + 1] != 0.0f;
        const float nn = F::COUNT ? Xs[nr * S + DP + 2] : 0.0f;
        const float eta = acc[pt][r] + bias[pt];
        float e0v = 0.0f, e1v = 0.0f;
        const float gv = F::elem(yy, nn, eta, kc[pt], e0v, e1v);
        s0_acc[pt] += on ? e0v : 0.0f;
        if constexpr (F::TWO_SUMS) s1_acc[pt] += on ? e1v : 0.0f;
        const float g = on ? gv : 0.0f;
        gb_acc[pt] += g;
        acc[pt][r] = g;
      };
      auto gemm2_step = [&](int pt, int r) {
        const int nr = (r & 3) + 8 * (r >> 2) + 4 * h;
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) {
          const float bf = Xs[nr * S + dt * 32 + l31];
          gwacc[pt][dt] =
              __builtin_amdgcn_mfma_f32_32x32x2f32(acc[pt][r], bf, gwacc[pt][dt], 0, 0, 0);
        }
      };

#pragma unroll
      for (int kk = 0; kk < DP / 2; ++kk) gemm1_step(0, kk);
      if constexpr (PT == 2) {
        static_assert(PT == 1 || DT == 1, "two particle tiles only with one feature tile");
#pragma unroll
        for (int i = 0; i < 16; ++i) {   // GEMM1(tile 1)  ||  element-wise(tile 0)
          gemm1_step(1, i);
          elementwise(0, i);
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {   // GEMM2(tile 0), GEMM2(tile 1)  ||  element-wise(tile 1)
          gemm2_step(0, r);
          elementwise(1, r);
          gemm2_step(1, r);
        }
      } else {
#pragma unroll
        for (int r = 0; r < 16; ++r) {   // GEMM2 of register r  ||  element-wise of register r+1
          elementwise(0, r);
          gemm2_step(0, r);
        }
      }
    }
    // The LDS slice is private to this wave and a wave's DS operations execute in program order, so re-staging
    // needs no workgroup barrier.
    if (it + 1 < iters) write_stage(next);
    tile = next;
  }
  __syncthreads();

  // ---- block reduction over the 4 waves in a fixed order, then one partial record ---------
  constexpr int REC = glmf_record_floats(DT, PT);
  constexpr int GWF = PT * DT * 1024;
  static_assert(GWF + 3 * PT * 64 + 4 * GLMF_WAVES <= GLMF_WAVES * TILE_F, "LDS too small for epilogue");
  float* red = lds;                       // [PT*DT*16][64] accumulator slots
  float* red2 = lds + GWF;                // [3*PT][64] S0 / gb / S1 per-lane slots
  double* red3 = reinterpret_cast<double*>(lds + GWF + 3 * PT * 64);   // [GLMF_WAVES][2] row terms, rows
  {
    const double lgw = wave_sum(lg_acc), cw = wave_sum(cnt_acc);
    if (lane == 0) {
      red3[2 * wave] = lgw;
      red3[2 * wave + 1] = cw;
    }
  }
  for (int wv = 0; wv < GLMF_WAVES; ++wv) {
    if (wave == wv) {
#pragma unroll
      for (int pt = 0; pt < PT; ++pt) {
#pragma unroll
        for (int dt = 0; dt < DT; ++dt)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int idx = ((pt * DT + dt) * 16 + r) * 64 + lane;
            red[idx] = (wv == 0 ? 0.0f : red[idx]) + gwacc[pt][dt][r];
          }
        const int i0 = (3 * pt) * 64 + lane, i1 = (3 * pt + 1) * 64 + lane, i2 = (3 * pt + 2) * 64 + lane;
        red2[i0] = (wv == 0 ? 0.0f : red2[i0]) + s0_acc[pt];
        red2[i1] = (wv == 0 ? 0.0f : red2[i1]) + gb_acc[pt];
        red2[i2] = (wv == 0 ? 0.0f : red2[i2]) + s1_acc[pt];
      }
    }
    __syncthreads();
  }
  float* rec = part + ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * REC;
  for (int i = threadIdx.x; i < GWF; i += 64 * GLMF_WAVES) rec[i] = red[i];
  // fold the two lane halves (n and n+4 rows) of S0 / gb / S1: 32 values per particle tile and sum
  for (int i = threadIdx.x; i < 3 * PT * 32; i += 64 * GLMF_WAVES) {
    const int q = i >> 5, j = i & 31;
    rec[GWF + i] = red2[q * 64 + j] + red2[q * 64 + 32 + j];
  }
  if (threadIdx.x == 0) {
    double lg = 0.0, cn = 0.0;
    for (int wv = 0; wv < GLMF_WAVES; ++wv) {
      lg += red3[2 * wv];
      cn += red3[2 * wv + 1];
    }
    double* ex = reinterpret_cast<double*>(rec + GWF + 3 * PT * 32);   // (REC is a multiple of 32 floats)
    ex[0] = lg;
    ex[1] = cn;
  }
}

// out = scale * post(sum over the workgroups' records), fp64 accumulation in a fixed order (the order of
// glm_finalize.h: thread (j, g) sums records g, g + GROUPS, ...; the groups are then added in increasing order).
// Jobs: gw[P,D], then gb[P], then one per particle that sums S0, S1 and the row sums and writes s, gaux (and cnt).
constexpr int GLMF_FIN_OUT = 8, GLMF_FIN_GROUPS = 32;

template <int FAM, int DT, int PT>
__global__ __launch_bounds__(GLMF_FIN_OUT * GLMF_FIN_GROUPS) void glm_family_finalize_kernel(
    const float* __restrict__ part, int nblocks, int D, int P, double scale, const float* __restrict__ aux,
    float* __restrict__ s, float* __restrict__ gw, float* __restrict__ gb, float* __restrict__ gaux,
    double* __restrict__ cnt) {
  using F = GlmFam<FAM>;
  constexpr int REC = glmf_record_floats(DT, PT);
  constexpr int GWF = PT * DT * 1024;
  __shared__ double sm[4][GLMF_FIN_GROUPS][GLMF_FIN_OUT];
  const int jj = threadIdx.x % GLMF_FIN_OUT, sg = threadIdx.x / GLMF_FIN_OUT;
  const int64_t PD = (int64_t)P * D, J = PD + 2 * (int64_t)P;
  const int64_t j = (int64_t)blockIdx.x * GLMF_FIN_OUT + jj;
  double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
  int kind = -1, p = 0;               // 0: gw entry, 1: gb, 2: the particle's scalars
  if (j < J) {
    int slot;
    if (j < PD) {
      kind = 0;
      p = (int)(j / D);
      const int d = (int)(j % D);
      const int pl = p % (32 * PT), pt = pl >> 5, i = pl & 31, dt = d >> 5, c = d & 31;
      const int hh = (i >> 2) & 1, reg = (i & 3) + 4 * (i >> 3);
      slot = ((pt * DT + dt) * 16 + reg) * 64 + c + 32 * hh;
    } else {
      const int64_t k = j - PD;
      kind = k >= P ? 2 : 1;
      p = (int)(k - (kind == 2 ? (int64_t)P : 0));
      const int pl = p % (32 * PT), pt = pl >> 5, i = pl & 31;
      slot = GWF + (3 * pt + (kind == 1 ? 1 : 0)) * 32 + i;
    }
    const int pass = p / (32 * PT);
    const float* base = part + (int64_t)pass * nblocks * REC;
    for (int blk = sg; blk < nblocks; blk += GLMF_FIN_GROUPS) {
      const float* r = base + (int64_t)blk * REC;
      a0 += (double)r[slot];
      if (kind == 2) {
        a1 += (double)r[slot + 64];                                       // S1: two rows after S0
        const double* ex = reinterpret_cast<const double*>(part + (int64_t)blk * REC + GWF + 3 * PT * 32);
        a2 += ex[0];                                                      // (the first pass's records)
        a3 += ex[1];
      }
    }
  }
  sm[0][sg][jj] = a0;
  sm[1][sg][jj] = a1;
  sm[2][sg][jj] = a2;
  sm[3][sg][jj] = a3;
  __syncthreads();
  if (sg == 0 && j < J) {
    double t0 = 0.0, t1 = 0.0, t2 = 0.0, t3 = 0.0;
#pragma unroll
    for (int k = 0; k < GLMF_FIN_GROUPS; ++k) {
      t0 += sm[0][k][jj];
      t1 += sm[1][k][jj];
      t2 += sm[2][k][jj];
      t3 += sm[3][k][jj];
    }
    const float* ap = F::A > 0 ? aux + (int64_t)p * F::A : nullptr;
    double sv = 0.0, fg = 1.0, ga[2] = {0.0, 0.0};
    if (kind == 2) {
      F::post(ap, t0, t1, sv, fg, ga);
      s[p] = (float)((sv + t2) * scale);
#pragma unroll
      for (int a = 0; a < F::A; ++a) gaux[(int64_t)p * F::A + a] = (float)(ga[a] * scale);
      if (p == 0) cnt[0] = t3;
    } else {
      F::post(ap, 0.0, 0.0, sv, fg, ga);
      const float v = (float)(t0 * scale * fg);
      if (kind == 0) gw[j] = v;
      else gb[p] = v;
    }
  }
}

template <int FAM, int DT, int PT>
static int glm_family_launch(const GlmFamilyPlan& pl, const float* X, const float* y, const float* w,
                             const float* b, const float* aux, const float* count, double count_scalar,
                             const uint8_t* mask, double scale, int64_t N, int D, int P, float* s, float* gw,
                             float* gb, float* gaux, double* cnt, float* part, hipStream_t st) {
  const bool vec4 = (D % 4 == 0) && ((reinterpret_cast<uintptr_t>(X) & 15) == 0);
  dim3 grid((unsigned)pl.nblocks, (unsigned)pl.npass), block(64 * GLMF_WAVES);
  auto k = vec4 ? glm_family_kernel<FAM, DT, PT, true> : glm_family_kernel<FAM, DT, PT, false>;
  if (pl.lds_bytes > 48 * 1024)
    (void)hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)pl.lds_bytes);
  hipLaunchKernelGGL(k, grid, block, pl.lds_bytes, st, X, y, w, b, aux, count, (float)count_scalar, mask, N, D, P,
                     pl.iters, part);
  int rc = check_launch("glm_family_kernel");
  if (rc != PA_OK) return rc;
  const int64_t J = (int64_t)P * D + 2 * (int64_t)P;
  hipLaunchKernelGGL((glm_family_finalize_kernel<FAM, DT, PT>),
                     dim3((unsigned)((J + GLMF_FIN_OUT - 1) / GLMF_FIN_OUT)),
                     dim3(GLMF_FIN_OUT * GLMF_FIN_GROUPS), 0, st, part, pl.nblocks, D, P, scale, aux, s, gw, gb,
                     gaux, cnt);
  return check_launch("glm_family_finalize_kernel");
}

template <int FAM>
static int glm_family_dispatch(const GlmFamilyPlan& pl, const float* X, const float* y, const float* w,
                               const float* b, const float* aux, const float* count, double count_scalar,
                               const uint8_t* mask, double scale, int64_t N, int D, int P, float* s, float* gw,
                               float* gb, float* gaux, double* cnt, float* part, hipStream_t st) {
#define PA_GLMF_CASE(DT_, PT_)                                                                              \
  if (pl.DT == DT_ && pl.PT == PT_)                                                                         \
    return glm_family_launch<FAM, DT_, PT_>(pl, X, y, w, b, aux, count, count_scalar, mask, scale, N, D, P, \
                                            s, gw, gb, gaux, cnt, part, st);
  PA_GLMF_CASE(1, 1)
  PA_GLMF_CASE(1, 2)
  PA_GLMF_CASE(2, 1)
  PA_GLMF_CASE(4, 1)
#undef PA_GLMF_CASE
  return fail(PA_ERR_UNSUPPORTED, "glm_family: no kernel for DT=%d PT=%d", pl.DT, pl.PT);
}

}  // namespace pa

extern "C" {

size_t pa_glm_family_workspace(int family, int64_t N, int64_t D, int64_t P, int max_blocks) {
  if (!pa::glmf_shape_ok(family, N, D, P) || max_blocks < 0) return 0;
  return pa::glmf_plan(N, D, P, pa::cu_count(), max_blocks).workspace_bytes;
}

int pa_glm_family_fwd_bwd(int family, const float* X, const float* y, const float* w, const float* b,
                          const float* aux, const float* count, double count_scalar, const uint8_t* mask,
                          double scale, int64_t N, int64_t D, int64_t P, int max_blocks, float* s, float* gw,
                          float* gb, float* gaux, double* cnt, void* workspace, size_t workspace_bytes,
                          pa_stream_t stream) {
  const int A = pa::glmf_aux_columns(family);
  PA_REQUIRE(A >= 0, "glm_family: unknown family %d", family);
  PA_REQUIRE(N >= 0 && D >= 1 && P >= 1 && max_blocks >= 0,
             "glm_family: bad shape N=%lld D=%lld P=%lld max_blocks=%d", (long long)N, (long long)D,
             (long long)P, max_blocks);
  if (D > 128)
    return pa::fail(PA_ERR_UNSUPPORTED, "glm_family: fused kernel supports D <= 128 (got %lld)", (long long)D);
  PA_REQUIRE(pa::glmf_shape_ok(family, N, D, P), "glm_family: shape too large");
  PA_REQUIRE(w && s && gw && gb && cnt, "glm_family: NULL parameter/output pointer");
  PA_REQUIRE(A == 0 || (aux && gaux), "glm_family: family %d needs aux[P,%d] and gaux", family, A);
  PA_REQUIRE(N == 0 || (X && y), "glm_family: NULL data pointer");
  hipStream_t st = pa::as_stream(stream);
  if (N == 0) {  // empty plate: every sum is 0 (torch: sum over an empty tensor)
    hipError_t e1 = hipMemsetAsync(s, 0, (size_t)P * 4, st);
    hipError_t e2 = hipMemsetAsync(gw, 0, (size_t)P * D * 4, st);
    hipError_t e3 = hipMemsetAsync(gb, 0, (size_t)P * 4, st);
    hipError_t e4 = A > 0 ? hipMemsetAsync(gaux, 0, (size_t)P * A * 4, st) : hipSuccess;
    hipError_t e5 = hipMemsetAsync(cnt, 0, sizeof(double), st);
    if (e1 != hipSuccess || e2 != hipSuccess || e3 != hipSuccess || e4 != hipSuccess || e5 != hipSuccess)
      return pa::fail(PA_ERR_LAUNCH, "glm_family: memset failed");
    return PA_OK;
  }
  const pa::GlmFamilyPlan pl = pa::glmf_plan(N, D, P, pa::cu_count(), max_blocks);
  PA_REQUIRE(workspace && workspace_bytes >= pl.workspace_bytes, "glm_family: workspace too small (%zu < %zu)",
             workspace_bytes, pl.workspace_bytes);
  PA_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 7) == 0, "glm_family: workspace must be 8-byte aligned");
  float* part = (float*)workspace;
#define PA_GLMF_FAMILY(F_)                                                                                       \
  if (family == F_)                                                                                              \
    return pa::glm_family_dispatch<F_>(pl, X, y, w, b, aux, count, count_scalar, mask, scale, N, (int)D, (int)P, \
                                       s, gw, gb, gaux, cnt, part, st);
  PA_GLMF_FAMILY(PA_GLM_NORMAL)
  PA_GLMF_FAMILY(PA_GLM_STUDENT_T)
  PA_GLMF_FAMILY(PA_GLM_POISSON_LOG)
  PA_GLMF_FAMILY(PA_GLM_BINOMIAL_LOGITS)
#undef PA_GLMF_FAMILY
  return pa::fail(PA_ERR_UNSUPPORTED, "glm_family: unknown family %d", family);
}

}  // extern "C"
