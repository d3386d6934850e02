// torch_ops.cpp -- TORCH_LIBRARY registration of the fused GLM site over the extern "C" launchers of
// libpyro_amd.so (include/pyro_amd.h): the ops appear in torch's dispatcher as pyro_amd::*, so that
// torch.jit.trace / torch.compile record them as graph nodes instead of losing the ctypes calls.
//
// Reference seam: pyro/ops/jit.py:104-109 (torch.jit.trace of a loss function over the unconstrained
// parameters) and pyro/infer/trace_elbo.py:162-257 (JitTrace_ELBO.differentiable_loss); the reference
// registers nothing because it has no native ops -- its traced graph is made of ATen nodes.  Here the
// observed GLM site (pyro/poutine/trace_struct.py:264-278 at the Bernoulli-logits site of SURVEY
// 8(d)'s model) is ONE node whose three outputs are the per-particle log-likelihood and its exact
// gradient factors; the autograd formula (registered from Python, pyro_amd/ops/torch_library.py) is a
// second node, pyro_amd::glm_chain.
//
// Host-only C++ (no kernels here): built by csrc/build.py into lib/libpyro_amd_torch.so and loaded
// with torch.ops.load_library.  Device memory comes from torch's allocator, the launches go to
// torch's current stream.
#include <ATen/ATen.h>
#include <c10/hip/HIPStream.h>
#include <torch/library.h>

#include <algorithm>
#include <optional>
#include <tuple>
#include <vector>

#include "pyro_amd.h"

namespace {

void check(int rc, const char* who) {
  TORCH_CHECK(rc == PA_OK, "pyro_amd::", who, ": ", pa_last_error());
}

pa_stream_t current_stream() { return (pa_stream_t)c10::hip::getCurrentHIPStream().stream(); }

const float* f32_ptr(const std::optional<at::Tensor>& t) {
  return t.has_value() && t->defined() ? t->data_ptr<float>() : nullptr;
}

void require_f32_gpu(const at::Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda() && t.scalar_type() == at::kFloat && t.is_contiguous(), "pyro_amd: ", name,
              " must be a contiguous float32 tensor on the GPU");
}

// X[N,D] -> the uint8 plane image of pa_glm_pack_planes
at::Tensor glm_pack_planes(const at::Tensor& X, int64_t format) {
  require_f32_gpu(X, "X");
  TORCH_CHECK(X.dim() == 2, "pyro_amd::glm_pack_planes: X must be [N, D]");
  const int64_t N = X.size(0), D = X.size(1);
  const size_t nbytes = pa_glm_planes_bytes((int)format, N, D);
  TORCH_CHECK(nbytes > 0 || N == 0, "pyro_amd::glm_pack_planes: no plane image for D = ", D);
  at::Tensor out = at::empty({(int64_t)(nbytes < 16 ? 16 : nbytes)}, X.options().dtype(at::kByte));
  check(pa_glm_pack_planes((int)format, X.data_ptr<float>(), N, D, out.data_ptr(), nbytes, current_stream()),
        "glm_pack_planes");
  return out;
}

// (ll, gw, gb, ws): the workspace is an OUTPUT so that the caller can keep it alive -- inside a chained
// tail (pa_chain_begin) the launcher only RECORDS the finalize phase, which reads the partial records
// in ws when the chain is flushed, after this function has returned
std::tuple<at::Tensor, at::Tensor, at::Tensor, at::Tensor> glm_bernoulli_planes(
    const at::Tensor& planes, const at::Tensor& y, const at::Tensor& w,
    const std::optional<at::Tensor>& b, double scale, int64_t N, int64_t D, int64_t format,
    const std::optional<at::Tensor>& moments) {
  require_f32_gpu(y, "y");
  require_f32_gpu(w, "w");
  TORCH_CHECK(planes.is_cuda() && planes.scalar_type() == at::kByte, "pyro_amd: planes must be a uint8 image");
  TORCH_CHECK(w.dim() == 2 && w.size(1) == D && y.dim() == 1 && y.size(0) == N,
              "pyro_amd::glm_bernoulli_planes: shapes y[N], w[P, D]");
  const int64_t P = w.size(0);
  if (b.has_value() && b->defined()) {
    require_f32_gpu(*b, "b");
    TORCH_CHECK(b->numel() == P, "pyro_amd::glm_bernoulli_planes: b[P]");
  }
  const size_t ws_bytes = pa_glm_bernoulli_planes_workspace(N, D, P);
  TORCH_CHECK(ws_bytes > 0, "pyro_amd::glm_bernoulli_planes: unsupported shape");
  at::Tensor ws = at::empty({(int64_t)ws_bytes}, w.options().dtype(at::kByte));
  at::Tensor ll = at::empty({P}, w.options()), gw = at::empty({P, D}, w.options()),
             gb = at::empty({P}, w.options());
  const double* mom = nullptr;          // pa_glm_label_moments of (X, y), float64[33] (or none)
  if (moments.has_value() && moments->defined()) {
    TORCH_CHECK(moments->is_cuda() && moments->scalar_type() == at::kDouble && moments->numel() == 33 &&
                    moments->is_contiguous(), "pyro_amd::glm_bernoulli_planes: moments = float64[33]");
    mom = moments->data_ptr<double>();
  }
  check(pa_glm_bernoulli_planes_fwd_bwd((int)format, planes.data_ptr(), y.data_ptr<float>(),
                                        w.data_ptr<float>(), f32_ptr(b), scale, N, D, P,
                                        ll.data_ptr<float>(), gw.data_ptr<float>(), gb.data_ptr<float>(),
                                        ws.data_ptr(), ws_bytes, mom, current_stream()),
        "glm_bernoulli_planes");
  return {ll, gw, gb, ws};
}

std::tuple<at::Tensor, at::Tensor, at::Tensor, at::Tensor> glm_bernoulli(
    const at::Tensor& X, const at::Tensor& y, const at::Tensor& w, const std::optional<at::Tensor>& b,
    const std::optional<at::Tensor>& mask, double scale) {
  require_f32_gpu(X, "X");
  require_f32_gpu(y, "y");
  require_f32_gpu(w, "w");
  TORCH_CHECK(X.dim() == 2 && w.dim() == 2 && w.size(1) == X.size(1) && y.dim() == 1 && y.size(0) == X.size(0),
              "pyro_amd::glm_bernoulli: shapes X[N, D], y[N], w[P, D]");
  const int64_t N = X.size(0), D = X.size(1), P = w.size(0);
  const uint8_t* m = nullptr;
  if (mask.has_value() && mask->defined()) {
    TORCH_CHECK(mask->is_cuda() && mask->is_contiguous() && mask->numel() == N &&
                    (mask->scalar_type() == at::kBool || mask->scalar_type() == at::kByte),
                "pyro_amd::glm_bernoulli: mask[N] bool");
    m = (const uint8_t*)mask->data_ptr();
  }
  if (b.has_value() && b->defined()) require_f32_gpu(*b, "b");
  const size_t ws_bytes = pa_glm_bernoulli_workspace(N, D, P);
  TORCH_CHECK(ws_bytes > 0, "pyro_amd::glm_bernoulli: unsupported shape");
  at::Tensor ws = at::empty({(int64_t)ws_bytes}, w.options().dtype(at::kByte));
  at::Tensor ll = at::empty({P}, w.options()), gw = at::empty({P, D}, w.options()),
             gb = at::empty({P}, w.options());
  check(pa_glm_bernoulli_fwd_bwd(X.data_ptr<float>(), y.data_ptr<float>(), w.data_ptr<float>(), f32_ptr(b),
                                 m, scale, N, D, P, ll.data_ptr<float>(), gw.data_ptr<float>(),
                                 gb.data_ptr<float>(), ws.data_ptr(), ws_bytes, current_stream()),
        "glm_bernoulli");
  return {ll, gw, gb, ws};
}

// (g[P] * gw[P, W], g[P] * gb[P]): the backward of the site
std::tuple<at::Tensor, at::Tensor> glm_chain(const at::Tensor& g, const at::Tensor& gw, const at::Tensor& gb) {
  require_f32_gpu(gw, "gw");
  require_f32_gpu(gb, "gb");
  at::Tensor gc = g.reshape({-1}).contiguous();
  const int64_t P = gc.numel();
  TORCH_CHECK(gc.scalar_type() == at::kFloat && gw.size(0) == P && gb.numel() == P, "pyro_amd::glm_chain: shapes");
  const int64_t W = P > 0 ? gw.numel() / P : 0;
  at::Tensor dw = at::empty_like(gw), db = at::empty_like(gb);
  check(pa_glm_chain(gc.data_ptr<float>(), gw.data_ptr<float>(), gb.data_ptr<float>(), P, W,
                     dw.data_ptr<float>(), db.data_ptr<float>(), current_stream()),
        "glm_chain");
  return {dw, db};
}

// pa_adam_step over the flat parameter buffer (pyro/optim/optim.py:117-155 + clipped_adam.py:52-100 +
// pyro/infer/util.py:85-91 zero_grads in one launch); every tensor argument is updated in place
void adam_step(at::Tensor param, at::Tensor grad, at::Tensor exp_avg, at::Tensor exp_avg_sq, at::Tensor step,
               double lr, double beta1, double beta2, double eps, double weight_decay, double clip_norm,
               double lrd, bool clipped, bool zero_grad) {
  TORCH_CHECK(param.is_cuda() && param.is_contiguous() && grad.is_contiguous() && exp_avg.is_contiguous() &&
                  exp_avg_sq.is_contiguous(), "pyro_amd::adam_step: contiguous GPU buffers");
  TORCH_CHECK(param.scalar_type() == at::kFloat || param.scalar_type() == at::kDouble,
              "pyro_amd::adam_step: float32 / float64");
  TORCH_CHECK(grad.scalar_type() == param.scalar_type() && exp_avg.scalar_type() == param.scalar_type() &&
                  exp_avg_sq.scalar_type() == param.scalar_type() && grad.numel() == param.numel() &&
                  exp_avg.numel() == param.numel() && exp_avg_sq.numel() == param.numel(),
              "pyro_amd::adam_step: param / grad / moments of one dtype and size");
  TORCH_CHECK(step.is_cuda() && step.scalar_type() == at::kLong && step.numel() == 2,
              "pyro_amd::adam_step: step = int64[2] {step counter, ticket}");
  check(pa_adam_step(param.scalar_type() == at::kFloat ? PA_F32 : PA_F64, param.data_ptr(), grad.data_ptr(),
                     exp_avg.data_ptr(), exp_avg_sq.data_ptr(), param.numel(), lr, beta1, beta2, eps,
                     weight_decay, clip_norm, lrd, clipped ? 1 : 0, step.data_ptr<int64_t>(), zero_grad ? 1 : 0,
                     current_stream()),
        "adam_step");
}


// ---- typed ops for the rest of a step (round 6): the operations a Pyro maintainer would bind first, with real
//      argument lists -- loadable from C++ / TorchScript, readable in a traced graph.  (Python keeps a generic
//      (Tensor[] tensors, int spec) trampoline for the remaining autograd Functions: ops/torch_library.py.)

int dtype_of(const at::Tensor& t, const char* who) {
  TORCH_CHECK(t.is_cuda() && (t.scalar_type() == at::kFloat || t.scalar_type() == at::kDouble), "pyro_amd::", who,
              ": float32 / float64 tensors on the GPU");
  return t.scalar_type() == at::kFloat ? PA_F32 : PA_F64;
}

// an operand of a site as a strided [rows, cols] view of the value's frame: a scalar, the full frame (contiguous),
// one row [cols] / [1, cols] or one column [rows, 1] -- ExpandedDistribution's stride-0 views
// (pyro/distributions/torch_distribution.py:483-488) without materialising them
pa_view2d view2d(const std::optional<at::Tensor>& t, int64_t rows, int64_t cols, at::ScalarType st, const char* who) {
  pa_view2d v{nullptr, 0, 0};
  if (!t.has_value() || !t->defined()) return v;
  TORCH_CHECK(t->is_cuda() && t->scalar_type() == st, "pyro_amd::", who, ": operand dtype / device");
  v.ptr = t->data_ptr();
  const int64_t n = t->numel();
  if (n == 1) return v;
  TORCH_CHECK(t->is_contiguous(), "pyro_amd::", who, ": operands must be contiguous");
  if (n == rows * cols) { v.stride_row = cols; v.stride_col = 1; }
  else if (n == cols && (t->dim() <= 1 || t->size(-1) == cols)) { v.stride_col = 1; }
  else if (n == rows) { v.stride_row = 1; }
  else TORCH_CHECK(false, "pyro_amd::", who, ": operand of ", n, " elements does not broadcast to [", rows, ", ", cols, "]");
  return v;
}

void frame_of(const at::Tensor& value, int64_t* rows, int64_t* cols) {
  *cols = value.dim() == 0 ? 1 : value.size(-1);
  *rows = *cols > 0 ? value.numel() / *cols : 0;
}

// site["fn"].log_prob(value) -> scale_and_mask -> sum over the last dim (+ the grand total):
// pyro/poutine/trace_struct.py:264-278, pyro/distributions/util.py:311-328
std::tuple<at::Tensor, at::Tensor> dist_log_prob_sum(int64_t dist, const at::Tensor& value,
                                                     const std::optional<at::Tensor>& p0,
                                                     const std::optional<at::Tensor>& p1,
                                                     const std::optional<at::Tensor>& mask, double scale) {
  const int dt = dtype_of(value, "dist_log_prob_sum");
  TORCH_CHECK(value.is_contiguous(), "pyro_amd::dist_log_prob_sum: contiguous value");
  int64_t rows, cols;
  frame_of(value, &rows, &cols);
  const auto st = value.scalar_type();
  std::optional<at::Tensor> val = value;
  const size_t ws_bytes = pa_dist_log_prob_sum_workspace(rows, cols);
  at::Tensor ws = at::empty({(int64_t)(ws_bytes < 16 ? 16 : ws_bytes)}, value.options().dtype(at::kByte));
  at::Tensor rowsum = at::empty({rows}, value.options()), total = at::empty({}, value.options());
  pa_view2d m{nullptr, 0, 0};
  if (mask.has_value() && mask->defined()) {
    TORCH_CHECK(mask->scalar_type() == at::kBool || mask->scalar_type() == at::kByte, "pyro_amd::dist_log_prob_sum: bool mask");
    m = view2d(mask, rows, cols, mask->scalar_type(), "dist_log_prob_sum");
  }
  check(pa_dist_log_prob_sum((int)dist, dt, rowsum.data_ptr(), total.data_ptr(),
                             view2d(val, rows, cols, st, "dist_log_prob_sum"),
                             view2d(p0, rows, cols, st, "dist_log_prob_sum"),
                             view2d(p1, rows, cols, st, "dist_log_prob_sum"), m, scale, rows, cols, ws.data_ptr(),
                             ws_bytes, current_stream()),
        "dist_log_prob_sum");
  return {rowsum, total};
}

// the ELBO assembly of Trace_ELBO in one launch: sum_i coef[i] * sum(log_prob_i) (pyro/infer/trace_elbo.py:
// 82-112, trace_struct.py:248-288); entries beyond PA_MULTI_MAX_ENTRIES are chained with accumulate = 1
at::Tensor multi_log_prob_sum(at::IntArrayRef dist, at::TensorList value, const c10::List<std::optional<at::Tensor>>& p0,
                              const c10::List<std::optional<at::Tensor>>& p1, at::ArrayRef<double> coef,
                              double coef_all) {
  const size_t n = value.size();
  TORCH_CHECK(n >= 1 && dist.size() == n && p0.size() == n && p1.size() == n && coef.size() == n,
              "pyro_amd::multi_log_prob_sum: one dist / p0 / p1 / coef per value");
  const int dt = dtype_of(value[0], "multi_log_prob_sum");
  at::Tensor total = at::zeros({}, value[0].options());
  std::vector<pa_site_entry> e(n);
  for (size_t i = 0; i < n; ++i) {
    TORCH_CHECK(value[i].scalar_type() == value[0].scalar_type() && value[i].is_contiguous(),
                "pyro_amd::multi_log_prob_sum: values of one dtype, contiguous");
    pa_site_entry& s = e[i];
    s = pa_site_entry{};
    s.dist = (int32_t)dist[i];
    frame_of(value[i], &s.rows, &s.cols);
    TORCH_CHECK(s.rows * s.cols <= PA_MULTI_MAX_ELEMS, "pyro_amd::multi_log_prob_sum: a site of more than ",
                PA_MULTI_MAX_ELEMS, " elements goes through dist_log_prob_sum");
    const auto st = value[i].scalar_type();
    std::optional<at::Tensor> v = value[i], a = p0.get(i), b = p1.get(i);
    s.value = view2d(v, s.rows, s.cols, st, "multi_log_prob_sum");
    s.p0 = view2d(a, s.rows, s.cols, st, "multi_log_prob_sum");
    s.p1 = view2d(b, s.rows, s.cols, st, "multi_log_prob_sum");
    s.mask = pa_view2d{nullptr, 0, 0};
    s.coef = coef[i];
    s.chain_next = -1;
  }
  for (size_t at_ = 0; at_ < n; at_ += PA_MULTI_MAX_ENTRIES) {
    const int k = (int)std::min<size_t>(PA_MULTI_MAX_ENTRIES, n - at_);
    check(pa_multi_log_prob_sum(dt, total.data_ptr(), e.data() + at_, k, coef_all, at_ == 0 ? 0 : 1, current_stream()),
          "multi_log_prob_sum");
  }
  return total;
}

// AutoNormal's draw of every latent site in one launch (pyro/infer/autoguide/guides.py:415-603):
// z_s = loc_s + softplus(rho_s) eps_s, eps from the keyed Philox stream at offsets[s] (+ *offset_dev)
std::tuple<std::vector<at::Tensor>, std::vector<at::Tensor>, std::vector<at::Tensor>> meanfield_normal_sample(
    at::TensorList loc, at::TensorList rho, int64_t P, int64_t seed, at::IntArrayRef offsets,
    const std::optional<at::Tensor>& offset_dev) {
  const size_t n = loc.size();
  TORCH_CHECK(n >= 1 && n <= PA_MF_MAX_SITES && rho.size() == n && offsets.size() == n && P >= 1,
              "pyro_amd::meanfield_normal_sample: 1..", PA_MF_MAX_SITES, " sites, one rho / offset per loc");
  const int dt = dtype_of(loc[0], "meanfield_normal_sample");
  std::vector<at::Tensor> z(n), scale(n), eps(n), loc_out(n);
  std::vector<pa_mf_site> s(n);
  for (size_t i = 0; i < n; ++i) {
    TORCH_CHECK(loc[i].scalar_type() == loc[0].scalar_type() && rho[i].scalar_type() == loc[0].scalar_type() &&
                    loc[i].is_contiguous() && rho[i].is_contiguous() && rho[i].numel() == loc[i].numel(),
                "pyro_amd::meanfield_normal_sample: loc / rho of one dtype and size per site");
    const int64_t m = loc[i].numel();
    z[i] = at::empty({P, m}, loc[i].options());
    eps[i] = at::empty({P, m}, loc[i].options());
    scale[i] = at::empty({m}, loc[i].options());
    loc_out[i] = at::empty({m}, loc[i].options());
    s[i] = pa_mf_site{};
    s[i].loc = loc[i].data_ptr(); s[i].rho = rho[i].data_ptr();
    s[i].z = z[i].data_ptr(); s[i].scale = scale[i].data_ptr(); s[i].loc_out = loc_out[i].data_ptr();
    s[i].eps = eps[i].data_ptr();
    s[i].n = m; s[i].offset = (uint64_t)offsets[i];
  }
  const uint64_t* od = nullptr;
  if (offset_dev.has_value() && offset_dev->defined()) {
    TORCH_CHECK(offset_dev->is_cuda() && offset_dev->scalar_type() == at::kLong, "pyro_amd::meanfield_normal_sample: offset_dev int64");
    od = (const uint64_t*)offset_dev->data_ptr();
  }
  check(pa_meanfield_normal_sample(dt, s.data(), (int)n, P, (uint64_t)seed, od, current_stream()), "meanfield_normal_sample");
  return {z, scale, eps};
}

// a positive-support latent under AutoNormal in one launch: value = lower + exp(u) and the Delta site's
// log-density -sum_c u (pyro/infer/autoguide/guides.py:494-519; biject_to(positive / greater_than))
std::tuple<at::Tensor, at::Tensor> exp_site(const at::Tensor& u, double lower) {
  const int dt = dtype_of(u, "exp_site");
  TORCH_CHECK(u.is_contiguous(), "pyro_amd::exp_site: contiguous u");
  int64_t rows, cols;
  frame_of(u, &rows, &cols);
  at::Tensor value = at::empty_like(u), ld = at::empty({rows}, u.options());
  check(pa_exp_site_fwd(dt, u.data_ptr(), rows, cols, lower, value.data_ptr(), ld.data_ptr(), current_stream()), "exp_site");
  return {value, ld};
}

at::Tensor exp_site_bwd(const at::Tensor& value, const std::optional<at::Tensor>& g_value,
                        const std::optional<at::Tensor>& g_log_density, double lower) {
  const int dt = dtype_of(value, "exp_site_bwd");
  int64_t rows, cols;
  frame_of(value, &rows, &cols);
  at::Tensor g_u = at::empty_like(value);
  check(pa_exp_site_bwd(dt, value.data_ptr(), g_value.has_value() && g_value->defined() ? g_value->data_ptr() : nullptr,
                        g_log_density.has_value() && g_log_density->defined() ? g_log_density->data_ptr() : nullptr,
                        rows, cols, lower, g_u.data_ptr(), current_stream()),
        "exp_site_bwd");
  return g_u;
}

// AutoMultivariateNormal's draw: z = loc + (softplus(rho) (*) tril(A)) eps and log q(z), all particles
// (pyro/infer/autoguide/guides.py:820-905)
std::tuple<at::Tensor, at::Tensor, at::Tensor> mvn_tril_sample(const at::Tensor& loc, const at::Tensor& rho,
                                                               const at::Tensor& A, int64_t P, int64_t seed,
                                                               int64_t offset, const std::optional<at::Tensor>& offset_dev) {
  const int dt = dtype_of(loc, "mvn_tril_sample");
  const int64_t n = loc.numel();
  TORCH_CHECK(rho.numel() == n && A.numel() == n * n && loc.is_contiguous() && rho.is_contiguous() && A.is_contiguous() &&
                  rho.scalar_type() == loc.scalar_type() && A.scalar_type() == loc.scalar_type() && P >= 1,
              "pyro_amd::mvn_tril_sample: loc[n], rho[n], A[n, n] of one dtype");
  at::Tensor eps = at::empty({P, n}, loc.options()), z = at::empty({P, n}, loc.options()), logq = at::empty({P}, loc.options());
  const uint64_t* od = nullptr;
  if (offset_dev.has_value() && offset_dev->defined()) od = (const uint64_t*)offset_dev->data_ptr();
  check(pa_mvn_tril_sample(dt, loc.data_ptr(), rho.data_ptr(), A.data_ptr(), n, P, (uint64_t)seed, (uint64_t)offset, od,
                           0, eps.data_ptr(), z.data_ptr(), logq.data_ptr(), current_stream()),
        "mvn_tril_sample");
  return {eps, z, logq};
}

// one elimination step of the plated sum-product: out = logsumexp over frame dim rdim of the sum of the terms,
// each term EXPANDED (stride 0) to the frame `sizes` (pyro/ops/contract.py:79-160, pyro/ops/einsum/torch_log.py:14-55)
at::Tensor logsumexp_terms(at::TensorList terms, at::IntArrayRef sizes, int64_t rdim) {
  const int nd = (int)sizes.size(), nt = (int)terms.size();
  TORCH_CHECK(nt >= 1 && nt <= PA_LSE_MAX_TERMS && nd >= 1 && nd <= PA_LSE_MAX_DIMS && rdim >= 0 && rdim < nd,
              "pyro_amd::logsumexp_terms: 1..", PA_LSE_MAX_TERMS, " terms over a frame of 1..", PA_LSE_MAX_DIMS, " dims");
  const int dt = dtype_of(terms[0], "logsumexp_terms");
  pa_lse_term t[PA_LSE_MAX_TERMS];
  std::vector<at::Tensor> keep;
  for (int k = 0; k < nt; ++k) {
    at::Tensor e = terms[k].expand(sizes);          // (a view: stride 0 where the term does not depend on a dim)
    TORCH_CHECK(e.scalar_type() == terms[0].scalar_type() && e.is_cuda(), "pyro_amd::logsumexp_terms: one dtype");
    t[k].ptr = e.data_ptr();
    for (int d = 0; d < PA_LSE_MAX_DIMS; ++d) t[k].strides[d] = d < nd ? (sizes[d] == 1 ? 0 : e.stride(d)) : 0;
    keep.push_back(e);
  }
  std::vector<int64_t> kept;
  for (int d = 0; d < nd; ++d) if (d != rdim) kept.push_back(sizes[d]);
  at::Tensor out = at::empty(kept, terms[0].options());
  check(pa_logsumexp_terms(dt, out.data_ptr(), nt, t, nd, sizes.data(), (int)rdim, current_stream()), "logsumexp_terms");
  return out;
}

// a chain of T enumerated variables with K states summed out for every batch element: log Z and its gradient
// (the unary / pairwise posteriors) in one launch (pyro/ops/contract.py:79-160 applied T times under pyro.markov;
// pyro/distributions/hmm.py:_sequential_logmatmulexp)
std::tuple<at::Tensor, at::Tensor, at::Tensor> logchain(const at::Tensor& unary, const at::Tensor& pairwise) {
  const int dt = dtype_of(unary, "logchain");
  TORCH_CHECK(unary.dim() == 3 && unary.is_contiguous() && pairwise.is_contiguous() && pairwise.scalar_type() == unary.scalar_type(),
              "pyro_amd::logchain: unary [B, T, K] contiguous, pairwise [B | 1, T - 1 | 1, K, K] contiguous");
  const int64_t B = unary.size(0), T = unary.size(1), K = unary.size(2);
  TORCH_CHECK(pairwise.dim() == 4 && pairwise.size(2) == K && pairwise.size(3) == K &&
                  (pairwise.size(0) == B || pairwise.size(0) == 1) && (pairwise.size(1) == T - 1 || pairwise.size(1) == 1),
              "pyro_amd::logchain: pairwise [B | 1, T - 1 | 1, K, K]");
  const int64_t sb = pairwise.size(0) == 1 ? 0 : pairwise.stride(0), ss = pairwise.size(1) == 1 ? 0 : pairwise.stride(1);
  const size_t ws_bytes = pa_logchain_workspace(dt, B, T, K);
  at::Tensor ws = at::empty({(int64_t)(ws_bytes < 16 ? 16 : ws_bytes)}, unary.options().dtype(at::kByte));
  at::Tensor log_z = at::empty({B}, unary.options()), gu = at::empty_like(unary),
             gp = at::zeros({B, T > 1 ? T - 1 : 0, K, K}, unary.options());
  check(pa_logchain_fwd_bwd(dt, unary.data_ptr(), pairwise.data_ptr(), sb, ss, B, T, K, log_z.data_ptr(), gu.data_ptr(),
                            gp.data_ptr(), ws.data_ptr(), ws_bytes, current_stream()),
        "logchain");
  return {log_z, gu, gp};
}

// a linear-Gaussian state-space model filtered and (with need_grads) smoothed in one launch: log p(x) per sequence, the
// filtered moments of the final state and the nine gradients of log_prob[b] (pyro/distributions/hmm.py:434-741
// GaussianHMM.log_prob / .filter over pyro/ops/gaussian.py sequential_gaussian_tensordot).  Layouts as
// kernels.gaussian_hmm_fwd_bwd: m0 [B | 1, h], P0 [B | 1, h, h], the six others [B | 1, T | 1, ...], x [B, T, o];
// grads: empty without need_grads, else in the order of the arguments (a step axis of 1 is already summed, a batch
// axis that the parameter shares is not)
struct GhmmLayout {
  int dt;
  int64_t B, T, h, o, sb[8], ss[8], steps[8];
};
// (``like``: the tensor whose dtype the parameters share -- the data, or the noise of an entry point without data)
GhmmLayout gaussian_hmm_param_layout(const at::Tensor* const* p, const at::Tensor& like, int64_t B_, int64_t T_,
                                     int64_t o_) {
  GhmmLayout l;
  l.dt = dtype_of(like, "gaussian_hmm");
  const at::Tensor& x = like;
  const at::Tensor& m0 = *p[0];
  TORCH_CHECK(m0.dim() == 2, "pyro_amd::gaussian_hmm: m0 [B | 1, hidden]");
  const int64_t B = l.B = B_, T = l.T = T_, o = l.o = o_, h = l.h = m0.size(1);
  const std::vector<int64_t> ev[8] = {{h}, {h, h}, {h, h}, {h}, {h, h}, {h, o}, {o}, {o, o}};
  int64_t(&sb)[8] = l.sb, (&ss)[8] = l.ss, (&steps)[8] = l.steps;
  for (int i = 0; i < 8; ++i) {
    const at::Tensor& t = *p[i];
    const int64_t lead = i < 2 ? 1 : 2, nd = lead + (int64_t)ev[i].size();
    TORCH_CHECK(t.is_cuda() && t.scalar_type() == x.scalar_type() && t.is_contiguous() && t.dim() == nd,
                "pyro_amd::gaussian_hmm: parameter ", i, ": a contiguous tensor of x's dtype with ", nd, " dims");
    int64_t n = 1;
    for (size_t d = 0; d < ev[i].size(); ++d) {
      TORCH_CHECK(t.size(lead + (int64_t)d) == ev[i][d], "pyro_amd::gaussian_hmm: parameter ", i, " has a wrong event shape");
      n *= ev[i][d];
    }
    TORCH_CHECK((t.size(0) == 1 || t.size(0) == B) && (i < 2 || t.size(1) == 1 || t.size(1) == T),
                "pyro_amd::gaussian_hmm: parameter ", i, ": leading dims [B | 1, T | 1]");
    steps[i] = i < 2 ? 1 : t.size(1);
    sb[i] = t.size(0) == 1 ? 0 : steps[i] * n;
    ss[i] = steps[i] == 1 ? 0 : n;
  }
  return l;
}
GhmmLayout gaussian_hmm_layout(const at::Tensor* const* p, const at::Tensor& x) {
  TORCH_CHECK(x.dim() == 3 && x.is_contiguous(), "pyro_amd::gaussian_hmm: x [B, T, obs] contiguous, m0 [B | 1, hidden]");
  return gaussian_hmm_param_layout(p, x, x.size(0), x.size(1), x.size(2));
}

std::tuple<at::Tensor, at::Tensor, at::Tensor, std::vector<at::Tensor>> gaussian_hmm(
    const at::Tensor& m0, const at::Tensor& P0, const at::Tensor& trans, const at::Tensor& trans_loc,
    const at::Tensor& trans_cov, const at::Tensor& obs, const at::Tensor& obs_loc, const at::Tensor& obs_cov,
    const at::Tensor& x, bool need_grads) {
  const at::Tensor* p[8] = {&m0, &P0, &trans, &trans_loc, &trans_cov, &obs, &obs_loc, &obs_cov};
  const GhmmLayout l = gaussian_hmm_layout(p, x);
  const int dt = l.dt;
  const int64_t B = l.B, T = l.T, h = l.h, o = l.o;
  const int64_t(&sb)[8] = l.sb, (&ss)[8] = l.ss, (&steps)[8] = l.steps;
  const auto opt = x.options();
  at::Tensor log_prob = at::empty({B}, opt), fm = at::empty({B, h}, opt), fP = at::empty({B, h, h}, opt);
  std::vector<at::Tensor> g;
  if (need_grads) {
    g = {at::empty({B, h}, opt), at::empty({B, h, h}, opt), at::empty({B, steps[2], h, h}, opt),
         at::empty({B, steps[3], h}, opt), at::empty({B, steps[4], h, h}, opt), at::empty({B, steps[5], h, o}, opt),
         at::empty({B, steps[6], o}, opt), at::empty({B, steps[7], o, o}, opt), at::empty({B, T, o}, opt)};
  }
  auto gp = [&](int i) { return need_grads ? g[i].data_ptr() : nullptr; };
  const size_t ws_bytes = pa_gaussian_hmm_workspace(dt, B, T, h, o, need_grads ? 1 : 0);
  at::Tensor ws = at::empty({(int64_t)(ws_bytes < 16 ? 16 : ws_bytes)}, opt.dtype(at::kByte));
  check(pa_gaussian_hmm_fwd_bwd(dt, m0.data_ptr(), sb[0], P0.data_ptr(), sb[1], trans.data_ptr(), sb[2], ss[2],
                                trans_loc.data_ptr(), sb[3], ss[3], trans_cov.data_ptr(), sb[4], ss[4], obs.data_ptr(),
                                sb[5], ss[5], obs_loc.data_ptr(), sb[6], ss[6], obs_cov.data_ptr(), sb[7], ss[7],
                                x.data_ptr(), B, T, h, o, log_prob.data_ptr(), fm.data_ptr(), fP.data_ptr(), gp(0), gp(1),
                                gp(2), gp(3), gp(4), gp(5), gp(6), gp(7), gp(8), ws.data_ptr(), ws_bytes,
                                current_stream()),
        "gaussian_hmm");
  return {log_prob, fm, fP, g};
}

// that model with every covariance divided by one s ~ Gamma(concentration, rate) per sequence, a jointly Student-t series
// (pyro/distributions/hmm.py:744-940 GammaGaussianHMM.log_prob / .filter): the filter at unit scale and the adjoint sweep
// in one launch.  concentration, rate [B | 1]; the rest as above -> quad [B], logdet [B] (log_prob = lgamma(a + n/2) -
// lgamma(a) + a log b - (a + n/2) log(b + quad/2) - logdet - n/2 log(2 pi), n = T obs), the filtered moments at unit
// scale and the nine gradients of that log_prob[b] with respect to m0 .. x
std::tuple<at::Tensor, at::Tensor, at::Tensor, at::Tensor, std::vector<at::Tensor>> gamma_gaussian_hmm(
    const at::Tensor& concentration, const at::Tensor& rate, const at::Tensor& m0, const at::Tensor& P0,
    const at::Tensor& trans, const at::Tensor& trans_loc, const at::Tensor& trans_cov, const at::Tensor& obs,
    const at::Tensor& obs_loc, const at::Tensor& obs_cov, const at::Tensor& x, bool need_grads) {
  const at::Tensor* p[8] = {&m0, &P0, &trans, &trans_loc, &trans_cov, &obs, &obs_loc, &obs_cov};
  const GhmmLayout l = gaussian_hmm_layout(p, x);
  const int dt = l.dt;
  const int64_t B = l.B, T = l.T, h = l.h, o = l.o;
  const int64_t(&sb)[8] = l.sb, (&ss)[8] = l.ss, (&steps)[8] = l.steps;
  for (const at::Tensor* t : {&concentration, &rate})
    TORCH_CHECK(t->is_cuda() && t->scalar_type() == x.scalar_type() && t->is_contiguous() && t->dim() == 1 &&
                    (t->size(0) == 1 || t->size(0) == B),
                "pyro_amd::gamma_gaussian_hmm: concentration and rate [B | 1] contiguous of x's dtype");
  const auto opt = x.options();
  at::Tensor quad = at::empty({B}, opt), logdet = at::empty({B}, opt), fm = at::empty({B, h}, opt),
             fP = at::empty({B, h, h}, opt);
  std::vector<at::Tensor> g;
  if (need_grads) {
    g = {at::empty({B, h}, opt), at::empty({B, h, h}, opt), at::empty({B, steps[2], h, h}, opt),
         at::empty({B, steps[3], h}, opt), at::empty({B, steps[4], h, h}, opt), at::empty({B, steps[5], h, o}, opt),
         at::empty({B, steps[6], o}, opt), at::empty({B, steps[7], o, o}, opt), at::empty({B, T, o}, opt)};
  }
  auto gp = [&](int i) { return need_grads ? g[i].data_ptr() : nullptr; };
  const size_t ws_bytes = pa_gaussian_hmm_workspace(dt, B, T, h, o, need_grads ? 1 : 0);
  at::Tensor ws = at::empty({(int64_t)(ws_bytes < 16 ? 16 : ws_bytes)}, opt.dtype(at::kByte));
  check(pa_gamma_gaussian_hmm_fwd_bwd(dt, concentration.data_ptr(), concentration.size(0) == 1 ? 0 : 1, rate.data_ptr(),
                                      rate.size(0) == 1 ? 0 : 1, m0.data_ptr(), sb[0], P0.data_ptr(), sb[1],
                                      trans.data_ptr(), sb[2], ss[2], trans_loc.data_ptr(), sb[3], ss[3],
                                      trans_cov.data_ptr(), sb[4], ss[4], obs.data_ptr(), sb[5], ss[5],
                                      obs_loc.data_ptr(), sb[6], ss[6], obs_cov.data_ptr(), sb[7], ss[7], x.data_ptr(), B,
                                      T, h, o, quad.data_ptr(), logdet.data_ptr(), fm.data_ptr(), fP.data_ptr(), gp(0),
                                      gp(1), gp(2), gp(3), gp(4), gp(5), gp(6), gp(7), gp(8), ws.data_ptr(), ws_bytes,
                                      current_stream()),
        "gamma_gaussian_hmm");
  return {quad, logdet, fm, fP, g};
}

// draws of that model's latent path given the data, forward filter and backward sample in two launches
// (pyro/distributions/hmm.py:596-604 GaussianHMM.rsample_posterior over pyro/ops/gaussian.py:600
// sequential_gaussian_filter_sample).  Layouts as kernels.gaussian_hmm_sample: the parameters and x as above, eps
// [S, B, T, h] standard normal -> z [S, B, T, h] and, with need_maps, the maps (c [B, T, h], G, L [B, T, h, h]) of
// z_T = c_T + L_T eps_T, z_{t-1} = c_{t-1} + G_{t-1} z_t + L_{t-1} eps_{t-1} (empty without)
std::tuple<at::Tensor, std::vector<at::Tensor>> gaussian_hmm_sample(
    const at::Tensor& m0, const at::Tensor& P0, const at::Tensor& trans, const at::Tensor& trans_loc,
    const at::Tensor& trans_cov, const at::Tensor& obs, const at::Tensor& obs_loc, const at::Tensor& obs_cov,
    const at::Tensor& x, const at::Tensor& eps, bool need_maps) {
  const at::Tensor* p[8] = {&m0, &P0, &trans, &trans_loc, &trans_cov, &obs, &obs_loc, &obs_cov};
  const GhmmLayout l = gaussian_hmm_layout(p, x);
  const int64_t B = l.B, T = l.T, h = l.h, o = l.o;
  const int64_t(&sb)[8] = l.sb, (&ss)[8] = l.ss;
  TORCH_CHECK(eps.is_cuda() && eps.scalar_type() == x.scalar_type() && eps.is_contiguous() && eps.dim() == 4 &&
                  eps.size(1) == B && eps.size(2) == T && eps.size(3) == h,
              "pyro_amd::gaussian_hmm_sample: eps [S, B, T, hidden] contiguous of x's dtype");
  const int64_t S = eps.size(0);
  const auto opt = x.options();
  at::Tensor z = at::empty({S, B, T, h}, opt);
  std::vector<at::Tensor> maps;
  if (need_maps) maps = {at::empty({B, T, h}, opt), at::empty({B, T, h, h}, opt), at::empty({B, T, h, h}, opt)};
  auto mp = [&](int i) { return need_maps ? maps[i].data_ptr() : nullptr; };
  const size_t ws_bytes = pa_gaussian_hmm_sample_workspace(l.dt, B, T, h, o);
  at::Tensor ws = at::empty({(int64_t)(ws_bytes < 16 ? 16 : ws_bytes)}, opt.dtype(at::kByte));
  check(pa_gaussian_hmm_sample(l.dt, m0.data_ptr(), sb[0], P0.data_ptr(), sb[1], trans.data_ptr(), sb[2], ss[2],
                               trans_loc.data_ptr(), sb[3], ss[3], trans_cov.data_ptr(), sb[4], ss[4], obs.data_ptr(),
                               sb[5], ss[5], obs_loc.data_ptr(), sb[6], ss[6], obs_cov.data_ptr(), sb[7], ss[7],
                               x.data_ptr(), B, T, h, o, S, eps.data_ptr(), z.data_ptr(), mp(0), mp(1), mp(2),
                               ws.data_ptr(), ws_bytes, current_stream()),
        "gaussian_hmm_sample");
  return {z, maps};
}

// the smoothed marginals of that model's states given all the data in one launch: Kalman filter, then the
// Rauch-Tung-Striebel sweep.  Layouts as kernels.gaussian_hmm_smooth: the parameters and x as above -> mean [B, T, h],
// cov [B, T, h, h] and, with need_cross, [cross [B, T - 1, h, h]] with cross[b, t] = Cov(z_t, z_{t+1} | x) (empty
// without)
std::tuple<at::Tensor, at::Tensor, std::vector<at::Tensor>> gaussian_hmm_smooth(
    const at::Tensor& m0, const at::Tensor& P0, const at::Tensor& trans, const at::Tensor& trans_loc,
    const at::Tensor& trans_cov, const at::Tensor& obs, const at::Tensor& obs_loc, const at::Tensor& obs_cov,
    const at::Tensor& x, bool need_cross) {
  const at::Tensor* p[8] = {&m0, &P0, &trans, &trans_loc, &trans_cov, &obs, &obs_loc, &obs_cov};
  const GhmmLayout l = gaussian_hmm_layout(p, x);
  const int64_t B = l.B, T = l.T, h = l.h, o = l.o;
  const int64_t(&sb)[8] = l.sb, (&ss)[8] = l.ss;
  const auto opt = x.options();
  at::Tensor mean = at::empty({B, T, h}, opt), cov = at::empty({B, T, h, h}, opt);
  std::vector<at::Tensor> cross;
  if (need_cross) cross = {at::empty({B, T - 1, h, h}, opt)};
  const size_t ws_bytes = pa_gaussian_hmm_smooth_workspace(l.dt, B, T, h, o);
  at::Tensor ws = at::empty({(int64_t)(ws_bytes < 16 ? 16 : ws_bytes)}, opt.dtype(at::kByte));
  check(pa_gaussian_hmm_smooth(l.dt, m0.data_ptr(), sb[0], P0.data_ptr(), sb[1], trans.data_ptr(), sb[2], ss[2],
                               trans_loc.data_ptr(), sb[3], ss[3], trans_cov.data_ptr(), sb[4], ss[4], obs.data_ptr(),
                               sb[5], ss[5], obs_loc.data_ptr(), sb[6], ss[6], obs_cov.data_ptr(), sb[7], ss[7],
                               x.data_ptr(), B, T, h, o, mean.data_ptr(), cov.data_ptr(),
                               need_cross ? cross[0].data_ptr() : nullptr, ws.data_ptr(), ws_bytes, current_stream()),
        "gaussian_hmm_smooth");
  return {mean, cov, cross};
}

// forward draws of that model in two launches (pyro/distributions/hmm.py:584-594 GaussianHMM.rsample over
// pyro/ops/gaussian.py:600 sequential_gaussian_filter_sample and Gaussian.left_condition(z).rsample()).  Layouts as
// kernels.gaussian_hmm_draw: the parameters as above, T steps, the standard normal eps0 [S, B, h], eps_z [S, B, T, h],
// eps_x [S, B, T, o] -> x [S, B, T, o] and, with need_states, [z [S, B, T, h]] (empty without)
std::tuple<at::Tensor, std::vector<at::Tensor>> gaussian_hmm_draw(
    const at::Tensor& m0, const at::Tensor& P0, const at::Tensor& trans, const at::Tensor& trans_loc,
    const at::Tensor& trans_cov, const at::Tensor& obs, const at::Tensor& obs_loc, const at::Tensor& obs_cov, int64_t T,
    const at::Tensor& eps0, const at::Tensor& eps_z, const at::Tensor& eps_x, bool need_states) {
  const at::Tensor* p[8] = {&m0, &P0, &trans, &trans_loc, &trans_cov, &obs, &obs_loc, &obs_cov};
  TORCH_CHECK(eps0.is_cuda() && eps0.dim() == 3 && eps0.is_contiguous() && obs.dim() == 4 && T >= 1,
              "pyro_amd::gaussian_hmm_draw: eps0 [S, B, hidden] contiguous, obs [B | 1, T | 1, hidden, obs], T >= 1");
  const int64_t S = eps0.size(0), B = eps0.size(1), o = obs.size(3);
  const GhmmLayout l = gaussian_hmm_param_layout(p, eps0, B, T, o);
  const int64_t h = l.h;
  const int64_t(&sb)[8] = l.sb, (&ss)[8] = l.ss;
  auto noise_ok = [&](const at::Tensor& e, int64_t n) {
    return e.is_cuda() && e.scalar_type() == eps0.scalar_type() && e.is_contiguous() && e.dim() == 4 &&
           e.size(0) == S && e.size(1) == B && e.size(2) == T && e.size(3) == n;
  };
  TORCH_CHECK(eps0.size(2) == h && noise_ok(eps_z, h) && noise_ok(eps_x, o),
              "pyro_amd::gaussian_hmm_draw: eps0 [S, B, hidden], eps_z [S, B, T, hidden], eps_x [S, B, T, obs] "
              "contiguous of the parameters' dtype");
  const auto opt = eps0.options();
  at::Tensor x = at::empty({S, B, T, o}, opt);
  std::vector<at::Tensor> states;
  if (need_states) states = {at::empty({S, B, T, h}, opt)};
  // (only the factors the strides make distinct: see include/pyro_amd.h)
  const int64_t Bw = (sb[1] || sb[4] || sb[7]) ? B : 1, Tw = (ss[4] || ss[7]) ? T : 1;
  const size_t ws_bytes = pa_gaussian_hmm_draw_workspace(l.dt, Bw, Tw, h, o);
  at::Tensor ws = at::empty({(int64_t)(ws_bytes < 16 ? 16 : ws_bytes)}, opt.dtype(at::kByte));
  check(pa_gaussian_hmm_draw(l.dt, m0.data_ptr(), sb[0], P0.data_ptr(), sb[1], trans.data_ptr(), sb[2], ss[2],
                             trans_loc.data_ptr(), sb[3], ss[3], trans_cov.data_ptr(), sb[4], ss[4], obs.data_ptr(),
                             sb[5], ss[5], obs_loc.data_ptr(), sb[6], ss[6], obs_cov.data_ptr(), sb[7], ss[7], B, T, h,
                             o, S, eps0.data_ptr(), eps_z.data_ptr(), eps_x.data_ptr(), x.data_ptr(),
                             need_states ? states[0].data_ptr() : nullptr, ws.data_ptr(), ws_bytes, current_stream()),
        "gaussian_hmm_draw");
  return {x, states};
}

// forward draws of a linear state-space model with arbitrary noise in one launch (pyro/distributions/hmm.py:1122-1138
// LinearHMM.rsample over _linear_integrate, hmm.py:32-48).  Layouts as kernels.linear_hmm_draw: trans
// [B | 1, T | 1, h, h], obs [B | 1, T | 1, h, o], T steps, the noise draws init [S, B, h], e [S, B, T, h], n [S, B, T, o]
// with loc and scale applied -> y [S, B, T, o] and, with need_states, [z [S, B, T, h]] (empty without)
std::tuple<at::Tensor, std::vector<at::Tensor>> linear_hmm_draw(const at::Tensor& trans, const at::Tensor& obs,
                                                                int64_t T, const at::Tensor& init, const at::Tensor& e,
                                                                const at::Tensor& n, bool need_states) {
  const int dt = dtype_of(init, "linear_hmm_draw");
  TORCH_CHECK(init.dim() == 3 && init.is_contiguous() && obs.dim() == 4 && trans.dim() == 4 && T >= 1,
              "pyro_amd::linear_hmm_draw: init [S, B, hidden] contiguous, trans [B | 1, T | 1, hidden, hidden], "
              "obs [B | 1, T | 1, hidden, obs], T >= 1");
  const int64_t S = init.size(0), B = init.size(1), h = init.size(2), o = obs.size(3);
  auto matrix_ok = [&](const at::Tensor& m, int64_t cols) {
    return m.is_cuda() && m.scalar_type() == init.scalar_type() && m.is_contiguous() &&
           (m.size(0) == 1 || m.size(0) == B) && (m.size(1) == 1 || m.size(1) == T) && m.size(2) == h &&
           m.size(3) == cols;
  };
  TORCH_CHECK(h >= 1 && o >= 1 && matrix_ok(trans, h) && matrix_ok(obs, o),
              "pyro_amd::linear_hmm_draw: trans [B | 1, T | 1, hidden, hidden], obs [B | 1, T | 1, hidden, obs] "
              "contiguous of the noise's dtype");
  auto noise_ok = [&](const at::Tensor& t, int64_t w) {
    return t.is_cuda() && t.scalar_type() == init.scalar_type() && t.is_contiguous() && t.dim() == 4 &&
           t.size(0) == S && t.size(1) == B && t.size(2) == T && t.size(3) == w;
  };
  TORCH_CHECK(noise_ok(e, h) && noise_ok(n, o),
              "pyro_amd::linear_hmm_draw: e [S, B, T, hidden], n [S, B, T, obs] contiguous of init's dtype");
  auto stride_batch = [&](const at::Tensor& m) { return m.size(0) == 1 ? 0 : m.size(1) * m.size(2) * m.size(3); };
  auto stride_step = [&](const at::Tensor& m) { return m.size(1) == 1 ? 0 : m.size(2) * m.size(3); };
  const auto opt = init.options();
  at::Tensor y = at::empty({S, B, T, o}, opt);
  std::vector<at::Tensor> states;
  if (need_states) states = {at::empty({S, B, T, h}, opt)};
  check(pa_linear_hmm_draw(dt, trans.data_ptr(), stride_batch(trans), stride_step(trans), obs.data_ptr(),
                           stride_batch(obs), stride_step(obs), B, T, h, o, S, init.data_ptr(), e.data_ptr(),
                           n.data_ptr(), y.data_ptr(), need_states ? states[0].data_ptr() : nullptr,
                           current_stream()),
        "linear_hmm_draw");
  return {y, states};
}

// mean, lower median and CRPS of a sample forecast in one launch that reads pred once (pyro/ops/stats.py
// crps_empirical with the median(0) and mean(0) of pyro/contrib/forecast/evaluate.py): pred [S, M] contiguous,
// truth [M] -> (mean, median, crps) [M] each
std::tuple<at::Tensor, at::Tensor, at::Tensor> forecast_scores(const at::Tensor& pred, const at::Tensor& truth) {
  const int dt = dtype_of(pred, "forecast_scores");
  TORCH_CHECK(pred.dim() == 2 && pred.is_contiguous() && pred.size(0) >= 1 && truth.is_cuda() && truth.dim() == 1 &&
                  truth.is_contiguous() && truth.scalar_type() == pred.scalar_type() && truth.size(0) == pred.size(1),
              "pyro_amd::forecast_scores: pred [S, M] and truth [M] contiguous of one dtype, S >= 1");
  const int64_t S = pred.size(0), M = pred.size(1);
  at::Tensor out = at::empty({3, M}, pred.options());
  check(pa_forecast_scores(dt, pred.data_ptr(), truth.data_ptr(), S, M, out[0].data_ptr(), out[1].data_ptr(),
                           out[2].data_ptr(), current_stream()),
        "forecast_scores");
  return {out[0], out[1], out[2]};
}

// one of the four orthonormal time transforms along ``dim`` in one launch (pyro/ops/tensor_utils.py dct / idct /
// haar_transform / inverse_haar_transform): op 0 dct, 1 idct, 2 haar, 3 inverse haar; x contiguous, read as
// [outer, N, inner] around dim without a transpose -> a tensor of x's shape.  The gradient of op is op ^ 1 of the
// incoming gradient (the transforms are orthonormal).
at::Tensor time_transform(const at::Tensor& x, int64_t op, int64_t dim) {
  const int dt = dtype_of(x, "time_transform");
  TORCH_CHECK(x.dim() >= 1 && x.is_contiguous() && dim >= -x.dim() && dim < x.dim() && op >= 0 && op <= 3,
              "pyro_amd::time_transform: x contiguous with at least one dim, dim inside it, op in 0..3");
  const int64_t d = dim < 0 ? dim + x.dim() : dim;
  int64_t outer = 1, inner = 1;
  for (int64_t i = 0; i < d; ++i) outer *= x.size(i);
  for (int64_t i = d + 1; i < x.dim(); ++i) inner *= x.size(i);
  at::Tensor y = at::empty_like(x);
  if (x.numel() == 0) return y;
  check(pa_time_transform(dt, (int)op, x.data_ptr(), y.data_ptr(), outer, x.size(d), inner, current_stream()),
        "time_transform");
  return y;
}

// the covariance matrix of a stationary Gaussian-process kernel by direct differences, one launch
// (pyro/contrib/gp/kernels/isotropic.py): family 0 RBF, 1 RationalQuadratic (alpha = scale_mixture), 2 Exponential,
// 3 Matern32, 4 Matern52; x [N, D], z [M, D] or none for z = x -> K [N, M].  Parameters stay on the device.
struct GpArgs {
  int dt;
  int64_t N, M, D;
  const void *z, *alpha;
};
GpArgs gp_args(const char* who, const at::Tensor& x, const std::optional<at::Tensor>& z, const at::Tensor& lengthscale,
               const at::Tensor& variance, const std::optional<at::Tensor>& alpha, int64_t family) {
  GpArgs a;
  a.dt = dtype_of(x, who);
  TORCH_CHECK(x.dim() == 2 && x.is_contiguous() && x.size(1) >= 1 && x.size(1) <= 64 && family >= 0 && family <= 4,
              "pyro_amd::", who, ": x [N, D] contiguous, 1 <= D <= 64, family in 0..4");
  a.N = x.size(0), a.D = x.size(1), a.M = a.N, a.z = nullptr, a.alpha = nullptr;
  auto same = [&](const at::Tensor& t) { return t.is_cuda() && t.is_contiguous() && t.scalar_type() == x.scalar_type(); };
  if (z.has_value() && z->defined()) {
    TORCH_CHECK(same(*z) && z->dim() == 2 && z->size(1) == a.D, "pyro_amd::", who, ": z [M, D] contiguous, of x's dtype");
    a.M = z->size(0), a.z = z->data_ptr();
  }
  TORCH_CHECK(same(lengthscale) && same(variance) && (lengthscale.numel() == 1 || lengthscale.numel() == a.D) &&
                  variance.numel() == 1,
              "pyro_amd::", who, ": lengthscale of 1 or D elements, variance of 1, of x's dtype");
  const bool has_alpha = alpha.has_value() && alpha->defined();
  TORCH_CHECK(has_alpha == (family == 1) && (!has_alpha || (same(*alpha) && alpha->numel() == 1)), "pyro_amd::", who,
              ": alpha (one element) with family 1 and only with it");
  if (has_alpha) a.alpha = alpha->data_ptr();
  return a;
}

at::Tensor gp_kernel(const at::Tensor& x, const std::optional<at::Tensor>& z, const at::Tensor& lengthscale,
                     const at::Tensor& variance, const std::optional<at::Tensor>& alpha, int64_t family) {
  const GpArgs a = gp_args("gp_kernel", x, z, lengthscale, variance, alpha, family);
  at::Tensor K = at::empty({a.N, a.M}, x.options());
  if (a.N == 0 || a.M == 0) return K;
  check(pa_gp_kernel_fwd(a.dt, (int)family, x.data_ptr(), a.z, lengthscale.data_ptr(), (int)lengthscale.numel(),
                         variance.data_ptr(), a.alpha, K.data_ptr(), a.N, a.M, a.D, current_stream()),
        "gp_kernel");
  return K;
}

// its gradients given G = dL/dK [N, M] contiguous: (gx, gz, g_lengthscale, g_variance, g_alpha), an empty tensor where
// want_* is false (gz also without a z, g_alpha also outside family 1); K is not an input -- everything is recomputed
std::tuple<at::Tensor, at::Tensor, at::Tensor, at::Tensor, at::Tensor> gp_kernel_bwd(
    const at::Tensor& x, const std::optional<at::Tensor>& z, const at::Tensor& lengthscale, const at::Tensor& variance,
    const std::optional<at::Tensor>& alpha, const at::Tensor& G, int64_t family, bool want_x, bool want_z,
    bool want_lengthscale, bool want_variance, bool want_alpha, int64_t forced_splits) {
  const GpArgs a = gp_args("gp_kernel_bwd", x, z, lengthscale, variance, alpha, family);
  TORCH_CHECK(G.is_cuda() && G.is_contiguous() && G.scalar_type() == x.scalar_type() && G.dim() == 2 && G.size(0) == a.N &&
                  G.size(1) == a.M && forced_splits >= 0,
              "pyro_amd::gp_kernel_bwd: G [N, M] contiguous, of x's dtype");
  want_z = want_z && a.z != nullptr;
  want_alpha = want_alpha && a.alpha != nullptr;
  const bool none = a.N == 0 || a.M == 0;      // (no launch: zeros; else the finalize kernel writes every wanted entry)
  auto out = [&](bool want, const at::Tensor& like) {
    return want ? (none ? at::zeros_like(like) : at::empty_like(like)) : at::empty({0}, x.options());
  };
  at::Tensor gx = out(want_x, x), gz = out(want_z, want_z ? *z : x), gl = out(want_lengthscale, lengthscale),
             gv = out(want_variance, variance), ga = out(want_alpha, want_alpha ? *alpha : variance);
  if (a.N == 0 || a.M == 0 || !(want_x || want_z || want_lengthscale || want_variance || want_alpha))
    return {gx, gz, gl, gv, ga};
  const size_t ws_bytes = pa_gp_kernel_bwd_workspace(a.N, a.M, a.D, a.z == nullptr, want_x, want_z, (int)forced_splits);
  at::Tensor ws = at::empty({(int64_t)((ws_bytes < 8 ? 8 : ws_bytes) + 7) / 8}, x.options().dtype(at::kDouble));
  auto ptr = [](bool want, at::Tensor& t) -> void* { return want ? t.data_ptr() : nullptr; };
  check(pa_gp_kernel_bwd(a.dt, (int)family, x.data_ptr(), a.z, lengthscale.data_ptr(), (int)lengthscale.numel(),
                         variance.data_ptr(), a.alpha, G.data_ptr(), a.N, a.M, a.D, ptr(want_x, gx), ptr(want_z, gz),
                         ptr(want_lengthscale, gl), ptr(want_variance, gv), ptr(want_alpha, ga), (int)forced_splits,
                         ws.data_ptr(), (size_t)ws.numel() * 8, current_stream()),
        "gp_kernel_bwd");
  return {gx, gz, gl, gv, ga};
}

// the same chain decoded in one launch: its most probable path (mode 0) or one joint posterior draw (mode 1), with the
// path's score / log Z (pyro/infer/discrete.py _sample_posterior_from_trace on a pyro.markov model).  pairwise
// [B | 1, T - 1 | 1, K, K] as for logchain (anything for T = 1); seed / offset: the 64-bit words as two's complement
std::tuple<at::Tensor, at::Tensor> logchain_decode(const at::Tensor& unary, const at::Tensor& pairwise, int64_t mode,
                                                   int64_t seed, int64_t offset,
                                                   const std::optional<at::Tensor>& offset_dev, int64_t step_blocks) {
  const int dt = dtype_of(unary, "logchain_decode");
  TORCH_CHECK(unary.dim() == 3 && unary.is_contiguous(), "pyro_amd::logchain_decode: unary [B, T, K] contiguous");
  const int64_t B = unary.size(0), T = unary.size(1), K = unary.size(2);
  int64_t sb = 0, ss = 0;
  const void* pp = nullptr;
  if (T > 1) {
    TORCH_CHECK(pairwise.is_contiguous() && pairwise.scalar_type() == unary.scalar_type() && pairwise.dim() == 4 &&
                    pairwise.size(2) == K && pairwise.size(3) == K && (pairwise.size(0) == B || pairwise.size(0) == 1) &&
                    (pairwise.size(1) == T - 1 || pairwise.size(1) == 1),
                "pyro_amd::logchain_decode: pairwise [B | 1, T - 1 | 1, K, K] contiguous, of unary's dtype");
    sb = pairwise.size(0) == 1 ? 0 : pairwise.stride(0);
    ss = pairwise.size(1) == 1 ? 0 : pairwise.stride(1);
    pp = pairwise.data_ptr();
  }
  const size_t ws_bytes = pa_logchain_decode_workspace(dt, B, T, K);
  at::Tensor ws = at::empty({(int64_t)(ws_bytes < 16 ? 16 : ws_bytes)}, unary.options().dtype(at::kByte));
  at::Tensor z = at::empty({B, T}, unary.options().dtype(at::kLong)), log_norm = at::empty({B}, unary.options());
  const uint64_t* od = nullptr;
  if (offset_dev.has_value() && offset_dev->defined()) od = (const uint64_t*)offset_dev->data_ptr();
  check(pa_logchain_decode(dt, unary.data_ptr(), pp, sb, ss, B, T, K, (int)mode, (uint64_t)seed, (uint64_t)offset, od,
                           (uint64_t)step_blocks, (int64_t*)z.data_ptr(), log_norm.data_ptr(), ws.data_ptr(), ws_bytes,
                           current_stream()),
        "logchain_decode");
  return {z, log_norm};
}

// the leaf of a plated mixture under TraceEnum_ELBO / the enumerated potential of HMC and NUTS: the observed site's
// log_prob against every value of the enumerated assignment (pyro/poutine/trace_struct.py:248-288), logsumexp over it
// (pyro/ops/contract.py:79-160) and the plate sum, forward and backward in one pass over the data, for B parameter
// sets (vectorised particles / chains).  a [B, K]; p0, p1 [B | 1, K | 1]; -> float64 [B, 1 + 3 K]:
// S, dS/da, dS/dp0, dS/dp1 per (b, k) (a shared parameter takes their sum)
at::Tensor mixture_fwd_bwd(int64_t dist, const at::Tensor& x, const at::Tensor& a, const at::Tensor& p0,
                           const std::optional<at::Tensor>& p1) {
  const int dt = dtype_of(x, "mixture_fwd_bwd");
  TORCH_CHECK(x.dim() == 1 && x.is_contiguous() && a.dim() == 2 && a.is_contiguous() && a.scalar_type() == x.scalar_type(),
              "pyro_amd::mixture_fwd_bwd: x [N] contiguous, a [B, K] contiguous, one dtype");
  const int64_t N = x.size(0), B = a.size(0), K = a.size(1);
  auto strides = [&](const at::Tensor& p, int64_t& sk, int64_t& sb) {
    TORCH_CHECK(p.dim() == 2 && p.is_contiguous() && p.scalar_type() == x.scalar_type() &&
                    (p.size(0) == B || p.size(0) == 1) && (p.size(1) == K || p.size(1) == 1),
                "pyro_amd::mixture_fwd_bwd: parameters [B | 1, K | 1] contiguous");
    sk = p.size(1) == 1 ? 0 : 1;
    sb = p.size(0) == 1 ? 0 : p.size(1);
  };
  int64_t s0 = 0, b0 = 0, s1 = 0, b1 = 0;
  strides(p0, s0, b0);
  if (p1.has_value()) strides(*p1, s1, b1);
  const size_t ws_bytes = pa_mixture_workspace((int)K, B);
  TORCH_CHECK(ws_bytes > 0, "pyro_amd::mixture_fwd_bwd: K = ", K, " outside [1, 64]");
  at::Tensor ws = at::empty({(int64_t)ws_bytes}, x.options().dtype(at::kByte));
  at::Tensor out = at::empty({B, 1 + 3 * K}, x.options().dtype(at::kDouble));
  check(pa_mixture_fwd_bwd(dt, (int)dist, x.data_ptr(), N, (int)K, B, a.data_ptr(), K, p0.data_ptr(), s0, b0,
                           p1.has_value() ? p1->data_ptr() : nullptr, s1, b1, ws.data_ptr(), ws_bytes,
                           (double*)out.data_ptr(), current_stream()),
        "mixture_fwd_bwd");
  return out;
}

// the enumerated Categorical-Categorical mixture factor of examples/lda.py:53-71 under TraceEnum_ELBO with its
// gradient, word-major half through the corpus index (pa_lda_build_index): pyro/infer/traceenum_elbo.py:112-214
std::tuple<at::Tensor, at::Tensor, at::Tensor> lda_factor_indexed(const at::Tensor& words, const at::Tensor& index,
                                                                  const at::Tensor& log_theta, const at::Tensor& log_phi) {
  const int dt = dtype_of(log_theta, "lda_factor_indexed");
  TORCH_CHECK(words.is_cuda() && words.scalar_type() == at::kLong && words.dim() == 2 && words.is_contiguous() &&
                  index.is_cuda() && index.scalar_type() == at::kByte && log_theta.dim() == 2 && log_phi.dim() == 2 &&
                  log_theta.is_contiguous() && log_phi.is_contiguous() && log_phi.scalar_type() == log_theta.scalar_type(),
              "pyro_amd::lda_factor_indexed: words int64 [Wd, B], index uint8, log_theta [B, T], log_phi [T, V]");
  const int64_t Wd = words.size(0), B = words.size(1), T = log_theta.size(1), V = log_phi.size(1);
  TORCH_CHECK(log_theta.size(0) == B && log_phi.size(0) == T, "pyro_amd::lda_factor_indexed: shapes");
  const size_t ws_bytes = pa_lda_factor_indexed_workspace(dt, Wd, B, T, V);
  at::Tensor ws = at::empty({(int64_t)(ws_bytes < 16 ? 16 : ws_bytes)}, log_theta.options().dtype(at::kByte));
  at::Tensor out_doc = at::empty({B}, log_theta.options()), g_theta = at::empty_like(log_theta), g_phi = at::empty_like(log_phi);
  check(pa_lda_factor_indexed_fwd_bwd(dt, words.data_ptr<int64_t>(), index.data_ptr(), (size_t)index.numel(),
                                      log_theta.data_ptr(), log_phi.data_ptr(), Wd, B, T, V, out_doc.data_ptr(),
                                      g_theta.data_ptr(), g_phi.data_ptr(), ws.data_ptr(), ws_bytes, current_stream()),
        "lda_factor_indexed");
  return {out_doc, g_theta, g_phi};
}

// F.linear over a tall batch with the Sigmoid behind it (and the gradient through the previous one) fused:
// Y = act(G' W^T + bias), G' = G (1 - y_mul) y_mul when y_mul is given (examples/lda.py:76-92's predictor)
at::Tensor tall_linear_act(const at::Tensor& G, const at::Tensor& weight, const std::optional<at::Tensor>& bias,
                           const std::optional<at::Tensor>& y_mul, bool sigmoid_out, bool transpose_weight) {
  require_f32_gpu(G, "G");
  TORCH_CHECK(G.dim() == 2 && weight.dim() == 2 && weight.is_cuda() && weight.scalar_type() == at::kFloat,
              "pyro_amd::tall_linear_act: G [B, R], weight 2-D float32");
  const int64_t B = G.size(0), R = G.size(1);
  // transpose_weight = true: F.linear's forward, Wm = weight^T (weight [C, R]); false: autograd's dx, Wm = weight [R, C]
  const int64_t C = transpose_weight ? weight.size(0) : weight.size(1);
  TORCH_CHECK((transpose_weight ? weight.size(1) : weight.size(0)) == R, "pyro_amd::tall_linear_act: weight does not match G");
  const int64_t rs = transpose_weight ? weight.stride(1) : weight.stride(0), cs = transpose_weight ? weight.stride(0) : weight.stride(1);
  if (y_mul.has_value() && y_mul->defined()) {
    require_f32_gpu(*y_mul, "y_mul");
    TORCH_CHECK(y_mul->numel() == B * R, "pyro_amd::tall_linear_act: y_mul [B, R]");
  }
  if (bias.has_value() && bias->defined()) {
    require_f32_gpu(*bias, "bias");
    TORCH_CHECK(bias->numel() == C, "pyro_amd::tall_linear_act: bias [C]");
  }
  at::Tensor Y = at::empty({B, C}, G.options());
  check(pa_tall_linear_act(G.data_ptr<float>(), B, R, weight.data_ptr<float>(), rs, cs, C, f32_ptr(bias), f32_ptr(y_mul),
                           sigmoid_out ? 1 : 0, Y.data_ptr<float>(), current_stream()),
        "tall_linear_act");
  return Y;
}

// one round of a span of asynchronous NUTS chains: every live chain consumes (peq, gq) at its cursor; a chain
// whose tree finishes adapts, stores its draw and begins its next transition in the same launch
// (pyro/infer/mcmc/nuts.py:184-522, adaptation.py:166-185); every state tensor is updated in place
void nuts_tree_run_advance(at::Tensor z, at::Tensor pe, at::Tensor grad, at::Tensor zq, at::Tensor rq, const at::Tensor& gq,
                           const at::Tensor& peq, const at::Tensor& inv_mass, at::Tensor step, int64_t max_tree_depth,
                           bool use_multinomial, int64_t seed, int64_t chain_offset, const at::Tensor& ctl,
                           at::Tensor da_state, double target_accept, at::Tensor welford, at::Tensor mean_accept,
                           at::Tensor counters, at::Tensor tc, at::Tensor n_done, const std::optional<at::Tensor>& done_flag,
                           const std::optional<at::Tensor>& slot2chain, const std::optional<at::Tensor>& zq_slot,
                           at::Tensor accept_prob, at::Tensor stats, at::Tensor workspace) {
  const int dt = dtype_of(z, "nuts_tree_run_advance");
  TORCH_CHECK(z.dim() == 2 && z.is_contiguous(), "pyro_amd::nuts_tree_run_advance: z [C, D] contiguous");
  const int64_t C = z.size(0), D = z.size(1);
  TORCH_CHECK(stats.scalar_type() == at::kInt && stats.dim() == 2 && stats.size(0) == 4 && stats.size(1) == C && stats.is_contiguous(),
              "pyro_amd::nuts_tree_run_advance: stats int32 [4, C] {n_leapfrog, depth, diverging, accepted}");
  TORCH_CHECK(ctl.scalar_type() == at::kLong && counters.scalar_type() == at::kLong && tc.scalar_type() == at::kInt &&
                  n_done.scalar_type() == at::kInt && workspace.scalar_type() == at::kByte,
              "pyro_amd::nuts_tree_run_advance: ctl / counters int64, tc / n_done int32, workspace uint8");
  const bool compact = slot2chain.has_value() && slot2chain->defined();
  const int64_t n_slots = compact ? slot2chain->numel() : C;
  int32_t* st = stats.data_ptr<int32_t>();
  check(pa_nuts_tree_run_advance(
            dt, z.data_ptr(), pe.data_ptr(), grad.data_ptr(), zq.data_ptr(), rq.data_ptr(), gq.data_ptr(), peq.data_ptr(),
            inv_mass.data_ptr(), inv_mass.dim() == 2 ? D : 0, step.data_ptr(), C, D, (int)max_tree_depth,
            use_multinomial ? 1 : 0, (uint64_t)seed, (uint64_t)chain_offset, ctl.data_ptr<int64_t>(), da_state.data_ptr(),
            target_accept, welford.data_ptr(), mean_accept.data_ptr(), counters.data_ptr<int64_t>(), tc.data_ptr<int32_t>(),
            n_done.data_ptr<int32_t>(),
            done_flag.has_value() && done_flag->defined() ? done_flag->data_ptr<int64_t>() : nullptr,
            compact ? slot2chain->data_ptr<int32_t>() : nullptr,
            compact && zq_slot.has_value() && zq_slot->defined() ? zq_slot->data_ptr() : nullptr, n_slots,
            accept_prob.data_ptr(), st, st + C, st + 2 * C, st + 3 * C, workspace.data_ptr(), (size_t)workspace.numel(),
            current_stream()),
        "nuts_tree_run_advance");
}

}  // namespace

TORCH_LIBRARY(pyro_amd, m) {
  m.def("glm_pack_planes(Tensor X, int format) -> Tensor");
  m.def("glm_bernoulli_planes(Tensor planes, Tensor y, Tensor w, Tensor? b, float scale, int N, int D, "
        "int format, Tensor? moments=None) -> (Tensor, Tensor, Tensor, Tensor)");
  m.def("glm_bernoulli(Tensor X, Tensor y, Tensor w, Tensor? b, Tensor? mask, float scale) -> "
        "(Tensor, Tensor, Tensor, Tensor)");
  m.def("adam_step(Tensor(a!) param, Tensor(b!) grad, Tensor(c!) exp_avg, Tensor(d!) exp_avg_sq, "
        "Tensor(e!) step, float lr, float beta1, float beta2, float eps, float weight_decay, float clip_norm, "
        "float lrd, bool clipped, bool zero_grad) -> ()");
  m.def("glm_chain(Tensor g, Tensor gw, Tensor gb) -> (Tensor, Tensor)");
  // typed schemas of the next ten (round 6)
  m.def("dist_log_prob_sum(int dist, Tensor value, Tensor? p0, Tensor? p1, Tensor? mask, float scale) -> "
        "(Tensor rowsum, Tensor total)");
  m.def("multi_log_prob_sum(int[] dist, Tensor[] value, Tensor?[] p0, Tensor?[] p1, float[] coef, float coef_all) "
        "-> Tensor");
  m.def("meanfield_normal_sample(Tensor[] loc, Tensor[] rho, int P, int seed, int[] offsets, Tensor? offset_dev) -> "
        "(Tensor[] z, Tensor[] scale, Tensor[] eps)");
  m.def("exp_site(Tensor u, float lower) -> (Tensor value, Tensor log_density)");
  m.def("exp_site_bwd(Tensor value, Tensor? g_value, Tensor? g_log_density, float lower) -> Tensor");
  m.def("mvn_tril_sample(Tensor loc, Tensor rho, Tensor A, int P, int seed, int offset, Tensor? offset_dev) -> "
        "(Tensor eps, Tensor z, Tensor logq)");
  m.def("logsumexp_terms(Tensor[] terms, int[] sizes, int rdim) -> Tensor");
  m.def("logchain(Tensor unary, Tensor pairwise) -> (Tensor log_z, Tensor grad_unary, Tensor grad_pairwise)");
  m.def("logchain_decode(Tensor unary, Tensor pairwise, int mode, int seed, int offset, Tensor? offset_dev, "
        "int step_blocks) -> (Tensor z, Tensor log_norm)");
  m.def("gaussian_hmm(Tensor m0, Tensor P0, Tensor trans, Tensor trans_loc, Tensor trans_cov, Tensor obs, "
        "Tensor obs_loc, Tensor obs_cov, Tensor x, bool need_grads) -> (Tensor log_prob, Tensor filter_mean, "
        "Tensor filter_cov, Tensor[] grads)");
  m.def("gamma_gaussian_hmm(Tensor concentration, Tensor rate, Tensor m0, Tensor P0, Tensor trans, Tensor trans_loc, "
        "Tensor trans_cov, Tensor obs, Tensor obs_loc, Tensor obs_cov, Tensor x, bool need_grads) -> (Tensor quad, "
        "Tensor logdet, Tensor filter_mean, Tensor filter_cov, Tensor[] grads)");
  m.def("gaussian_hmm_sample(Tensor m0, Tensor P0, Tensor trans, Tensor trans_loc, Tensor trans_cov, Tensor obs, "
        "Tensor obs_loc, Tensor obs_cov, Tensor x, Tensor eps, bool need_maps) -> (Tensor z, Tensor[] maps)");
  m.def("gaussian_hmm_smooth(Tensor m0, Tensor P0, Tensor trans, Tensor trans_loc, Tensor trans_cov, Tensor obs, "
        "Tensor obs_loc, Tensor obs_cov, Tensor x, bool need_cross) -> (Tensor mean, Tensor cov, Tensor[] cross)");
  m.def("gaussian_hmm_draw(Tensor m0, Tensor P0, Tensor trans, Tensor trans_loc, Tensor trans_cov, Tensor obs, "
        "Tensor obs_loc, Tensor obs_cov, int T, Tensor eps0, Tensor eps_z, Tensor eps_x, bool need_states) -> "
        "(Tensor x, Tensor[] states)");
  m.def("linear_hmm_draw(Tensor trans, Tensor obs, int T, Tensor init, Tensor e, Tensor n, bool need_states) -> "
        "(Tensor y, Tensor[] states)");
  m.def("forecast_scores(Tensor pred, Tensor truth) -> (Tensor mean, Tensor median, Tensor crps)");
  m.def("time_transform(Tensor x, int op, int dim) -> Tensor");
  m.def("gp_kernel(Tensor x, Tensor? z, Tensor lengthscale, Tensor variance, Tensor? alpha, int family) -> Tensor");
  m.def("gp_kernel_bwd(Tensor x, Tensor? z, Tensor lengthscale, Tensor variance, Tensor? alpha, Tensor G, int family, "
        "bool want_x, bool want_z, bool want_lengthscale, bool want_variance, bool want_alpha, int forced_splits) -> "
        "(Tensor gx, Tensor gz, Tensor g_lengthscale, Tensor g_variance, Tensor g_alpha)");
  m.def("mixture_fwd_bwd(int dist, Tensor x, Tensor a, Tensor p0, Tensor? p1) -> Tensor");
  m.def("lda_factor_indexed(Tensor words, Tensor index, Tensor log_theta, Tensor log_phi) -> "
        "(Tensor out_doc, Tensor g_theta, Tensor g_phi)");
  m.def("tall_linear_act(Tensor G, Tensor weight, Tensor? bias, Tensor? y_mul, bool sigmoid_out, "
        "bool transpose_weight) -> Tensor");
  m.def("nuts_tree_run_advance(Tensor(a!) z, Tensor(b!) pe, Tensor(c!) grad, Tensor(d!) zq, Tensor(e!) rq, Tensor gq, "
        "Tensor peq, Tensor inv_mass, Tensor(f!) step, int max_tree_depth, bool use_multinomial, int seed, "
        "int chain_offset, Tensor ctl, Tensor(g!) da_state, float target_accept, Tensor(h!) welford, "
        "Tensor(i!) mean_accept, Tensor(j!) counters, Tensor(k!) tc, Tensor(l!) n_done, Tensor(m!)? done_flag, "
        "Tensor? slot2chain, Tensor(n!)? zq_slot, Tensor(o!) accept_prob, Tensor(p!) stats, Tensor(q!) workspace) -> ()");
}

// HIP tensors carry the CUDA dispatch key in a ROCm build of torch
TORCH_LIBRARY_IMPL(pyro_amd, CUDA, m) {
  m.impl("glm_pack_planes", &glm_pack_planes);
  m.impl("glm_bernoulli_planes", &glm_bernoulli_planes);
  m.impl("glm_bernoulli", &glm_bernoulli);
  m.impl("glm_chain", &glm_chain);
  m.impl("adam_step", &adam_step);
  m.impl("dist_log_prob_sum", &dist_log_prob_sum);
  m.impl("multi_log_prob_sum", &multi_log_prob_sum);
  m.impl("meanfield_normal_sample", &meanfield_normal_sample);
  m.impl("exp_site", &exp_site);
  m.impl("exp_site_bwd", &exp_site_bwd);
  m.impl("mvn_tril_sample", &mvn_tril_sample);
  m.impl("logsumexp_terms", &logsumexp_terms);
  m.impl("logchain", &logchain);
  m.impl("logchain_decode", &logchain_decode);
  m.impl("gaussian_hmm", &gaussian_hmm);
  m.impl("gamma_gaussian_hmm", &gamma_gaussian_hmm);
  m.impl("gaussian_hmm_sample", &gaussian_hmm_sample);
  m.impl("gaussian_hmm_smooth", &gaussian_hmm_smooth);
  m.impl("gaussian_hmm_draw", &gaussian_hmm_draw);
  m.impl("linear_hmm_draw", &linear_hmm_draw);
  m.impl("forecast_scores", &forecast_scores);
  m.impl("time_transform", &time_transform);
  m.impl("gp_kernel", &gp_kernel);
  m.impl("gp_kernel_bwd", &gp_kernel_bwd);
  m.impl("mixture_fwd_bwd", &mixture_fwd_bwd);
  m.impl("lda_factor_indexed", &lda_factor_indexed);
  m.impl("tall_linear_act", &tall_linear_act);
  m.impl("nuts_tree_run_advance", &nuts_tree_run_advance);
}
