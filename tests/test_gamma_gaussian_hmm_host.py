"""GammaGaussianHMM on the host: the torch route of distributions/hmm.py (the sequential filter that keeps quad and
logdet apart, differentiated by autograd) against the fixtures of the unmodified reference
(tests/golden/gamma_gaussian_hmm.npz, float64), the two identities the kernel's backward sweep rests on, and the class's
shape rules.  Errors are gaussian_hmm_cases.rel_err = max |got - want| / (1 + max |want|) per array (log_prob: per
element); float64 throughout, tolerance 1e-9, the project's golden tolerance.
"""
import math

import numpy as np
import pytest
import torch

import pyro_amd.distributions as dist
from pyro_amd.distributions import hmm
from tests import gamma_gaussian_hmm_cases as ggc
from tests import gaussian_hmm_cases as gc

TOL64 = 1e-9
F64, CPU = torch.float64, torch.device("cpu")


@pytest.mark.parametrize("case", ggc.CASES)
def test_torch_route_against_the_reference(case):
    """log_prob, all eleven gradients, the Gamma posterior, the normal's loc and the inverse of its covariance"""
    err, per = ggc.errors(ggc.leaves(case, F64, CPU), case, dist)
    print(case, err, {k: "%.1e" % v for k, v in per.items()})
    assert set(per) == {"g_" + k for k in ggc.NAMES} | {"concentration", "rate", "loc", "filter_precision"}
    assert max(err.values()) < TOL64 and max(per.values()) < TOL64, (err, per)


def _weight(t):
    """(w = (a + n/2) / (b + quad/2), quad, n) of the leaves, detached, by the unit-scale filter"""
    with torch.no_grad():
        quad, _, _, _ = hmm._kalman_terms(*gc.build(t, "", dist)._parts, t["x"])
        n = t["x"].shape[-2] * t["x"].shape[-1]
        return (t["a"] + 0.5 * n) / (t["b"] + 0.5 * quad), quad, n


@pytest.mark.parametrize("case", ggc.CASES)
def test_scaled_gaussian_identity(case):
    """the gradient with respect to the nine model leaves is the one of the GAUSSIAN log_prob (the existing
    _kalman_filter) at covariances divided by w, w held constant; at the scale_tril leaves that includes the 1 / w on
    the covariance gradients"""
    g = ggc.golden(case)
    t = ggc.leaves(case, F64, CPU)
    w, _, _ = _weight(t)
    B = t["x"].shape[0]
    w = w.expand(B)
    # the parts as the class lays them out ([..., T | 1, ...] with the series axis in front or absent)
    m0, P0, F, q, Q, H, r, R = gc.build(t, "", dist)._parts
    lp, _, _ = hmm._kalman_filter(m0, P0 / w[:, None, None], F, q, Q / w[:, None, None, None], H, r,
                                  R / w[:, None, None, None], t["x"])
    grads = torch.autograd.grad(lp.sum(), [t[k] for k in gc.NAMES])
    for k, v in zip(gc.NAMES, grads):
        assert gc.rel_err(v.numpy(), g["g_" + k]) < TOL64, k


@pytest.mark.parametrize("case", ggc.CASES)
def test_closed_forms_for_the_gamma(case):
    """d/da = digamma(a + n/2) - digamma(a) + log b - log(b + quad/2), d/db = a / b - w (summed over the series for
    a shared Gamma); the posterior's rate is b + quad/2"""
    g = ggc.golden(case)
    t = ggc.leaves(case, F64, CPU, requires_grad=False)
    w, quad, n = _weight(t)
    a, b = t["a"], t["b"]
    ga = torch.digamma(a + 0.5 * n) - torch.digamma(a) + b.log() - (b + 0.5 * quad).log()
    gb = a / b - w
    assert gc.rel_err(ga.sum_to_size(a.shape).numpy(), g["g_a"]) < TOL64
    assert gc.rel_err(gb.sum_to_size(b.shape).numpy(), g["g_b"]) < TOL64
    assert gc.rel_err((b + 0.5 * quad).numpy(), g["rate"]) < TOL64
    assert gc.rel_err((a + 0.5 * n).expand(quad.shape).numpy(), g["concentration"]) < TOL64


def _model(B=(), T=None, h=3, o=2, scale_batch=(), seed=0, dtype=F64):
    gen = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=gen, dtype=dtype)                            # noqa: E731
    steps = () if T is None else (T,)

    def cov(shape, n):
        A = r(*shape, n, n)
        return A @ A.transpose(-1, -2) / n + 0.5 * torch.eye(n, dtype=dtype)
    F = r(*steps, h, h)
    F = F * (0.9 / torch.linalg.matrix_norm(F, ord=2))[..., None, None]
    a = 1.0 + 3.0 * torch.rand(scale_batch, generator=gen, dtype=dtype)
    b = 0.5 + 2.5 * torch.rand(scale_batch, generator=gen, dtype=dtype)
    parts = dict(a=a, b=b, m0=0.3 * r(*B, h), P0=cov(B, h), F=F, q=0.3 * r(*steps, h), Q=cov(steps, h),
                 H=r(*steps, h, o) / h ** 0.5, r=0.3 * r(*steps, o), R=cov(steps, o))
    return parts


def _build(p, **kw):
    va = kw.get("validate_args")
    return dist.GammaGaussianHMM(dist.Gamma(p["a"], p["b"]), dist.MultivariateNormal(p["m0"], p["P0"]), p["F"],
                                 dist.MultivariateNormal(p["q"], p["Q"]), p["H"],
                                 dist.MultivariateNormal(p["r"], p["R"], validate_args=va), **kw)


def test_shape_rules_expand_and_duration():
    gen = torch.Generator().manual_seed(5)
    # the Gamma's batch shape joins the broadcast
    p = _model(B=(3,), scale_batch=(2, 1))
    d = _build(p)
    assert d.batch_shape == (2, 3) and d.event_shape == (1, 2) and d.duration is None
    assert d.hidden_dim == 3 and d.obs_dim == 2
    # time-homogeneous parameters take data of any length
    for T in (1, 4, 9):
        x = torch.randn(2, 3, T, 2, generator=gen, dtype=F64)
        lp = d.log_prob(x)
        assert lp.shape == (2, 3) and torch.isfinite(lp).all()
        gamma, mvn = d.filter(x)
        assert gamma.batch_shape == (2, 3) and mvn.batch_shape == (2, 3) and mvn.event_shape == (3,)
        assert not gamma.rate.requires_grad and not mvn.loc.requires_grad
    # a value with more leading dims broadcasts; a row of it gives the same
    x = torch.randn(4, 2, 3, 5, 2, generator=gen, dtype=F64)
    lp = d.log_prob(x)
    assert lp.shape == (4, 2, 3) and torch.equal(lp[1], d.log_prob(x[1]))
    # expand: the same numbers on a larger batch shape
    e = d.expand((5, 2, 3))
    assert e.batch_shape == (5, 2, 3) and e.event_shape == (1, 2) and isinstance(e, dist.GammaGaussianHMM)
    assert torch.equal(e.log_prob(x[1]), d.log_prob(x[1]).expand(5, 2, 3))
    assert e.filter(x[1])[0].batch_shape == (5, 2, 3)
    # duration: stated for homogeneous parameters, derived from per-step ones, checked against them
    assert _build(p, duration=7).duration == 7 and _build(p, duration=7).event_shape == (1, 2)
    ph = _model(B=(3,), T=6)
    dh = _build(ph)
    assert dh.duration == 6 and dh.event_shape == (6, 2) and dh.batch_shape == (3,)
    assert dh.log_prob(torch.randn(3, 6, 2, generator=gen, dtype=F64)).shape == (3,)
    with pytest.raises(ValueError):
        _build(ph, duration=5)
    with pytest.raises(ValueError):
        dh.log_prob(torch.randn(3, 5, 2, generator=gen, dtype=F64))
    with pytest.raises(ValueError):
        dh.log_prob(torch.randn(3, 6, 3, generator=gen, dtype=F64))
    # the arguments are checked: a Gamma first, event shapes that fit
    with pytest.raises(ValueError):
        dist.GammaGaussianHMM(dist.Normal(p["a"], p["b"]), dist.MultivariateNormal(p["m0"], p["P0"]), p["F"],
                              dist.MultivariateNormal(p["q"], p["Q"]), p["H"], dist.MultivariateNormal(p["r"], p["R"]))
    with pytest.raises(ValueError):
        dist.GammaGaussianHMM(dist.Gamma(p["a"], p["b"]), dist.MultivariateNormal(p["m0"], p["P0"]), p["F"],
                              dist.MultivariateNormal(p["r"], p["R"]), p["H"], dist.MultivariateNormal(p["r"], p["R"]))
    # torch's own Gamma serves as well
    dt = dist.GammaGaussianHMM(torch.distributions.Gamma(p["a"], p["b"]), dist.MultivariateNormal(p["m0"], p["P0"]),
                               p["F"], dist.MultivariateNormal(p["q"], p["Q"]), p["H"],
                               dist.MultivariateNormal(p["r"], p["R"]))
    assert torch.equal(dt.log_prob(x[1]), d.log_prob(x[1]))
    assert "GammaGaussianHMM" in dist.__all__


def test_independent_normal_observation_noise():
    """Independent(Normal, 1) against the same model with a diagonal MultivariateNormal, values and gradients"""
    p = _model(B=(2,), T=5, seed=3)
    scale = (0.5 + torch.rand(5, 2, generator=torch.Generator().manual_seed(4), dtype=F64)).requires_grad_()
    x = torch.randn(2, 5, 2, generator=torch.Generator().manual_seed(6), dtype=F64)
    args = (dist.Gamma(p["a"], p["b"]), dist.MultivariateNormal(p["m0"], p["P0"]), p["F"],
            dist.MultivariateNormal(p["q"], p["Q"]), p["H"])
    lp_i = dist.GammaGaussianHMM(*args, dist.Independent(dist.Normal(p["r"], scale), 1)).log_prob(x)
    lp_m = dist.GammaGaussianHMM(*args, dist.MultivariateNormal(p["r"], torch.diag_embed(scale * scale))).log_prob(x)
    assert gc.rel_err(lp_i.detach().numpy(), lp_m.detach().numpy()) < 1e-12
    gi, = torch.autograd.grad(lp_i.sum(), scale)
    gm, = torch.autograd.grad(lp_m.sum(), scale)
    assert gc.rel_err(gi.numpy(), gm.numpy()) < 1e-12


def test_gaussian_limit():
    """a = b = A -> infinity: s concentrates at 1 and the model becomes GaussianHMM.  With n = T obs_dim,

        log_prob_t - log_prob_Gaussian = ((quad - n)^2 - 2 n) / (8 A) + O(1 / A^2)

    (Stirling for lgamma(A + n/2) - lgamma(A) and the series of log(1 + quad / 2A)).  At A = 1e6 the first-order term is
    computed here and subtracted; what remains is bounded by the second-order terms, each at most (quad + n)^3 / (8 A^2),
    plus the rounding of the lgamma pair and of A log A against (A + n/2) log(A + quad/2) -- numbers of size A log A ~
    1.4e7 that cancel: 16 float64 epsilons of that."""
    A = 1e6
    p = _model(B=(3,), seed=11)
    p["a"], p["b"] = torch.tensor(A, dtype=F64), torch.tensor(A, dtype=F64)
    x = 2.0 * torch.randn(3, 7, 2, generator=torch.Generator().manual_seed(12), dtype=F64)
    n = 7 * 2
    lp_t = _build(p).log_prob(x)
    gauss = dist.GaussianHMM(dist.MultivariateNormal(p["m0"], p["P0"]), p["F"], dist.MultivariateNormal(p["q"], p["Q"]),
                             p["H"], dist.MultivariateNormal(p["r"], p["R"]))
    lp_g = gauss.log_prob(x)
    quad = -2.0 * (lp_g + hmm._kalman_terms(*gauss._parts, x)[1] + 0.5 * n * math.log(2 * math.pi))
    first = ((quad - n) ** 2 - 2 * n) / (8 * A)
    tol = (quad + n) ** 3 / (8 * A * A) + 16 * 2.0 ** -52 * A * math.log(A)
    print("Gaussian limit: difference", (lp_t - lp_g).numpy(), "first-order term", first.numpy(), "tolerance",
          tol.numpy())
    assert (first.abs() > 10 * tol).any()                 # the term is visible at this A, not lost in the tolerance
    assert ((lp_t - lp_g - first).abs() <= tol).all()
    assert ((lp_t - lp_g).abs() <= first.abs() + tol).all()


def test_a_bad_series_is_nan_alone_on_the_torch_route():
    """(through the filter's own function: a MultivariateNormal cannot be built from such an R)"""
    p = _model(B=(3,), seed=21)
    x = torch.randn(3, 4, 2, generator=torch.Generator().manual_seed(22), dtype=F64)
    parts = list(_build(p)._unit._parts)
    good = hmm._kalman_terms(*parts, x)
    R = parts[7].expand(3, 1, 2, 2).clone()
    R[1] = -40.0 * torch.eye(2, dtype=F64)
    parts[7] = R
    bad = hmm._kalman_terms(*parts, x)
    for u, v in zip(good[:2], bad[:2]):
        assert torch.isnan(v[1]) and torch.equal(u[[0, 2]], v[[0, 2]])
    lp = hmm._student_log_prob(p["a"], p["b"], bad[0], bad[1], 8)
    assert torch.isnan(lp[1]) and torch.isfinite(lp[[0, 2]]).all()


def test_route_choice(monkeypatch):
    """CPU tensors, dimensions over the limit, other dtypes and the switch turned off go to the torch route; ``a`` and
    ``b`` are among the tensors checked; the kernel wrapper is not called."""
    from pyro_amd import kernels
    calls = []
    monkeypatch.setattr(kernels, "gamma_gaussian_hmm_fwd_bwd", lambda *a, **k: calls.append(1) or 1 / 0)
    case = "b3_t7_h3_o2_gamma_shared"
    t = ggc.leaves(case, F64, CPU, requires_grad=False)
    d = ggc.build(t, dist)
    assert not d._takes_kernel(t["x"])
    assert torch.isfinite(d.log_prob(t["x"])).all() and not calls
    # as if the tensors were on the device: the limits, the dtypes and the switch decide
    monkeypatch.setattr(kernels, "on_device", lambda x: True)
    assert d._takes_kernel(t["x"])
    assert not d._takes_kernel(t["x"].to(torch.float16))
    monkeypatch.setattr(hmm, "FUSED_GAUSSIAN_HMM", False)
    assert not d._takes_kernel(t["x"])
    monkeypatch.setattr(hmm, "FUSED_GAUSSIAN_HMM", True)
    t32 = dict(t, a=t["a"].float())
    assert not ggc.build(t32, dist)._takes_kernel(t["x"])                  # a Gamma of another dtype
    monkeypatch.setattr(kernels, "on_device", lambda x: x is not t["b"])
    assert not d._takes_kernel(t["x"])                                     # a rate that is not on the device
    monkeypatch.setattr(kernels, "on_device", lambda x: True)
    p = _model(B=(2,), h=17, o=2)
    assert not _build(p)._takes_kernel(torch.zeros(2, 3, 2, dtype=F64))
    p = _model(B=(2,), h=16, o=16)
    assert _build(p)._takes_kernel(torch.zeros(2, 3, 16, dtype=F64))


def test_typed_op_schema_and_shape_function():
    """pyro_amd::gamma_gaussian_hmm beside pyro_amd::gaussian_hmm: a typed schema and a shape function (no device
    here), and the autograd Function as a named dispatcher op pair"""
    from pyro_amd.csrc.build import build_library, build_torch_ops
    from pyro_amd.ops import contract, torch_library

    build_library()
    build_torch_ops()
    names = torch_library.registered_ops()
    assert torch_library.available() and "pyro_amd::gamma_gaussian_hmm" in names
    assert "pyro_amd::fn_gamma_gaussian_hmm" in names and "pyro_amd::fn_gamma_gaussian_hmm_bwd" in names
    assert contract._GammaGaussianHMM.op_name == "pyro_amd::fn_gamma_gaussian_hmm"
    assert str(torch.ops.pyro_amd.gamma_gaussian_hmm.default._schema) == (
        "pyro_amd::gamma_gaussian_hmm(Tensor concentration, Tensor rate, Tensor m0, Tensor P0, Tensor trans, "
        "Tensor trans_loc, Tensor trans_cov, Tensor obs, Tensor obs_loc, Tensor obs_cov, Tensor x, bool need_grads) -> "
        "(Tensor quad, Tensor logdet, Tensor filter_mean, Tensor filter_cov, Tensor[] grads)")
    m = lambda *sh: torch.empty(sh, device="meta")                                        # noqa: E731
    args = (m(1), m(5), m(1, 3), m(5, 3, 3), m(1, 1, 3, 3), m(5, 7, 3), m(1, 1, 3, 3), m(1, 7, 3, 2), m(1, 1, 2),
            m(5, 1, 2, 2), m(5, 7, 2))
    quad, logdet, fm, fP, grads = torch.ops.pyro_amd.gamma_gaussian_hmm(*args, True)
    assert quad.shape == (5,) and logdet.shape == (5,) and fm.shape == (5, 3) and fP.shape == (5, 3, 3)
    assert [tuple(g.shape) for g in grads] == [(5, 3), (5, 3, 3), (5, 1, 3, 3), (5, 7, 3), (5, 1, 3, 3),
                                               (5, 7, 3, 2), (5, 1, 2), (5, 1, 2, 2), (5, 7, 2)]
    assert torch.ops.pyro_amd.gamma_gaussian_hmm(*args, False)[4] == []


def test_c_abi_argument_errors_before_any_launch():
    from pyro_amd import _lib
    lib = _lib.load()
    assert lib.pa_abi_version() == 9
    f = lib.pa_gamma_gaussian_hmm_fwd_bwd
    none6 = [None, 0, 0] * 6

    def call(B, T, h, o, dtype=_lib.PA_F32):
        return f(dtype, None, 0, None, 0, None, 0, None, 0, *none6, None, B, T, h, o, None, None, None, None,
                 *([None] * 9), None, 0, None)

    assert call(0, 5, 3, 2) == _lib.PA_OK                                  # B = 0: nothing to do
    assert call(2, 0, 3, 2) == _lib.PA_ERR_INVALID                         # T >= 1
    assert call(2, 5, 17, 2) == _lib.PA_ERR_UNSUPPORTED and call(2, 5, 2, 17) == _lib.PA_ERR_UNSUPPORTED
    assert b"gamma_gaussian_hmm" in lib.pa_last_error()
    assert call(2, 5, 3, 2) == _lib.PA_ERR_INVALID and b"NULL" in lib.pa_last_error()
    assert call(2, 5, 3, 2, dtype=7) == _lib.PA_ERR_INVALID
