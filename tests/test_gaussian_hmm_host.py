"""GaussianHMM without a device: the plain-torch sequential filter of pyro_amd/distributions/hmm.py (the route of
CPU tensors, and the float64 restatement the kernel is tested against) on the fixtures of the unmodified reference
(tests/golden/gaussian_hmm.npz); shapes, expand, prefix_condition, constructor errors, route choice, rsample.

Tolerance: 1e-9, the project's golden tolerance for float64, on |got - want| / (1 + max |want|) for values,
gradients and filter moments (the filter measured 1e-13 .. 2e-12 when the fixtures were made)."""
import math

import numpy as np
import pytest
import torch

import pyro_amd.distributions as dist
from pyro_amd import kernels
from pyro_amd.distributions import hmm
from tests import gaussian_hmm_cases as gc

TOL = 1e-9
CPU = torch.device("cpu")


@pytest.mark.parametrize("case", gc.CASES)
def test_torch_route_matches_the_reference(case):
    g = gc.golden(case)
    t = gc.leaves(case, torch.float64, CPU)
    lp, grads = gc.value_and_grads(t, case, dist)
    err = {"log_prob": float(np.max(np.abs(lp - g["log_prob"]) / (1 + np.abs(g["log_prob"]))))}
    for k in gc.NAMES:
        err["g_" + k] = gc.rel_err(grads[k], g["g_" + k])
    post = gc.build(t, case, dist).filter(t["x"])
    assert not post.loc.requires_grad and not post.covariance_matrix.requires_grad
    err["filter_mean"] = gc.rel_err(post.loc.numpy(), g["filter_mean"])
    err["filter_cov"] = gc.rel_err(post.covariance_matrix.numpy(), g["filter_cov"])
    print(case, {k: "%.1e" % v for k, v in err.items()})
    assert max(err.values()) < TOL, err


def test_torch_classes_and_other_parametrisations_reach_the_callers_tensors():
    """torch's own distribution classes; covariance_matrix, precision_matrix and scale: same value, and the
    gradient arrives at the tensor the caller made."""
    import torch.distributions as td
    case = "b2_t9_h4_o3_het"
    g = gc.golden(case)
    t = gc.leaves(case, torch.float64, CPU)
    cov = lambda L: L @ L.transpose(-1, -2)                                               # noqa: E731
    P0 = cov(t["L0"]).detach().requires_grad_()
    Qp = torch.linalg.inv(cov(t["Lq"])).detach().requires_grad_()
    d = dist.GaussianHMM(td.MultivariateNormal(t["m0"], covariance_matrix=P0), t["F"],
                         td.MultivariateNormal(t["q"], precision_matrix=Qp), t["H"],
                         td.MultivariateNormal(t["r"], scale_tril=t["Lr"]))
    lp = d.log_prob(t["x"])
    np.testing.assert_allclose(lp.detach().numpy(), g["log_prob"], rtol=1e-9)
    gP0, gQp, gm0 = torch.autograd.grad(lp.sum(), [P0, Qp, t["m0"]])
    assert gP0.abs().max() > 0 and gQp.abs().max() > 0
    assert gc.rel_err(gm0.numpy(), g["g_m0"]) < TOL
    # Independent(Normal): the scale
    case = "b3_t6_h3_o2_indep"
    t = gc.leaves(case, torch.float64, CPU)
    d = dist.GaussianHMM(td.MultivariateNormal(t["m0"], scale_tril=t["L0"]), t["F"],
                         td.MultivariateNormal(t["q"], scale_tril=t["Lq"]), t["H"],
                         td.Independent(td.Normal(t["r"], t["Lr"]), 1))
    gs, = torch.autograd.grad(d.log_prob(t["x"]).sum(), [t["Lr"]])
    assert gc.rel_err(gs.numpy(), gc.golden(case)["g_Lr"]) < TOL


def test_shapes_and_expand():
    t = gc.leaves("b3_t7_h3_o2_shared", torch.float64, CPU, requires_grad=False)
    d = gc.build(t, "b3_t7_h3_o2_shared", dist)
    assert d.batch_shape == (3,) and d.event_shape == (1, 2) and d.duration is None     # time-homogeneous
    assert d.hidden_dim == 3 and d.obs_dim == 2 and d.has_rsample
    assert d.support.event_dim == 2
    # ... and takes data of any length
    lp7 = d.log_prob(t["x"])
    lp4 = d.log_prob(t["x"][:, :4])
    assert lp7.shape == lp4.shape == (3,) and not torch.equal(lp7, lp4)
    e = d.expand((5, 3))
    assert e.batch_shape == (5, 3) and e.event_shape == (1, 2) and e.hidden_dim == 3
    torch.testing.assert_close(e.log_prob(t["x"]), lp7.expand(5, 3), rtol=1e-12, atol=0)
    h = gc.build(gc.leaves("b2_t9_h4_o3_het", torch.float64, CPU, False), "b2_t9_h4_o3_het", dist)
    assert h.batch_shape == (2,) and h.event_shape == (9, 3) and h.duration == 9
    with pytest.raises(ValueError, match="time steps"):
        h.log_prob(torch.zeros(2, 5, 3, dtype=torch.float64))
    d9 = dist.GaussianHMM(dist.MultivariateNormal(t["m0"], scale_tril=t["L0"]), t["F"],
                          dist.MultivariateNormal(t["q"], scale_tril=t["Lq"]), t["H"],
                          dist.MultivariateNormal(t["r"], scale_tril=t["Lr"]), duration=9)
    assert d9.duration == 9 and d9.event_shape == (1, 2)
    assert d9.rsample((4,)).shape == (4, 3, 9, 2)


@pytest.mark.parametrize("case", ["b3_t7_h3_o2_shared", "b2_t9_h4_o3_het"])
def test_prefix_condition_is_filter_plus_slicing(case):
    """p(x) = p(x[:t]) p(x[t:] | x[:t]); the conditional's initial distribution is filter(x[:t])"""
    t = gc.leaves(case, torch.float64, CPU, requires_grad=False)
    T = t["x"].shape[-2]
    d = gc.build(t, case, dist)
    if d.duration is None:
        d = dist.GaussianHMM(dist.MultivariateNormal(t["m0"], scale_tril=t["L0"]), t["F"],
                             dist.MultivariateNormal(t["q"], scale_tril=t["Lq"]), t["H"],
                             dist.MultivariateNormal(t["r"], scale_tril=t["Lr"]), duration=T)
    k = 3
    right = d.prefix_condition(t["x"][:, :k])
    assert right.duration == T - k and right.batch_shape == d.batch_shape
    left = d.log_prob(t["x"][:, :k]) if d.event_shape[0] == 1 else None
    if left is None:        # heterogeneous: the first k steps' parameters
        parts = d._parts[:2] + tuple(p.narrow(-nd - 1, 0, k) for p, nd in zip(d._parts[2:], (2, 1, 2, 2, 1, 2)))
        left_d = dist.GaussianHMM._from_parts(parts, k, None)
        left = left_d.log_prob(t["x"][:, :k])
        post = left_d.filter(t["x"][:, :k])
    else:
        post = d.filter(t["x"][:, :k])
    torch.testing.assert_close(right._parts[0], post.loc, rtol=0, atol=0)
    torch.testing.assert_close(left + right.log_prob(t["x"][:, k:]), d.log_prob(t["x"]), rtol=1e-11, atol=1e-11)
    with pytest.raises(ValueError):
        d.prefix_condition(t["x"])                      # nothing left to condition


def test_constructor_errors():
    t = gc.leaves("b3_t7_h3_o2_shared", torch.float64, CPU, requires_grad=False)
    init = dist.MultivariateNormal(t["m0"], scale_tril=t["L0"])
    trans = dist.MultivariateNormal(t["q"], scale_tril=t["Lq"])
    obs = dist.MultivariateNormal(t["r"], scale_tril=t["Lr"])
    with pytest.raises(ValueError, match="initial_dist"):
        dist.GaussianHMM(torch.distributions.Normal(t["m0"], 1.0), t["F"], trans, t["H"], obs)
    with pytest.raises(ValueError, match="transition_dist"):
        dist.GaussianHMM(init, t["F"], torch.distributions.Gamma(t["q"].exp(), 1.0), t["H"], obs)
    with pytest.raises(ValueError, match="observation_dist"):
        dist.GaussianHMM(init, t["F"], trans, t["H"], torch.distributions.Independent(
            torch.distributions.Laplace(t["r"], 1.0), 1))
    with pytest.raises(ValueError, match="transition_matrix"):
        dist.GaussianHMM(init, [[1.0]], trans, t["H"], obs)
    with pytest.raises(ValueError, match="observation_matrix"):
        dist.GaussianHMM(init, t["F"], trans, None, obs)
    with pytest.raises(ValueError, match="dims"):
        dist.GaussianHMM(init, t["F"], trans, t["H"][:2], obs)             # hidden 2 against 3
    with pytest.raises(ValueError, match="duration"):
        het = gc.leaves("b2_t9_h4_o3_het", torch.float64, CPU, False)
        dist.GaussianHMM(dist.MultivariateNormal(het["m0"], scale_tril=het["L0"]), het["F"],
                         dist.MultivariateNormal(het["q"], scale_tril=het["Lq"]), het["H"],
                         dist.MultivariateNormal(het["r"], scale_tril=het["Lr"]), duration=4)
    d = dist.GaussianHMM(init, t["F"], trans, t["H"], obs)
    with pytest.raises(ValueError, match="duration"):
        d.rsample()
    with pytest.raises(ValueError, match="value"):
        d.log_prob(torch.zeros(3, 7, 5, dtype=torch.float64))


def test_route_choice(monkeypatch):
    """CPU tensors and dimensions over the limit go to the torch route, and so does everything with the switch
    off; the kernel wrapper is not called."""
    calls = []
    monkeypatch.setattr(kernels, "gaussian_hmm_fwd_bwd", lambda *a, **k: calls.append(1) or 1 / 0)
    t = gc.leaves("b3_t7_h3_o2_shared", torch.float64, CPU, requires_grad=False)
    d = gc.build(t, "b3_t7_h3_o2_shared", dist)
    assert not d._takes_kernel(t["x"])
    assert torch.isfinite(d.log_prob(t["x"])).all() and not calls
    assert kernels.GAUSSIAN_HMM_MAX_HIDDEN >= 16 and kernels.GAUSSIAN_HMM_MAX_OBS >= 16
    # as if the tensors were on the device: the limits and the dtype decide
    monkeypatch.setattr(kernels, "on_device", lambda x: True)
    assert d._takes_kernel(t["x"])
    monkeypatch.setattr(hmm, "FUSED_GAUSSIAN_HMM", False)
    assert not d._takes_kernel(t["x"])
    monkeypatch.setattr(hmm, "FUSED_GAUSSIAN_HMM", True)
    for h, o, want in ((kernels.GAUSSIAN_HMM_MAX_HIDDEN, kernels.GAUSSIAN_HMM_MAX_OBS, True),
                       (kernels.GAUSSIAN_HMM_MAX_HIDDEN + 1, 2, False), (2, kernels.GAUSSIAN_HMM_MAX_OBS + 1, False)):
        eye = lambda n: torch.eye(n, dtype=torch.float64)                                 # noqa: E731
        big = dist.GaussianHMM(dist.MultivariateNormal(torch.zeros(h, dtype=torch.float64), eye(h)), 0.5 * eye(h),
                               dist.MultivariateNormal(torch.zeros(h, dtype=torch.float64), eye(h)),
                               torch.ones(h, o, dtype=torch.float64) / h,
                               dist.MultivariateNormal(torch.zeros(o, dtype=torch.float64), eye(o)))
        x = torch.zeros(3, o, dtype=torch.float64)
        assert big._takes_kernel(x) is want, (h, o)
        assert not big._takes_kernel(x.to(torch.float16))
    monkeypatch.undo()
    assert torch.isfinite(big.log_prob(x))              # over the limit, on the CPU: the torch route


def test_typed_op_schema_and_shape_function():
    """pyro_amd::gaussian_hmm beside pyro_amd::logchain: a typed schema and a shape function (no device here),
    and the autograd Function as a named dispatcher op pair"""
    from pyro_amd.csrc.build import build_library, build_torch_ops
    from pyro_amd.ops import contract, torch_library

    build_library()
    build_torch_ops()
    names = torch_library.registered_ops()
    assert torch_library.available() and "pyro_amd::gaussian_hmm" in names
    assert "pyro_amd::fn_gaussian_hmm" in names and "pyro_amd::fn_gaussian_hmm_bwd" in names
    assert contract._GaussianHMM.op_name == "pyro_amd::fn_gaussian_hmm"
    assert str(torch.ops.pyro_amd.gaussian_hmm.default._schema) == (
        "pyro_amd::gaussian_hmm(Tensor m0, Tensor P0, Tensor trans, Tensor trans_loc, Tensor trans_cov, Tensor obs, "
        "Tensor obs_loc, Tensor obs_cov, Tensor x, bool need_grads) -> (Tensor log_prob, Tensor filter_mean, "
        "Tensor filter_cov, Tensor[] grads)")
    m = lambda *sh: torch.empty(sh, device="meta")                                        # noqa: E731
    lp, fm, fP, grads = torch.ops.pyro_amd.gaussian_hmm(m(1, 3), m(5, 3, 3), m(1, 1, 3, 3), m(5, 7, 3), m(1, 1, 3, 3),
                                                        m(1, 7, 3, 2), m(1, 1, 2), m(5, 1, 2, 2), m(5, 7, 2), True)
    assert lp.shape == (5,) and fm.shape == (5, 3) and fP.shape == (5, 3, 3)
    assert [tuple(g.shape) for g in grads] == [(5, 3), (5, 3, 3), (5, 1, 3, 3), (5, 7, 3), (5, 1, 3, 3),
                                               (5, 7, 3, 2), (5, 1, 2), (5, 1, 2, 2), (5, 7, 2)]
    assert torch.ops.pyro_amd.gaussian_hmm(m(1, 3), m(5, 3, 3), m(1, 1, 3, 3), m(5, 7, 3), m(1, 1, 3, 3), m(1, 7, 3, 2),
                                           m(1, 1, 2), m(5, 1, 2, 2), m(5, 7, 2), False)[3] == []


def test_c_abi_argument_errors_before_any_launch():
    from pyro_amd import _lib
    lib = _lib.load()
    f = lib.pa_gaussian_hmm_fwd_bwd
    none6 = [None, 0, 0] * 6

    def call(B, T, h, o, dtype=_lib.PA_F32):
        return f(dtype, None, 0, None, 0, *none6, None, B, T, h, o, None, None, None, *([None] * 9), None, 0, None)

    assert call(0, 5, 3, 2) == _lib.PA_OK                                  # B = 0: nothing to do
    assert call(2, 0, 3, 2) == _lib.PA_ERR_INVALID                         # T >= 1
    assert call(2, 5, 17, 2) == _lib.PA_ERR_UNSUPPORTED and call(2, 5, 2, 17) == _lib.PA_ERR_UNSUPPORTED
    assert call(2, 5, 3, 2) == _lib.PA_ERR_INVALID and b"NULL" in lib.pa_last_error()
    assert call(2, 5, 3, 2, dtype=7) == _lib.PA_ERR_INVALID
    # the per-step workspace exists only for the backward sweep: hidden + hidden^2 elements per step and sequence
    assert lib.pa_gaussian_hmm_workspace(_lib.PA_F32, 4, 10, 3, 2, 0) == 0
    assert lib.pa_gaussian_hmm_workspace(_lib.PA_F32, 4, 10, 3, 2, 1) == 4 * 10 * (3 + 9) * 4
    assert lib.pa_gaussian_hmm_workspace(_lib.PA_F64, 4, 10, 3, 2, 1) == 4 * 10 * (3 + 9) * 8


def test_rsample_moments():
    """the mean of 20 000 draws of the last observation within 5 standard errors of the analytic mean"""
    torch.manual_seed(0)
    t = gc.leaves("b3_t7_h3_o2_shared", torch.float64, CPU, requires_grad=False)
    T, n = 7, 20000
    d = dist.GaussianHMM(dist.MultivariateNormal(t["m0"][0], scale_tril=t["L0"][0]), t["F"],
                         dist.MultivariateNormal(t["q"], scale_tril=t["Lq"]), t["H"],
                         dist.MultivariateNormal(t["r"], scale_tril=t["Lr"]), duration=T)
    x = d.rsample((n,))
    assert x.shape == (n, T, 2)
    cov = lambda L: L @ L.T                                                               # noqa: E731
    m, P = t["m0"][0], cov(t["L0"][0])
    for _ in range(T):
        m = m @ t["F"] + t["q"]
        P = t["F"].T @ P @ t["F"] + cov(t["Lq"])
    mean = m @ t["H"] + t["r"]
    var = (t["H"].T @ P @ t["H"] + cov(t["Lr"])).diagonal()
    got = x[:, -1].mean(0)
    assert ((got - mean).abs() < 5 * (var / n).sqrt()).all(), (got, mean)
    assert abs(x[:, -1].var(0) / var - 1).max() < 5 * math.sqrt(2.0 / n)
