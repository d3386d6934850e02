"""LinearHMM, IndependentHMM, StudentTReparam and LinearHMMReparam on the host, float64 on the CPU, against the
fixtures of the unmodified reference (tests/golden/linear_hmm.npz): shape rules, the torch route of rsample against the
reference's draws from the same noise, the site log-probabilities of the reparameterised trace with the auxiliary
Gamma sites conditioned to the reference's values, site names, gradients and one SVI step.

Tolerances: draws 1e-12 on gaussian_hmm_cases.rel_err, what tests/test_gaussian_hmm_draw_host.py applies to the
float64 torch route; site log-probabilities rtol 1e-9, what tests/test_gaussian_hmm_host.py applies to log_prob
against the reference."""
import numpy as np
import pytest
import torch

import pyro_amd as pyro
import pyro_amd.distributions as dist
from pyro_amd import kernels, poutine
from pyro_amd.distributions import hmm
from pyro_amd.infer.reparam import LinearHMMReparam, StudentTReparam
from tests import gaussian_hmm_cases as gc
from tests import linear_hmm_cases as lc

F64 = torch.float64
CPU = torch.device("cpu")
TOL_DRAW = 1e-12
RTOL_LP = 1e-9


def _normal(loc, scale):
    """torch's Normal: the package's own draws through the device sampler alone"""
    return dist.Independent(torch.distributions.Normal(loc, scale), 1)


@pytest.fixture
def cpu_backend(oracle_backend, monkeypatch):
    """The elementwise families (the auxiliary Gamma sites, the guide's Normal) answered by the numpy oracle, which
    declares every tensor to be on the device: the state-space kernels, which it does not answer, are switched off."""
    monkeypatch.setattr(hmm, "FUSED_GAUSSIAN_HMM", False)
    monkeypatch.setattr(hmm, "FUSED_LINEAR_HMM", False)
    torch.set_default_dtype(F64)
    yield
    torch.set_default_dtype(torch.float32)


def _draw_case(case, dtype=F64, requires_grad=False):
    g = lc.golden("draw", case)
    t = lc.tensors(g, lc.PARAMS, dtype, CPU, requires_grad)
    noise = [torch.tensor(g[k], dtype=dtype) for k in lc.NOISE]
    S, B, T, o = g["x"].shape
    d = lc.build(t, dist, T, exp=case.endswith("exp"), normal=torch.distributions.Normal)
    return g, t, d, noise, (S, B, T, t["F"].shape[-1], o)


# ---- shapes ------------------------------------------------------------------------------------------------------
def test_shape_rules_and_checks():
    h, o, T = 3, 2, 5
    init = _normal(torch.zeros(h), torch.ones(h))
    trans = dist.StudentT(torch.full((h,), 3.0), torch.zeros(h), torch.ones(h)).to_event(1)
    obs = dist.StudentT(torch.full((o,), 3.0), torch.zeros(o), torch.ones(o)).to_event(1)
    F, H = 0.5 * torch.eye(h), torch.ones(h, o)
    # nothing carries a time axis: one step, no duration, and no draws
    d = dist.LinearHMM(init, F, trans, H, obs)
    assert d.batch_shape == () and d.event_shape == (1, o) and d.duration is None
    assert d.hidden_dim == h and d.obs_dim == o and d.has_rsample and d.transforms == []
    with pytest.raises(ValueError, match="duration"):
        d.rsample()
    with pytest.raises(NotImplementedError, match=r"LinearHMM.log_prob\(\) is not implemented"):
        d.log_prob(torch.zeros(T, o))
    # the duration names the time axis of time-homogeneous parameters
    d = dist.LinearHMM(init, F, trans, H, obs, duration=T)
    assert d.event_shape == (T, o) and d.duration == T and d.rsample((4,)).shape == (4, T, o)
    assert d.transition_matrix.shape == (1, h, h) and d.observation_dist.batch_shape == (1,)
    assert d.support.event_dim == 2
    # the time axis comes from broadcasting, and a duration that contradicts it raises
    d = dist.LinearHMM(init, F.expand(T, h, h), trans, H, obs)
    assert d.event_shape == (T, o) and d.duration == T and d.observation_matrix.shape == (T, h, o)
    assert d.transition_dist.batch_shape == (T,) and d.initial_dist.batch_shape == ()
    with pytest.raises(ValueError, match="duration"):
        dist.LinearHMM(init, F.expand(T, h, h), trans, H, obs, duration=T + 1)
    # batch shapes broadcast; everything is expanded eagerly
    d = dist.LinearHMM(init.expand((4,)), F, trans.expand((1, T)), H.expand(7, 1, 1, h, o), obs)
    assert d.batch_shape == (7, 4) and d.event_shape == (T, o)
    assert d.initial_dist.batch_shape == (7, 4) and d.transition_matrix.shape == (7, 4, T, h, h)
    assert d.observation_dist.batch_shape == (7, 4, T) and d.observation_dist.event_shape == (o,)
    assert d.rsample((2,)).shape == (2, 7, 4, T, o)
    # wrong event shapes and matrices
    for bad in (lambda: dist.LinearHMM(obs, F, trans, H, obs), lambda: dist.LinearHMM(init, F, obs, H, obs),
                lambda: dist.LinearHMM(init, F, trans, H, trans), lambda: dist.LinearHMM(init, H, trans, H, obs),
                lambda: dist.LinearHMM(init, F, trans, torch.ones(o), obs),
                lambda: dist.LinearHMM(init, F, dist.StudentT(3.0, 0.0, 1.0).expand((h,)), H, obs)):
        with pytest.raises(ValueError):
            bad()


def test_expand_and_transforms():
    g, t, d, noise, (S, B, T, h, o) = _draw_case("h3_o2_b2_t5_exp")
    assert len(d.transforms) == 1 and isinstance(d.observation_dist.base_dist, torch.distributions.StudentT)
    assert d.observation_dist.event_shape == (o,) and d.support.event_dim == 2
    e = d.expand((4, B))
    assert e.batch_shape == (4, B) and e.event_shape == (T, o) and e.duration == T and e.transforms is d.transforms
    assert e.initial_dist.batch_shape == (4, B) and e.transition_matrix.shape == (4, B, 1, h, h)
    assert e.observation_dist.batch_shape == (4, B, 1) and e.observation_matrix.shape == (4, B, 1, h, o)
    x = e.rsample((2,))
    assert x.shape == (2, 4, B, T, o) and (x > 0).all()


def test_independent_hmm():
    B, o, T, h = 2, 3, 5, 2
    base = dist.LinearHMM(_normal(torch.zeros(B, o, h), 1.0), 0.5 * torch.eye(h),
                          dist.StudentT(3.0, torch.zeros(h), 1.0).to_event(1), torch.ones(h, 1),
                          dist.StudentT(3.0, torch.zeros(1), 1.0).to_event(1), duration=T)
    d = dist.IndependentHMM(base)
    assert d.batch_shape == (B,) and d.event_shape == (T, o) and d.duration == T and d.has_rsample
    assert d.support.event_dim == 2
    assert d.rsample((4,)).shape == (4, B, T, o)
    e = d.expand((6, B))
    assert e.batch_shape == (6, B) and e.event_shape == (T, o) and e.base_dist.batch_shape == (6, B, o)
    with pytest.raises(NotImplementedError):
        d.log_prob(torch.zeros(B, T, o))
    with pytest.raises(ValueError):
        dist.IndependentHMM(dist.LinearHMM(_normal(torch.zeros(h), 1.0), 0.5 * torch.eye(h),
                                           _normal(torch.zeros(h), 1.0), torch.ones(h, 1),
                                           _normal(torch.zeros(1), 1.0), duration=T))
    # over a GaussianHMM base the log_prob is the sum of the base's
    gb = dist.GaussianHMM(_normal(torch.zeros(B, o, h, dtype=F64), 1.0), 0.5 * torch.eye(h, dtype=F64),
                          _normal(torch.zeros(h, dtype=F64), 0.7), torch.ones(h, 1, dtype=F64),
                          _normal(torch.zeros(1, dtype=F64), 1.3), duration=T)
    x = torch.randn(B, T, o, dtype=F64, generator=torch.Generator().manual_seed(3))
    want = sum(gb.log_prob(x[:, :, i, None].unsqueeze(1))[:, i] for i in range(o))
    got = dist.IndependentHMM(gb).log_prob(x)
    assert got.shape == (B,)
    np.testing.assert_allclose(got.numpy(), want.numpy(), rtol=1e-12)


# ---- draws -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", lc.DRAW_CASES)
def test_draws_against_the_reference(case):
    g, t, d, noise, (S, B, T, h, o) = _draw_case(case)
    assert d.batch_shape == (B,) and d.event_shape == (T, o)
    x = d.rsample((S,), noise=noise)
    err = gc.rel_err(x.numpy(), g["x"])
    print(case, "torch route f64 against the reference %.1e" % err)
    assert x.shape == (S, B, T, o) and err <= TOL_DRAW
    # sample_shape () and a two-dim sample shape
    assert gc.rel_err(d.rsample(noise=[e[0] for e in noise]).numpy(), g["x"][0]) <= TOL_DRAW
    two = d.rsample((S, 1), noise=[e.unsqueeze(1) for e in noise])
    assert two.shape == (S, 1, B, T, o) and gc.rel_err(two[:, 0].numpy(), g["x"]) <= TOL_DRAW


def test_noise_drawn_inside_is_the_components_own_in_the_reference_order():
    g, t, d, noise, (S, B, T, h, o) = _draw_case("h3_o2_b3_t7_Fhet")
    torch.manual_seed(7)
    init = d.initial_dist.rsample((S,))
    e = d.transition_dist.expand((B, T)).rsample((S,))
    n = d.observation_dist.expand((B, T)).rsample((S,))
    want = d.rsample((S,), noise=(init, e, n))
    torch.manual_seed(7)
    assert torch.equal(d.rsample((S,)), want)


def test_bad_noise_shapes_raise():
    g, t, d, (init, e, n), (S, B, T, h, o) = _draw_case("h3_o2_b3_t7_Hhet")
    for bad in ((init[:2], e, n), (init, e[:, :, 1:], n), (init, e, n[..., :1]), (init, e), (init, n, e),
                (init[0], e[0], n[0])):
        with pytest.raises(ValueError, match="expected noise"):
            d.rsample((S,), noise=bad)


def test_route_choice(monkeypatch):
    """the kernel route is taken for device tensors alone: with the device test and the wrapper patched, a CPU model
    goes to the wrapper exactly when the switch is on, the dimensions are within the limits and nothing needs a
    gradient"""
    case = "h3_o2_b3_t7_Fhet"
    g, t, d, noise, (S, B, T, h, o) = _draw_case(case)
    calls = []

    def fake(*args, **kw):
        calls.append((args, kw))
        init = args[3]
        return init.new_zeros(init.shape[:2] + (T, o)), None
    monkeypatch.setattr(kernels, "linear_hmm_draw", fake)
    assert d.rsample((S,), noise=noise).abs().sum() > 0 and not calls            # CPU tensors: the loop
    monkeypatch.setattr(kernels, "on_device", lambda t: True)
    x = d.rsample((S,), noise=noise)
    assert len(calls) == 1 and x.shape == (S, B, T, o) and not x.any()
    args, kw = calls[0]
    assert len(args) == 6 and args[2] == T and not kw
    # F per series and per step, H shared and time-homogeneous: the eager expansion is undone
    assert tuple(args[0].shape) == (B, T, h, h) and tuple(args[1].shape) == (1, 1, h, o)
    assert [tuple(a.shape) for a in args[3:]] == [(S, B, h), (S, B, T, h), (S, B, T, o)]
    assert torch.equal(args[3], noise[0]) and all(a.is_contiguous() for a in args[:2] + args[3:])
    # noise drawn inside, parameters without a gradient: still the kernel
    assert d.rsample((2, 2)).shape == (2, 2, B, T, o) and len(calls) == 2
    assert tuple(calls[1][0][4].shape) == (4, B, T, h)
    # the switch
    monkeypatch.setattr(hmm, "FUSED_LINEAR_HMM", False)
    assert d.rsample((S,), noise=noise).any() and len(calls) == 2
    monkeypatch.setattr(hmm, "FUSED_LINEAR_HMM", True)
    # something needs a gradient under grad mode: the loop; under no_grad: the kernel
    _, tg, dg, _, _ = _draw_case(case, requires_grad=True)
    assert dg.rsample((S,), noise=noise).requires_grad and len(calls) == 2
    assert dg.rsample((S,)).requires_grad and len(calls) == 2
    with torch.no_grad():
        assert not dg.rsample((S,), noise=noise).requires_grad and len(calls) == 3
    # mixed dtypes and dimensions over the limit: the loop
    with pytest.raises(RuntimeError):
        d.rsample((S,), noise=[e.float() for e in noise])
    assert len(calls) == 3
    nh = kernels.GAUSSIAN_HMM_MAX_HIDDEN + 1
    wide = dist.LinearHMM(_normal(torch.zeros(nh), 1.0), 0.5 * torch.eye(nh),
                          _normal(torch.zeros(nh), 1.0), torch.ones(nh, 2) / nh,
                          _normal(torch.zeros(2), 1.0), duration=3)
    assert wide.rsample((4,)).shape == (4, 3, 2) and len(calls) == 3


def test_wrapper_and_op_are_declared():
    from pyro_amd import _lib
    from pyro_amd.ops import torch_library
    assert "pa_linear_hmm_draw" in _lib._SIGNATURES and callable(kernels.linear_hmm_draw)
    assert torch_library.available() and "pyro_amd::linear_hmm_draw" in torch_library.registered_ops()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        z = torch.zeros
        kernels.linear_hmm_draw(z(1, 1, 2, 2), z(1, 1, 2, 1), 3, z(4, 1, 2), z(4, 1, 3, 2), z(4, 1, 3, 1))


# ---- gradients ---------------------------------------------------------------------------------------------------
def test_gradients_against_finite_differences():
    """rsample under grad mode is differentiable in F, H and a component's scale: autograd against a central
    difference in float64, along one random direction per tensor.  The draws of a StudentT are reparameterised in
    its scale as loc + scale * (standard draw), so with the generator reseeded the perturbed draws are the same
    standard draws at another scale."""
    case = "h3_o2_b3_t7_Fhet"
    g = lc.golden("draw", case)
    S, B, T, o = g["x"].shape
    w = torch.randn(S, B, T, o, dtype=F64, generator=torch.Generator().manual_seed(1))

    def f(t):
        torch.manual_seed(13)
        return (lc.build(t, dist, T, normal=torch.distributions.Normal).rsample((S,)) * w).sum()

    t = lc.tensors(g, lc.PARAMS, F64, CPU)
    for k in ("F", "H", "obs_scale", "trans_scale"):
        t[k].requires_grad_(True)
    out = f(t)
    assert out.requires_grad
    names = ("F", "H", "obs_scale", "trans_scale")
    grads = torch.autograd.grad(out, [t[k] for k in names])
    gen = torch.Generator().manual_seed(2)
    for k, gr in zip(names, grads):
        v = torch.randn(t[k].shape, dtype=F64, generator=gen)
        eps = 1e-6
        with torch.no_grad():
            hi = f({**t, k: t[k] + eps * v})
            lo = f({**t, k: t[k] - eps * v})
        fd, ad = float((hi - lo) / (2 * eps)), float((gr * v).sum())
        print(k, "finite difference %.10e autograd %.10e" % (fd, ad))
        # a central difference at eps = 1e-6 in float64: truncation eps^2, rounding 1e-16 / eps, both relative
        assert abs(fd - ad) <= 1e-7 * (1 + abs(ad)), k


# ---- the reparameterised trace -----------------------------------------------------------------------------------
def _rep_model(case, dtype=F64, device=CPU, requires_grad=(), plate=False):
    parts, indep, exp = lc.REP_CASES[case]
    g = lc.golden("rep", case)
    t = lc.tensors(g, lc.PARAMS + ("init_df", "x"), dtype, device)
    for k in requires_grad:
        t[k].requires_grad_(True)
    T = t["x"].shape[-2]

    def model():
        d = lc.build(t, dist, T, exp=exp, normal=torch.distributions.Normal)
        if indep:
            d = dist.IndependentHMM(d)
        if plate:           # (inference checks that every batch dim is a declared plate)
            with pyro.plate("series", t["x"].shape[0], dim=-1):
                return pyro.sample("hmm", d, obs=t["x"])
        return pyro.sample("hmm", d, obs=t["x"])

    rep = LinearHMMReparam(**{p: StudentTReparam() for p in parts})
    aux = {str(s): torch.tensor(g["value_" + str(s)], dtype=dtype, device=device) for s in g["sites"] if s != "hmm"}
    return g, t, poutine.reparam(model, config={"hmm": rep}), aux


@pytest.mark.parametrize("case", lc.REP_CASES)
def test_site_names_and_log_probs_against_the_reference(case, cpu_backend):
    g, t, model, aux = _rep_model(case)
    tr = poutine.trace(poutine.condition(model, data=aux)).get_trace()
    tr.compute_log_prob()
    sites = [s for s, site in tr.nodes.items() if site["type"] == "sample"]
    assert sites == [str(s) for s in g["sites"]]
    parts = lc.REP_CASES[case][0]
    assert sites == ["hmm_%s_gamma" % p for p in parts] + ["hmm"]
    for s in sites:
        got, want = tr.nodes[s]["log_prob"].detach().numpy(), g["log_prob_" + s]
        print(case, s, "max relative error %.1e" % np.max(np.abs(got - want) / np.abs(want)))
        assert got.shape == want.shape
        np.testing.assert_allclose(got, want, rtol=RTOL_LP)
    assert tr.nodes["hmm"]["is_observed"] and tr.nodes["hmm"]["value"] is t["x"]
    fn = tr.nodes["hmm"]["fn"]
    if lc.REP_CASES[case][2]:
        assert isinstance(fn, torch.distributions.TransformedDistribution)
        assert isinstance(fn.base_dist, dist.GaussianHMM)
    elif lc.REP_CASES[case][1]:
        assert isinstance(fn, dist.IndependentHMM) and isinstance(fn.base_dist, dist.GaussianHMM)
    else:
        assert isinstance(fn, dist.GaussianHMM) and fn.duration == t["x"].shape[-2]


def test_auxiliary_sites_are_drawn_when_not_conditioned(cpu_backend):
    g, t, model, aux = _rep_model("trans_obs")
    pyro.set_rng_seed(0)
    tr = poutine.trace(model).get_trace()
    for s, v in aux.items():
        got = tr.nodes[s]["value"]
        assert got.shape == v.shape and (got > 0).all() and not tr.nodes[s]["is_observed"]
    assert torch.isfinite(tr.log_prob_sum())


def test_reparam_needs_a_duration():
    h = 2
    d = dist.LinearHMM(_normal(torch.zeros(h), 1.0), 0.5 * torch.eye(h),
                       dist.StudentT(3.0, torch.zeros(h), 1.0).to_event(1), torch.ones(h, 1),
                       dist.StudentT(3.0, torch.zeros(1), 1.0).to_event(1))
    with pytest.raises(ValueError, match="duration"):
        LinearHMMReparam(trans=StudentTReparam()).apply({"name": "hmm", "fn": d, "value": None, "is_observed": False})


def test_svi_step(cpu_backend):
    from pyro_amd.infer import SVI, Trace_ELBO
    from pyro_amd.infer.autoguide import AutoNormal
    g, t, model, aux = _rep_model("trans_obs", plate=True)
    pyro.clear_param_store()
    pyro.set_rng_seed(1)
    guide = AutoNormal(model)
    svi = SVI(model, guide, pyro.optim.Adam({"lr": 0.01}), Trace_ELBO())
    loss = svi.step()
    assert np.isfinite(loss)
    assert {"AutoNormal.locs.hmm_trans_gamma", "AutoNormal.locs.hmm_obs_gamma"} <= set(pyro.get_param_store().keys())
    pyro.clear_param_store()
