"""contrib.gp on the CPU (no GPU needed), against tests/golden/gp.npz -- the UNMODIFIED reference in float64 -- and
against the float64 restatement by direct differences (tests/gp_cases.py).

(a) every kernel class, ``conditional``, the models' losses, gradients and ``forward`` at 1e-12 relative to
    1 + the largest entry;
(b) the ten training losses within ten times the deviation the reference shows against itself when y is perturbed by
    1e-13 relative, entry by entry (the rule of tests/test_forecast_host.py);
(c) ``Parameterized``: parameter names, constraints, modes, re-``autoguide``, the auxiliary site of a non-real support;
(d) shape and argument errors; CPU tensors never reach kernels.gp_kernel_*;
(e) the restatement's closed-form derivatives against autograd, and the restatement against the torch route in float64
    per entry within 2^-52 (D + 8) (|x/l|^2 + |z/l|^2) |variance f'(r2)| + 1e-15: the first-order conditioning of the
    expansion r2 = X2 - 2 X Z^T + Z2, not a measurement."""
import numpy as np
import pytest
import torch

import pyro_amd as pyro
import pyro_amd.contrib.gp as gp
import pyro_amd.distributions as dist
from pyro_amd import poutine
from pyro_amd.infer import Trace_ELBO
from pyro_amd.nn import PyroSample

from . import gp_cases as gc

F64 = torch.float64


def _close(got, want, rtol=1e-12):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (got.shape, want.shape)
    bound = rtol * (1 + np.abs(want).max()) if want.size else 0.0
    assert np.abs(got - want).max(initial=0.0) <= bound, (np.abs(got - want).max(), bound)


@pytest.fixture
def cpu_backend(oracle_backend):
    """The numpy oracle answers the ELBO's assembly for CPU tensors (tests/oracle_backend.py).  It declares every tensor
    to be on the device; the GP kernels route by ``is_cuda`` itself, so their switch stays on."""
    torch.set_default_dtype(F64)
    yield
    torch.set_default_dtype(torch.float32)


# ---- (a) ------------------------------------------------------------------------------------------------------------
def test_kernel_classes_match_the_reference():
    g, data = gc.golden(), gc.fixture_data()
    table = gc.kernel_table(gp)
    assert sorted(k.split("/")[1] for k in g if k.startswith("kern/") and k.endswith("/K")) == sorted(table)
    for kid, kern in table.items():
        with torch.no_grad():
            _close(kern(data["X"]).numpy(), g["kern/%s/K" % kid])
            _close(kern(data["X"], data["Xnew"]).numpy(), g["kern/%s/KZ" % kid])
            _close(kern(data["X"], diag=True).numpy(), g["kern/%s/diag" % kid])


@pytest.mark.parametrize("scale,whiten,full", gc.CONDITIONAL_CASES)
def test_conditional_matches_the_reference(scale, whiten, full):
    g, data = gc.golden(), gc.fixture_data()
    kern = gc.kernel_table(gp)["matern52_ard"]
    with torch.no_grad():
        loc, cov = gp.util.conditional(data["Xnew"], data["X"], kern, data["f_loc"],
                                       data["f_scale_tril"] if scale else None, full_cov=full, whiten=whiten)
    key = "cond/%d%d%d/" % (scale, whiten, full)
    _close(loc.numpy(), g[key + "loc"])
    _close(cov.numpy(), g[key + "cov"])


@pytest.mark.parametrize("name", gc.MODELS)
@pytest.mark.parametrize("variant", ["plain", "prior"])
def test_model_loss_and_gradients_match_the_reference(name, variant, cpu_backend):
    g, data = gc.golden(), gc.fixture_data()
    model = gc.build_model(gp, name, data, prior=(PyroSample, dist) if variant == "prior" else None)
    loss, grads = gc.loss_and_grads(model, Trace_ELBO())
    key = "model/%s/%s/" % (name, variant)
    _close(loss, g[key + "loss"])
    want = sorted(k[len(key + "grad_"):] for k in g if k.startswith(key + "grad_"))
    assert sorted(grads) == want
    for pname in want:
        _close(grads[pname], g[key + "grad_" + pname])


@pytest.mark.parametrize("name", gc.MODELS)
def test_model_forward_matches_the_reference(name):
    g, data = gc.golden(), gc.fixture_data()
    model = gc.build_model(gp, name, data)
    for full, noiseless in gc.FORWARD_CASES:
        with torch.no_grad():
            loc, cov = model(data["Xnew"], full_cov=full, noiseless=noiseless)
        key = "model/%s/forward/%d%d/" % (name, full, noiseless)
        _close(loc.numpy(), g[key + "loc"])
        _close(cov.numpy(), g[key + "cov"])


# ---- (b) ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", gc.MODELS)
def test_training_losses_within_the_reference_sensitivity(name, cpu_backend):
    g, data = gc.golden(), gc.fixture_data()
    model = gc.build_model(gp, name, data)
    losses = np.array(gp.util.train(model, torch.optim.Adam(model.parameters(), lr=0.01), num_steps=gc.TRAIN_STEPS))
    want, other = g["model/%s/train" % name], g["model/%s/p_train" % name]
    allowed = gc.allowed(want, other)
    dev = np.abs(losses - want)
    print("%s: largest deviation %.2e, allowed there %.2e" % (name, dev.max(), allowed[dev.argmax()]))
    assert losses.shape == (gc.TRAIN_STEPS,) and (dev <= allowed).all(), (dev, allowed)


def test_train_defaults_run_and_lower_the_loss(cpu_backend):
    model = gc.build_model(gp, "gpr", gc.fixture_data())
    losses = gp.util.train(model, num_steps=5)
    assert len(losses) == 5 and losses[-1] < losses[0]


# ---- (c) ------------------------------------------------------------------------------------------------------------
def test_parameterized_names_constraints_and_reautoguide(cpu_backend):
    kern = gp.kernels.RBF(3, lengthscale=torch.ones(3))
    assert sorted(n for n, _ in kern.named_parameters()) == ["lengthscale_unconstrained", "variance_unconstrained"]
    kern.lengthscale = PyroSample(dist.LogNormal(torch.zeros(3), torch.ones(3)).to_event())
    assert sorted(n for n, _ in kern.named_parameters()) == ["lengthscale_map_unconstrained", "variance_unconstrained"]
    assert (kern.lengthscale_map > 0).all() and kern.lengthscale_map.shape == (3,)
    kern.autoguide("lengthscale", dist.Normal)
    names = sorted(n for n, _ in kern.named_parameters())
    assert names == ["lengthscale_loc", "lengthscale_scale_unconstrained", "variance_unconstrained"]
    assert torch.equal(kern.lengthscale_scale, torch.ones(3))
    kern.autoguide("lengthscale", dist.MultivariateNormal)
    names = sorted(n for n, _ in kern.named_parameters())
    assert names == ["lengthscale_loc", "lengthscale_scale_tril_unconstrained", "variance_unconstrained"]
    assert torch.equal(kern.lengthscale_scale_tril, torch.eye(3))
    kern.autoguide("lengthscale", dist.Delta)
    assert sorted(n for n, _ in kern.named_parameters()) == ["lengthscale_map_unconstrained", "variance_unconstrained"]
    with pytest.raises(ValueError, match="no prior"):
        kern.autoguide("variance", dist.Normal)
    with pytest.raises(NotImplementedError):
        kern.autoguide("lengthscale", dist.Gamma)
    with pytest.warns(UserWarning, match="deprecated"):
        kern.set_prior("variance", dist.LogNormal(torch.tensor(0.0), torch.tensor(1.0)))
    assert "variance_map_unconstrained" in dict(kern.named_parameters())
    # a real support keeps a plain parameter
    lin = gp.kernels.Linear(3)
    lin.bias = PyroSample(dist.Normal(torch.zeros(2), torch.ones(2)).to_event())
    assert "bias_map" in dict(lin.named_parameters())
    lin.autoguide("bias", dist.Normal)
    assert {"bias_loc", "bias_scale_unconstrained"} <= set(dict(lin.named_parameters()))


def test_modes_and_the_auxiliary_site_of_a_positive_support(cpu_backend):
    data = gc.fixture_data()
    model = gc.build_model(gp, "gpr", data, prior=(PyroSample, dist))
    assert model.mode == "model" and model.kernel.mode == "model"
    tr = poutine.trace(model.model).get_trace()
    assert tr.nodes["kernel.lengthscale"]["fn"] is model.kernel._priors["lengthscale"]
    assert "y" in tr.nodes and tr.nodes["y"]["is_observed"]
    tr = poutine.trace(model.guide).get_trace()
    assert model.mode == "guide" and model.kernel.mode == "guide"
    np.testing.assert_allclose(tr.nodes["kernel.lengthscale"]["value"].detach().numpy(), gc.LENGTHSCALE_AT, rtol=1e-15)
    assert "kernel.lengthscale_latent" not in tr.nodes
    model.kernel.autoguide("lengthscale", dist.Normal)
    tr = poutine.trace(model.guide).get_trace()
    aux = tr.nodes["kernel.lengthscale_latent"]
    assert aux["infer"].get("is_auxiliary") and aux["value"].shape == (3,)
    site = tr.nodes["kernel.lengthscale"]
    np.testing.assert_allclose(site["value"].detach().numpy(), aux["value"].detach().exp().numpy(), rtol=1e-15)
    # the point mass carries log |d latent / d value| = -sum(latent)
    tr.compute_log_prob()
    np.testing.assert_allclose(float(site["log_prob"].detach()), -float(aux["value"].detach().sum()), rtol=1e-12)
    loss = Trace_ELBO().differentiable_loss(model.model, model.guide)
    loss.backward()
    grads = dict(model.named_parameters())
    assert grads["kernel.lengthscale_loc"].grad is not None and torch.isfinite(loss)


# ---- (d) ------------------------------------------------------------------------------------------------------------
def test_shape_and_argument_errors():
    data = gc.fixture_data()
    k = gp.kernels
    with pytest.raises(ValueError, match="active dimensionals"):
        k.RBF(3, active_dims=[0, 1])
    with pytest.raises(ValueError, match="1 or 2 dimensional"):
        k.RBF(3)(torch.zeros(2, 3, 3))
    with pytest.raises(ValueError, match="same number of features"):
        k.Linear(3)(torch.zeros(4, 3), torch.zeros(4))
    with pytest.raises(ValueError, match="same number of features"):
        k.RBF(3)(torch.zeros(4, 3), torch.zeros(4))
    with pytest.raises(TypeError):
        k.Sum(1.0, k.RBF(3))
    with pytest.raises(TypeError):
        k.Product(k.RBF(3), "x")
    assert k.Sum(k.RBF(1, active_dims=[2]), k.Linear(1, active_dims=[0])).active_dims == [0, 2]
    with pytest.raises(ValueError, match="number of input data points"):
        gp.models.GPRegression(data["X"], data["y"][:-1], k.RBF(3))
    with pytest.raises(ValueError, match="DTC"):
        gp.models.SparseGPRegression(data["X"], data["y"], k.RBF(3), data["Xu"], approx="XYZ")
    model = gp.models.GPRegression(data["X"], data["y"], k.RBF(3))
    with pytest.raises(ValueError, match="number of dimensions"):
        model(torch.zeros(3, dtype=F64))
    with pytest.raises(ValueError, match="shape of features"):
        model(torch.zeros(3, 2, dtype=F64))
    with pytest.raises(AssertionError):
        gp.models.GPRegression(data["X"].numpy(), data["y"], k.RBF(3))
    # y = None: the prior's mean and variance
    loc, var = gp.models.GPRegression(data["X"], None, k.RBF(3, variance=torch.tensor(2.0, dtype=F64)),
                                      noise=torch.tensor(0.5, dtype=F64)).model()
    np.testing.assert_allclose(var.detach().numpy(), 2.5 + 1e-6, rtol=1e-12)
    assert loc.shape == (gc.N_FIX,)


def test_iter_sample_grows_with_its_own_draws():
    data = gc.fixture_data()
    model = gc.build_model(gp, "gpr", data)
    sampler = model.iter_sample(noiseless=True)
    torch.manual_seed(0)
    with torch.no_grad():
        a = sampler(data["Xnew"][:1])
        b = sampler(data["Xnew"][:1] + 1e-9)
    assert a.shape == (1,) and abs(float(a - b)) < 1e-2


def test_cpu_tensors_never_reach_the_kernel(cpu_backend, monkeypatch):
    from pyro_amd import kernels

    def refuse(*a, **k):
        raise AssertionError("a CPU tensor reached the HIP kernel")
    monkeypatch.setattr(kernels, "gp_kernel_fwd", refuse)
    monkeypatch.setattr(kernels, "gp_kernel_bwd", refuse)
    assert gp.kernels.FUSED_GP_KERNEL is True
    data = gc.fixture_data()
    for name in gc.MODELS:
        model = gc.build_model(gp, name, data)
        gc.loss_and_grads(model, Trace_ELBO())
        model(data["Xnew"], full_cov=True)
    for dtype in (torch.float32, F64):
        kern = gp.kernels.Matern52(3).to(dtype)
        kern(data["X"].to(dtype), data["Xnew"].to(dtype)).sum().backward()


def test_the_ops_are_registered():
    from pyro_amd.ops import torch_library
    assert torch_library.available()
    names = torch_library.registered_ops()
    assert {"pyro_amd::gp_kernel", "pyro_amd::gp_kernel_bwd", "pyro_amd::fn_gp_kernel", "pyro_amd::fn_gp_kernel_bwd"} <= set(names)
    m = lambda *sh: torch.empty(sh, device="meta")      # noqa: E731
    assert torch.ops.pyro_amd.gp_kernel(m(5, 3), m(7, 3), m(3), m(1), None, 0).shape == (5, 7)
    assert torch.ops.pyro_amd.gp_kernel(m(5, 3), None, m(1), m(1), m(1), 1).shape == (5, 5)
    outs = torch.ops.pyro_amd.gp_kernel_bwd(m(5, 3), m(7, 3), m(3), m(1), None, m(5, 7), 0, True, True, False, True, True, 0)
    assert [tuple(o.shape) for o in outs] == [(5, 3), (7, 3), (0,), (1,), (0,)]


# ---- (e) ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", gc.FAMILIES)
@pytest.mark.parametrize("ard", [False, True])
def test_closed_form_derivatives_match_autograd_of_the_restatement(family, ard):
    D = 5
    x, z = gc.points(1, 9, D), gc.points(2, 6, D)
    ls, var, alpha = gc.parameters(3, D, ard, family)
    G = torch.as_tensor(np.random.default_rng(4).standard_normal((9, 6)))
    leaves = [t.clone().requires_grad_() for t in (x, z, ls, var)] + ([alpha.clone().requires_grad_()] if alpha is not None else [])
    K = gc.restate_K(family, leaves[0], leaves[1], leaves[2], leaves[3], leaves[4] if alpha is not None else None)
    grads = torch.autograd.grad((K * G).sum(), leaves)
    out = gc.restate(family, x, z, ls, var, alpha, G)
    for got, want in zip([out["gx"], out["gz"], out["g_ls"], out["g_var"], out["g_alpha"]], grads):
        _close(got.numpy(), want.numpy(), rtol=1e-13)
    # z = None: both roles
    leaf = x.clone().requires_grad_()
    Gs = torch.as_tensor(np.random.default_rng(5).standard_normal((9, 9)))
    (want,) = torch.autograd.grad((gc.restate_K(family, leaf, leaf, ls, var, alpha) * Gs).sum(), [leaf])
    _close(gc.restate(family, x, None, ls, var, alpha, Gs)["gx"].numpy(), want.numpy(), rtol=1e-13)


@pytest.mark.parametrize("family", gc.FAMILIES)
@pytest.mark.parametrize("D", [1, 2, 5, 17, 64])
@pytest.mark.parametrize("shift", [0.0, 1e3])
def test_torch_route_against_the_restatement_within_the_conditioning_bound(family, D, shift):
    worst = 0.0
    for seed in range(5):
        x, z = gc.points(seed, 12, D, shift), gc.points(seed + 50, 8, D, shift)
        z[5] = x[4]                                     # a duplicate across the two sets
        ls, var, alpha = gc.parameters(seed, D, D > 1, family)
        kern = gc.build_stationary(gp, family, D, ls, var, alpha)
        for zz in (z, None):
            with torch.no_grad():
                got = kern(x, zz)
            want = gc.restate_K(family, x, zz, ls, var, alpha)
            ratio = ((got - want).abs() / gc.conditioning_bound(family, x, zz, ls, var, alpha)).max().item()
            worst = max(worst, ratio)
    print("%s D=%d shift=%g: worst |difference| / bound %.3f" % (family, D, shift, worst))
    assert worst <= 1.0
