"""VariationalSparseGP and the likelihoods on the CPU in float64 (the dense route: util.conditional)."""
import numpy as np
import pytest
import torch
import torch.distributions as td

from . import gp_cases as gc
from .test_gp_sgpr_host import model_data


def vsgp(gp, data, dtype, device, whiten, case):
    """The model of both test files: Gaussian likelihood, a q(u) away from its initial value."""
    import pyro_amd as pyro
    pyro.clear_param_store()
    c = lambda t: t.to(dtype=dtype, device=device)      # noqa: E731
    two = case == "two_outputs"
    y = torch.stack((data["y"], data["y"].flip(0) * 0.5)) if two else data["y"]
    N, M = data["X"].size(0), data["Xu"].size(0)
    model = gp.models.VariationalSparseGP(
        c(data["X"]), c(y), gc.model_kernel(gp, dtype, device), c(data["Xu"]).clone(),
        gp.likelihoods.Gaussian(torch.tensor(0.2, dtype=dtype, device=device)),
        mean_function=(lambda X: 0.3 * X[:, 0] - 0.1) if case == "mean_function" else None,
        num_data=3 * N if case == "num_data" else None, whiten=whiten)
    g = np.random.default_rng(11)
    shape = (2,) if two else ()
    model.u_loc.data = c(torch.as_tensor(g.standard_normal(shape + (M,))))
    model.u_scale_tril_unconstrained.data = c(torch.as_tensor(0.3 * g.standard_normal(shape + (M, M))).tril())
    return model


def closed_form_loss(model, expected=False):
    """-(scale sum_n log N(y_n; loc_n, var_n + noise) - KL(q(u) || p(u))) from torch.distributions and util.conditional;
    with ``expected`` the data term is E_q(f) log N(y_n; f_n, noise) = log N(y_n; loc_n, noise) - var_n / (2 noise)."""
    from pyro_amd.contrib import gp
    M = model.Xu.size(0)
    eye = torch.eye(M, dtype=model.Xu.dtype, device=model.Xu.device)
    Luu = torch.linalg.cholesky(model.kernel(model.Xu) + model.jitter * eye)
    loc, var = gp.util.conditional(model.X, model.Xu, model.kernel, model.u_loc, model.u_scale_tril, Luu,
                                   whiten=model.whiten, jitter=model.jitter)
    loc, noise = loc + model.mean_function(model.X), model.likelihood.variance
    if expected:
        data_term = (td.Normal(loc, noise.sqrt()).log_prob(model.y) - var / (2 * noise)).sum()
    else:
        data_term = td.Normal(loc, (var + noise).sqrt()).log_prob(model.y).sum()
    prior = td.MultivariateNormal(torch.zeros_like(model.u_loc), scale_tril=eye if model.whiten else Luu)
    kl = td.kl_divergence(td.MultivariateNormal(model.u_loc, scale_tril=model.u_scale_tril), prior).sum()
    return -(model.num_data / model.X.size(0) * data_term - kl)


def dense_loss_and_grads(model):
    for p in model.parameters():
        p.grad = None
    loss = closed_form_loss(model)
    loss.backward()
    return float(loss.detach()), {n: p.grad.detach().cpu().numpy().copy() for n, p in model.named_parameters()
                                  if p.grad is not None}


@pytest.mark.parametrize("case", ["one_output", "two_outputs", "num_data", "mean_function"])
@pytest.mark.parametrize("whiten", [False, True])
def test_loss_is_the_closed_form(oracle_backend, whiten, case):
    """The Gaussian likelihood observes Normal(f_loc, sqrt(f_var + variance)), as the reference's does, so the loss is
    the closed form with log N(y_n; loc_n, var_n + noise).  The collapsed expectation log N(y_n; loc_n, noise) -
    var_n / (2 noise) is NOT what this likelihood computes; by Jensen's inequality it lies below, so its loss is an
    upper bound, strictly where var > 0."""
    from pyro_amd.contrib import gp
    from pyro_amd.infer import TraceMeanField_ELBO
    model = vsgp(gp, model_data("few_rows"), torch.float64, "cpu", whiten, case)
    loss, grads = gc.loss_and_grads(model, TraceMeanField_ELBO())
    want, want_grads = dense_loss_and_grads(model)
    assert abs(loss - want) <= 1e-12 * (1 + abs(want)), (loss, want)
    assert sorted(grads) == sorted(want_grads)
    for name in grads:
        assert np.abs(grads[name] - want_grads[name]).max() <= 1e-10 * (1 + np.abs(want_grads[name]).max()), name
    assert loss < float(closed_form_loss(model, expected=True).detach())
    names = [n for n, _ in model.named_parameters()]
    assert {"Xu", "u_loc", "u_scale_tril_unconstrained", "likelihood.variance_unconstrained"} <= set(names)


def test_likelihoods_at_zero_variance_and_their_event_shapes(oracle_backend):
    from pyro_amd import poutine
    from pyro_amd.contrib.gp import likelihoods as lk
    g = np.random.default_rng(3)
    f = torch.as_tensor(g.standard_normal((3, 5)))
    zero = torch.zeros_like(f)
    counts = torch.as_tensor(g.integers(0, 4, size=(2, 3, 5))).double()
    cases = [(lk.Gaussian(torch.tensor(0.3, dtype=torch.float64)), f, counts, td.Normal(f, 0.3 ** 0.5), 3),
             (lk.Binary(), f, (counts > 1).double(), td.Bernoulli(logits=f), 3),
             (lk.Binary(response_function=lambda v: torch.sigmoid(2 * v)), f, (counts > 1).double(),
              td.Bernoulli(logits=2 * f), 3),
             (lk.Poisson(), f, counts, td.Poisson(f.exp()), 3),
             (lk.MultiClass(3), f, counts[:, 0].long().clamp(max=2), td.Categorical(logits=f.t()), 2)]
    for likelihood, f_loc, y, want, event_dim in cases:
        site = poutine.trace(likelihood).get_trace(f_loc, zero, y).nodes["y"]
        assert site["is_observed"] and site["fn"].event_shape == y.shape[-event_dim:] and site["fn"].batch_shape == ()
        got = site["fn"].log_prob(y)
        assert abs(float(got) - float(want.log_prob(y).sum())) <= 1e-12 * (1 + abs(float(got))), type(likelihood)
    assert lk.Poisson()(f, zero).shape == f.shape and lk.MultiClass(3)(f, zero).shape == (5,)


def test_bad_arguments_raise():
    from pyro_amd.contrib import gp
    data = model_data("few_rows")
    kernel = gc.model_kernel(gp)
    with pytest.raises(AssertionError):
        gp.models.VariationalSparseGP(data["X"], data["y"], kernel, data["Xu"].numpy(), gp.likelihoods.Gaussian())
    with pytest.raises(ValueError):
        gp.models.VariationalSparseGP(data["X"], data["y"][:-1], kernel, data["Xu"], gp.likelihoods.Gaussian())
    model = gp.models.VariationalSparseGP(data["X"], data["y"], kernel, data["Xu"], gp.likelihoods.Gaussian())
    with pytest.raises(ValueError):
        model(data["Xnew"][:, :2])
    f = torch.zeros(4, 5, dtype=torch.float64)
    with pytest.raises(ValueError):
        gp.likelihoods.MultiClass(3)(f, f)            # four latent functions for three classes
    with pytest.raises(ValueError):
        gp.likelihoods.MultiClass(3)(f[0], f[0])      # no class dimension
