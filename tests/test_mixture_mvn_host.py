"""The full-covariance MultivariateNormal mixture leaf on the host: which observed sites TraceEnum_ELBO hands to
kernels.mixture_mvn_fwd_bwd (here a float64 torch stand-in), and that loss and gradients through it equal the
generic contraction's (contract.FUSED_MIXTURE = False)."""
import pytest
import torch

from tests.mvn_mixture_cases import make_gmm, mvn_leaf_reference

N, K, D = 40, 3, 3


@pytest.fixture
def mvn_calls(oracle_backend, monkeypatch):
    from pyro_amd import kernels

    calls = []

    def standin(x, a, loc, W):
        calls.append((tuple(a.shape), tuple(loc.shape), tuple(W.shape)))
        assert x.is_contiguous() and a.is_contiguous() and loc.is_contiguous() and W.is_contiguous()
        return mvn_leaf_reference(x, a, loc, W)

    monkeypatch.setattr(kernels, "mixture_mvn_fwd_bwd", standin)
    return calls


def _run(monkeypatch, fused, model, guide, x, num_particles=1):
    import pyro_amd as pyro
    import pyro_amd.ops.contract as c
    from pyro_amd.infer import TraceEnum_ELBO

    monkeypatch.setattr(c, "FUSED_MIXTURE", fused)
    pyro.clear_param_store()
    pyro.set_rng_seed(1)
    elbo = TraceEnum_ELBO(max_plate_nesting=1, num_particles=num_particles, vectorize_particles=num_particles > 1)
    loss = elbo.loss_and_grads(model, guide, x)
    grads = {n: p.grad.detach().clone() for n, p in pyro.get_param_store().named_parameters()}
    return loss, grads


def _assert_same(a, b, rtol=1e-10):
    la, ga = a
    lb, gb = b
    assert abs(la - lb) <= rtol * abs(lb), (la, lb)
    assert set(ga) == set(gb)
    for n in gb:
        scale = float(gb[n].abs().max()) + 1e-300
        assert float((ga[n] - gb[n]).abs().max()) <= rtol * scale, (n, ga[n], gb[n])


@pytest.mark.parametrize("form,particles", [("tril", 1), ("tril_shared", 1), ("cov", 1), ("prec", 1),
                                            ("loc_shared", 1), ("particles", 3)])
def test_accepted_forms_go_to_the_leaf(mvn_calls, monkeypatch, form, particles):
    model, guide, x = make_gmm(N, K, D, torch.float64, "cpu", form=form)
    fused = _run(monkeypatch, True, model, guide, x, particles)
    assert len(mvn_calls) == 1, mvn_calls
    a_shape, loc_shape, w_shape = mvn_calls[0]
    assert a_shape == (particles, K)
    assert loc_shape == (1, 1 if form == "loc_shared" else K, D)
    assert w_shape == (1, 1 if form == "tril_shared" else K, D, D)
    generic = _run(monkeypatch, False, model, guide, x, particles)
    assert len(mvn_calls) == 1
    _assert_same(fused, generic)


def test_subsampled_plate_goes_to_the_leaf(mvn_calls, monkeypatch):
    model, guide, x = make_gmm(N, K, D, torch.float64, "cpu", form="tril", subsample_size=17)
    fused = _run(monkeypatch, True, model, guide, x)
    assert len(mvn_calls) == 1
    _assert_same(fused, _run(monkeypatch, False, model, guide, x))


@pytest.mark.parametrize("form,k,d", [("mask", K, D), ("loc_per_row", K, D), ("row_weights", K, D), ("tril", 65, D),
                                      ("tril", K, 65), ("value_grad", K, D)])
def test_rejected_forms_take_the_generic_path(mvn_calls, monkeypatch, form, k, d):
    model, guide, x = make_gmm(N, k, d, torch.float64, "cpu", form=form)
    fused = _run(monkeypatch, True, model, guide, x)
    assert mvn_calls == []
    _assert_same(fused, _run(monkeypatch, False, model, guide, x))


def test_leaf_stand_in_equals_torch_log_prob():
    """The reference the tests hold the kernel to is torch's MultivariateNormal.log_prob with logsumexp and
    autograd: S, R = dS/da, W^T m = dS/dloc and the gradient to W agree with the stand-in's statistics."""
    import math

    from tests.mvn_mixture_cases import random_tril

    g = torch.Generator().manual_seed(5)
    B, Kk, Dd, Nn = 2, 4, 5, 30
    x = torch.randn(Nn, Dd, generator=g, dtype=torch.float64) * 2
    a = torch.log_softmax(torch.randn(B, Kk, generator=g, dtype=torch.float64), -1).requires_grad_()
    loc = torch.randn(B, Kk, Dd, generator=g, dtype=torch.float64).requires_grad_()
    L = random_tril(B * Kk, Dd, g).reshape(B, Kk, Dd, Dd)
    W = torch.linalg.solve_triangular(L, torch.eye(Dd, dtype=torch.float64), upper=False).requires_grad_()
    Linv = torch.linalg.inv(torch.tril(W))
    lp = torch.distributions.MultivariateNormal(loc[:, :, None], scale_tril=Linv[:, :, None]).log_prob(x)  # [B,K,N]
    S = torch.logsumexp(a[:, :, None] + lp, 1).sum(-1)
    S.sum().backward()
    s, R, m, G = mvn_leaf_reference(x, a, loc, W)
    assert torch.allclose(s, S.detach(), rtol=1e-12, atol=0)
    assert torch.allclose(R, a.grad, rtol=1e-12, atol=1e-12)
    assert torch.allclose(torch.einsum("bkji,bkj->bki", torch.tril(W.detach()), m), loc.grad, rtol=1e-10,
                          atol=1e-10)
    dW = torch.diag_embed(R.unsqueeze(-1) / torch.diagonal(W.detach(), dim1=-2, dim2=-1)) - G
    assert torch.allclose(torch.tril(dW), torch.tril(W.grad), rtol=1e-10, atol=1e-10)
    assert math.isfinite(float(S.sum()))
