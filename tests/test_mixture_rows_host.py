"""The per-row-weights mixture leaf on the host: which enumerated mixtures TraceEnum_ELBO hands to
kernels.mixture_rows_fwd_bwd / mixture_rows_diag_normal_fwd_bwd (here float64 torch stand-ins), with which shapes,
layout and ``want_da``; that loss and gradients through the stand-ins equal the generic contraction's
(contract.FUSED_MIXTURE = False) and the unmodified reference's (tests/golden/mixture_rows.npz); and which forms stay
on the generic path."""
import os

import numpy as np
import pytest
import torch

from tests.event_mixture_cases import FAMILIES, dist_id
from tests.row_mixture_cases import (ACCEPTED, REJECTED, make_row_mixture, row_init, row_leaf_reference,
                                     unflat_params)

N, K = 40, 3
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mixture_rows.npz")


@pytest.fixture
def row_calls(oracle_backend, monkeypatch):
    """calls of the two leaves as (leaf, a's shape, a's strides, want_da[, family id])"""
    from pyro_amd import kernels

    names = {dist_id(f): f for f in FAMILIES}
    calls = []

    def scalar(dist, x, a, p0, s0, p1, s1, p0_bs=0, p1_bs=0, want_da=True):
        B, _, Kk = a.shape
        calls.append(("scalar", tuple(a.shape), tuple(a.stride()), bool(want_da), int(dist)))
        assert x.dim() == 1 and x.is_contiguous() and p0.is_contiguous() and a.shape[1] == x.shape[0]
        S, da, d0, d1 = row_leaf_reference(names[int(dist)], x, a, unflat_params(p0, s0, p0_bs, B, Kk),
                                           unflat_params(p1, s1, p1_bs, B, Kk))
        return S, (da if want_da else None), d0, d1

    def diag(x, a, loc, scale, want_da=True):
        calls.append(("diag", tuple(a.shape), tuple(a.stride()), bool(want_da)))
        assert x.dim() == 2 and x.is_contiguous() and loc.is_contiguous() and scale.is_contiguous()
        assert a.shape[1] == x.shape[0] and loc.dim() == 3 and scale.dim() == 3
        S, da, dl, dc = row_leaf_reference("Normal", x, a, loc, scale)
        return S, (da if want_da else None), dl, dc

    monkeypatch.setattr(kernels, "mixture_rows_fwd_bwd", scalar)
    monkeypatch.setattr(kernels, "mixture_rows_diag_normal_fwd_bwd", diag)
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
    grads = {n: p.grad.detach().clone() for n, p in pyro.get_param_store().named_parameters() if p.grad is not None}
    return loss, grads


def _assert_same(a, b, rtol=1e-10):
    la, ga = a
    lb, gb = b
    assert abs(la - lb) <= rtol * abs(lb), (la, lb)
    assert set(ga) == set(gb)
    for n in gb:
        scale = float(gb[n].abs().max()) + 1e-300
        assert float((ga[n] - gb[n]).abs().max()) <= rtol * scale, (n, ga[n], gb[n])


def _build(form, family="Normal", D=None, n=N, k=K):
    init = row_init(family, n, k, D, seed=5)
    return make_row_mixture(form, init, torch.float64, "cpu", family=family,
                            subsample_size=17 if form == "subsample" else None)


@pytest.mark.parametrize("D", [None, 3])
@pytest.mark.parametrize("form", ACCEPTED)
def test_accepted_forms_make_one_call_of_the_leaf(row_calls, monkeypatch, form, D):
    model, guide, x = _build(form, D=D)
    P = 3 if form == "particles" else 1
    rows = 17 if form == "subsample" else N
    fused = _run(monkeypatch, True, model, guide, x, P)
    assert len(row_calls) == 1, row_calls
    leaf, shape, stride, want_da = row_calls[0][:4]
    assert leaf == ("scalar" if D is None else "diag")
    assert shape == (P, rows, K)
    assert want_da == (form != "detached")
    # the Categorical's own factor is handed over as the view it is: row-major [rows, K] memory, no copy
    assert stride[2] == 1 and stride[1] == K and (P == 1 or stride[0] == rows * K), stride
    if D is None:
        assert row_calls[0][4] == dist_id("Normal")
    generic = _run(monkeypatch, False, model, guide, x, P)
    assert len(row_calls) == 1
    _assert_same(fused, generic)


@pytest.mark.parametrize("family", FAMILIES)
def test_every_scalar_family_goes_to_the_leaf(row_calls, monkeypatch, family):
    model, guide, x = _build("experts", family=family)
    fused = _run(monkeypatch, True, model, guide, x)
    assert [c[0] for c in row_calls] == ["scalar"] and row_calls[0][4] == dist_id(family), row_calls
    _assert_same(fused, _run(monkeypatch, False, model, guide, x))


def test_constant_and_per_row_terms_are_combined(row_calls, monkeypatch):
    """A factor of the assignment that is constant along the plate next to the per-row one: both reach the leaf in
    one a [1, N, K] (here through the contraction directly: a [K, 1] term and a [K, N] term)."""
    import pyro_amd.ops.contract as c

    model, guide, x = _build("experts")
    monkeypatch.setattr(c, "FUSED_MIXTURE", True)
    seen = []
    real = c._try_fused_mixture

    def with_constant(terms, sum_ids, frames):
        dense = [t for t in terms if t.tensor is not None]
        if len(dense) == 1 and dense[0].tensor.dim() == 2:
            extra = torch.linspace(-1.0, 0.5, K, dtype=torch.float64).reshape(K, 1)
            terms = list(terms) + [c.Term(extra, dense[0].ids, dense[0].ordinal)]
            out = real(terms, sum_ids, frames)
            lazy = [t for t in terms if t.tensor is None][0].lazy
            both = torch.logsumexp(dense[0].tensor + extra + lazy.materialize(), 0).sum()
            seen.append((out.detach(), both.detach()))
            return out
        return real(terms, sum_ids, frames)

    monkeypatch.setattr(c, "_try_fused_mixture", with_constant)
    _run(monkeypatch, True, model, guide, x)
    assert len(seen) == 1 and len(row_calls) == 1 and row_calls[0][1] == (1, N, K)
    out, both = seen[0]
    assert out is not None and abs(float(out) - float(both)) <= 1e-10 * abs(float(both))


@pytest.mark.parametrize("form", REJECTED)
def test_rejected_forms_take_the_generic_path(row_calls, monkeypatch, form):
    D = {"event": 10, "mvn": 3}.get(form)
    model, guide, x = _build(form, D=D)
    fused = _run(monkeypatch, True, model, guide, x)
    assert row_calls == []
    _assert_same(fused, _run(monkeypatch, False, model, guide, x))


def test_switch_turns_the_path_off(row_calls, monkeypatch):
    model, guide, x = _build("experts")
    _run(monkeypatch, False, model, guide, x)
    assert row_calls == []


@pytest.mark.parametrize("family,D", [(f, None) for f in FAMILIES] + [("Normal", 4)])
def test_leaf_stand_in_equals_torch_autograd(family, D):
    """The reference the tests hold the kernels to equals torch's own logsumexp of log_prob and its autograd, a
    shared parameter (its gradient summed over the broadcast axis) and -inf weights included."""
    from tests.event_mixture_cases import family_data, family_params, torch_family

    g = torch.Generator().manual_seed(3)
    B, Kk, Nn = 2, 4, 30
    P0, P1 = family_params(family, Kk, D or 1, g)
    x = family_data(family, P0, P1, Nn, g)
    a = torch.log_softmax(torch.randn(B, Nn, Kk, generator=g, dtype=torch.float64), -1)
    a[0, 3, 1] = a[1, 7, 0] = -float("inf")
    a.requires_grad_()
    if D is None:
        x, P0, P1 = x[:, 0], P0[:, 0], None if P1 is None else P1[:, 0]
    p0 = P0[None].clone().requires_grad_()                                   # [1, K(, D)]: shared across the sets
    p1 = None if P1 is None else P1[None].clone().requires_grad_()
    if D is None:
        lp = torch_family(family, p0[:, None, :], None if p1 is None else p1[:, None, :]).log_prob(x[:, None])
    else:
        lp = torch_family(family, p0[:, None], None if p1 is None else p1[:, None]).log_prob(x[:, None, :]).sum(-1)
    S = torch.logsumexp(a + lp, -1).sum(-1)
    S.sum().backward()
    s, da, d0, d1 = row_leaf_reference(family, x, a, p0, p1)
    assert torch.allclose(s, S.detach(), rtol=1e-12, atol=0)
    assert torch.allclose(da, a.grad, rtol=1e-12, atol=1e-12)
    assert torch.allclose(d0.sum(0, keepdim=True), p0.grad, rtol=1e-12, atol=1e-12 * float(p0.grad.abs().max()))
    if p1 is not None:
        assert torch.allclose(d1.sum(0, keepdim=True), p1.grad, rtol=1e-12, atol=1e-12 * float(p1.grad.abs().max()))


@pytest.mark.parametrize("form", ["experts", "grouped"])
def test_leaf_matches_reference(row_calls, monkeypatch, form):
    """Loss and gradients of the unmodified reference's TraceEnum_ELBO (float64) through the leaf's stand-in."""
    gold = np.load(GOLDEN)
    init = {k.split("/", 2)[2]: torch.as_tensor(gold[k]) for k in gold.files if k.startswith(form + "/init/")}
    model, guide, x = make_row_mixture(form, init, torch.float64, "cpu")
    loss, grads = _run(monkeypatch, True, model, guide, x)
    assert len(row_calls) == 1
    ref = float(gold[form + "/loss"])
    assert abs(loss - ref) <= 1e-9 * abs(ref), (loss, ref)
    names = [k.split("/", 2)[2] for k in gold.files if k.startswith(form + "/grad/")]
    assert set(names) == set(grads) and names
    for n in names:
        r = torch.as_tensor(gold[form + "/grad/" + n])
        assert float((grads[n] - r).abs().max()) <= 1e-9 * (float(r.abs().max()) + 1e-300), n
