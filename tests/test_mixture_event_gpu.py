"""The event-shaped mixture leaf (csrc/mixture_event.hip) on the device: the kernel against float64 torch for every
family over a grid of K, D, N, B, sharing and dtype; confident Bernoulli components; offset Normal data; TraceEnum_ELBO
against the generic contraction (plain and subsampled), a captured SVI step against the eager one, the NUTS potential
over vectorised chains, and the memory of a large evaluation."""
import math

import numpy as np
import pytest
import torch

from tests.event_mixture_cases import (FAMILIES, dist_id, event_leaf_reference, family_data, family_params,
                                       make_mixture)

pytestmark = pytest.mark.gpu


def _inputs(family, K, D, N, B, share, gpu, seed=0, confident=False):
    """float64 inputs on the device: x [N, D]; a [B, K]; p0, p1 [B | 1, K | 1, D | 1] (p1 None for one-parameter
    families).  ``share``: None, "k" (p0 one row for every component), "d" (p0 one value per component) or "b" (both
    parameters one set for every b)."""
    g = torch.Generator().manual_seed(seed)
    P0, P1 = family_params(family, K, D, g, confident)
    x = family_data(family, P0, P1, N, g)
    if not confident:                      # (the leaf's parameters near, not at, the data's)
        Q0, Q1 = family_params(family, K, D, g)
        P0 = 0.7 * P0 + 0.3 * Q0
        P1 = None if P1 is None else 0.7 * P1 + 0.3 * Q1
    a = torch.log_softmax(torch.randn(B, K, generator=g, dtype=torch.float64), -1)
    jit = lambda p: p * (1.0 + 0.05 * torch.rand(B, *p.shape, generator=g, dtype=torch.float64))  # noqa: E731
    p0, p1 = jit(P0), None if P1 is None else jit(P1)
    if share == "k":
        p0 = p0[:, :1]
    elif share == "d":
        p0 = p0[:, :, :1]
    elif share == "b":
        p0 = p0[:1]
        p1 = None if p1 is None else p1[:1]
    return [None if t is None else t.to(gpu) for t in (x, a, p0, p1)]


def _rel_errors(got, ref):
    """max |got - ref| / max |ref| per output (S, dS/da, dS/dp0, dS/dp1)."""
    out = []
    for g_, r in zip(got, ref):
        if r is None:
            continue
        scale = float(r.abs().max()) or 1.0
        out.append(float((g_.double() - r).abs().max()) / scale)
    return out


def _check(family, dtype, x, a, p0, p1):
    from pyro_amd import kernels

    cast = lambda t: None if t is None else t.to(dtype).contiguous()  # noqa: E731
    args = [cast(t) for t in (x, a, p0, p1)]
    got = kernels.mixture_event_fwd_bwd(dist_id(family), *args)
    again = kernels.mixture_event_fwd_bwd(dist_id(family), *args)
    for p, q in zip(got, again):
        assert (p is None and q is None) or torch.equal(p, q), "two runs differ"
    ref = event_leaf_reference(family, *args)
    err = _rel_errors(got, ref)
    if dtype == torch.float64:
        bound = [1e-10] * len(err)
    else:
        # the f32 rule of the GLM kernel: no worse than 4x torch's own f32 computation against float64, plus 1e-6 of
        # the result's scale
        base = event_leaf_reference(family, *args, dtype=torch.float32)
        bound = [4.0 * e + 1e-6 for e in _rel_errors(base, ref)]
    for name, e, b in zip(("S", "da", "dp0", "dp1"), err, bound):
        assert e <= b, (name, e, b)
    return got, ref


# (K, D, N, B, shared): every K and D of the limits' grid, ragged N, B in {1, 4}
GRID = [
    (1, 1, 1, 1, None),
    (3, 9, 257, 4, "k"),
    (16, 100, 1000, 1, "d"),
    (64, 784, 300, 1, None),
    (16, 1024, 513, 4, "b"),
    (3, 1024, 100, 1, None),
    (64, 9, 20_000, 4, None),
    (16, 784, 5000, 1, None),
    (1, 100, 70_001, 1, "d"),
]


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("K,D,N,B,share", GRID)
@pytest.mark.parametrize("family", FAMILIES)
def test_kernel_against_float64_torch(gpu, family, dtype, K, D, N, B, share):
    x, a, p0, p1 = _inputs(family, K, D, N, B, share, gpu, seed=K * 131 + D)
    _check(family, dtype, x, a, p0, p1)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("family", FAMILIES)
def test_switched_off_component(gpu, family, dtype):
    """a = -inf for one component: no responsibility, no gradient, S of the others."""
    x, a, p0, p1 = _inputs(family, 5, 37, 2000, 2, None, gpu, seed=12)
    a = a.clone()
    a[:, 2] = -math.inf
    got, _ = _check(family, dtype, x, a, p0, p1)
    assert float(got[1][:, 2].abs().max()) == 0.0 and float(got[2][:, 2].abs().max()) == 0.0


def test_confident_bernoulli_components(gpu):
    """|logits| up to 20, D = 784, data drawn from the components: x l - softplus(l) must not cancel."""
    x, a, p0, p1 = _inputs("Bernoulli", 16, 784, 3000, 1, None, gpu, seed=21, confident=True)
    _check("Bernoulli", torch.float32, x, a, p0, p1)


def test_offset_normal_data_does_not_cancel(gpu):
    """Data centred at 1e3 with unit spread, D = 64, f32: x - loc is formed before the square."""
    g = torch.Generator().manual_seed(11)
    K, D, N = 8, 64, 50_000
    centres = 1e3 + 3.0 * torch.randn(K, D, generator=g, dtype=torch.float64)
    x = centres[torch.randint(0, K, (N,), generator=g)] + torch.randn(N, D, generator=g, dtype=torch.float64)
    loc = (centres + 0.2 * torch.randn(K, D, generator=g, dtype=torch.float64))[None]
    scale = torch.ones(1, K, D, dtype=torch.float64)
    a = torch.log_softmax(torch.randn(1, K, generator=g, dtype=torch.float64), -1)
    _check("Normal", torch.float32, *[t.to(gpu) for t in (x, a, loc, scale)])


def test_nan_row_propagates(gpu):
    from pyro_amd import kernels

    x, a, p0, p1 = _inputs("Normal", 3, 20, 300, 1, None, gpu, seed=14)
    x = x.clone()
    x[17, 2] = float("nan")
    S = kernels.mixture_event_fwd_bwd(dist_id("Normal"), x, a, p0.contiguous(), p1.contiguous())[0]
    assert torch.isnan(S).all()


def _elbo_run(monkeypatch, fused, model, guide, x):
    import pyro_amd as pyro
    import pyro_amd.ops.contract as c
    from pyro_amd.infer import TraceEnum_ELBO

    monkeypatch.setattr(c, "FUSED_MIXTURE", fused)
    pyro.clear_param_store()
    pyro.set_rng_seed(1)
    loss = TraceEnum_ELBO(max_plate_nesting=1).loss_and_grads(model, guide, x)
    return loss, {n: p.grad.detach().clone() for n, p in pyro.get_param_store().named_parameters()}


@pytest.fixture
def event_calls(monkeypatch):
    from pyro_amd import kernels

    calls, real = [], kernels.mixture_event_fwd_bwd
    monkeypatch.setattr(kernels, "mixture_event_fwd_bwd", lambda *a: calls.append(tuple(a[2].shape)) or real(*a))
    return calls


@pytest.mark.parametrize("dtype,subsample", [(torch.float64, None), (torch.float32, None), (torch.float32, 6000)])
@pytest.mark.parametrize("family", FAMILIES)
def test_elbo_leaf_is_fused_and_equals_the_generic_contraction(gpu, monkeypatch, event_calls, family, dtype,
                                                               subsample):
    """TraceEnum_ELBO on an event-shaped mixture (N = 20 000, K = 7, D = 50): one launch of the leaf, loss and every
    gradient equal to the generic contraction's within the MVN leaf test's tolerances."""
    model, guide, x = make_mixture(family, 20_000, 7, 50, dtype, gpu, subsample_size=subsample)
    la, ga = _elbo_run(monkeypatch, True, model, guide, x)
    assert event_calls == [(1, 7)], event_calls
    lb, gb = _elbo_run(monkeypatch, False, model, guide, x)
    assert len(event_calls) == 1
    rtol = 1e-10 if dtype == torch.float64 else 2e-5
    assert abs(la - lb) <= rtol * abs(lb), (la, lb)
    for n in gb:
        scale = float(gb[n].abs().max()) + 1e-30
        assert float((ga[n] - gb[n]).abs().max()) <= (1e-9 if dtype == torch.float64 else 2e-4) * scale, n


def test_captured_svi_step_equals_the_eager_one(gpu, event_calls):
    """SVI(model, guide, Adam, TraceEnum_ELBO) on a Bernoulli mixture for 20 steps, captured and eager: the same
    kernels in the same order on the same inputs (tolerance as the MVN leaf's test)."""
    import pyro_amd as pyro
    from pyro_amd.infer import SVI, TraceEnum_ELBO

    model, guide, x = make_mixture("Bernoulli", 20_000, 7, 50, torch.float32, gpu)

    def run(capture):
        pyro.clear_param_store()
        pyro.set_rng_seed(1)
        svi = SVI(model, guide, pyro.optim.Adam({"lr": 0.01}), TraceEnum_ELBO(max_plate_nesting=1), hip_graph=capture)
        losses = [svi.step(x) for _ in range(20)]
        params = {n: p.detach().clone() for n, p in pyro.get_param_store().items()}
        return svi, np.array(losses), params

    pyro.enable_validation(False)
    try:
        svi_c, lc, pc = run(True)
        assert svi_c.hip_graph and svi_c._graphs, "the step was not captured"
        svi_e, le, pe = run(False)
        assert not svi_e._graphs
    finally:
        pyro.enable_validation(True)
    assert len(event_calls) >= 2
    np.testing.assert_allclose(lc, le, rtol=1e-6)
    for n in pe:
        torch.testing.assert_close(pc[n], pe[n], rtol=1e-6, atol=1e-6 * float(pe[n].abs().max()))


def test_nuts_potential_over_vectorised_chains(gpu, monkeypatch, event_calls):
    """The enumerated potential of a Bernoulli mixture for 4 vectorised chains: ONE launch of the leaf with the chains
    as its 4 parameter sets, potential and gradient equal to the generic contraction's (float64); a short NUTS run
    over the same model completes with finite samples."""
    import pyro_amd as pyro
    import pyro_amd.distributions as dist
    import pyro_amd.ops.contract as c
    from pyro_amd.infer.mcmc import MCMC, NUTS, initialize_model
    from pyro_amd.ops.indexing import Vindex

    dtype = torch.float64
    K, N, D, C = 3, 500, 20, 4
    g = torch.Generator().manual_seed(4)
    P0, _ = family_params("Bernoulli", K, D, g)
    data = family_data("Bernoulli", P0, None, N, g).to(gpu, dtype)

    def model(data):
        phi = pyro.sample("phi", dist.Dirichlet(torch.ones(K, dtype=dtype, device=gpu)))
        with pyro.plate("num_clusters", K):
            logits = pyro.sample("logits", dist.Normal(torch.zeros(D, dtype=dtype, device=gpu), 2.0).to_event(1))
        with pyro.plate("data", N):
            a = pyro.sample("assignments", dist.Categorical(phi))
            pyro.sample("obs", dist.Bernoulli(logits=Vindex(logits.unsqueeze(-3))[..., a, :]).to_event(1), obs=data)

    def run(fused):
        monkeypatch.setattr(c, "FUSED_MIXTURE", fused)
        pyro.set_rng_seed(0)
        init, pot, _, _ = initialize_model(model, (data,), max_plate_nesting=1, num_chains=C)
        z = {n: v.detach().clone().requires_grad_(True) for n, v in sorted(init.items())}
        n0 = len(event_calls)
        pe = pot(z)
        assert len(event_calls) - n0 == (1 if fused else 0), event_calls
        return pe.detach(), [t.detach() for t in torch.autograd.grad(pe.sum(), list(z.values()))]

    pa_, ga = run(True)
    assert event_calls[-1] == (C, K), event_calls
    pb, gb = run(False)
    torch.testing.assert_close(pa_, pb, rtol=1e-11, atol=0)
    for x, y in zip(ga, gb):
        torch.testing.assert_close(x, y, rtol=1e-9, atol=1e-9 * float(y.abs().max()))

    monkeypatch.setattr(c, "FUSED_MIXTURE", True)
    pyro.set_rng_seed(2)
    n0 = len(event_calls)
    mcmc = MCMC(NUTS(model, max_plate_nesting=1), num_samples=4, warmup_steps=4, num_chains=C)
    mcmc.run(data)
    assert len(event_calls) > n0
    for v in mcmc.get_samples().values():
        assert torch.isfinite(v).all()
    assert (C, K) in set(event_calls[n0:]), set(event_calls[n0:])


def test_large_evaluation_allocates_nothing_of_size_k_n(gpu, event_calls):
    """N = 1e6, K = 16, D = 128, f32 Bernoulli: one loss_and_grads through the leaf allocates at most the row buffer,
    the workspace and small tensors -- below one [K, N] f32 tensor (64 MB), let alone [K, N, D] (8 GB).  Validation
    is off: the support check of the observed [N, D] values allocates masks of the data's size whatever path the
    site takes."""
    import pyro_amd as pyro
    from pyro_amd.infer import TraceEnum_ELBO

    N, K, D = 1_000_000, 16, 128
    model, guide, x = make_mixture("Bernoulli", N, K, D, torch.float32, gpu)
    pyro.clear_param_store()
    elbo = TraceEnum_ELBO(max_plate_nesting=1)
    pyro.enable_validation(False)
    try:
        elbo.loss_and_grads(model, guide, x)         # (parameters created, kernels loaded)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        loss = elbo.loss_and_grads(model, guide, x)
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - base
    finally:
        pyro.enable_validation(True)
    assert math.isfinite(loss)
    assert len(event_calls) == 2
    assert peak < K * N * 4, "peak %.1f MB over the data" % (peak / 2**20)


def test_limits_raise_unsupported(gpu):
    from pyro_amd import kernels

    x = torch.zeros(10, kernels.MIXTURE_EVENT_MAX_D + 1, device=gpu)
    a = torch.zeros(1, 3, device=gpu)
    with pytest.raises(kernels.Unsupported):
        kernels.mixture_event_fwd_bwd(dist_id("Bernoulli"), x, a, torch.zeros(1, 3, x.shape[1], device=gpu), None)
    x = torch.zeros(10, 4, device=gpu)
    a = torch.zeros(1, 65, device=gpu)
    with pytest.raises(kernels.Unsupported):
        kernels.mixture_event_fwd_bwd(dist_id("Poisson"), x, a, torch.ones(1, 65, 4, device=gpu), None)
