"""The full-covariance MultivariateNormal mixture leaf (csrc/mixture_mvn.hip) on the device: the kernel against
float64 torch over a grid of K, D, N, B, sharing and dtype; offset data; edges; TraceEnum_ELBO against the generic
contraction (plain and subsampled), a captured SVI step against the eager one, the NUTS potential over vectorised
chains, and the memory of a large evaluation."""
import math

import numpy as np
import pytest
import torch

from tests.mvn_mixture_cases import make_gmm, mvn_leaf_reference, random_tril

pytestmark = pytest.mark.gpu


def _inputs(K, D, N, B, loc_shared, tril_shared, gpu, seed=0, offset=0.0, spread=0.3):
    """float64 inputs on the device: x [N, D]; a [B, K]; loc [B | 1, K | 1, D]; W [B | 1, K | 1, D, D]."""
    g = torch.Generator().manual_seed(seed)
    Kl, Kw = (1 if loc_shared else K), (1 if tril_shared else K)
    centres = 3.0 * torch.randn(B, Kl, D, generator=g, dtype=torch.float64)
    pick = torch.randint(0, Kl, (N,), generator=g)
    x = offset + centres[0, pick] + torch.randn(N, D, generator=g, dtype=torch.float64)
    loc = offset + centres + 0.2 * torch.randn(B, Kl, D, generator=g, dtype=torch.float64)
    a = torch.log_softmax(torch.randn(B, K, generator=g, dtype=torch.float64), -1)
    L = random_tril(B * Kw, D, g, spread).reshape(B, Kw, D, D) * 1.3
    W = torch.linalg.solve_triangular(L, torch.eye(D, dtype=torch.float64), upper=False)
    return [t.to(gpu) for t in (x, a, loc, W)]


def _leaf_in(dtype, x, a, loc, W, B_loc=True, B_w=True):
    cast = lambda t: t.to(dtype).contiguous()  # noqa: E731
    return cast(x), cast(a), cast(loc if B_loc else loc[:1]), cast(W if B_w else W[:1])


def _rel_errors(got, ref):
    """max |got - ref| / max |ref| per output (S, R, m, G)."""
    out = []
    for g_, r in zip(got, ref):
        scale = float(r.abs().max()) or 1.0
        out.append(float((g_.double() - r).abs().max()) / scale)
    return out


def _check(dtype, x, a, loc, W):
    from pyro_amd import kernels

    args = _leaf_in(dtype, x, a, loc, W)
    got = kernels.mixture_mvn_fwd_bwd(*args)
    again = kernels.mixture_mvn_fwd_bwd(*args)
    for p, q in zip(got, again):
        assert torch.equal(p, q), "two runs differ"
    ref = mvn_leaf_reference(*[t.double() for t in args])
    err = _rel_errors(got, ref)
    if dtype == torch.float64:
        bound = [1e-10] * 4
    else:
        # the f32 rule of the GLM kernel: no worse than 4x torch's own f32 computation of the same statistics
        # against float64, floor 1e-5
        base = mvn_leaf_reference_f32(*args)
        bound = [max(4.0 * e, 1e-5) for e in _rel_errors(base, ref)]
    for name, e, b in zip("SRmG", err, bound):
        assert e <= b, (name, e, b)
    return got, ref


def mvn_leaf_reference_f32(x, a, loc, W):
    """torch's own f32 computation of (S, R, m, G) over the [B, K, N, D] frame: the same formulas as
    mvn_leaf_reference in the input dtype.  (z = W d by einsum: torch's MultivariateNormal.log_prob runs a batched
    hipBLAS triangular solve whose workspace allocation fails at K = D = 64 here.)"""
    B, K = a.shape
    N, D = x.shape
    Wf = torch.tril(W).expand(B, K, D, D)
    d = x[None, None] - loc.expand(B, K, D)[:, :, None, :]
    z = torch.einsum("bkij,bknj->bkni", Wf, d)
    logdet = torch.log(torch.diagonal(Wf, dim1=-2, dim2=-1)).sum(-1)
    t = (a + logdet)[:, :, None] - 0.5 * D * math.log(2 * math.pi) - 0.5 * (z * z).sum(-1)
    lse = torch.logsumexp(t, 1)
    r = torch.exp(t - lse[:, None])
    return (lse.sum(-1), r.sum(-1), torch.einsum("bkn,bkni->bki", r, z),
            torch.tril(torch.einsum("bkn,bkni,bknj->bkij", r, z, d)))


# (K, D, N, B, loc shared, scale_tril shared): every value of every axis, K = D = 64 in both dtypes
GRID = [
    (1, 1, 1, 1, False, False),
    (3, 2, 63, 3, True, False),
    (16, 7, 64, 1, False, True),
    (3, 8, 65, 3, False, False),
    (16, 9, 100_003, 1, False, False),
    (64, 16, 1000, 3, True, True),
    (3, 31, 4097, 1, False, False),
    (16, 32, 100_003, 3, False, False),
    (64, 64, 20_000, 1, False, False),
    (1, 64, 65, 3, False, True),
    (64, 1, 100_003, 3, False, False),
]


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("K,D,N,B,loc_shared,tril_shared", GRID)
def test_kernel_against_float64_torch(gpu, dtype, K, D, N, B, loc_shared, tril_shared):
    x, a, loc, W = _inputs(K, D, N, B, loc_shared, tril_shared, gpu, seed=K * 131 + D)
    _check(dtype, x, a, loc, W)


def test_kernel_parameters_shared_across_sets(gpu):
    """loc and W of stride 0 across the sets (one set's parameters, B sets of weights): every set equals its own
    single evaluation."""
    from pyro_amd import kernels

    x, a, loc, W = _inputs(5, 12, 3001, 4, False, False, gpu, seed=9)
    S, R, m, G = kernels.mixture_mvn_fwd_bwd(x, a, loc[:1].contiguous(), W[:1].contiguous())
    for b in range(4):
        one = kernels.mixture_mvn_fwd_bwd(x, a[b:b + 1].contiguous(), loc[:1].contiguous(), W[:1].contiguous())
        for p, q in zip((S, R, m, G), one):
            torch.testing.assert_close(p[b:b + 1], q, rtol=1e-12, atol=1e-12 * float(q.abs().max()))


def test_offset_data_does_not_cancel(gpu):
    """Data centred at 1e3 with unit spread, D = 32, f32: d = x - loc is formed before the product."""
    x, a, loc, W = _inputs(8, 32, 50_000, 1, False, False, gpu, seed=11, offset=1e3)
    _check(torch.float32, x, a, loc, W)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_edges(gpu, dtype):
    from pyro_amd import kernels

    # a component switched off: no responsibility, S of the others
    x, a, loc, W = _inputs(5, 6, 2000, 1, False, False, gpu, seed=12)
    a = a.clone()
    a[0, 2] = -math.inf
    got, ref = _check(dtype, x, a, loc, W)
    assert float(got[1][0, 2]) == 0.0 and float(got[2][0, 2].abs().max()) == 0.0
    # a nearly singular factor: smallest diagonal of L 1e-3 of its largest
    x, a, loc, W = _inputs(4, 10, 5000, 1, False, False, gpu, seed=13)
    L = torch.linalg.inv(W)
    L[0, 1, 7, 7] = 1e-3 * float(torch.diagonal(L[0, 1]).max())
    W = torch.linalg.solve_triangular(L, torch.eye(10, dtype=torch.float64, device=gpu), upper=False)
    _check(dtype, x, a, loc, W)
    # a row holding NaN: S is NaN, as in the generic path
    x, a, loc, W = _inputs(3, 4, 300, 1, False, False, gpu, seed=14)
    x = x.clone()
    x[17, 2] = float("nan")
    S = kernels.mixture_mvn_fwd_bwd(*_leaf_in(dtype, x, a, loc, W))[0]
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
def mvn_calls(monkeypatch):
    from pyro_amd import kernels

    calls, real = [], kernels.mixture_mvn_fwd_bwd
    monkeypatch.setattr(kernels, "mixture_mvn_fwd_bwd", lambda *a: calls.append(tuple(a[1].shape)) or real(*a))
    return calls


@pytest.mark.parametrize("subsample", [None, 6000])
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_elbo_leaf_is_fused_and_equals_the_generic_contraction(gpu, monkeypatch, mvn_calls, dtype, subsample):
    """TraceEnum_ELBO on a full-covariance GMM (Dirichlet weights, per-component locs and scale_tril, N = 20 000,
    K = 7, D = 5): one launch of the leaf, loss and every gradient equal to the generic contraction's within the
    tolerances of test_enum_gpu.py::test_mixture_leaf_is_fused_and_equals_the_generic_contraction."""
    model, guide, x = make_gmm(20_000, 7, 5, dtype, gpu, form="tril", subsample_size=subsample)
    la, ga = _elbo_run(monkeypatch, True, model, guide, x)
    assert mvn_calls == [(1, 7)], mvn_calls
    lb, gb = _elbo_run(monkeypatch, False, model, guide, x)
    assert len(mvn_calls) == 1
    rtol = 1e-10 if dtype == torch.float64 else 2e-5
    assert abs(la - lb) <= rtol * abs(lb), (la, lb)
    for n in gb:
        scale = float(gb[n].abs().max()) + 1e-30
        assert float((ga[n] - gb[n]).abs().max()) <= (1e-9 if dtype == torch.float64 else 2e-4) * scale, n


def test_captured_svi_step_equals_the_eager_one(gpu, mvn_calls):
    """SVI(model, guide, Adam, TraceEnum_ELBO) for 20 steps, captured and eager: the same kernels in the same order
    on the same inputs.  Tolerance: 1e-6 relative in f32 -- the captured step also replays torch's own small ops
    (the triangular solve for W, the Adam update), whose reduction order may differ between a graph replay and an
    eager launch by a few ulps per step, and Adam carries such differences over 20 steps."""
    import pyro_amd as pyro
    from pyro_amd.infer import SVI, TraceEnum_ELBO

    model, guide, x = make_gmm(20_000, 7, 5, torch.float32, gpu, form="tril")

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
    assert len(mvn_calls) >= 2
    np.testing.assert_allclose(lc, le, rtol=1e-6)
    for n in pe:
        torch.testing.assert_close(pc[n], pe[n], rtol=1e-6, atol=1e-6 * float(pe[n].abs().max()))


def test_nuts_potential_over_vectorised_chains(gpu, monkeypatch, mvn_calls):
    """The enumerated potential of an MVN mixture for 4 vectorised chains: ONE launch of the leaf with the chains
    as its 4 parameter sets, potential and gradient equal to the generic contraction's (float64); a short NUTS run
    over the same model completes with finite samples."""
    import pyro_amd as pyro
    import pyro_amd.distributions as dist
    import pyro_amd.ops.contract as c
    from pyro_amd.infer.mcmc import MCMC, NUTS, initialize_model
    from pyro_amd.ops.indexing import Vindex

    dtype = torch.float64
    K, N, D, C = 3, 500, 4, 4
    g = torch.Generator().manual_seed(4)
    data = (torch.randn(N, D, generator=g, dtype=dtype) + 3.0 * torch.randint(0, K, (N, 1), generator=g)).to(gpu)
    L = (random_tril(K, D, g) * 2.0).to(gpu)

    def model(data):
        phi = pyro.sample("phi", dist.Dirichlet(torch.ones(K, dtype=dtype, device=gpu)))
        with pyro.plate("num_clusters", K):
            means = pyro.sample("means", dist.Normal(torch.zeros(D, dtype=dtype, device=gpu), 5.0).to_event(1))
        with pyro.plate("data", N):
            a = pyro.sample("assignments", dist.Categorical(phi))
            pyro.sample("obs", dist.MultivariateNormal(Vindex(means.unsqueeze(-3))[..., a, :], scale_tril=L[a]),
                        obs=data)

    def run(fused):
        monkeypatch.setattr(c, "FUSED_MIXTURE", fused)
        pyro.set_rng_seed(0)
        init, pot, _, _ = initialize_model(model, (data,), max_plate_nesting=1, num_chains=C)
        z = {n: v.detach().clone().requires_grad_(True) for n, v in sorted(init.items())}
        n0 = len(mvn_calls)
        pe = pot(z)
        assert len(mvn_calls) - n0 == (1 if fused else 0), mvn_calls
        return pe.detach(), [t.detach() for t in torch.autograd.grad(pe.sum(), list(z.values()))]

    pa_, ga = run(True)
    assert mvn_calls[-1] == (C, K), mvn_calls
    pb, gb = run(False)
    torch.testing.assert_close(pa_, pb, rtol=1e-11, atol=0)
    for x, y in zip(ga, gb):
        torch.testing.assert_close(x, y, rtol=1e-9, atol=1e-9 * float(y.abs().max()))

    monkeypatch.setattr(c, "FUSED_MIXTURE", True)
    pyro.set_rng_seed(2)
    n0 = len(mvn_calls)
    mcmc = MCMC(NUTS(model, max_plate_nesting=1), num_samples=4, warmup_steps=4, num_chains=C)
    mcmc.run(data)
    assert len(mvn_calls) > n0
    for v in mcmc.get_samples().values():
        assert torch.isfinite(v).all()
    assert (C, K) in set(mvn_calls[n0:]), set(mvn_calls[n0:])


def test_large_evaluation_allocates_nothing_of_size_k_n(gpu, mvn_calls):
    """N = 1e6, K = 16, D = 32, f32: one loss_and_grads through the leaf allocates at most the row buffer, the
    workspace and small tensors -- far below one [K, N] f32 tensor (64 MB), let alone [K, N, D] (2 GB)."""
    import pyro_amd as pyro
    from pyro_amd.infer import TraceEnum_ELBO

    N, K, D = 1_000_000, 16, 32
    model, guide, x = make_gmm(N, K, D, torch.float32, gpu, form="tril")
    pyro.clear_param_store()
    elbo = TraceEnum_ELBO(max_plate_nesting=1)
    elbo.loss_and_grads(model, guide, x)             # (parameters created, kernels loaded)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    loss = elbo.loss_and_grads(model, guide, x)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    assert math.isfinite(loss)
    assert len(mvn_calls) == 2
    assert peak < K * N * 4, "peak %.1f MB over the data" % (peak / 2**20)
