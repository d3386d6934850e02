"""The per-row-weights mixture leaves (csrc/mixture_rows.hip) on the device: the kernels against float64 torch over a
grid of K, N, B, sharing, family, D, layout of the weights and dtype, with and without the responsibilities; -inf
weights, a dead row, a NaN row; TraceEnum_ELBO against the generic contraction and the unmodified reference, a captured
SVI step against the eager one, the NUTS potential over vectorised chains, the limits, and the memory of one call."""
import math
import os

import numpy as np
import pytest
import torch

from tests.event_mixture_cases import FAMILIES, dist_id, family_data, family_params
from tests.row_mixture_cases import flat_params, make_row_mixture, row_init, row_leaf_reference

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mixture_rows.npz")


def _inputs(family, K, D, N, B, share, layout, gpu, seed=0):
    """float64 inputs on the device: x [N] (D None) or [N, D]; a [B, N, K] log-probabilities per row -- ``layout``
    "rows": row-major [N, K] memory per set, "cols": [K, N]-contiguous memory seen as [N, K] (served by a copy),
    "sliced": K columns of a wider row-major matrix (read in place), "shared": one row-major set for every b
    (set-stride 0); p0, p1 [B | 1, K | 1(, D)] (p1 None for one-parameter families).  ``share``: None,
    "k" (p0 one value for every component) or "b" (both parameters one set for every b)."""
    g = torch.Generator().manual_seed(seed)
    d = 1 if D is None else D
    P0, P1 = family_params(family, K, d, g)
    x = family_data(family, P0, P1, N, g)
    Q0, Q1 = family_params(family, K, d, g)          # (the leaf's parameters near, not at, the data's)
    P0 = 0.7 * P0 + 0.3 * Q0
    P1 = None if P1 is None else 0.7 * P1 + 0.3 * Q1
    jit = lambda p: p * (1.0 + 0.05 * torch.rand(B, *p.shape, generator=g, dtype=torch.float64))  # noqa: E731
    p0, p1 = jit(P0), None if P1 is None else jit(P1)
    if D is None:
        x, p0, p1 = x[:, 0], p0[..., 0], None if p1 is None else p1[..., 0]
    if share == "k":
        p0 = p0[:, :1]
    elif share == "b":
        p0 = p0[:1]
        p1 = None if p1 is None else p1[:1]
    Ba = 1 if layout == "shared" else B
    a = torch.log_softmax(2.0 * torch.randn(Ba, N, K, generator=g, dtype=torch.float64), -1)
    x, a, p0, p1 = [None if t is None else t.to(gpu) for t in (x, a, p0, p1)]
    return x, a, p0, p1


def _lay_out(a, B, layout):
    """a [B | 1, N, K] contiguous -> the view of the requested memory layout"""
    if layout == "cols":
        a = a.permute(0, 2, 1).contiguous().permute(0, 2, 1)
        assert a.stride(1) == 1 or a.shape[1] == 1 or a.shape[2] == 1
    elif layout == "sliced":           # (the first K of K + 3 columns: component stride 1, row stride K + 3, no copy)
        wide = torch.full((a.shape[0], a.shape[1], a.shape[2] + 3), float("nan"), dtype=a.dtype, device=a.device)
        wide[..., :a.shape[2]] = a
        a = wide[..., :a.shape[2]]
        assert a.stride(2) == 1 and a.stride(1) == a.shape[2] + 3
    return a.expand(B, a.shape[1], a.shape[2])


def _call(family, x, a, p0, p1, want_da):
    from pyro_amd import kernels

    B, _, K = a.shape
    if x.dim() == 2:
        return kernels.mixture_rows_diag_normal_fwd_bwd(x, a, p0.contiguous(), p1.contiguous(), want_da=want_da)
    f0, s0, bs0 = flat_params(p0, B, K)
    f1, s1, bs1 = flat_params(p1, B, K)
    return kernels.mixture_rows_fwd_bwd(dist_id(family), x, a, f0, s0, f1, s1, bs0, bs1, want_da=want_da)


def _rel_errors(got, ref):
    """max |got - ref| / max |ref| per output (S, dS/da, dS/dp0, dS/dp1) that both have"""
    out = []
    for g_, r in zip(got, ref):
        if r is None or g_ is None:
            continue
        r = r.expand(g_.shape) if r.shape != g_.shape else r
        scale = float(r.abs().max()) or 1.0
        out.append(float((g_.double() - r).abs().max()) / scale)
    return out


def _check(family, dtype, x, a, p0, p1, B, layout="rows", want_da=True):
    cast = lambda t: None if t is None else t.to(dtype)  # noqa: E731
    x, a, p0, p1 = [cast(t) for t in (x, a, p0, p1)]
    a = _lay_out(a, B, layout)
    got = _call(family, x, a, p0, p1, want_da)
    again = _call(family, x, a, p0, p1, want_da)
    for p, q in zip(got, again):
        assert (p is None and q is None) or torch.equal(p, q), "two runs differ"
    assert (got[1] is None) == (not want_da)
    if want_da:
        assert got[1].dtype == dtype and got[1].shape == a.shape and got[1].is_contiguous()
    ref = row_leaf_reference(family, x, a, p0, p1)
    names = [n for n, g_, r in zip(("S", "da", "dp0", "dp1"), got, ref) if g_ is not None and r is not None]
    err = _rel_errors(got, ref)
    if dtype == torch.float64:
        bound = [1e-10] * len(err)
    else:
        # the f32 rule of tests/test_mixture_event_gpu.py::_check: no worse than 4x torch's own f32 computation
        # against float64, plus 1e-6 of the result's scale
        base = row_leaf_reference(family, x, a, p0, p1, dtype=torch.float32)
        base = [b_ if g_ is not None else None for b_, g_ in zip(base, got)]
        bound = [4.0 * e + 1e-6 for e in _rel_errors(base, ref)]
    for name, e, b in zip(names, err, bound):
        print("%s %s K=%d N=%d %s: error %.3g, bound %.3g" % (family, dtype, a.shape[2], a.shape[1], name, e, b))
    for name, e, b in zip(names, err, bound):
        assert e <= b, (name, e, b)
    return got, ref


# (K, N, B, shared parameters, layout of a, responsibilities wanted): every K of the limits' grid, ragged N
GRID = [
    (1, 1, 1, None, "rows", True),
    (3, 257, 4, "k", "rows", True),
    (3, 1000, 1, None, "cols", True),
    (16, 5003, 1, None, "rows", False),
    (16, 20_001, 4, "b", "shared", True),
    (64, 300, 1, None, "cols", False),
    (64, 70_001, 1, None, "rows", True),
    (16, 70_001, 4, None, "cols", True),
    # every lane layout the launcher can pick (KP = 2 and 32 next to 1, 4, 16, 64), and a row stride other than K
    (2, 4099, 1, None, "sliced", True),
    (32, 3001, 4, None, "rows", True),
    (7, 9001, 1, "k", "sliced", False),
]


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("K,N,B,share,layout,want_da", GRID)
@pytest.mark.parametrize("family", FAMILIES)
def test_kernel_against_float64_torch(gpu, family, dtype, K, N, B, share, layout, want_da):
    x, a, p0, p1 = _inputs(family, K, None, N, B, share, layout, gpu, seed=K * 131 + N)
    _check(family, dtype, x, a, p0, p1, B, layout, want_da)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("D", [1, 4, 5, 8])
@pytest.mark.parametrize("K,N,B,share,layout,want_da", GRID)
def test_diagonal_kernel_against_float64_torch(gpu, dtype, D, K, N, B, share, layout, want_da):
    x, a, p0, p1 = _inputs("Normal", K, D, N, B, share, layout, gpu, seed=K * 131 + N + D)
    _check("Normal", dtype, x, a, p0, p1, B, layout, want_da)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("D", [None, 5])
def test_switched_off_entries_and_a_dead_row(gpu, dtype, D):
    """-inf weights: no responsibility there; a row whose every weight is -inf: S = -inf, no responsibilities, and
    the other rows' responsibilities and the parameter gradients as without it."""
    x, a, p0, p1 = _inputs("Normal", 5, D, 2000, 2, None, "rows", gpu, seed=12)
    a = a.clone()
    a[:, ::3, 2] = -math.inf
    a[1, 40:44, :4] = -math.inf            # (one-hot rows)
    got, ref = _check("Normal", dtype, x, a, p0, p1, 2)
    assert float(got[1][:, ::3, 2].abs().max()) == 0.0
    assert torch.equal(got[1][1, 40:44, 4], torch.ones(4, dtype=dtype, device=gpu))
    dead = a.clone()
    dead[0, 17] = -math.inf
    S, da, d0, d1 = _call("Normal", *[t.to(dtype) for t in (x, dead, p0, p1)], True)
    assert S[0].item() == -math.inf and torch.equal(S[1], got[0][1])
    assert float(da[0, 17].abs().max()) == 0.0
    keep = torch.ones(2000, dtype=torch.bool, device=gpu)
    keep[17] = False
    assert torch.equal(da[:, keep], got[1][:, keep])
    alive = dead.clone()
    alive[0, 17] = 0.0
    alive[0, 17, 1:] = -math.inf
    _, _, e0, e1 = _call("Normal", *[t.to(dtype) for t in (x, alive, p0, p1)], True)
    # (the dead row gives the parameter gradients nothing: they differ from the run where it is alive with one
    #  component by that row's own term only)
    assert torch.isfinite(d0).all() and torch.isfinite(d1).all()
    assert float((d0 - e0)[1].abs().max()) == 0.0 and float((d0 - e0)[0].reshape(5, -1)[1:].abs().max()) == 0.0


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("D", [1, 3, 5])
def test_infinite_first_feature_is_a_dead_row(gpu, dtype, D):
    """x[row][0] = inf: every term of the row is -inf -- S = -inf, no responsibilities, finite parameter gradients equal
    to those of the run where that row's weights are -inf --, also where D is below the kernel's padded feature
    count (the padded slots take nothing from x)."""
    x, a, p0, p1 = [t.to(dtype) for t in _inputs("Normal", 3, D, 500, 1, None, "rows", gpu, seed=15)]
    bad = x.clone()
    bad[17, 0] = math.inf
    S, da, dl, dc = _call("Normal", bad, a, p0, p1, True)
    assert S[0].item() == -math.inf and float(da[0, 17].abs().max()) == 0.0
    off = a.clone()
    off[0, 17] = -math.inf
    _, da2, dl2, dc2 = _call("Normal", x, off, p0, p1, True)
    assert torch.isfinite(dl).all() and torch.isfinite(dc).all()
    assert torch.equal(da, da2) and torch.equal(dl, dl2) and torch.equal(dc, dc2)


@pytest.mark.parametrize("D", [None, 5])
def test_nan_row_propagates(gpu, D):
    x, a, p0, p1 = _inputs("Normal", 3, D, 300, 1, None, "rows", gpu, seed=14)
    clean = _call("Normal", x, a, p0, p1, True)
    bad = x.clone()
    bad[17] = float("nan")
    S, da, _, _ = _call("Normal", bad, a, p0, p1, True)
    assert torch.isnan(S).all() and torch.isnan(da[0, 17]).all()
    keep = torch.ones(300, dtype=torch.bool, device=gpu)
    keep[17] = False
    assert torch.equal(da[:, keep], clean[1][:, keep])
    a = a.clone()
    a[0, 5, 1] = float("nan")
    S, da, _, _ = _call("Normal", x, a, p0, p1, True)
    assert torch.isnan(S).all() and torch.isnan(da[0, 5]).all()


@pytest.fixture
def row_calls(monkeypatch):
    from pyro_amd import kernels

    calls = []
    real_s, real_d = kernels.mixture_rows_fwd_bwd, kernels.mixture_rows_diag_normal_fwd_bwd

    def scalar(dist, x, a, *rest, **kw):
        calls.append(("scalar", tuple(a.shape), kw.get("want_da", True)))
        return real_s(dist, x, a, *rest, **kw)

    def diag(x, a, *rest, **kw):
        calls.append(("diag", tuple(a.shape), kw.get("want_da", True)))
        return real_d(x, a, *rest, **kw)

    monkeypatch.setattr(kernels, "mixture_rows_fwd_bwd", scalar)
    monkeypatch.setattr(kernels, "mixture_rows_diag_normal_fwd_bwd", diag)
    return calls


def _elbo_run(monkeypatch, fused, model, guide, x):
    import pyro_amd as pyro
    import pyro_amd.ops.contract as c
    from pyro_amd.infer import TraceEnum_ELBO

    monkeypatch.setattr(c, "FUSED_MIXTURE", fused)
    pyro.clear_param_store()
    pyro.set_rng_seed(1)
    loss = TraceEnum_ELBO(max_plate_nesting=1).loss_and_grads(model, guide, x)
    return loss, {n: p.grad.detach().clone() for n, p in pyro.get_param_store().named_parameters()
                  if p.grad is not None}


@pytest.mark.parametrize("dtype,subsample", [(torch.float64, None), (torch.float32, None), (torch.float32, 6000)])
@pytest.mark.parametrize("form,D", [("experts", None), ("grouped", None), ("labels", None), ("experts", 5),
                                    ("detached", None)])
def test_elbo_leaf_is_fused_and_equals_the_generic_contraction(gpu, monkeypatch, row_calls, form, D, dtype, subsample):
    """TraceEnum_ELBO on a mixture with per-row weights (N = 20 000, K = 7): one launch of the leaf, loss and every
    gradient equal to the generic contraction's within the tolerances tests/test_mixture_event_gpu.py uses for that
    comparison."""
    init = row_init("Normal", 20_000, 7, D, seed=2)
    model, guide, x = make_row_mixture(form, init, dtype, gpu, subsample_size=subsample)
    la, ga = _elbo_run(monkeypatch, True, model, guide, x)
    rows = subsample or 20_000
    assert row_calls == [("scalar" if D is None else "diag", (1, rows, 7), form != "detached")], row_calls
    lb, gb = _elbo_run(monkeypatch, False, model, guide, x)
    assert len(row_calls) == 1
    rtol = 1e-10 if dtype == torch.float64 else 2e-5
    print("loss", la, lb)
    assert abs(la - lb) <= rtol * abs(lb), (la, lb)
    assert set(ga) == set(gb)
    for n in gb:
        scale = float(gb[n].abs().max()) + 1e-30
        err = float((ga[n] - gb[n]).abs().max())
        print(n, err / scale)
        assert err <= (1e-9 if dtype == torch.float64 else 2e-4) * scale, n


def test_backward_scales_the_responsibilities_once(gpu):
    """The backward to the weights multiplies the leaf's private buffer in place: g * r for any g, and a second
    backward of the same forward is refused by torch instead of scaling twice."""
    from pyro_amd.ops import contract

    x, a, p0, p1 = _inputs("Normal", 3, None, 1000, 1, None, "rows", gpu, seed=16)
    a.requires_grad_()
    f0, s0, bs0 = flat_params(p0, 1, 3)
    f1, s1, bs1 = flat_params(p1, 1, 3)
    S = contract._MixtureRowsFactor.invoke(dist_id("Normal"), s0, s1, bs0, bs1, True, x, a, f0, f1)
    ref = row_leaf_reference("Normal", x, a, p0, p1)
    (g,) = torch.autograd.grad((2.5 * S).sum(), a, retain_graph=True)
    assert float((g - 2.5 * ref[1]).abs().max()) <= 1e-10
    with pytest.raises(RuntimeError):
        torch.autograd.grad((2.5 * S).sum(), a)


@pytest.mark.parametrize("form", ["experts", "grouped"])
def test_leaf_matches_reference(gpu, monkeypatch, row_calls, form):
    """Loss and gradients of the unmodified reference's TraceEnum_ELBO (float64) through the kernel."""
    gold = np.load(GOLDEN)
    init = {k.split("/", 2)[2]: torch.as_tensor(gold[k]) for k in gold.files if k.startswith(form + "/init/")}
    model, guide, x = make_row_mixture(form, init, torch.float64, gpu)
    loss, grads = _elbo_run(monkeypatch, True, model, guide, x)
    assert len(row_calls) == 1
    ref = float(gold[form + "/loss"])
    assert abs(loss - ref) <= 1e-9 * abs(ref), (loss, ref)
    names = [k.split("/", 2)[2] for k in gold.files if k.startswith(form + "/grad/")]
    assert set(names) == set(grads) and names
    for n in names:
        r = torch.as_tensor(gold[form + "/grad/" + n]).to(gpu)
        assert float((grads[n] - r).abs().max()) <= 1e-9 * (float(r.abs().max()) + 1e-300), n


def test_captured_svi_step_equals_the_eager_one(gpu, row_calls):
    """SVI(model, guide, Adam, TraceEnum_ELBO) on the "experts" mixture for 20 steps, captured and eager: the same
    kernels in the same order on the same inputs (tolerance as the event leaf's test)."""
    import pyro_amd as pyro
    from pyro_amd.infer import SVI, TraceEnum_ELBO

    model, guide, x = make_row_mixture("experts", row_init("Normal", 20_000, 7, seed=3), torch.float32, gpu)

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
    assert len(row_calls) >= 2
    np.testing.assert_allclose(lc, le, rtol=1e-6)
    for n in pe:
        torch.testing.assert_close(pc[n], pe[n], rtol=1e-6, atol=1e-6 * float(pe[n].abs().max()))


def test_nuts_potential_over_vectorised_chains(gpu, monkeypatch, row_calls):
    """The enumerated potential of a gated Normal mixture for 4 vectorised chains: ONE launch of the leaf per
    evaluation with the chains as its 4 parameter sets (gate weights and component locations per chain), potential
    and gradient equal to the generic contraction's (float64); a short NUTS run completes with finite samples."""
    import pyro_amd as pyro
    import pyro_amd.distributions as dist
    import pyro_amd.ops.contract as c
    from pyro_amd.infer.mcmc import MCMC, NUTS, initialize_model
    from pyro_amd.ops.indexing import Vindex

    dtype = torch.float64
    K, N, F, C = 3, 500, 2, 4
    init = row_init("Normal", N, K, F=F, seed=4)
    data, X = init["x"].to(gpu), init["X"].to(gpu)

    def model(data):
        W = pyro.sample("W", dist.Normal(torch.zeros(F, K, dtype=dtype, device=gpu), 1.0).to_event(2))
        with pyro.plate("num_clusters", K):
            locs = pyro.sample("locs", dist.Normal(torch.zeros((), dtype=dtype, device=gpu), 3.0))
        logits = torch.matmul(X, W)
        if logits.dim() > 2:
            logits = logits.squeeze(-3)
        with pyro.plate("data", N):
            z = pyro.sample("assignments", dist.Categorical(logits=logits))
            # (with a leading chain dim the cluster dim has to move off the data plate's dim first)
            pyro.sample("obs", dist.Normal(Vindex(locs.unsqueeze(-2))[..., z], 1.0), obs=data)

    def run(fused):
        monkeypatch.setattr(c, "FUSED_MIXTURE", fused)
        pyro.set_rng_seed(0)
        init_z, pot, _, _ = initialize_model(model, (data,), max_plate_nesting=1, num_chains=C)
        z = {n: v.detach().clone().requires_grad_(True) for n, v in sorted(init_z.items())}
        n0 = len(row_calls)
        pe = pot(z)
        assert len(row_calls) - n0 == (1 if fused else 0), row_calls
        return pe.detach(), [t.detach() for t in torch.autograd.grad(pe.sum(), list(z.values()))]

    pa_, ga = run(True)
    assert row_calls[-1] == ("scalar", (C, N, K), True), row_calls
    pb, gb = run(False)
    torch.testing.assert_close(pa_, pb, rtol=1e-11, atol=0)
    for x, y in zip(ga, gb):
        torch.testing.assert_close(x, y, rtol=1e-9, atol=1e-9 * float(y.abs().max()))

    monkeypatch.setattr(c, "FUSED_MIXTURE", True)
    pyro.set_rng_seed(2)
    n0 = len(row_calls)
    mcmc = MCMC(NUTS(model, max_plate_nesting=1), num_samples=4, warmup_steps=4, num_chains=C)
    mcmc.run(data)
    assert len(row_calls) > n0
    for v in mcmc.get_samples().values():
        assert torch.isfinite(v).all()
    assert ("scalar", (C, N, K), True) in set(row_calls[n0:]), set(row_calls[n0:])


def test_limits_raise_unsupported(gpu):
    from pyro_amd import kernels

    x = torch.zeros(10, device=gpu)
    one = torch.ones(65, device=gpu)
    with pytest.raises(kernels.Unsupported):
        kernels.mixture_rows_fwd_bwd(dist_id("Normal"), x, torch.zeros(1, 10, 65, device=gpu), one, 1, one, 1)
    with pytest.raises(kernels.Unsupported):
        kernels.mixture_rows_fwd_bwd(dist_id("Normal"), x, torch.zeros(1, 10, 3, device=gpu).expand(65536, 10, 3),
                                     one, 0, one, 0, want_da=False)
    with pytest.raises(kernels.Unsupported):
        kernels.mixture_rows_fwd_bwd(99, x, torch.zeros(1, 10, 3, device=gpu), one, 1, one, 1)
    with pytest.raises(kernels.Unsupported):
        kernels.mixture_rows_diag_normal_fwd_bwd(torch.zeros(10, 9, device=gpu), torch.zeros(1, 10, 3, device=gpu),
                                                 torch.zeros(1, 3, 9, device=gpu), torch.ones(1, 3, 9, device=gpu))
    with pytest.raises(kernels.Unsupported):
        kernels.mixture_rows_diag_normal_fwd_bwd(torch.zeros(10, 4, device=gpu), torch.zeros(1, 10, 65, device=gpu),
                                                 torch.zeros(1, 65, 4, device=gpu), torch.ones(1, 65, 4, device=gpu))
    # the C entry point itself answers PA_ERR_UNSUPPORTED before any launch
    lib = kernels._lib.load()
    rc = lib.pa_mixture_rows_fwd_bwd(kernels._lib.PA_F32, dist_id("Normal"), None, 10, 65, 1, None, 1, 65, 0, None, 1,
                                     0, None, 1, 0, None, None, 0, None, None)
    assert rc == kernels._lib.PA_ERR_UNSUPPORTED


@pytest.mark.parametrize("want_da", [True, False])
def test_one_call_allocates_the_responsibilities_and_the_workspace(gpu, want_da):
    """N = 1e6, K = 16, f32: one call allocates at most the responsibilities (B N K values, only when they are
    wanted), the workspace its _workspace function states, and 1 MB -- what its outputs are, not a measurement."""
    from pyro_amd import kernels

    N, K = 1_000_000, 16
    g = torch.Generator().manual_seed(0)
    x = torch.randn(N, generator=g).to(gpu)
    a = torch.log_softmax(torch.randn(N, K, generator=g), -1).to(gpu).reshape(1, N, K)
    p0 = torch.linspace(-2, 2, K, device=gpu)
    p1 = torch.ones(K, device=gpu)
    args = (dist_id("Normal"), x, a, p0, 1, p1, 1)
    kernels.mixture_rows_fwd_bwd(*args, want_da=want_da)       # (kernels loaded)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = kernels.mixture_rows_fwd_bwd(*args, want_da=want_da)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    assert math.isfinite(float(out[0][0]))
    ws = kernels._lib.load().pa_mixture_rows_workspace(K, 1)
    allowed = (N * K * 4 if want_da else 0) + ws + 2**20
    print("peak %d bytes, allowed %d" % (peak, allowed))
    assert peak <= allowed, (peak, allowed)
