"""Device tests of the fused plated regression sites (csrc/glm_family.hip; Normal, StudentT, Poisson, Binomial): the
kernel entry by entry against the float64 restatement of tests/glm_family_cases.py at every seam of the launch plan,
its edge cases, the cross-check with the Bernoulli kernel, and the site class through Trace_ELBO, the vectorised NUTS
potential, a captured SVI step and Predictive.

The bound per entry is max(4 * e32, 4 * 2^-23 * A): e32 the entry's error in the float32 torch route on the CPU
against the same float64 reference (the project's four-times rule), A the float64 sum of the absolute values of the
addends that make up the entry (the floor, at the magnitude a float32 sum's rounding scales with)."""
import numpy as np
import pytest
import torch

from tests import glm_family_cases as cases

pytestmark = pytest.mark.gpu

OUTPUTS = ("s", "gw", "gb", "gaux")


def _call(gpu, family, a, scale, max_blocks=0):
    from pyro_amd import kernels
    d = lambda t: t.to(gpu) if isinstance(t, torch.Tensor) else t      # noqa: E731
    out = kernels.glm_family_fwd_bwd(cases.FAMILY_ID[family], d(a["X"]), d(a["y"]), d(a["w"]), d(a["b"]), d(a["aux"]),
                                     d(a["count"]), d(a["mask"]), scale, _max_blocks=max_blocks)
    torch.cuda.synchronize()
    return dict(zip(OUTPUTS + ("cnt",), out))


def _check(family, a, scale, got, what):
    ref, bound = cases.bounds(family, a["X"], a["y"], a["w"], a["b"], a["aux"], a["count"], a["mask"], scale, False)
    for k in OUTPUTS:
        if ref[k] is None:
            assert got[k] is None or k == "gb"
            continue
        cases.assert_within(got[k], ref[k], bound[k], "%s %s %s" % (family, what, k))
    n = a["X"].shape[0] if a["mask"] is None else int(a["mask"].sum())
    assert got["cnt"].dtype == torch.float64 and got["cnt"].shape == (1,) and float(got["cnt"]) == float(n)


@pytest.mark.parametrize("case", cases.kernel_cases(), ids=cases.case_id)
@pytest.mark.parametrize("family", cases.FAMILIES)
def test_kernel_entry_by_entry(gpu, family, case):
    N, D, P, bias, masked, scale, max_blocks = case
    a = cases.make_inputs(family, N, D, P, bias, masked, seed=1000 + 7 * N + 3 * D + P,
                          per_row_count=(N + D) % 2 == 0)
    _check(family, a, scale, _call(gpu, family, a, scale, max_blocks), cases.case_id(case))


@pytest.mark.parametrize("D", [32, 5])
@pytest.mark.parametrize("family", cases.FAMILIES)
def test_garbage_in_masked_rows_contributes_exactly_nothing(gpu, family, D):
    """NaN in y, inf in X (and NaN in the Binomial count) of masked rows: every output bit-identical to the call
    with those rows zeroed."""
    a = cases.make_inputs(family, 300, D, 33, True, True, seed=5)
    off = ~a["mask"]
    clean, dirty = dict(a), dict(a)
    for k, fill in (("X", float("inf")), ("y", float("nan")), ("count", float("nan"))):
        if isinstance(a[k], torch.Tensor):
            clean[k], dirty[k] = a[k].clone(), a[k].clone()
            clean[k][off] = 0.0
            dirty[k][off] = fill
    dirty["X"][off, ::2] = float("-inf")
    want, got = _call(gpu, family, clean, 3.5), _call(gpu, family, dirty, 3.5)
    for k in OUTPUTS + ("cnt",):
        if want[k] is not None:
            assert bool(torch.isfinite(got[k]).all()), k
            assert torch.equal(got[k].view(torch.uint8), want[k].view(torch.uint8)), (family, k)
    _check(family, a, 3.5, got, "masked garbage")


@pytest.mark.parametrize("family", cases.FAMILIES)
def test_all_false_mask_and_empty_plate_give_zeros(gpu, family):
    a = cases.make_inputs(family, 129, 7, 33, True, True, seed=6)
    a["mask"] = torch.zeros(129, dtype=torch.bool)
    empty = cases.make_inputs(family, 0, 7, 33, True, False, seed=6)
    for inp in (a, empty):
        got = _call(gpu, family, inp, 3.5)
        for k in OUTPUTS + ("cnt",):
            if got[k] is not None:
                assert got[k].numel() > 0 and not bool(got[k].any()), (family, k)
        assert got["gw"].shape == (33, 7) and got["s"].shape == (33,)


@pytest.mark.parametrize("family,times", [("student_t", 1e4), ("normal", 1e3)])
def test_far_residuals_stay_finite_and_within_the_bound(gpu, family, times):
    a = cases.make_inputs(family, 129, 8, 33, True, False, seed=8)
    a["y"][5] += times * float(a["aux"][:, -1].max()) * 1.5
    a["y"][77] -= times * float(a["aux"][:, -1].max()) * 1.5
    got = _call(gpu, family, a, 1.0)
    for k in OUTPUTS:
        assert bool(torch.isfinite(got[k]).all()), k
    _check(family, a, 1.0, got, "far residual")


@pytest.mark.parametrize("shape", [(300, 32, 64, True), (129, 5, 33, False), (1100, 64, 3, True), (127, 128, 32, True),
                                   (33, 4, 1, False)], ids=lambda s: "N%d-D%d-P%d" % s[:3])
def test_binomial_of_one_trial_is_the_bernoulli_kernel(gpu, shape):
    """PA_GLM_BINOMIAL_LOGITS with n = 1 against the exact-f32 Bernoulli kernel (variant 1): the same f32 chains in the
    same order, so gw and gb are bit-equal; ll within the bound."""
    from pyro_amd import kernels
    N, D, P, masked = shape
    a = cases.make_inputs("binomial", N, D, P, True, masked, seed=9)
    a["count"] = 1.0
    a["y"] = (a["y"] > 2).float()
    got = _call(gpu, "binomial", a, 3.5)
    d = lambda t: None if t is None else t.to(gpu)      # noqa: E731
    kernels.glm_set_variant(kernels.GLM_EXACT_F32)
    try:
        ll, gw, gb = kernels.glm_bernoulli_fwd_bwd(d(a["X"]), d(a["y"]), d(a["w"]), d(a["b"]), d(a["mask"]), 3.5)
        torch.cuda.synchronize()
    finally:
        kernels.glm_set_variant(kernels.GLM_AUTO)
    assert torch.equal(got["gw"], gw) and torch.equal(got["gb"], gb)
    ref, bound = cases.bounds("binomial", a["X"], a["y"], a["w"], a["b"], None, 1.0, a["mask"], 3.5, False)
    cases.assert_within(ll, ref["s"], bound["s"], "bernoulli ll")
    cases.assert_within(got["s"], ref["s"], bound["s"], "binomial ll")


def test_unsupported_layouts_are_refused(gpu):
    from pyro_amd import _lib, kernels
    lib = _lib.load()
    assert lib.pa_glm_family_workspace(0, 100, 129, 4, 0) == 0 and lib.pa_glm_family_workspace(7, 100, 8, 4, 0) == 0
    rc = lib.pa_glm_family_fwd_bwd(0, None, None, None, None, None, None, 0.0, None, 1.0, 100, 129, 4, 0, None, None,
                                   None, None, None, None, 0, None)
    assert rc == _lib.PA_ERR_UNSUPPORTED
    with pytest.raises(kernels.Unsupported):
        a = cases.make_inputs("normal", 16, 4, 2, True, False, seed=1)
        a["X"] = a["X"].double()
        _call(gpu, "normal", a, 1.0)


# ---- the site class -------------------------------------------------------------------------------------------------
def _class_inputs(name, N, P):
    """The fixture's data at N = 300 (its first particle alone for P = 1); a generated set of the same kind at 1000."""
    family = cases.family_of(name)
    g = {k.split("/", 1)[1]: v for k, v in np.load(cases.GOLDEN).items() if k.startswith(name + "/")}
    t = lambda v: torch.as_tensor(np.asarray(v), dtype=torch.float32)      # noqa: E731
    if N == 300:
        X, y, mask, plate = t(g["X"]), t(g["y"]), torch.as_tensor(g["mask"]), 1000
        count = None
        if family == "binomial":
            count = t(g["count"]) if name == "binomial_rows" else cases.SCALAR_COUNT
    else:
        a = cases.make_inputs(family, N, 5, 3, True, True, seed=77, per_row_count=name == "binomial_rows")
        X, y, mask, count, plate = a["X"], a["y"], a["mask"], a["count"], 2500
    lat = {k: t(g[k]) for k in ("w", "b") + cases.AUX_NAMES[family][::-1]}
    if P == 1:
        lat = {k: v[0, 0] for k, v in lat.items()}
    return g, family, X, y, mask, count, plate, lat


def _spy(monkeypatch):
    from pyro_amd import kernels
    calls, real = [], kernels.glm_family_fwd_bwd

    def spy(*args, **kwargs):
        calls.append(args[0])
        return real(*args, **kwargs)
    monkeypatch.setattr(kernels, "glm_family_fwd_bwd", spy)
    return calls


@pytest.mark.parametrize("P", [1, 3])
@pytest.mark.parametrize("N", [300, 1000])
@pytest.mark.parametrize("name", cases.GOLDEN_MODELS)
def test_one_launch_per_step_and_the_fixture_values(gpu, monkeypatch, name, N, P):
    import pyro_amd as pyro
    import pyro_amd.distributions as dist
    from pyro_amd import poutine
    from pyro_amd.distributions import families
    g, family, X, y, mask, count, plate, lat = _class_inputs(name, N, P)
    flat = {k: v.reshape(P, -1) for k, v in lat.items()}
    aux = [flat[k][:, 0] for k in cases.AUX_NAMES[family]]
    ref, bound = cases.bounds(family, X, y, flat["w"], flat["b"][:, 0], torch.stack(aux, -1) if aux else None, count,
                              mask, plate / N, True)
    if N == 300 and P == 3:          # the reference's own numbers, to the rounding of the inputs to float32
        fixture = [("s", g["ll"]), ("gw", g["grad_w"][:, 0]), ("gb", g["grad_b"][:, 0])]
        fixture += [("gaux", np.stack([g["grad_" + a][:, 0] for a in cases.AUX_NAMES[family]], -1))] if aux else []
        for k, want in fixture:
            err = float((ref[k] - torch.as_tensor(want)).abs().max()) / (1.0 + float(np.abs(want).max()))
            assert err <= 2e-6, (k, err)
    model = cases.make_model(pyro, dist, poutine, name)
    d = lambda v: v.to(gpu) if isinstance(v, torch.Tensor) else v      # noqa: E731
    calls = _spy(monkeypatch)
    for fused in (True, False):
        del calls[:]
        monkeypatch.setattr(families, "FUSED_GLM_FAMILIES", fused)
        pyro.clear_param_store()
        guide = cases.make_guide(pyro, dist, {k: d(v) for k, v in lat.items()})
        elbo = pyro.infer.Trace_ELBO(num_particles=P, vectorize_particles=P > 1, max_plate_nesting=1)
        loss = elbo.loss_and_grads(model, guide, d(X), d(y), d(mask), plate, d(count))
        torch.cuda.synchronize()
        assert calls == ([cases.FAMILY_ID[family]] if fused else []), (name, fused, calls)
        grads = {k: v.grad for k, v in pyro.get_param_store().named_parameters()}
        cases.assert_step_within(loss, grads, ref, bound, family, P)


def test_vectorised_nuts_potential_takes_the_fused_poisson_site(gpu, monkeypatch):
    """Three chains: potential_fn and its gradient from one launch, against the float64 restatement and the
    materialised route."""
    import pyro_amd as pyro
    import pyro_amd.distributions as dist
    from pyro_amd.distributions import families
    from pyro_amd.infer.mcmc import initialize_model
    a = cases.make_inputs("poisson", 600, 5, 3, True, False, seed=31)
    X, y = a["X"].to(gpu), a["y"].to(gpu)

    def model(X, y):
        w = pyro.sample("w", dist.Normal(X.new_zeros(X.shape[1]), 1.0).to_event(1))
        b = pyro.sample("b", dist.Normal(X.new_zeros(()), 1.0))
        with pyro.plate("data", X.shape[0]):
            pyro.sample("obs", dist.Poisson(torch.exp(X @ w + b) if w.dim() == 1 else
                                            torch.exp((w @ X.t()).squeeze(-2) + b)), obs=y)

    calls = _spy(monkeypatch)
    z0 = {"w": a["w"].to(gpu), "b": a["b"].to(gpu)}
    ref, bound = cases.bounds("poisson", a["X"], a["y"], a["w"], a["b"], None, None, None, 1.0, True)
    w64, b64 = a["w"].double(), a["b"].double()
    prior = 0.5 * (w64 * w64).sum(-1) + 0.5 * b64 * b64 + 0.5 * 6 * np.log(2 * np.pi)
    slack = cases.F32_FLOOR * (prior.abs() + 6.0)
    out = {}
    for fused in (True, False):
        del calls[:]
        monkeypatch.setattr(families, "FUSED_GLM_FAMILIES", fused)
        pyro.set_rng_seed(0)
        init, pot, _, _ = initialize_model(model, (X, y), num_chains=3, max_plate_nesting=1)
        del calls[:]
        z = {k: v.clone().requires_grad_(True) for k, v in z0.items()}
        pe = pot(z)
        gw, gb = torch.autograd.grad(pe.sum(), [z["w"], z["b"]])
        torch.cuda.synchronize()
        assert (len(calls) == 1) if fused else not calls, (fused, calls)
        assert pe.shape == (3,)
        cases.assert_within(pe, prior - ref["s"], bound["s"] + slack, "potential")
        cases.assert_within(gw, w64 - ref["gw"], bound["gw"] + cases.F32_FLOOR * w64.abs(), "d potential / d w")
        cases.assert_within(gb, b64 - ref["gb"], bound["gb"] + cases.F32_FLOOR * b64.abs(), "d potential / d b")
        out[fused] = (pe, gw, gb)
    for k, (a_, b_) in enumerate(zip(out[True], out[False])):        # the two routes against each other
        lim = 2.0 * ((bound["s"] + slack, bound["gw"] + cases.F32_FLOOR * w64.abs(),
                      bound["gb"] + cases.F32_FLOOR * b64.abs())[k])
        cases.assert_within(a_, b_.detach().cpu().double(), lim, "fused against materialised, output %d" % k)


@pytest.mark.parametrize("name", ["normal", "binomial_scalar"])
def test_svi_captures_its_step_on_the_fused_site(gpu, monkeypatch, name):
    """SVI built with the reference's constructor captures its step by itself, with the fused site in it (the kernel
    is called while the step is eager and while it is captured, never by a replay); the 30 losses follow the eager
    run's.  Binomial: the scalar count is a 0-dim DEVICE tensor, which the site must not read on the host."""
    import pyro_amd as pyro
    import pyro_amd.distributions as dist
    from pyro_amd import poutine
    from pyro_amd.infer import SVI, Trace_ELBO
    from pyro_amd.infer.autoguide import AutoNormal
    _, family, X, y, mask, count, plate, _ = _class_inputs(name, 1000, 3)
    X, y, mask = X.to(gpu), y.to(gpu), mask.to(gpu)
    if count is not None:
        count = torch.full((), float(count), device=gpu)
    model = cases.make_model(pyro, dist, poutine, name)
    calls = _spy(monkeypatch)
    runs = {}
    for graph in (False, True):
        del calls[:]
        pyro.clear_param_store()
        pyro.set_rng_seed(11)
        guide = AutoNormal(model, init_scale=0.1)
        elbo = Trace_ELBO(num_particles=8, vectorize_particles=True, max_plate_nesting=1)
        optim = pyro.optim.Adam({"lr": 0.01})
        svi = SVI(model, guide, optim, elbo) if graph else SVI(model, guide, optim, elbo, hip_graph=False)
        try:
            losses = [svi.step(X, y, mask, plate, count) for _ in range(30)]
            if graph:
                assert svi._auto_graph and svi.hip_graph and len(svi._graphs) == 1      # captured, not fallen back
                assert 1 <= len(calls) < 30, len(calls)
            else:
                assert len(calls) == 30, len(calls)
            assert set(calls) == {cases.FAMILY_ID[family]}
        finally:
            svi.release()
        runs[graph] = torch.tensor(losses, dtype=torch.float64)
    assert bool(torch.isfinite(runs[True]).all())
    # (the floor at the magnitude of the loss itself: the sums behind it are larger)
    cases.assert_within(runs[True], runs[False], cases.F32_FLOOR * runs[False].abs(), "captured losses")


def test_nuts_keeps_the_generic_potential_for_the_new_families(gpu, monkeypatch):
    """The direct NUTS potential (infer/mcmc/direct.py) knows the Bernoulli site only: a Poisson or Normal regression
    under NUTS with several chains must not engage it (it would score the site as Bernoulli), takes the fused site
    through the generic potential, and its chains find the coefficients."""
    import pyro_amd as pyro
    import pyro_amd.distributions as dist
    from pyro_amd.infer.mcmc import MCMC, NUTS
    g = torch.Generator().manual_seed(0)
    N, D, C = 2000, 3, 8
    X = torch.randn((N, D), generator=g)
    true = torch.tensor([0.5, -0.3, 0.2])
    data = {"poisson": torch.poisson(torch.exp(X @ true + 0.4), generator=g),
            "normal": X @ true + 0.4 + 0.7 * torch.randn((N,), generator=g)}
    X = X.to(gpu)

    def make(family):
        def model(X, y):
            w = pyro.sample("w", dist.Normal(X.new_zeros(X.shape[1]), 1.0).to_event(1))
            b = pyro.sample("b", dist.Normal(X.new_zeros(()), 1.0))
            with pyro.plate("data", X.shape[0]):
                eta = w @ X.t()
                eta = (eta.squeeze(-2) if eta.dim() > 1 else eta) + b
                if family == "poisson":
                    pyro.sample("obs", dist.Poisson(torch.exp(eta)), obs=y)
                else:
                    pyro.sample("obs", dist.Normal(eta, 0.7), obs=y)
        return model

    calls = _spy(monkeypatch)
    for family, y in data.items():
        del calls[:]
        pyro.set_rng_seed(2)
        kernel = NUTS(make(family), max_tree_depth=5)
        assert kernel.use_direct_potential
        mcmc = MCMC(kernel, num_samples=40, warmup_steps=60, num_chains=C)
        mcmc.run(X, y.to(gpu))
        assert kernel._direct is None, family
        assert calls and set(calls) == {cases.FAMILY_ID[family]}
        s = mcmc.get_samples()
        assert s["w"].shape == (C * 40, D)
        assert float((s["w"].mean(0).cpu() - true).abs().max()) < 0.1, (family, s["w"].mean(0))
        assert abs(float(s["b"].mean()) - 0.4) < 0.1, (family, float(s["b"].mean()))


@pytest.mark.parametrize("name", ["normal", "student_t", "poisson", "binomial_rows"])
def test_predictive_and_sample_draw_from_the_fused_site(gpu, name):
    import pyro_amd as pyro
    import pyro_amd.distributions as dist
    from pyro_amd import poutine
    from pyro_amd.distributions import families
    from pyro_amd.infer import Predictive
    _, family, X, y, mask, count, plate, lat = _class_inputs(name, 300, 3)
    d = lambda v: v.to(gpu) if isinstance(v, torch.Tensor) else v      # noqa: E731
    model = cases.make_model(pyro, dist, poutine, name)
    # the site as the model builds it without an observation: the fused class, drawn from through the ordinary one
    pyro.set_rng_seed(3)
    tr = poutine.trace(poutine.condition(model, data={k: d(v) for k, v in lat.items()})).get_trace(
        d(X), None, d(mask), plate, d(count))
    fn, direct = tr.nodes["obs"]["fn"], tr.nodes["obs"]["value"]
    assert isinstance(fn, families._LinearPredictor), type(fn)
    assert direct.shape == (3, 300) == tuple(fn.batch_shape) and fn.sample((2,)).shape == (2, 3, 300)
    post = {k: d(v).reshape((3,) + ((5,) if k == "w" else ())) for k, v in lat.items()}
    draws = Predictive(model, posterior_samples=post, return_sites=["obs"])(d(X), None, d(mask), plate, d(count))["obs"]
    assert draws.shape[0] == 3 and draws.shape[-1] == 300 and draws.numel() == 900
    for v in (direct, draws.reshape(3, 300)):
        assert bool(torch.isfinite(v).all()) and bool(fn.support.check(v).all())
        if family in ("poisson", "binomial"):
            assert bool((v >= 0).all()) and bool((v == v.round()).all())
        if family == "binomial":
            assert bool((v <= d(count)).all())
