"""Host tests of the fused plated regression sites (Normal, StudentT, Poisson, Binomial over a lazy linear predictor):
the fixture written by the unmodified reference against the package's materialised route and against the float64
restatement the device tests lean on; the recognition logic of ops/lazy.py and distributions/families.py on the CPU
(the predicates that say "device tensor" are answered with yes, tests/oracle_backend.py; the kernel is answered by
the restatement); the case table's coverage."""
import numpy as np
import pytest
import torch

from tests import glm_family_cases as cases


@pytest.fixture(autouse=True)
def _cpu_backend(oracle_backend):
    yield


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(cases.GOLDEN))


def _close(got, want, tol, what):
    got, want = torch.as_tensor(got, dtype=torch.float64), torch.as_tensor(want, dtype=torch.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    err = float((got - want).abs().max()) / (1.0 + float(want.abs().max()))
    assert err <= tol, (what, err)


def _fixture_inputs(golden, name, dtype=torch.float64):
    g = {k.split("/", 1)[1]: v for k, v in golden.items() if k.startswith(name + "/")}
    t = lambda a: torch.as_tensor(a, dtype=dtype)       # noqa: E731
    family = cases.family_of(name)
    count = None
    if family == "binomial":
        count = t(g["count"]) if name == "binomial_rows" else cases.SCALAR_COUNT
    latents = {k: t(g[k]) for k in ("w", "b") + cases.AUX_NAMES[family][::-1]}
    return g, family, t(g["X"]), t(g["y"]), torch.as_tensor(g["mask"]), count, latents


def _kernel_standin(calls=None):
    """kernels.glm_family_fwd_bwd answered by the float64 restatement (inputs and outputs in the caller's dtype)."""
    def fn(family, X, y, w, b, aux, count, mask, scale, _max_blocks=0):
        if calls is not None:
            calls.append(family)
        out = cases.torch_route(cases.FAMILIES[family], X, y, w, b, aux, count, mask, scale, torch.float64, False)
        cnt = torch.tensor([float(X.shape[0] if mask is None else int(mask.sum()))], dtype=torch.float64)
        f = lambda t: None if t is None else t.to(X.dtype)     # noqa: E731
        return f(out["s"]), f(out["gw"]), f(out["gb"]), f(out["gaux"]), cnt
    return fn


@pytest.mark.parametrize("name", cases.GOLDEN_MODELS)
def test_restatement_and_materialised_route_agree_with_the_reference_fixture(golden, name):
    import pyro_amd as pyro
    import pyro_amd.distributions as dist
    from pyro_amd import poutine
    g, family, X, y, mask, count, lat = _fixture_inputs(golden, name)
    scale = float(g["plate_size"]) / X.shape[0]
    # the float64 restatement
    aux = [lat[k][:, 0] for k in cases.AUX_NAMES[family]]
    out = cases.torch_route(family, X, y, lat["w"][:, 0], lat["b"][:, 0], torch.stack(aux, -1) if aux else None, count,
                            mask, scale, torch.float64, True)
    _close(out["s"], g["ll"], 1e-12, "restatement ll")
    _close(out["gw"], g["grad_w"][:, 0], 1e-12, "restatement grad w")
    _close(out["gb"], g["grad_b"][:, 0], 1e-12, "restatement grad b")
    for k, a in enumerate(cases.AUX_NAMES[family]):
        _close(out["gaux"][:, k], g["grad_" + a][:, 0], 1e-12, "restatement grad " + a)
    # the package, float64: nothing is deferred in that dtype, the site is the ordinary class over [P, N] tensors
    leaves = {k: v.clone().requires_grad_(True) for k, v in lat.items()}
    model = cases.make_model(pyro, dist, poutine, name)
    tr = poutine.trace(poutine.condition(model, data=leaves)).get_trace(X, y, mask, int(g["plate_size"]), count)
    assert not isinstance(tr.nodes["obs"]["fn"], dist.families._LinearPredictor)
    tr.compute_log_prob()
    ll = tr.nodes["obs"]["log_prob"].sum(-1)
    _close(ll.detach(), g["ll"], 1e-12, "package ll")
    grads = torch.autograd.grad(ll.sum(), list(leaves.values()))
    for k, gr in zip(leaves, grads):
        _close(gr, g["grad_" + k], 1e-12, "package grad " + k)


def test_magnitude_pieces_add_up_to_the_derivatives():
    """The addends behind the float32 floor (cases.magnitudes) are the addends of the restatement: their sums of
    absolute values bound the entries."""
    for family in cases.FAMILIES:
        a = cases.make_inputs(family, 64, 5, 3, True, True, 7)
        for full in (False, True):
            ref = cases.torch_route(family, a["X"], a["y"], a["w"], a["b"], a["aux"], a["count"], a["mask"], 2.0,
                                    torch.float64, full)
            A = cases.magnitudes(family, a["X"], a["y"], a["w"], a["b"], a["aux"], a["count"], a["mask"], 2.0, full)
            for k in ref:
                if ref[k] is not None:
                    assert bool((ref[k].abs() <= A[k] * (1 + 1e-12) + 1e-300).all()), (family, full, k)


def test_case_table_covers_every_size_and_path():
    table = cases.kernel_cases()
    assert 35 <= len(table) <= 50 and len(set(table)) == len(table)
    assert {c[0] for c in table} == {1, 31, 32, 33, 127, 128, 129, 300, 1100}
    assert {c[1] for c in table} >= {1, 3, 4, 31, 32, 33, 64, 127, 128}
    assert {c[2] for c in table} >= {1, 31, 32, 33, 64, 65}
    assert {c[3] for c in table} == {True, False} and {c[4] for c in table} == {True, False}
    assert {c[5] for c in table} == {1.0, 3.5}
    assert {(c[0], c[6]) for c in table if c[6]} == {(300, 1), (1100, 2)}
    for vec4 in (True, False):                # both staging forms at one, two and four feature tiles
        assert {(c[1] + 31) // 32 for c in table if (c[1] % 4 == 0) == vec4} >= {1, 2, 4}


# ---- recognition ------------------------------------------------------------------------------------------------------
N, D, P = 300, 5, 3


def _operands(seed=0, dtype=torch.float32):
    from pyro_amd.ops import lazy
    gen = torch.Generator().manual_seed(seed)
    X = torch.randn((N, D), generator=gen, dtype=dtype)
    w3 = 0.3 * torch.randn((P, 1, D), generator=gen, dtype=dtype)
    w1 = 0.3 * torch.randn((D,), generator=gen, dtype=dtype)
    b = 0.3 * torch.randn((P, 1), generator=gen, dtype=dtype)
    sigma = 0.5 + torch.rand((P, 1), generator=gen, dtype=dtype)
    nu = 2.0 + 5.0 * torch.rand((P, 1), generator=gen, dtype=dtype)
    n = torch.randint(1, 21, (N,), generator=gen).to(dtype)
    yc = torch.floor(n * torch.rand((N,), generator=gen, dtype=dtype))
    yr = torch.randn((N,), generator=gen, dtype=dtype)
    L = lazy.as_latent
    return dict(X=X, w3=w3, w1=w1, b=b, sigma=sigma, nu=nu, n=n, yc=yc, yr=yr,
                Lw3=L(w3), Lw1=L(w1), Lb=L(b), Lsigma=L(sigma), Lnu=L(nu))


def _plain_eta(o, form):
    return (o["w3"] @ o["X"].t()).squeeze(-2) + o["b"] if form == "wXt" else o["X"] @ o["w1"] + 0.25


def _lazy_eta(o, form):
    return (o["Lw3"] @ o["X"].t()).squeeze(-2) + o["Lb"] if form == "wXt" else o["X"] @ o["Lw1"] + 0.25


@pytest.mark.parametrize("form", ["wXt", "Xw"])
def test_each_spelling_yields_the_fused_site(form, monkeypatch):
    import pyro_amd.distributions as dist
    from pyro_amd import _lib, kernels
    from pyro_amd.distributions import families
    from pyro_amd.ops import lazy
    o = _operands()
    sg, nu = (o["Lsigma"], o["Lnu"]) if form == "wXt" else (1.5, 4.0)
    psg, pnu = (o["sigma"], o["nu"]) if form == "wXt" else (1.5, 4.0)
    eta = _plain_eta(o, form)
    d = lambda: _lazy_eta(o, form)       # noqa: E731
    assert isinstance(d(), lazy.DeferredMatmul) and d().link is None
    assert isinstance(d().exp(), lazy.DeferredMatmul) and d().exp().link == "exp"
    assert isinstance(torch.exp(d()), lazy.DeferredMatmul) and torch.exp(d()).link == "exp"
    sites = [
        (_lib.GLM_NORMAL, dist.Normal(d(), sg), dist.Normal(eta, psg), o["yr"]),
        (_lib.GLM_NORMAL, dist.Normal(loc=d(), scale=sg), dist.Normal(eta, psg), o["yr"]),
        (_lib.GLM_STUDENT_T, dist.StudentT(nu, d(), sg), dist.StudentT(pnu, eta, psg), o["yr"]),
        (_lib.GLM_STUDENT_T, dist.StudentT(df=nu, loc=d(), scale=sg), dist.StudentT(pnu, eta, psg), o["yr"]),
        (_lib.GLM_POISSON_LOG, dist.Poisson(torch.exp(d())), dist.Poisson(eta.exp()), o["yc"]),
        (_lib.GLM_POISSON_LOG, dist.Poisson(rate=d().exp()), dist.Poisson(eta.exp()), o["yc"]),
        (_lib.GLM_BINOMIAL_LOGITS, dist.Binomial(o["n"], logits=d()), dist.Binomial(o["n"], logits=eta), o["yc"]),
        (_lib.GLM_BINOMIAL_LOGITS, dist.Binomial(total_count=20, logits=d()), dist.Binomial(20, logits=eta),
         o["yc"]),
        (_lib.GLM_BINOMIAL_LOGITS, dist.Binomial(torch.tensor(20), None, d()), dist.Binomial(20, logits=eta),
         o["yc"]),
    ]
    calls = []
    monkeypatch.setattr(kernels, "glm_family_fwd_bwd", _kernel_standin(calls))
    mask = torch.arange(N) % 5 != 0
    for family, site, plain, y in sites:
        assert isinstance(site, families._LinearPredictor) and site.family == family, (family, type(site))
        assert site.batch_shape == plain.batch_shape and site.event_shape == ()
        assert type(site.support) is type(plain.support)
        assert set(site.arg_constraints) == set(plain.arg_constraints)
        torch.testing.assert_close(site.log_prob(y), plain.log_prob(y), rtol=1e-5, atol=1e-5)
        n0 = len(calls)
        ll = site.fused_log_prob_batch(y, 2.5, mask)
        assert len(calls) == n0 + 1 and calls[-1] == family
        want = (plain.log_prob(y) * mask).sum(-1) * 2.5
        assert ll.shape == plain.batch_shape[:-1]
        torch.testing.assert_close(ll, want, rtol=2e-5, atol=1e-3)
        assert site.expand(site.batch_shape) is site
        assert not isinstance(site.expand((2,) + tuple(site.batch_shape)), families._LinearPredictor)
        draw = site.sample()
        assert draw.shape == plain.batch_shape and bool(site.support.check(draw).all())


def test_fused_site_chains_gradients_to_every_latent(monkeypatch):
    """The site's autograd Function: gradients of w, b, sigma and nu from the kernel's outputs plus the closed-form
    normaliser equal autograd through the materialised site (float64 stand-in behind float32 tensors)."""
    import pyro_amd.distributions as dist
    from pyro_amd import kernels
    from pyro_amd.ops import lazy
    monkeypatch.setattr(kernels, "glm_family_fwd_bwd", _kernel_standin())
    o = _operands(3)
    leaves = {k: o[k].clone().requires_grad_(True) for k in ("w3", "b", "sigma", "nu")}
    lat = {k: lazy.as_latent(v) for k, v in leaves.items()}
    mask = torch.arange(N) % 4 != 1
    site = dist.StudentT(lat["nu"], (lat["w3"] @ o["X"].t()).squeeze(-2) + lat["b"], lat["sigma"])
    got = torch.autograd.grad(site.fused_log_prob_batch(o["yr"], 3.0, mask).sum(), list(leaves.values()))
    plain = {k: o[k].double().requires_grad_(True) for k in leaves}
    eta = (plain["w3"] @ o["X"].double().t()).squeeze(-2) + plain["b"]
    lp = torch.distributions.StudentT(plain["nu"], eta, plain["sigma"]).log_prob(o["yr"].double())
    want = torch.autograd.grad((lp * mask).sum() * 3.0, list(plain.values()))
    for k, a, b in zip(leaves, got, want):
        assert a.shape == leaves[k].shape
        torch.testing.assert_close(a.double(), b, rtol=1e-5, atol=1e-4, msg=k)


def test_each_fallback_yields_the_ordinary_class_with_the_plain_values(monkeypatch):
    import pyro_amd.distributions as dist
    from pyro_amd import kernels
    from pyro_amd.distributions import families
    from pyro_amd.ops import lazy
    calls = []
    monkeypatch.setattr(kernels, "glm_family_fwd_bwd", _kernel_standin(calls))
    o = _operands(1)
    eta = _plain_eta(o, "wXt")
    d = lambda: _lazy_eta(o, "wXt")       # noqa: E731
    row_sigma = 0.5 + torch.rand(N)
    wide_sigma = 0.5 + torch.rand(P, N)
    cases_ = [
        ("per-row sigma", lambda: dist.Normal(d(), row_sigma), dist.Normal(eta, row_sigma), o["yr"]),
        ("aux with a data dim", lambda: dist.Normal(d(), wide_sigma), dist.Normal(eta, wide_sigma), o["yr"]),
        ("per-row nu", lambda: dist.StudentT(2.0 + row_sigma, d(), 1.0), dist.StudentT(2.0 + row_sigma, eta, 1.0),
         o["yr"]),
        ("probs=", lambda: dist.Binomial(o["n"], probs=torch.sigmoid(d())),
         dist.Binomial(o["n"], probs=torch.sigmoid(eta)), o["yc"]),
        ("identity-link rate", lambda: dist.Poisson(d() * d()), dist.Poisson(eta * eta), o["yc"]),
        ("exp-link loc", lambda: dist.Normal(torch.exp(d()), 1.0), dist.Normal(eta.exp(), 1.0), o["yr"]),
        ("exp-link logits", lambda: dist.Binomial(o["n"], logits=d().exp()), dist.Binomial(o["n"], logits=eta.exp()),
         o["yc"]),
        ("count that is a latent", lambda: dist.Binomial(o["n"].clone().requires_grad_(True), logits=d()),
         dist.Binomial(o["n"], logits=eta), o["yc"]),
    ]
    for what, make, plain, y in cases_:
        site = make()
        assert type(site) is type(plain) and not isinstance(site, families._LinearPredictor), what
        torch.testing.assert_close(site.log_prob(y), plain.log_prob(y), msg=what)
    # the switch: every constructor is the ordinary one
    monkeypatch.setattr(families, "FUSED_GLM_FAMILIES", False)
    for site, plain, y in ((dist.Normal(d(), o["Lsigma"]), dist.Normal(eta, o["sigma"]), o["yr"]),
                           (dist.StudentT(o["Lnu"], d(), o["Lsigma"]), dist.StudentT(o["nu"], eta, o["sigma"]), o["yr"]),
                           (dist.Poisson(torch.exp(d())), dist.Poisson(eta.exp()), o["yc"]),
                           (dist.Binomial(o["n"], logits=d()), dist.Binomial(o["n"], logits=eta), o["yc"])):
        assert type(site) is type(plain)
        torch.testing.assert_close(site.log_prob(y), plain.log_prob(y))
    monkeypatch.setattr(families, "FUSED_GLM_FAMILIES", True)
    # layouts the recognition never defers: float64, CPU, D > 128, a non-contiguous X
    o64 = _operands(1, torch.float64)
    assert type((o64["Lw3"] @ o64["X"].t())) is torch.Tensor
    wide = torch.randn(N, 130)
    assert type(lazy.as_latent(torch.randn(P, 1, 130)) @ wide.t()) is torch.Tensor
    strided = torch.randn(N, 2 * D)[:, ::2]
    assert type(o["Lw3"] @ strided.t()) is torch.Tensor
    monkeypatch.setattr(lazy, "_on_device", lambda t: t.is_cuda)
    assert type(lazy.as_latent(o["w3"]) @ o["X"].t()) is torch.Tensor
    monkeypatch.setattr(lazy, "_on_device", lambda t: True)
    # what only the scoring call knows: a tensor scale, a mask that is not [N], float64 behind a widened predicate
    site = dist.Normal(d(), o["Lsigma"])
    assert isinstance(site, families._LinearPredictor)
    assert site.fused_log_prob_batch(o["yr"], torch.tensor(2.0), None) is None
    assert site.fused_log_prob_batch(o["yr"], 2.0, torch.ones(P, N, dtype=torch.bool)) is None
    assert site.fused_log_prob_batch(o["yr"].expand(P, N), 2.0, None) is None
    monkeypatch.setattr(lazy, "_DTYPES", (torch.float32, torch.float64))
    o64 = _operands(1, torch.float64)
    site64 = dist.Normal((o64["Lw3"] @ o64["X"].t()).squeeze(-2) + o64["Lb"], o64["Lsigma"])
    assert isinstance(site64, families._LinearPredictor)
    assert site64.fused_log_prob_batch(o64["yr"], 2.0, None) is None and not calls
    torch.testing.assert_close(site64.log_prob(o64["yr"]),
                               torch.distributions.Normal(_plain_eta(o64, "wXt"), o64["sigma"]).log_prob(o64["yr"]))


def test_a_linked_product_used_any_other_way_is_what_plain_tensors_give():
    import pyro_amd.distributions as dist
    from pyro_amd.distributions import families
    from pyro_amd.ops import lazy
    o = _operands(2)
    ref = torch.exp(_plain_eta(o, "wXt"))
    e = lambda: torch.exp(_lazy_eta(o, "wXt"))       # noqa: E731
    assert isinstance(e(), lazy.DeferredMatmul) and e().shape == ref.shape
    assert e().as_linear_logits() is None and e().as_linear_predictor()[1] == "exp"
    bern = dist.Bernoulli(logits=e())
    assert type(bern) is dist.Bernoulli and not isinstance(bern, families._BernoulliLinear)
    torch.testing.assert_close(bern.logits, ref)
    for got, want in ((e() + 1.0, ref + 1.0), (1.0 + e(), 1.0 + ref), (e() * 2, ref * 2), (e()[1], ref[1]),
                      (e()[:, 3:7], ref[:, 3:7]), (e().exp(), ref.exp()), (torch.exp(e()), ref.exp()),
                      (e() + o["Lb"], ref + o["b"]), (e().squeeze(-1), ref.squeeze(-1)), (torch.log(e()), ref.log()),
                      (e().sum(-1), ref.sum(-1)), (-e(), -ref)):
        assert type(got) is torch.Tensor
        torch.testing.assert_close(got, want)
    # the unlinked product is still the Bernoulli site's, and a link leaves the original object alone
    d = _lazy_eta(o, "wXt")
    d.exp()
    assert d.link is None and isinstance(dist.Bernoulli(logits=d), families._BernoulliLinear)
    # an un-squeezed product may carry the link, but is no regression site
    raw = torch.exp(o["Lw3"] @ o["X"].t())
    assert isinstance(raw, lazy.DeferredMatmul) and raw.as_linear_predictor() is None
    assert type(dist.Poisson(raw)) is dist.Poisson
    torch.testing.assert_close(dist.Poisson(raw).rate, torch.exp(o["w3"] @ o["X"].t()))


def test_the_direct_nuts_recogniser_cannot_take_the_new_site_for_the_bernoulli_one():
    """infer/mcmc/direct.py finds the Bernoulli GLM site by its ``lazy`` attribute and class name: the new class has
    neither."""
    import inspect

    import pyro_amd.distributions as dist
    from pyro_amd.distributions import families
    from pyro_amd.infer.mcmc import direct
    o = _operands(4)
    site = dist.Poisson(torch.exp(_lazy_eta(o, "wXt")))
    assert isinstance(site, families._LinearPredictor) and not hasattr(site, "lazy")
    assert type(site.predictor).__name__ == "LinearLogits"
    assert hasattr(dist.Bernoulli(logits=_lazy_eta(o, "wXt")), "lazy")
    assert '"_BernoulliLinear"' in inspect.getsource(direct)


def test_student_t_is_still_torchs_class():
    import pyro_amd.distributions as dist
    from pyro_amd.contrib.forecast import util as fc_util
    from pyro_amd.distributions.base import TorchDistributionMixin
    assert issubclass(dist.StudentT, torch.distributions.StudentT) and issubclass(dist.StudentT, TorchDistributionMixin)
    st = dist.StudentT(torch.tensor(3.0), torch.zeros(4), torch.ones(4))
    assert type(st) is dist.StudentT and isinstance(st, torch.distributions.StudentT)
    assert type(st.expand((2, 4))) is dist.StudentT and st.expand((2, 4)).batch_shape == (2, 4)
    assert st.to_event(1).event_shape == (4,)
    assert any(k is dist.StudentT for k in vars(fc_util).values() if isinstance(k, type)) or \
        any(dist.StudentT in v for v in vars(fc_util).values() if isinstance(v, dict))
    for cls in (dist.Normal, dist.Poisson, dist.Binomial, dist.StudentT):     # torch's expand builds by __new__()
        assert isinstance(cls.__new__(cls), cls)


@pytest.mark.parametrize("name", cases.GOLDEN_MODELS)
@pytest.mark.parametrize("particles", [1, 3])
def test_one_kernel_call_per_step_and_the_fixture_values(golden, name, particles, monkeypatch):
    """Trace_ELBO.loss_and_grads on the fixture models in float32 with the kernel answered by the float64 restatement:
    exactly one call per step, loss and gradients those of the fixture to float32 input rounding; none with the
    switch off."""
    import pyro_amd as pyro
    import pyro_amd.distributions as dist
    from pyro_amd import kernels, poutine
    from pyro_amd.distributions import families
    g, family, X, y, mask, count, lat = _fixture_inputs(golden, name, torch.float32)
    if particles == 1:
        lat = {k: v[0, 0] for k, v in lat.items()}
    model = cases.make_model(pyro, dist, poutine, name)
    # the reference values AT the float32-rounded inputs (the fixture's own to 1e-6 of the sums)
    P = particles
    flat = {k: v.reshape(P, -1) for k, v in lat.items()}
    aux = [flat[k][:, 0] for k in cases.AUX_NAMES[family]]
    scale = float(g["plate_size"]) / X.shape[0]
    ref, bound = cases.bounds(family, X, y, flat["w"], flat["b"][:, 0], torch.stack(aux, -1) if aux else None, count,
                              mask, scale, True)
    if particles == 3:
        _close(ref["s"], g["ll"], 2e-6, "float32-rounded inputs")
    for fused in (True, False):
        calls = []
        monkeypatch.setattr(kernels, "glm_family_fwd_bwd", _kernel_standin(calls))
        monkeypatch.setattr(families, "FUSED_GLM_FAMILIES", fused)
        pyro.clear_param_store()
        guide = cases.make_guide(pyro, dist, lat)
        elbo = pyro.infer.Trace_ELBO(num_particles=P, vectorize_particles=P > 1, max_plate_nesting=1)
        loss = elbo.loss_and_grads(model, guide, X, y, mask, int(g["plate_size"]), count)
        assert len(calls) == (1 if fused else 0), (name, fused, calls)
        grads = {k: v.grad for k, v in pyro.get_param_store().named_parameters()}
        cases.assert_step_within(loss, grads, ref, bound, family, P)
