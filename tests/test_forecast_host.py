"""contrib.forecast on the CPU in float64 against tests/golden/forecast.npz (the unmodified reference running the same
model text, tests/forecast_cases.py).

The element-wise families and the ELBO's assembly are answered by the numpy oracle (``cpu_backend``, as in
tests/test_linear_hmm_host.py); the state-space classes take their torch routes.

(a) fixed latents: the log_prob of every site and the trace's log_prob_sum at 1e-12 relative, without a particle plate
    and with one of 5 at max_plate_nesting 1 and 2, for every noise model of fc.NOISES.
(b) the training trajectory: 40 steps of AutoDelta + ClippedAdam.  The first loss at 1e-12 relative; every later loss
    and the final parameters within ten times the deviation the REFERENCE shows against itself when the data are
    perturbed by 1e-13 relative (where that deviation happens to vanish, the largest of the same array).
(c) reshape_batch and prefix_condition over every registered type.
(d) the forecast: shapes, batching, and the splice of prefix and prior shown with noise of scale 1e-9.
(e) the scores and the backtest's records.   (f) the refused options."""
import numpy as np
import pytest
import torch

import pyro_amd as pyro
import pyro_amd.distributions as dist
from pyro_amd import optim
from pyro_amd.contrib.forecast import (Forecaster, ForecastingModel, backtest, eval_crps, eval_mae, eval_rmse)
from pyro_amd.contrib.forecast import util
from pyro_amd.distributions import hmm
from pyro_amd.infer.autoguide import AutoDelta, init_to_value
from pyro_amd.ops import stats
from tests import forecast_cases as fc

F64 = torch.float64
RTOL = 1e-12


def _allowed(want, perturbed):
    """The trajectory's bound, entry by entry: ten times the deviation the reference shows against itself under the
    1e-13 perturbation.  Where that deviation happens to round to zero in an entry, the largest deviation of the same
    array stands in, unscaled: the entries of one tensor come out of the same perturbed arithmetic, and rounding in a
    40-step trajectory scales with the tensor, not with an entry that happens to lie near zero."""
    own = np.abs(want - perturbed)
    return np.maximum(10 * own, own.max())
T = torch.distributions.transforms


@pytest.fixture
def cpu_backend(oracle_backend, monkeypatch):
    """The numpy oracle for the element-wise families, which declares every tensor to be on the device: the kernels it
    does not answer are switched off."""
    monkeypatch.setattr(hmm, "FUSED_GAUSSIAN_HMM", False)
    monkeypatch.setattr(hmm, "FUSED_LINEAR_HMM", False)
    monkeypatch.setattr(stats, "FUSED_FORECAST_SCORES", False)
    torch.set_default_dtype(F64)
    yield
    torch.set_default_dtype(torch.float32)


@pytest.fixture(scope="module")
def inputs():
    return fc.tensors(fc.golden("inputs"))


def _close(got, want, rtol=RTOL):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want)
    assert got.shape == want.shape, (got.shape, want.shape)
    np.testing.assert_allclose(got, want, rtol=rtol, atol=0)


# ---- (a) ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("config,particles,nesting", fc.CONFIGS, ids=[c[0] for c in fc.CONFIGS])
@pytest.mark.parametrize("noise", fc.NOISES)
def test_fixed_latents(noise, config, particles, nesting, inputs, cpu_backend):
    g = fc.golden("fixed/%s/%s" % (noise, config))
    aux = {k[len("value_"):]: torch.tensor(v) for k, v in g.items() if k.startswith("value_")}
    tr = fc.run_fixed(fc.namespace(), noise, inputs, particles, nesting, aux)
    sites = fc.sample_sites(tr)
    assert sites == [str(s) for s in g["sites"]]
    for s in sites:
        _close(tr.nodes[s]["log_prob"].detach().numpy(), g["log_prob_" + s])
    _close(float(tr.log_prob_sum()), g["log_prob_sum"])
    assert tr.nodes["residual"]["is_observed"]


# ---- (b) ---------------------------------------------------------------------------------------------------------
def _train(inputs, **kwargs):
    pyro.clear_param_store()
    model, _ = fc.make_model(fc.namespace(), "hmm", inputs)
    init = {k: v.clone() for k, v in fc.latent_values(inputs, None, 1).items()}
    guide = AutoDelta(model, init_loc_fn=init_to_value(values=init))
    return Forecaster(model, inputs["data"], inputs["covariates"][:fc.T_OBS], guide=guide,
                      optim=optim.ClippedAdam(dict(fc.OPTIM)), num_steps=fc.NUM_STEPS, log_every=0, **kwargs)


def test_training_trajectory(inputs, cpu_backend):
    g = fc.golden("train")
    forecaster = _train(inputs)
    losses = np.array(forecaster.losses)
    assert losses.shape == (fc.NUM_STEPS,)
    _close(losses[0], g["losses"][0])
    allowed = _allowed(g["losses"], g["losses_perturbed"])
    dev = np.abs(losses - g["losses"])
    print("losses: largest deviation %.2e, allowed there %.2e; the reference against itself %.2e"
          % (dev.max(), allowed[dev.argmax()], np.abs(g["losses"] - g["losses_perturbed"]).max()))
    assert (dev <= allowed).all(), (dev, allowed)
    store = pyro.get_param_store()
    names = [k[len("param_"):] for k in g if k.startswith("param_") and not k.startswith("param_perturbed_")]
    assert sorted(names) == sorted(store.keys())
    for name in names:
        want, other = g["param_" + name], g["param_perturbed_" + name]
        got = store[name].detach().numpy()
        assert got.shape == want.shape
        assert (np.abs(got - want) <= _allowed(want, other)).all(), name
    pyro.clear_param_store()


# ---- (c) ---------------------------------------------------------------------------------------------------------
def _elementwise():
    """(distribution of batch (2, 3), a value in its support) for every registered element-wise family; the
    parameters are torch tensors and the families torch's under the package's mixin where the package's own refuse
    host tensors."""
    gen = torch.Generator().manual_seed(5)
    u = lambda *s: 0.5 + torch.rand(*s, generator=gen, dtype=F64)          # noqa: E731
    n = lambda *s: torch.randn(*s, generator=gen, dtype=F64)              # noqa: E731
    x, pos, unit = n(2, 3), u(2, 3), torch.rand(2, 3, generator=gen, dtype=F64) * 0.9 + 0.05
    return {"Normal": (dist.Normal(n(2, 3), u(3)), x), "StudentT": (dist.StudentT(2 + u(2, 1), n(3), u(2, 3)), x),
            "Laplace": (dist.Laplace(n(2, 3), u(2, 3)), x), "Cauchy": (dist.Cauchy(n(1, 3), u(2, 3)), x),
            "LogNormal": (dist.LogNormal(n(2, 3), u(2, 3)), pos), "Gamma": (dist.Gamma(u(2, 3), u(3)), pos),
            "Exponential": (dist.Exponential(u(2, 3)), pos), "Poisson": (dist.Poisson(u(2, 3)), pos.round()),
            "Bernoulli": (dist.Bernoulli(logits=n(2, 3)), (x > 0).to(F64)), "Beta": (dist.Beta(u(2, 3), u(2, 3)), unit),
            "Uniform": (dist.Uniform(n(2, 3) - 3, u(2, 3) + 3), x.clamp(-2, 2))}


def test_registered_types():
    families = tuple(c for c in util.TENSOR_FAMILIES if c is not dist.MultivariateNormal)
    assert set(c.__name__ for c in families) == set(_elementwise())
    assert set(util.ELEMENTWISE_TRANSFORMS) == {T.AffineTransform, T.ExpTransform, T.SigmoidTransform, T.AbsTransform,
                                               T.PowerTransform}
    for cls in (dist.MultivariateNormal, dist.Independent, dist.MaskedDistribution, dist.TransformedDistribution,
                dist.GaussianHMM, dist.LinearHMM, dist.IndependentHMM) + families:
        assert util.reshape_batch.dispatch(cls) is not util.reshape_batch.dispatch(object), cls
    for cls in (dist.MultivariateNormal, dist.Independent, dist.MaskedDistribution, dist.TransformedDistribution,
                dist.IndependentHMM) + families:
        assert util.prefix_condition.dispatch(cls) is not util.prefix_condition.dispatch(object), cls
    with pytest.raises(NotImplementedError):
        util.reshape_batch(dist.Dirichlet(torch.ones(3)), (1,))
    with pytest.raises(NotImplementedError):
        util.prefix_condition(dist.Dirichlet(torch.ones(2, 3)), torch.zeros(1, 3))
    with pytest.raises(NotImplementedError):
        util.reshape_transform_batch(T.TanhTransform(), (2, 3), (6,))


@pytest.mark.parametrize("name", sorted(["Normal", "StudentT", "Laplace", "Cauchy", "LogNormal", "Gamma", "Exponential",
                                         "Poisson", "Bernoulli", "Beta", "Uniform"]))
def test_reshape_and_prefix_elementwise(name, cpu_backend):
    d, x = _elementwise()[name]
    want = d.log_prob(x)
    for new in fc.RESHAPES:
        r = util.reshape_batch(d, new)
        assert type(r) is type(d) and r.batch_shape == new
        assert torch.equal(r.log_prob(x.reshape(new)), want.reshape(new))
    # time is dim -2: the conditional distribution of an element-wise family is its parameter slice
    c = util.prefix_condition(d, x[:1])
    assert type(c) is type(d) and c.batch_shape == (1, 3)
    assert torch.equal(c.log_prob(x[1:]), want[1:])
    # the wrappers
    for wrapped, value in ((d.to_event(1), x), (d.mask(x > 0), x),):
        w = wrapped.log_prob(value)
        lead = wrapped.batch_shape
        for new in ((6,), (3, 2)) if len(lead) == 2 else ((1, 2), (2, 1)):
            r = util.reshape_batch(wrapped, new)
            assert torch.equal(r.log_prob(value.reshape(new + tuple(value.shape[len(lead):]))), w.reshape(new))
    masked = util.prefix_condition(d.mask(x > 0), x[:1])
    assert torch.equal(masked.log_prob(x[1:]), d.mask(x > 0).log_prob(x)[1:])
    ind = util.prefix_condition(d.to_event(2), x[:1])
    assert ind.event_shape == (1, 3) and torch.equal(ind.log_prob(x[1:]), want[1:].sum())


def test_reshape_and_prefix_transformed_and_mvn(cpu_backend):
    gen = torch.Generator().manual_seed(6)
    loc, scale = torch.randn(2, 3, generator=gen, dtype=F64), 0.5 + torch.rand(2, 3, generator=gen, dtype=F64)
    base = dist.Normal(loc, scale)
    x = torch.randn(2, 3, generator=gen, dtype=F64)
    # (transforms, a value in the support, whether the transforms' parameters are independent of time)
    for transforms, value, homogeneous in (([T.AffineTransform(loc, scale)], x, False),
                                           ([T.ExpTransform()], x.exp(), True),
                                           ([T.SigmoidTransform()], x.sigmoid(), True),
                                           ([T.AbsTransform()], x.abs(), True),
                                           ([T.ExpTransform(), T.PowerTransform(scale)], x.exp() ** scale, False),
                                           ([T.AffineTransform(0.3, 2.0), T.ExpTransform()], x.exp(), True)):
        d = dist.TransformedDistribution(base, transforms)
        if not isinstance(transforms[0], T.AbsTransform):
            want = d.log_prob(value)
            for new in fc.RESHAPES:
                r = util.reshape_batch(d, new)
                assert r.batch_shape == new and torch.equal(r.log_prob(value.reshape(new)), want.reshape(new))
            if homogeneous:        # (prefix_condition keeps the transforms as they are, like the reference's)
                c = util.prefix_condition(d, value[:1])
                assert torch.equal(c.log_prob(value[1:]), want[1:])
        else:                      # (not invertible: no log_prob; the draws' shape tells)
            assert util.reshape_batch(d, (6,)).rsample().shape == (6,)
    tril = torch.randn(2, 3, 3, generator=gen, dtype=F64).tril(-1) + torch.diag_embed(scale)
    mvn = dist.MultivariateNormal(loc, scale_tril=tril)
    for new in ((2, 1), (1, 2), (1, 2, 1)):
        assert torch.equal(util.reshape_batch(mvn, new).log_prob(x.reshape(new + (3,))), mvn.log_prob(x).reshape(new))
    c = util.prefix_condition(mvn, x[:1])
    assert torch.equal(c.log_prob(x[1:]), mvn.log_prob(x)[1:])


@pytest.mark.parametrize("name,independent", (("gaussian_hmm", False), ("independent_hmm", True)))
def test_reshape_hmm(name, independent, cpu_backend):
    g = fc.golden("reshape/" + name)
    p = fc.tensors({k: v for k, v in g.items() if not k.startswith("log_prob")})
    d = fc.build_hmm(dist, p, independent)
    x = p["x"].squeeze(-1).transpose(-1, -2) if independent else p["x"]
    batch = tuple(d.batch_shape)
    want = d.log_prob(x)
    _close(want.numpy(), g["log_prob"])
    news = fc.RESHAPES if not independent else ((2, 1), (1, 2), (1, 2, 1))
    for new in news:
        r = util.reshape_batch(d, new)
        assert type(r) is type(d) and r.batch_shape == new and r.event_shape == d.event_shape
        lp = r.log_prob(x.reshape(new + tuple(x.shape[len(batch):])))
        assert torch.equal(lp, want.reshape(new)), new
        _close(lp.numpy(), g["log_prob_" + "x".join(map(str, new))])


def test_reshape_gaussian_hmm_keeps_shared_parameters_shared():
    h, o, steps = 3, 2, 7
    normal = lambda loc, scale: dist.Independent(torch.distributions.Normal(loc, scale), 1)     # noqa: E731
    F, H = 0.5 * torch.eye(h, dtype=F64), torch.ones(h, o, dtype=F64)
    scale = 0.5 + torch.rand(5, 1, h, dtype=F64)                      # per series, time-homogeneous
    d = dist.GaussianHMM(normal(torch.zeros(h, dtype=F64), 1.0), F, normal(torch.zeros(h, dtype=F64), scale), H,
                         normal(torch.zeros(o, dtype=F64), torch.ones(o, dtype=F64)), duration=steps)
    assert d.batch_shape == (5,)
    for new in ((5, 1), (1, 5, 1), (5,)):
        r = util.reshape_batch(d, new)
        assert r.batch_shape == new and r.duration == steps
        for before, after in zip(d._parts, r._parts):
            assert after.data_ptr() == before.data_ptr() and after.numel() == before.numel()
        m0, P0, F_, q, Q, H_, r_, R = r._parts
        # shared by all series and time-homogeneous: still one matrix
        assert all(n == 1 for n in F_.shape[:-2]) and all(n == 1 for n in H_.shape[:-2])
        assert all(n == 1 for n in R.shape[:-2]) and Q.shape[-3] == 1
    # what the Kalman kernel is handed: one copy of everything but the per-series transition covariance -- also of
    # the transition location, which broadcasting against the scale left as a stride-0 view of batch shape (5, 1)
    q = util.reshape_batch(d, (5, 1))._parts[3]
    assert q.shape == (5, 1, 1, h) and q.stride(0) == 0
    handed = util.reshape_batch(d, (5, 1))._kernel_parts((5, 1))
    assert [p.shape[0] for p in handed] == [1, 1, 1, 1, 5, 1, 1, 1]
    x = torch.randn(5, steps, o, dtype=F64)
    assert torch.equal(util.reshape_batch(d, (5, 1)).log_prob(x.unsqueeze(1)), d.log_prob(x).unsqueeze(1))
    # any other reshape expands, as the reference does
    d2 = d.expand((2, 5))
    assert util.reshape_batch(d2, (10,)).batch_shape == (10,)


def test_prefix_condition_hmm_is_the_class_method(cpu_backend):
    g = fc.golden("reshape/gaussian_hmm")
    p = fc.tensors({k: v for k, v in g.items() if not k.startswith("log_prob")})
    d = fc.build_hmm(dist, p)
    x = p["x"]
    a, b = util.prefix_condition(d, x[..., :2, :]), d.prefix_condition(x[..., :2, :])
    assert type(a) is dist.GaussianHMM and a.duration == b.duration == 3
    assert all(torch.equal(u, v) for u, v in zip(a._parts, b._parts))
    pi = fc.tensors({k: v for k, v in fc.golden("reshape/independent_hmm").items() if not k.startswith("log_prob")})
    di = fc.build_hmm(dist, pi, True)
    xi = pi["x"].squeeze(-1).transpose(-1, -2)
    c = util.prefix_condition(di, xi[..., :2, :])
    assert type(c) is dist.IndependentHMM and c.event_shape == (3, 3)
    want = di.base_dist.prefix_condition(pi["x"][..., :2, :])
    assert all(torch.equal(u, v) for u, v in zip(c.base_dist._parts, want._parts))


# ---- (d) ---------------------------------------------------------------------------------------------------------
def test_forecast_shapes(inputs, cpu_backend):
    g = fc.golden("forecast")
    forecaster = _train(inputs)
    data, cov = inputs["data"], inputs["covariates"]
    assert forecaster.max_plate_nesting == 1
    for nesting in (1, 2):
        forecaster.max_plate_nesting = nesting
        out = forecaster(data, cov, num_samples=4)
        assert tuple(out.shape) == tuple(g["shape_nest%d" % nesting])
        assert tuple(out.shape) == (4,) + (1,) * (nesting - 1) + (fc.T_AHEAD, fc.OBS)
    forecaster.max_plate_nesting = 1
    out = forecaster(data, cov, num_samples=20, batch_size=7)
    assert out.shape == (20, fc.T_AHEAD, fc.OBS) and bool(torch.isfinite(out).all())
    assert forecaster(data, cov[:fc.T_OBS], num_samples=3).shape == (0, fc.OBS)         # nothing to forecast
    pyro.clear_param_store()


class _Walk(ForecastingModel):
    """A random walk drawn INSIDE the time plate plus a level: the prediction is a function of time-local noise."""

    def model(self, zero_data, covariates):
        level = pyro.sample("level", dist.Normal(zero_data[..., :1, :], 1.0).to_event(1))
        with self.time_plate:
            jumps = pyro.sample("jumps", dist.Normal(zero_data.new_zeros(fc.OBS), 0.1).to_event(1))
        self.seen = {"level": level, "jumps": jumps}                    # (what the sample statements returned)
        self.predict(dist.Normal(zero_data, 1e-9), level + jumps.cumsum(-2))


def test_forecast_splices_prefix_and_prior(inputs, cpu_backend):
    pyro.clear_param_store()
    pyro.set_rng_seed(11)
    data, cov = inputs["data"], inputs["covariates"]
    model = _Walk()
    init = {"level": data[:1].clone(), "jumps": torch.cat([torch.zeros(1, fc.OBS), data[1:] - data[:-1]])}
    guide = AutoDelta(model, init_loc_fn=init_to_value(values=init))
    forecaster = Forecaster(model, data, cov[:fc.T_OBS], guide=guide, num_steps=0)
    out = forecaster(data, cov, num_samples=3)
    level, jumps = model.seen["level"], model.seen["jumps"]
    assert jumps.shape == (3, fc.T_OBS + fc.T_AHEAD, fc.OBS)
    # the prefix is the guide's (the same for every sample), the rest the prior's draws (different)
    with torch.no_grad():
        guide_jumps = guide(data, cov[:fc.T_OBS])["jumps"]
    assert torch.equal(jumps[:, :fc.T_OBS], guide_jumps.expand(3, -1, -1))
    assert not torch.equal(jumps[0, fc.T_OBS:], jumps[1, fc.T_OBS:])
    assert level.shape == (3, 1, fc.OBS) and torch.equal(level, data[:1].expand(3, -1, -1))
    right_pred = (level + jumps.cumsum(-2))[..., fc.T_OBS:, :]
    assert out.shape == right_pred.shape and float((out - right_pred).abs().max()) <= 1e-8
    pyro.clear_param_store()


# ---- (e) ---------------------------------------------------------------------------------------------------------
def test_scores_against_the_reference():
    g = fc.golden("eval")
    pred, truth = torch.tensor(g["pred"]), torch.tensor(g["truth"])
    _close(eval_mae(pred, truth), g["mae"])
    _close(eval_rmse(pred, truth), g["rmse"])
    _close(eval_crps(pred, truth), g["crps"])
    assert all(isinstance(f(pred, truth), float) for f in (eval_mae, eval_rmse, eval_crps))
    # point estimates of other shapes broadcast as the reference's do; the crps keeps its shape rule
    assert isinstance(eval_mae(pred[:, :, :1], truth), float)
    with pytest.raises(ValueError):
        eval_crps(pred[:, :, :1], truth)


def test_backtest_records(inputs, monkeypatch):
    g = fc.golden("eval")
    calls = []
    real = stats.forecast_scores
    monkeypatch.setattr(stats, "forecast_scores", lambda *a: calls.append(a) or real(*a))
    data, cov = inputs["data"][:12], inputs["covariates"][:12]
    records = backtest(data, cov, lambda: None, forecaster_fn=fc.StubForecaster, min_train_window=8, test_window=2,
                       num_samples=10)
    assert len(records) == 3 and len(calls) == 3                      # one pass over the samples per window
    assert sorted(records[0]) == [str(k) for k in g["backtest_keys"]]
    assert [[r["t0"], r["t1"], r["t2"]] for r in records] == g["backtest_windows"].tolist()
    assert all(r["seed"] == 1234567890 and r["num_samples"] == 10 and r["params"] == {} for r in records)
    for name in ("mae", "rmse", "crps"):
        _close([r[name] for r in records], g["backtest_" + name])
    # metrics of the caller's own are called as they are; windows by stride and train_window
    records = backtest(data, cov, lambda: None, forecaster_fn=fc.StubForecaster, train_window=6, test_window=3,
                       stride=2, num_samples=4, metrics={"n": lambda pred, truth: pred.shape[0]},
                       transform=lambda pred, truth: (pred * 2, truth * 2))
    assert [(r["t0"], r["t1"], r["t2"], r["n"]) for r in records] == [(0, 6, 9, 4), (2, 8, 11, 4)]
    with pytest.raises(ValueError, match="warm start"):
        backtest(data, cov, lambda: None, forecaster_fn=fc.StubForecaster, train_window=6,
                 forecaster_options={"warm_start": True})


# ---- (f) ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("option", ({"time_reparam": "dct"}, {"time_reparam": "haar"}, {"dct_gradients": True},
                                    {"subsample_aware": True}, {"warm_start": True}))
def test_refused_options(option, inputs):
    model, _ = fc.make_model(fc.namespace(), "hmm", inputs)
    with pytest.raises(NotImplementedError, match=next(iter(option))):
        Forecaster(model, inputs["data"], inputs["covariates"][:fc.T_OBS], num_steps=0, **option)


def test_model_contract(inputs):
    class NoPredict(ForecastingModel):
        def model(self, zero_data, covariates):
            pass

    with pytest.raises(AssertionError, match="predict"):
        NoPredict()(inputs["data"], inputs["covariates"][:fc.T_OBS])
    with pytest.raises(TypeError):
        ForecastingModel()                                             # abstract
    with pytest.raises(AssertionError, match="outside"):
        NoPredict().time_plate
