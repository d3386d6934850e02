"""contrib.forecast on the device: the fixed-latent traces and the training trajectory of tests/test_forecast_host.py
repeated there, and spies that show which kernels a Forecaster reaches.

float64: the fixture's bounds (1e-12 relative on the fixed-latent log-densities; the trajectory within ten times the
reference's own deviation under a 1e-13 perturbation of the data; where that vanishes, the largest of the same array).
float32, fixed latents: the project's rule on gaussian_hmm_cases.rel_err -- the error against the float64 fixture is
at most four times the error of the float32 CPU route (the numpy oracle for the element-wise families, the torch
routes of the state-space classes) on the same float32 inputs, measured when the test runs, with floor 4 * 2^-23.

Routing: one loss evaluation is ONE launch of the Kalman kernel, the parameters the model shares between particles
reach it as one matrix (batch stride 0); a forecast runs the filter and the fused draw; a backtest with the default
metrics scores each window with one launch of the forecast-score kernel."""
import numpy as np
import pytest
import torch

import pyro_amd as pyro
from pyro_amd import kernels, optim
from pyro_amd.contrib.forecast import Forecaster, backtest
from pyro_amd.distributions import hmm
from pyro_amd.infer.autoguide import AutoDelta, init_to_value
from pyro_amd.ops import stats
from tests import forecast_cases as fc
from tests import gaussian_hmm_cases as gc

pytestmark = pytest.mark.gpu
F64, F32 = torch.float64, torch.float32
RTOL = 1e-12


def _allowed(want, perturbed):
    """The trajectory's bound, entry by entry: ten times the deviation the reference shows against itself under the
    1e-13 perturbation.  Where that deviation happens to round to zero in an entry, the largest deviation of the same
    array stands in, unscaled: the entries of one tensor come out of the same perturbed arithmetic, and rounding in a
    40-step trajectory scales with the tensor, not with an entry that happens to lie near zero."""
    own = np.abs(want - perturbed)
    return np.maximum(10 * own, own.max())
FLOOR32 = 4 * 2.0 ** -23
_BASE = {}


@pytest.fixture(autouse=True)
def _default_dtype():
    yield
    torch.set_default_dtype(F32)
    pyro.clear_param_store()


def _inputs(dtype, device):
    return fc.tensors(fc.golden("inputs"), dtype, device)


def _aux(g, dtype, device):
    return {k[len("value_"):]: torch.tensor(v, dtype=dtype, device=device) for k, v in g.items()
            if k.startswith("value_")}


def _spy(monkeypatch, name):
    calls = []
    real = getattr(kernels, name)

    def spy(*a, **kw):
        calls.append((a, kw))
        return real(*a, **kw)
    monkeypatch.setattr(kernels, name, spy)
    return calls


def _cpu_route_errors(noise, config, particles, nesting):
    """rel_err per site of the float32 CPU route against the fixture (once per case): the oracle stands in for the
    element-wise kernels for the length of this call only."""
    key = (noise, config)
    if key not in _BASE:
        from tests import oracle_backend as ob
        g = fc.golden("fixed/%s/%s" % key)
        with pytest.MonkeyPatch.context() as m:
            ob.install(m)
            m.setattr(hmm, "FUSED_GAUSSIAN_HMM", False)
            m.setattr(hmm, "FUSED_LINEAR_HMM", False)
            t = _inputs(F32, "cpu")
            tr = fc.run_fixed(fc.namespace(), noise, t, particles, nesting, _aux(g, F32, "cpu"))
            _BASE[key] = {s: gc.rel_err(tr.nodes[s]["log_prob"].detach().numpy(), g["log_prob_" + s])
                          for s in fc.sample_sites(tr)}
    return _BASE[key]


# ---- (a) ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("config,particles,nesting", fc.CONFIGS, ids=[c[0] for c in fc.CONFIGS])
@pytest.mark.parametrize("noise", fc.NOISES)
def test_fixed_latents_float64(noise, config, particles, nesting, gpu, monkeypatch):
    torch.set_default_dtype(F64)
    calls = _spy(monkeypatch, "gaussian_hmm_fwd_bwd")
    g = fc.golden("fixed/%s/%s" % (noise, config))
    tr = fc.run_fixed(fc.namespace(), noise, _inputs(F64, gpu), particles, nesting, _aux(g, F64, gpu))
    sites = fc.sample_sites(tr)
    assert sites == [str(s) for s in g["sites"]]
    for s in sites:
        got = tr.nodes[s]["log_prob"].detach().cpu().numpy()
        assert got.shape == g["log_prob_" + s].shape
        np.testing.assert_allclose(got, g["log_prob_" + s], rtol=RTOL, atol=0, err_msg=s)
    np.testing.assert_allclose(float(tr.log_prob_sum()), g["log_prob_sum"], rtol=RTOL)
    assert len(calls) == (1 if "hmm" in noise or noise == "student_linear" else 0)


@pytest.mark.parametrize("config,particles,nesting", fc.CONFIGS, ids=[c[0] for c in fc.CONFIGS])
@pytest.mark.parametrize("noise", fc.NOISES)
def test_fixed_latents_float32(noise, config, particles, nesting, gpu):
    base = _cpu_route_errors(noise, config, particles, nesting)
    g = fc.golden("fixed/%s/%s" % (noise, config))
    tr = fc.run_fixed(fc.namespace(), noise, _inputs(F32, gpu), particles, nesting, _aux(g, F32, gpu))
    for s in fc.sample_sites(tr):
        got = tr.nodes[s]["log_prob"].detach().cpu().numpy()
        assert got.dtype == np.float32
        err, bound = gc.rel_err(got, g["log_prob_" + s]), max(4 * base[s], FLOOR32)
        print("%s %s %s: device %.2e, CPU route %.2e" % (noise, config, s, err, base[s]))
        assert err <= bound, (s, err, bound)


# ---- (b) ---------------------------------------------------------------------------------------------------------
def _train(t, **kwargs):
    pyro.clear_param_store()
    model, _ = fc.make_model(fc.namespace(), "hmm", t)
    init = {k: v.clone() for k, v in fc.latent_values(t, None, 1).items()}
    guide = AutoDelta(model, init_loc_fn=init_to_value(values=init))
    kwargs.setdefault("optim", optim.ClippedAdam(dict(fc.OPTIM)))
    kwargs.setdefault("num_steps", fc.NUM_STEPS)
    return Forecaster(model, t["data"], t["covariates"][:fc.T_OBS], guide=guide, log_every=0, **kwargs)


def test_training_trajectory_float64(gpu, monkeypatch):
    torch.set_default_dtype(F64)
    calls = _spy(monkeypatch, "gaussian_hmm_fwd_bwd")
    g = fc.golden("train")
    forecaster = _train(_inputs(F64, gpu))
    losses = np.array(forecaster.losses)
    np.testing.assert_allclose(losses[0], g["losses"][0], rtol=RTOL)
    allowed = _allowed(g["losses"], g["losses_perturbed"])
    dev = np.abs(losses - g["losses"])
    print("losses: largest deviation %.2e, allowed there %.2e" % (dev.max(), allowed[dev.argmax()]))
    assert (dev <= allowed).all(), (dev, allowed)
    store = pyro.get_param_store()
    for key in g:
        if key.startswith("param_") and not key.startswith("param_perturbed_"):
            want, other = g[key], g["param_perturbed_" + key[len("param_"):]]
            got = store[key[len("param_"):]].detach().cpu().numpy()
            assert (np.abs(got - want) <= _allowed(want, other)).all(), key
    assert len(calls) == fc.NUM_STEPS             # every step is an eager one: ONE Kalman launch each


# ---- routing -----------------------------------------------------------------------------------------------------
def test_one_loss_evaluation_is_one_kalman_launch_with_shared_parameters_shared(gpu, monkeypatch):
    calls = _spy(monkeypatch, "gaussian_hmm_fwd_bwd")
    t = _inputs(F32, gpu)
    pyro.clear_param_store()
    pyro.set_rng_seed(3)
    model, _ = fc.make_model(fc.namespace(), "hmm", t)
    Forecaster(model, t["data"], t["covariates"][:fc.T_OBS], num_steps=1, num_particles=fc.PARTICLES, log_every=0)
    assert len(calls) == 1
    (m0, P0, F, q, Q, H, r, R, x), kw = calls[0]
    assert kw.get("need_grads", True)
    B = fc.PARTICLES
    assert x.shape == (B, fc.T_OBS, fc.OBS)
    # what the model shares between the particles -- the initial distribution, both matrices, both locations -- is
    # one matrix for all sequences (batch stride 0); the two covariances follow the particles' scale latents
    for shared in (m0, P0, F, q, H, r):
        assert shared.shape[0] == 1, tuple(shared.shape)
    assert Q.shape[0] == B and R.shape[0] == B
    # ... and everything is time-homogeneous
    for timed in (F, q, Q, H, r, R):
        assert timed.shape[1] == 1, tuple(timed.shape)


def test_forecast_runs_the_filter_and_the_fused_draw(gpu, monkeypatch):
    t = _inputs(F32, gpu)
    pyro.set_rng_seed(4)
    forecaster = _train(t, num_steps=2)
    filters, draws = _spy(monkeypatch, "gaussian_hmm_fwd_bwd"), _spy(monkeypatch, "gaussian_hmm_draw")
    out = forecaster(t["data"], t["covariates"], num_samples=7)
    assert out.shape == (7, fc.T_AHEAD, fc.OBS) and bool(torch.isfinite(out).all())
    assert len(filters) == 1 and filters[0][1].get("need_filter") and not filters[0][1].get("need_grads", True)
    assert len(draws) == 1
    assert forecaster(t["data"], t["covariates"], num_samples=20, batch_size=7).shape == (20, fc.T_AHEAD, fc.OBS)
    forecaster.max_plate_nesting = 2
    assert forecaster(t["data"], t["covariates"], num_samples=4).shape == (4, 1, fc.T_AHEAD, fc.OBS)


def test_backtest_scores_each_window_with_one_launch(gpu, monkeypatch):
    t = _inputs(F32, gpu)
    scores = _spy(monkeypatch, "forecast_scores")
    data, cov = t["data"][:12], t["covariates"][:12]
    records = backtest(data, cov, lambda: fc.make_model(fc.namespace(), "hmm", t)[0], min_train_window=8,
                       test_window=2, num_samples=10, forecaster_options={"num_steps": 2, "log_every": 0})
    assert [(r["t0"], r["t1"], r["t2"]) for r in records] == [(0, 8, 10), (0, 9, 11), (0, 10, 12)]
    assert len(scores) == 3                                             # one launch per window for the three scores
    for (pred, truth), _ in scores:
        assert pred.shape == (10, 2 * fc.OBS) and truth.shape == (2 * fc.OBS,)
    assert all(np.isfinite(r[k]) and isinstance(r[k], float) for r in records for k in ("mae", "rmse", "crps"))
    monkeypatch.setattr(stats, "FUSED_FORECAST_SCORES", False)
    again = backtest(data, cov, lambda: fc.make_model(fc.namespace(), "hmm", t)[0], min_train_window=8,
                     test_window=2, num_samples=10, forecaster_options={"num_steps": 2, "log_every": 0})
    assert len(scores) == 3
    for a, b in zip(records, again):                                    # the same seed: the same forecasts
        for k in ("mae", "rmse", "crps"):
            assert abs(a[k] - b[k]) <= 1e-5 * (1 + abs(b[k])), (k, a[k], b[k])


@pytest.mark.parametrize("dtype", (F64, F32), ids=("f64", "f32"))
def test_expanded_parameters_score_like_their_contiguous_copies(dtype, gpu, monkeypatch):
    """GaussianHMM hands a parameter whose batch dims are all expanded (stride 0) to the kernel as ONE matrix: log_prob
    and the gradients at the leaves are those of the same distribution built from contiguous copies, bit for bit in
    log_prob (a sequence's arithmetic does not depend on the layout) and within the dtype's rounding in the
    gradients (the kernel sums a shared parameter's gradient over the sequences, autograd the copies')."""
    import pyro_amd.distributions as dist
    calls = _spy(monkeypatch, "gaussian_hmm_fwd_bwd")
    B, steps, h, o = 5, 9, 3, 2
    gen = torch.Generator().manual_seed(21)
    rnd = lambda *s: torch.randn(*s, generator=gen, dtype=F64).to(dtype).to(gpu)       # noqa: E731
    leaves = {"q": 0.3 * rnd(h), "r": 0.3 * rnd(o), "F": 0.5 * rnd(h, h), "H": rnd(h, o),
              "sq": 0.5 + rnd(B, 1, h).abs(), "sr": 0.5 + rnd(B, 1, o).abs()}
    x = rnd(B, steps, o)

    def run(contiguous):
        t = {k: v.clone().requires_grad_() for k, v in leaves.items()}
        lay = (lambda v: v.contiguous()) if contiguous else (lambda v: v)
        d = dist.GaussianHMM(dist.Normal(torch.zeros(h, dtype=dtype, device=gpu), 1.0).to_event(1),
                             lay(t["F"].expand(B, 1, h, h)),
                             dist.Normal(lay(t["q"].expand(B, 1, h)), t["sq"]).to_event(1),
                             lay(t["H"].expand(B, 1, h, o)),
                             dist.Normal(lay(t["r"].expand(B, 1, o)), t["sr"]).to_event(1), duration=steps)
        lp = d.log_prob(x)
        return lp.detach(), torch.autograd.grad(lp.sum(), list(t.values()))

    lp_view, g_view = run(False)
    (m0, P0, F, q, Q, H, r, R, _), _ = calls[-1]
    assert [p.shape[0] for p in (F, q, Q, H, r, R)] == [1, 1, B, 1, 1, B]
    lp_copy, g_copy = run(True)
    (m0, P0, F, q, Q, H, r, R, _), _ = calls[-1]
    assert [p.shape[0] for p in (F, q, Q, H, r, R)] == [B, B, B, B, B, B]
    assert torch.equal(lp_view, lp_copy)
    tol = (2.0 ** -52 if dtype == F64 else 2.0 ** -23) * 64
    for name, a, b in zip(leaves, g_view, g_copy):
        assert a.shape == b.shape
        err = float((a - b).abs().max() / (1 + b.abs().max()))
        print("%s grad %s: %.2e" % (dtype, name, err))
        assert err <= tol, (name, err)
