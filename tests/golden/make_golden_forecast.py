"""Generate tests/golden/forecast.npz from the UNMODIFIED reference (pyro-ppl/pyro 1.9.1), float64 on the CPU.

    python tests/golden/make_golden_forecast.py

The reference is imported as tests/golden/make_golden_linear_hmm.py imports it (oracle/refshim stands in for
opt_einsum).  The model text and the score cases are the tests' own (tests/forecast_cases.py over a namespace,
tests/forecast_scores_cases.py), run here on the reference; only the data file depends on it.

scores/<kind>_<S>_<M>/      pred, truth and the reference's pred.mean(0), pred.median(0).values, crps_empirical
inputs/                     data, covariates, constants and PARTICLES draws of the latents (forecast_cases.make_inputs)
fixed/<noise>/<config>/     sites, log_prob_<site> and log_prob_sum of the training trace with the latents fixed by
                            poutine.condition; value_<site> of the auxiliary Gamma sites of the reparameterised model
train/                      losses and final AutoDelta parameters of 40 steps from the first draw of the latents, and
                            the same with the data perturbed by 1e-13 relative (losses_perturbed, ...)
forecast/                   the shape of a forecast for max_plate_nesting 1 and 2
reshape/<type>/             parameters, value and log_prob of reshape_batch(d, new) for each new batch shape
eval/                       pred, truth and eval_mae, eval_rmse, eval_crps; the record keys and windows of a backtest
                            over 3 windows with a stub forecaster
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.join(ROOT, "oracle", "refshim"))  # after `import torch` on purpose
sys.path.insert(0, os.environ.get("PYRO_REFERENCE", "/root/reference"))

import pyro  # noqa: E402
import pyro.distributions as dist  # noqa: E402
from pyro import poutine  # noqa: E402
from pyro.contrib.forecast import Forecaster, ForecastingModel, backtest, eval_crps, eval_mae, eval_rmse  # noqa: E402
from pyro.contrib.forecast.util import reshape_batch  # noqa: E402
from pyro.infer.autoguide import AutoDelta, init_to_value  # noqa: E402
from pyro.infer.reparam import LinearHMMReparam, StudentTReparam  # noqa: E402
from pyro.ops.stats import crps_empirical  # noqa: E402
from pyro.optim import ClippedAdam  # noqa: E402



def _cases(name):
    """A case module of this repository's tests by its path (the reference has a ``tests`` package of its own)."""
    import importlib.util
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tests", name + ".py"))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


fc, fsc = _cases("forecast_cases"), _cases("forecast_scores_cases")

assert pyro.__version__ == "1.9.1"
torch.set_default_dtype(torch.float64)
NS = types.SimpleNamespace(pyro=pyro, dist=dist, poutine=poutine, ForecastingModel=ForecastingModel,
                           LinearHMMReparam=LinearHMMReparam, StudentTReparam=StudentTReparam)


def scores(flat):
    for kind, S, M in fsc.GOLDEN:
        pred, truth = fsc.make(kind, S, M)
        key = "scores/%s_%d_%d/" % (kind, S, M)
        flat[key + "pred"], flat[key + "truth"] = pred.numpy(), truth.numpy()
        flat[key + "mean"] = pred.mean(0).numpy()
        flat[key + "median"] = pred.median(0).values.numpy()
        flat[key + "crps"] = crps_empirical(pred, truth).numpy()


def fixed(t, flat):
    for noise in fc.NOISES:
        for k, (config, particles, nesting) in enumerate(fc.CONFIGS):
            torch.manual_seed(3000 + k)
            tr = fc.run_fixed(NS, noise, t, particles, nesting)
            sites = fc.sample_sites(tr)
            key = "fixed/%s/%s/" % (noise, config)
            flat[key + "sites"] = np.array(sites)
            for s in sites:
                flat[key + "log_prob_" + s] = tr.nodes[s]["log_prob"].detach().numpy()
                if s not in fc.LATENTS and s != "residual":
                    flat[key + "value_" + s] = tr.nodes[s]["value"].detach().numpy()
            flat[key + "log_prob_sum"] = np.array(float(tr.log_prob_sum()))
            print(noise, config, tuple(tr.nodes["residual"]["log_prob"].shape), float(tr.log_prob_sum()))


def train(t, data):
    pyro.clear_param_store()
    model, _ = fc.make_model(NS, "hmm", t)
    init = {k: v.clone() for k, v in fc.latent_values(t, None, 1).items()}
    guide = AutoDelta(model, init_loc_fn=init_to_value(values=init))
    forecaster = Forecaster(model, data, t["covariates"][:fc.T_OBS], guide=guide, optim=ClippedAdam(dict(fc.OPTIM)),
                            num_steps=fc.NUM_STEPS, log_every=0)
    params = {k: v.detach().clone().numpy() for k, v in pyro.get_param_store().items()}
    return forecaster, np.array(forecaster.losses), params


def training(t, flat):
    forecaster, losses, params = train(t, t["data"])
    _, again, _ = train(t, t["data"])
    assert np.array_equal(losses, again), "the reference does not train deterministically"
    scale = 1.0 + 1e-13 * torch.tensor(np.random.default_rng(7).choice([-1.0, 1.0], size=tuple(t["data"].shape)))
    _, losses_p, params_p = train(t, t["data"] * scale)
    print("losses %.4f -> %.4f, perturbed deviation %.2e" % (losses[0], losses[-1], np.abs(losses - losses_p).max()))
    flat["train/losses"], flat["train/losses_perturbed"] = losses, losses_p
    for k, v in params.items():
        flat["train/param_" + k], flat["train/param_perturbed_" + k] = v, params_p[k]
    # the forecast's shape, for max_plate_nesting 1 and (forced) 2
    forecaster, _, _ = train(t, t["data"])
    for nesting in (1, 2):
        forecaster.max_plate_nesting = nesting
        out = forecaster(t["data"], t["covariates"], num_samples=4)
        flat["forecast/shape_nest%d" % nesting] = np.array(out.shape)
        print("forecast", nesting, tuple(out.shape))


def reshapes(rng, flat):
    for name, independent in (("gaussian_hmm", False), ("independent_hmm", True)):
        p = fc.hmm_batch(rng, o=1 if independent else 2)
        tp = fc.tensors(p)
        d = fc.build_hmm(dist, tp, independent)
        x = tp["x"]
        if independent:          # batch (2,), event (T, 3)
            x = x.squeeze(-1).transpose(-1, -2)
        batch = tuple(d.batch_shape)
        for k, v in p.items():
            flat["reshape/%s/%s" % (name, k)] = v
        flat["reshape/%s/log_prob" % name] = d.log_prob(x).numpy()
        news = fc.RESHAPES if not independent else ((2, 1), (1, 2), (1, 2, 1))
        for new in news:
            lp = reshape_batch(d, new).log_prob(x.reshape(new + tuple(x.shape[len(batch):])))
            assert lp.shape == new
            flat["reshape/%s/log_prob_%s" % (name, "x".join(map(str, new)))] = lp.numpy()


def evaluation(rng, t, flat):
    pred = torch.tensor(rng.standard_normal((20, fc.T_AHEAD, fc.OBS)))
    truth = torch.tensor(rng.standard_normal((fc.T_AHEAD, fc.OBS)))
    flat["eval/pred"], flat["eval/truth"] = pred.numpy(), truth.numpy()
    flat["eval/mae"], flat["eval/rmse"] = np.array(eval_mae(pred, truth)), np.array(eval_rmse(pred, truth))
    flat["eval/crps"] = np.array(eval_crps(pred, truth))
    data, cov = t["data"][:12], t["covariates"][:12]
    records = backtest(data, cov, lambda: None, forecaster_fn=fc.StubForecaster, min_train_window=8, test_window=2,
                       num_samples=10)
    assert len(records) == 3
    flat["eval/backtest_keys"] = np.array(sorted(records[0]))
    flat["eval/backtest_windows"] = np.array([[r["t0"], r["t1"], r["t2"]] for r in records])
    for name in ("mae", "rmse", "crps"):
        flat["eval/backtest_" + name] = np.array([r[name] for r in records])
    print("backtest", sorted(records[0]), flat["eval/backtest_windows"].tolist())


def main():
    rng = np.random.default_rng(20261020)
    flat = {}
    scores(flat)
    arrays = fc.make_inputs(rng)
    for k, v in arrays.items():
        flat["inputs/" + k] = v
    t = fc.tensors(arrays)
    fixed(t, flat)
    training(t, flat)
    reshapes(rng, flat)
    evaluation(rng, t, flat)
    path = os.path.join(HERE, "forecast.npz")
    np.savez_compressed(path, **flat)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
