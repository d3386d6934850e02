"""The tiny forecasting model of the contrib.forecast tests and of the generator of tests/golden/forecast.npz.

The model text is written once, over a namespace ``ns`` that names the backend -- ``ns.pyro``, ``ns.dist``,
``ns.poutine``, ``ns.ForecastingModel``, ``ns.LinearHMMReparam``, ``ns.StudentTReparam`` -- so the generator runs it on
the unmodified reference and the tests on this package.  T_OBS = 24 observed steps, T_AHEAD = 6 to forecast, OBS = 3
series, FEATURES = 2 covariates; latents ``bias`` [OBS], ``weight`` [FEATURES, OBS], ``trans_scale`` [HIDDEN] and
``obs_scale`` [OBS].  Every global latent carries the time plate's dim at size 1 (its prior's parameters are shaped
[1, ...]), as the reference's own forecasting models do, so that it broadcasts against time under a particle plate.

NOISES names what ``predict`` is handed:
  hmm             GaussianHMM, hidden 3, transition and observation scales the two scale latents
  normal0         Normal with event dim 0
  normal1         Normal with event dim 1
  transformed     TransformedDistribution(Normal, AffineTransform), event dim 0
  masked          Normal masked by a fixed pattern, event dim 0
  indep_hmm       IndependentHMM over OBS univariate GaussianHMMs with hidden 1
  student_linear  LinearHMM with StudentT transition and observation noise under LinearHMMReparam
"""
import os
import types

import numpy as np
import torch

T_OBS, T_AHEAD, OBS, HIDDEN, FEATURES, PARTICLES = 24, 6, 3, 3, 2, 5
NOISES = ("hmm", "normal0", "normal1", "transformed", "masked", "indep_hmm", "student_linear")
LATENTS = ("bias", "weight", "trans_scale", "obs_scale")
# a run of the model: (name, particles or None, max_plate_nesting)
CONFIGS = (("single", None, 1), ("p5_nest1", PARTICLES, 1), ("p5_nest2", PARTICLES, 2))
OPTIM = {"lr": 0.05, "betas": (0.9, 0.99), "lrd": 0.1 ** (1 / 40), "clip_norm": 10.0}
NUM_STEPS = 40
RESHAPES = ((6,), (3, 2), (2, 3, 1), (1, 2, 1, 3))         # new batch shapes of a distribution with batch (2, 3)
_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "forecast.npz")
_CACHE = {}


def golden(prefix):
    """{name: read-only numpy array} of the fixture's entries under ``prefix``/."""
    if not _CACHE:
        with np.load(_PATH) as z:
            for key in z.files:
                a = z[key]
                a.setflags(write=False)
                _CACHE[key] = a
    return {k[len(prefix) + 1:]: v for k, v in _CACHE.items() if k.startswith(prefix + "/")}


def namespace():
    """This package as the backend."""
    import pyro_amd
    from pyro_amd import distributions, poutine
    from pyro_amd.contrib.forecast import ForecastingModel
    from pyro_amd.infer.reparam import LinearHMMReparam, StudentTReparam
    return types.SimpleNamespace(pyro=pyro_amd, dist=distributions, poutine=poutine, ForecastingModel=ForecastingModel,
                                 LinearHMMReparam=LinearHMMReparam, StudentTReparam=StudentTReparam)


def make_inputs(rng):
    """The data, the covariates over T_OBS + T_AHEAD steps, the constants of the noise models and PARTICLES draws of
    the latents, as float64 numpy arrays."""
    T = T_OBS + T_AHEAD
    cov = rng.standard_normal((T, FEATURES))
    F = rng.standard_normal((HIDDEN, HIDDEN))
    F = 0.9 * F / np.linalg.norm(F, ord=2)
    out = {"covariates": cov,
           "data": cov[:T_OBS] @ rng.standard_normal((FEATURES, OBS)) + 0.5 + 0.3 * rng.standard_normal((T_OBS, OBS)),
           "F": F, "H": rng.standard_normal((HIDDEN, OBS)) / np.sqrt(HIDDEN),
           "mask": rng.random((T, OBS)) < 0.7,
           "bias": 0.5 * rng.standard_normal((PARTICLES, OBS)),
           "weight": 0.5 * rng.standard_normal((PARTICLES, FEATURES, OBS)),
           "trans_scale": 0.2 + 0.3 * rng.random((PARTICLES, HIDDEN)),
           "obs_scale": 0.2 + 0.3 * rng.random((PARTICLES, OBS))}
    return out


def tensors(arrays, dtype=torch.float64, device="cpu"):
    return {k: torch.tensor(v, device=device) if v.dtype == bool else torch.tensor(v, dtype=dtype, device=device)
            for k, v in arrays.items()}


def make_model(ns, noise, t):
    """The tiny model with the noise model ``noise``; ``t``: the tensors of make_inputs (the constants are read)."""
    pyro, dist = ns.pyro, ns.dist

    class TinyModel(ns.ForecastingModel):
        def model(self, zero_data, covariates):
            duration = zero_data.size(-2)
            slot = zero_data[..., :1, :]                                         # [1, OBS]: the time dim at size 1
            bias = pyro.sample("bias", dist.Normal(slot, 10.0).to_event(1))
            weight = pyro.sample("weight", dist.Normal(zero_data.new_zeros(1, FEATURES, OBS), 1.0).to_event(2))
            trans_scale = pyro.sample("trans_scale",
                                      dist.LogNormal(zero_data.new_full((1, HIDDEN), -1.0), 1.0).to_event(1))
            obs_scale = pyro.sample("obs_scale", dist.LogNormal(slot - 1.0, 1.0).to_event(1))
            prediction = bias + (covariates.unsqueeze(-1) * weight).sum(-2)      # [..., duration, OBS]
            zh, zo = zero_data.new_zeros(HIDDEN), zero_data.new_zeros(OBS)
            if noise == "hmm":
                d = dist.GaussianHMM(dist.Normal(zh, 1.0).to_event(1), t["F"],
                                     dist.Normal(zh, trans_scale).to_event(1), t["H"],
                                     dist.Normal(zo, obs_scale).to_event(1), duration=duration)
            elif noise == "normal0":
                d = dist.Normal(zero_data, obs_scale)
            elif noise == "normal1":
                d = dist.Normal(zero_data, obs_scale).to_event(1)
            elif noise == "transformed":
                d = dist.TransformedDistribution(dist.Normal(zero_data, obs_scale),
                                                 [torch.distributions.transforms.AffineTransform(0.3, 2.0)])
            elif noise == "masked":
                d = dist.Normal(zero_data, obs_scale).mask(t["mask"][:duration])
            elif noise == "indep_hmm":
                # OBS univariate chains: batch [..., OBS], time axis of size 1, hidden 1
                ts = trans_scale[..., :OBS].transpose(-1, -2).unsqueeze(-1)
                os_ = obs_scale.transpose(-1, -2).unsqueeze(-1)
                one = zero_data.new_ones(1)
                base = dist.GaussianHMM(dist.Normal(0 * one, one).to_event(1), 0.8 * one.reshape(1, 1),
                                        dist.Normal(0 * one, ts).to_event(1), one.reshape(1, 1),
                                        dist.Normal(0 * one, os_).to_event(1), duration=duration)
                d = dist.IndependentHMM(base)
            elif noise == "student_linear":
                d = dist.LinearHMM(dist.Normal(zh, 1.0).to_event(1), t["F"],
                                   dist.StudentT(3.5, zh, trans_scale).to_event(1), t["H"],
                                   dist.StudentT(4.5, zo, obs_scale).to_event(1), duration=duration)
            else:
                raise ValueError(noise)
            self.predict(d, prediction)

    model = TinyModel()
    if noise == "student_linear":
        rep = ns.LinearHMMReparam(trans=ns.StudentTReparam(), obs=ns.StudentTReparam())
        return model, ns.poutine.reparam(model, config={"residual": rep})
    return model, model


def latent_values(t, particles, nesting):
    """The latents' values as the sites have them under ``plate("particles", particles, dim=-1 - nesting)`` (None: no
    plate, the first draw)."""
    out = {}
    for name in LATENTS:
        v = t[name]
        if particles is None:
            out[name] = v[:1].reshape((1,) + tuple(v.shape[1:]))
        else:
            out[name] = v.reshape((particles,) + (1,) * nesting + tuple(v.shape[1:]))
    return out


def run_fixed(ns, noise, t, particles, nesting, aux=None):
    """The trace of the training model with the latents (and ``aux``: further sites) fixed by poutine.condition."""
    _, model = make_model(ns, noise, t)
    values = dict(latent_values(t, particles, nesting), **(aux or {}))
    conditioned = ns.poutine.condition(model, data=values)
    data, cov = t["data"], t["covariates"][:T_OBS]
    if particles is None:
        tr = ns.poutine.trace(conditioned).get_trace(data, cov)
    else:
        def in_plate(*args):
            with ns.pyro.plate("particles", particles, dim=-1 - nesting):
                return conditioned(*args)
        tr = ns.poutine.trace(in_plate).get_trace(data, cov)
    tr.compute_log_prob()
    return tr


def sample_sites(tr):
    return [name for name, site in tr.nodes.items()
            if site["type"] == "sample" and type(site["fn"]).__name__ != "_Subsample"]


def hmm_batch(rng, batch=(2, 3), T=5, h=2, o=2):
    """Parameters of a GaussianHMM with batch shape ``batch``, time-dependent transitions, and a value for it."""
    F = rng.standard_normal(batch + (T, h, h))
    F = 0.9 * F / np.linalg.norm(F, ord=2, axis=(-2, -1))[..., None, None]
    return {"init_scale": 0.5 + rng.random(batch + (h,)), "F": F,
            "trans_scale": 0.5 + rng.random(batch[-1:] + (1, h)),      # shared by the leading batch dim, over time
            "H": rng.standard_normal((h, o)), "obs_scale": 0.5 + rng.random(batch + (T, o)),
            "x": rng.standard_normal(batch + (T, o))}


def build_hmm(dist, p, independent=False):
    """The GaussianHMM of hmm_batch's parameters; ``independent``: an IndependentHMM over it (obs must be 1)."""
    h = p["F"].shape[-1]
    zeros = p["F"].new_zeros(h)
    d = dist.GaussianHMM(dist.Normal(zeros, p["init_scale"]).to_event(1), p["F"],
                         dist.Normal(zeros, p["trans_scale"]).to_event(1), p["H"],
                         dist.Normal(p["H"].new_zeros(p["H"].shape[-1]), p["obs_scale"]).to_event(1))
    return dist.IndependentHMM(d) if independent else d


class StubForecaster:
    """Stands in for a trained forecaster: a fixed function of the window."""

    def __init__(self, model, data, covariates, **options):
        self.t1 = data.size(-2)

    def __call__(self, data, covariates, num_samples, batch_size=None):
        f = covariates.size(-2) - data.size(-2)
        steps = torch.arange(f, dtype=data.dtype).reshape(1, f, 1)
        draws = torch.linspace(-1.0, 1.0, num_samples, dtype=data.dtype).reshape(-1, 1, 1)
        return data[..., -1:, :] + 0.1 * steps + draws
