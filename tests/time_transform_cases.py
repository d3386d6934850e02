"""Cases, bounds and models of the time-transform tests and of the generator of tests/golden/time_transforms.npz.

Kernel cases are (N, outer, inner, kind): x [outer, N, inner], the transform along dim -2.  N runs over powers of two,
their neighbours and lengths with odd tails at several Haar levels; inner over the strip width of the kernel (4; 2 for
f64 over 1024 steps) and its neighbours; outer * inner over column counts whose strips straddle an outer index.  The
fixture holds the reference's four transforms of FIXTURE-shaped inputs ([1, N, 2], every kind) for N <= 129; the large
lengths are checked against the float64 torch route on the CPU.

Bounds (derived, not measured), with u the unit roundoff of the dtype and A = max |x|:
  DCT, IDCT      (N + 2) u sqrt(2 N) A            N sequential terms plus a rounded table entry, times sum |terms|
  Haar, inverse  4 max(1, ceil(log2 N)) u sqrt(N) A   three roundings per level, values bounded by sqrt(N) A

The drift model is the tiny forecasting model of tests/forecast_cases.py with one time-local latent, ``drift`` [T, OBS]
inside the time plate, whose cumulative sum enters the prediction; written over a namespace like that module's.
"""
import math
import os

import numpy as np
import torch

try:
    from . import forecast_cases as fc
except ImportError:                          # loaded by its path, by the generator of the fixture
    import importlib.util
    _spec = importlib.util.spec_from_file_location(
        "forecast_cases", os.path.join(os.path.dirname(os.path.abspath(__file__)), "forecast_cases.py"))
    fc = importlib.util.module_from_spec(_spec)
    _spec.loader.exec_module(fc)

OPS = ("dct", "idct", "haar_transform", "inverse_haar_transform")
INVERSE = {"dct": "idct", "idct": "dct", "haar_transform": "inverse_haar_transform",
           "inverse_haar_transform": "haar_transform"}
KINDS = ("normal", "walk", "offset")
SMALL_N = (1, 2, 3, 4, 5, 7, 8, 9, 31, 32, 33, 63, 64, 65, 127, 129)
LARGE_N = (1000, 2048)
FIXTURE_SHAPE = (1, 2)                       # (outer, inner) of the fixture's inputs
_OUTERS, _INNERS = (1, 2, 3), (1, 3, 4, 5, 17)
_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "time_transforms.npz")
_CACHE = {}


def _cases():
    out = []
    for i, n in enumerate(SMALL_N):
        out += [(n,) + FIXTURE_SHAPE + (kind,) for kind in KINDS]
        out.append((n, _OUTERS[i % 3], _INNERS[i % 5], KINDS[i % 3]))
        out.append((n, _OUTERS[(i + 1) % 3], _INNERS[(i + 2) % 5], KINDS[(i + 1) % 3]))
    # the large lengths: f64 strips are 2 wide over 1024 steps, so inner 1, 2, 3 there; 3, 4, 5 around the width 4
    out += [(1000, 1, 5, "normal"), (1000, 3, 3, "walk"), (1000, 2, 4, "offset"),
            (2048, 1, 3, "walk"), (2048, 2, 1, "normal"), (2048, 1, 2, "offset"), (2048, 1, 5, "normal")]
    return tuple(out)


CASES = _cases()


def case_id(case):
    return "N%d_o%d_i%d_%s" % case


def make(case, dtype=torch.float64):
    """The input of a case, [outer, N, inner] on the CPU (seeded by the case itself)."""
    n, outer, inner, kind = case
    rng = np.random.default_rng([n, outer, inner, KINDS.index(kind)])
    x = rng.standard_normal((outer, n, inner))
    if kind == "walk":
        x = np.cumsum(x, axis=1)
    elif kind == "offset":
        x = 1e3 * x + 50.0
    return torch.tensor(x, dtype=dtype)


def unit_roundoff(dtype):
    return 2.0 ** -53 if dtype == torch.float64 else 2.0 ** -24


def bound(op, n, dtype, amax):
    u = unit_roundoff(dtype)
    if op in ("dct", "idct"):
        return (n + 2) * u * math.sqrt(2 * n) * amax
    return 4 * max(1, math.ceil(math.log2(n))) * u * math.sqrt(n) * amax


def along_time(fn, x):
    """``fn`` of tensor_utils applied along dim -2 of x [outer, N, inner]."""
    if fn.__name__ in ("dct", "idct"):
        return fn(x, dim=-2)
    return fn(x.transpose(-1, -2)).transpose(-1, -2)


def golden(prefix):
    """{name: read-only numpy array} of the fixture's entries under ``prefix``/."""
    if not _CACHE:
        with np.load(_PATH) as z:
            for key in z.files:
                a = z[key]
                a.setflags(write=False)
                _CACHE[key] = a
    return {k[len(prefix) + 1:]: v for k, v in _CACHE.items() if k.startswith(prefix + "/")}


# ---- the transform classes -------------------------------------------------------------------------------------------
TRANSFORM_CASES = tuple([("dct", dict(smooth=s), d) for s in (0.0, 1.0, -0.5) for d in (-1, -2)]
                        + [("haar", dict(flip=f), d) for f in (False, True) for d in (-1, -2)])


def transform_id(case):
    name, options, dim = case
    return "%s_%s_d%d" % (name, "_".join("%s%s" % kv for kv in options.items()), -dim)


def transform_input():
    return torch.tensor(np.random.default_rng(77).standard_normal((2, 5, 6)))


def build_transform(transforms, case, **more):
    name, options, dim = case
    cls = transforms.DiscreteCosineTransform if name == "dct" else transforms.HaarTransform
    return cls(dim=dim, **options, **more)


# ---- the periodic helpers --------------------------------------------------------------------------------------------
def periodic_inputs():
    x = torch.tensor(np.random.default_rng(78).standard_normal((7, 5)))
    return {"repeat": ((x, 4, 0), (x, 13, 1), (x, 3, -1)),
            "cumsum": ((x, 3, 0), (x, 2, 1), (x, 7, -2)),
            "features": ((10,), (10, 7.5), (30, 365.25, 7))}


# ---- the drift model and its reparameterised traces ------------------------------------------------------------------
DRIFT_NOISES = ("hmm", "normal0")
REPARAMS = ("haar", "dct_smooth1")
DRIFT_LATENTS = ("bias", "trans_scale", "obs_scale")


def namespace():
    from pyro_amd.infer.reparam import DiscreteCosineReparam, HaarReparam
    ns = fc.namespace()
    ns.HaarReparam, ns.DiscreteCosineReparam = HaarReparam, DiscreteCosineReparam
    return ns


def make_drift_model(ns, noise, t):
    pyro, dist = ns.pyro, ns.dist
    HIDDEN, OBS = fc.HIDDEN, fc.OBS

    class DriftModel(ns.ForecastingModel):
        def model(self, zero_data, covariates):
            duration = zero_data.size(-2)
            slot = zero_data[..., :1, :]
            bias = pyro.sample("bias", dist.Normal(slot, 10.0).to_event(1))
            trans_scale = pyro.sample("trans_scale",
                                      dist.LogNormal(zero_data.new_full((1, HIDDEN), -1.0), 1.0).to_event(1))
            obs_scale = pyro.sample("obs_scale", dist.LogNormal(slot - 1.0, 1.0).to_event(1))
            with self.time_plate:
                drift = pyro.sample("drift", dist.Normal(zero_data, 0.1).to_event(1))
            prediction = bias + drift.cumsum(-2)
            if noise == "hmm":
                zh, zo = zero_data.new_zeros(HIDDEN), zero_data.new_zeros(OBS)
                d = dist.GaussianHMM(dist.Normal(zh, 1.0).to_event(1), t["F"],
                                     dist.Normal(zh, trans_scale).to_event(1), t["H"],
                                     dist.Normal(zo, obs_scale).to_event(1), duration=duration)
            else:
                d = dist.Normal(zero_data, obs_scale)
            self.predict(d, prediction)

    return DriftModel()


def reparam_config(ns, which):
    """An explicit config function: the site ``drift`` along dim -2 (its time dim, a batch dim of the site)."""
    def config(msg):
        if msg["name"] != "drift":
            return None
        if which == "haar":
            return ns.HaarReparam(dim=-2, experimental_allow_batch=True)
        return ns.DiscreteCosineReparam(dim=-2, smooth=1.0, experimental_allow_batch=True)
    return config


def aux_name(which):
    return "drift_haar" if which == "haar" else "drift_dct"


def drift_coefficients(dtype=torch.float64, device="cpu"):
    """PARTICLES draws of the auxiliary site's value, [PARTICLES, T_OBS, OBS]."""
    c = 0.1 * np.random.default_rng(79).standard_normal((fc.PARTICLES, fc.T_OBS, fc.OBS))
    return torch.tensor(c, dtype=dtype, device=device)


def run_reparam_trace(ns, noise, which, t, particles, nesting, coef):
    """The trace of the drift model under poutine.reparam, the global latents and the auxiliary site fixed by
    poutine.condition."""
    model = ns.poutine.reparam(make_drift_model(ns, noise, t), config=reparam_config(ns, which))
    values = {k: v for k, v in fc.latent_values(t, particles, nesting).items() if k in DRIFT_LATENTS}
    if particles is None:
        values[aux_name(which)] = coef[:1]
    else:
        values[aux_name(which)] = coef.reshape((particles,) + (1,) * nesting + tuple(coef.shape[1:]))
    conditioned = ns.poutine.condition(model, data=values)
    data, cov = t["data"], t["covariates"][:fc.T_OBS]
    if particles is None:
        tr = ns.poutine.trace(conditioned).get_trace(data, cov)
    else:
        def in_plate(*args):
            with ns.pyro.plate("particles", particles, dim=-1 - nesting):
                return conditioned(*args)
        tr = ns.poutine.trace(in_plate).get_trace(data, cov)
    tr.compute_log_prob()
    return tr


def trace_key(noise, which, config):
    return "traces/%s/%s/%s" % (noise, which, config)


# ---- the model of the HMCForecaster tests ----------------------------------------------------------------------------
HMC_T, HMC_AHEAD = 16, 4
HMC_POSTERIOR_MEAN, HMC_POSTERIOR_SD = 2.0 / 1.25, math.sqrt(0.2)        # exact: 1 / (1 + 1 / 0.25) = 0.2


def hmc_data(dtype=torch.float64, device="cpu"):
    sign = torch.tensor([1.0, -1.0], dtype=dtype, device=device).repeat((HMC_T + HMC_AHEAD) // 2)
    return (2.0 * sign[:HMC_T]).unsqueeze(-1), torch.zeros(HMC_T + HMC_AHEAD, 0, dtype=dtype, device=device)


def make_hmc_model(noise="normal"):
    """drift_t ~ Normal(0, 1) inside the time plate, prediction = drift, noise Normal(0, 0.5): every drift_t has the
    exact, independent posterior Normal(x_t / 1.25, sqrt 0.2).  ``noise="hmm"``: a GaussianHMM with hidden 2 instead."""
    import pyro_amd
    import pyro_amd.distributions as dist
    from pyro_amd.contrib.forecast import ForecastingModel

    class Model(ForecastingModel):
        def model(self, zero_data, covariates):
            with self.time_plate:
                drift = pyro_amd.sample("drift", dist.Normal(zero_data, 1.0).to_event(1))
            if noise == "normal":
                d = dist.Normal(zero_data, 0.5)
            else:
                zh, zo = zero_data.new_zeros(2), zero_data.new_zeros(1)
                F = zero_data.new_tensor([[0.5, 0.1], [0.0, 0.3]])
                H = zero_data.new_tensor([[1.0], [0.5]])
                d = dist.GaussianHMM(dist.Normal(zh, 1.0).to_event(1), F, dist.Normal(zh, 0.3).to_event(1), H,
                                     dist.Normal(zo, 0.5).to_event(1), duration=zero_data.size(-2))
            self.predict(d, drift)

    return Model()
