"""The GammaGaussianHMM fixtures of tests/golden/gamma_gaussian_hmm.npz (made by
tests/golden/make_golden_gamma_gaussian_hmm.py from the unmodified reference, float64) as the host and device tests use
them: loaded once, never modified."""
import os

import numpy as np
import torch

from tests import gaussian_hmm_cases as gc

NAMES = ("a", "b") + gc.NAMES
CASES = ("b3_t1_h2_o1", "b3_t7_h3_o2_shared", "b2_t9_h4_o3_het", "b2_t33_h8_o5", "b2_t40_h16_o16",
         "b2_t17_h5_o16_het", "b2_t12_h1_o1", "b3_t7_h3_o2_gamma_shared", "b2_t9_h4_o3_heavy",
         "b2_t12_h4_o3_outliers")
_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gamma_gaussian_hmm.npz")
_CACHE = {}
rel_err = gc.rel_err


def golden(case):
    """{name: float64 numpy array} of one case: the inputs NAMES, "g_" + name, log_prob, and of filter():
    concentration, rate, loc, filter_precision (the INVERSE of the final state's unit-scale covariance)."""
    if not _CACHE:
        with np.load(_PATH) as z:
            for key in z.files:
                c, name = key.split("/")
                _CACHE.setdefault(c, {})[name] = z[key]
        for c in _CACHE.values():
            for a in c.values():
                a.setflags(write=False)
    return _CACHE[case]


def leaves(case, dtype, device, requires_grad=True):
    g = golden(case)
    return {k: torch.tensor(g[k], dtype=dtype, device=device, requires_grad=requires_grad) for k in NAMES}


def build(t, dist, validate_args=None):
    """The GammaGaussianHMM of the leaf tensors ``t`` with the distribution classes of module ``dist``."""
    return dist.GammaGaussianHMM(dist.Gamma(t["a"], t["b"]), dist.MultivariateNormal(t["m0"], scale_tril=t["L0"]),
                                 t["F"], dist.MultivariateNormal(t["q"], scale_tril=t["Lq"]), t["H"],
                                 dist.MultivariateNormal(t["r"], scale_tril=t["Lr"]), validate_args=validate_args)


def value_and_grads(t, dist):
    """(log_prob, {name: gradient of sum(log_prob)}) as float64 numpy arrays, through the class."""
    lp = build(t, dist).log_prob(t["x"])
    grads = torch.autograd.grad(lp.sum(), [t[k] for k in NAMES])
    return lp.detach().cpu().double().numpy(), {k: g.detach().cpu().double().numpy() for k, g in zip(NAMES, grads)}


def posterior(t, dist):
    """{concentration, rate, loc, filter_precision} of filter() as float64 numpy arrays; filter_precision is the inverse
    of the returned normal's covariance, formed in float64 on the CPU."""
    gamma, mvn = build(t, dist).filter(t["x"])
    B = t["x"].shape[0]
    np64 = lambda v: v.detach().cpu().double()                                            # noqa: E731
    return {"concentration": np64(gamma.concentration).expand(B).numpy(), "rate": np64(gamma.rate).expand(B).numpy(),
            "loc": np64(mvn.loc).numpy(), "filter_precision": torch.linalg.inv(np64(mvn.covariance_matrix)).numpy()}


def errors(t, case, dist):
    """{"log_prob", "grads" (the nine of the model), "grad_a", "grad_b", "rate", "filter" (concentration, loc and the
    inverse covariance)}: the errors of the class's route for the leaves ``t`` against the fixture, and the per-array
    figures."""
    g = golden(case)
    lp, grads = value_and_grads(t, dist)
    post = posterior(t, dist)
    per = {"g_" + k: rel_err(grads[k], g["g_" + k]) for k in NAMES}
    per.update({k: rel_err(post[k], g[k]) for k in post})
    lp_err = float(np.max(np.abs(lp - g["log_prob"]) / (1 + np.abs(g["log_prob"]))))
    return {"log_prob": lp_err, "grads": max(per["g_" + k] for k in gc.NAMES), "grad_a": per["g_a"],
            "grad_b": per["g_b"], "rate": per["rate"],
            "filter": max(per["concentration"], per["loc"], per["filter_precision"])}, per
