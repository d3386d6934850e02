"""The GaussianHMM fixtures of tests/golden/gaussian_hmm.npz (made by tests/golden/make_golden_gaussian_hmm.py from
the unmodified reference, float64) as the host and device tests use them: loaded once, never modified."""
import os

import numpy as np
import torch

NAMES = ("m0", "L0", "F", "q", "Lq", "H", "r", "Lr", "x")
CASES = ("b3_t1_h2_o1", "b3_t7_h3_o2_shared", "b2_t9_h4_o3_het", "b2_t33_h8_o5", "b2_t40_h16_o16",
         "b2_t17_h5_o16_het", "b2_t12_h1_o1", "b3_t6_h3_o2_indep")
_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gaussian_hmm.npz")
_CACHE = {}


def golden(case):
    """{name: float64 numpy array} of one case: the inputs NAMES, "g_" + name, log_prob, filter_mean, filter_cov."""
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


def build(t, case, dist, validate_args=None):
    """The GaussianHMM of the case from the leaf tensors ``t`` with the distribution classes of module ``dist``."""
    init = dist.MultivariateNormal(t["m0"], scale_tril=t["L0"])
    trans = dist.MultivariateNormal(t["q"], scale_tril=t["Lq"])
    if case.endswith("indep"):
        obs = dist.Independent(dist.Normal(t["r"], t["Lr"]), 1)
    else:
        obs = dist.MultivariateNormal(t["r"], scale_tril=t["Lr"])
    return dist.GaussianHMM(init, t["F"], trans, t["H"], obs, validate_args=validate_args)


def rel_err(got, want):
    """max |got - want| / (1 + max |want|): the measure the issue states its figures in."""
    got = np.asarray(got, dtype=np.float64)
    want = np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    if want.size == 0:
        return 0.0
    return float(np.max(np.abs(got - want)) / (1.0 + np.max(np.abs(want))))


def value_and_grads(t, case, dist):
    """(log_prob, {name: gradient of sum(log_prob)}) as float64 numpy arrays, through the class."""
    lp = build(t, case, dist).log_prob(t["x"])
    grads = torch.autograd.grad(lp.sum(), [t[k] for k in NAMES])
    return lp.detach().cpu().double().numpy(), {k: g.detach().cpu().double().numpy() for k, g in zip(NAMES, grads)}
