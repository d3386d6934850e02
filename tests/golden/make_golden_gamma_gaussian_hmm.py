"""Generate tests/golden/gamma_gaussian_hmm.npz from the UNMODIFIED reference (pyro-ppl/pyro 1.9.1): for every case the
inputs of a GammaGaussianHMM, its log_prob, the autograd gradients of sum(log_prob) with respect to all eleven inputs
and the two posteriors of filter(), all float64 on the CPU.

    python tests/golden/make_golden_gamma_gaussian_hmm.py

The reference is imported as tests/golden/make_golden_gaussian_hmm.py imports it; the seven MultivariateNormal cases,
the input recipe and the scale_tril convention of the gradients are that file's.  The Gamma: a ~ U(1, 4) and
b ~ U(0.5, 3) per series.  Three more cases: a scalar Gamma shared by the series, a = b = 0.6 (a heavy tail: fewer than
two degrees of freedom), and data with three steps multiplied by 10 (outliers).

Stored of filter(): the Gamma's ``concentration`` and ``rate``, the normal's ``loc`` and, as ``filter_precision``, its
``scale_tril @ scale_tril^T`` -- the reference builds the normal with scale_tril = cholesky(precision), so that product
is the INVERSE of the final state's unit-scale covariance.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, HERE)

import make_golden_gaussian_hmm as base  # noqa: E402  (puts the reference on the path)
import pyro.distributions as dist  # noqa: E402

# name: (B, T, hidden, obs, batch layout, time layout, variant)
CASES = {name: spec[:6] + ("series",) for name, spec in base.CASES.items() if spec[6] == "mvn"}
CASES["b3_t7_h3_o2_gamma_shared"] = (3, 7, 3, 2, "shared", "hom", "scalar")
CASES["b2_t9_h4_o3_heavy"] = (2, 9, 4, 3, "batched", "hom", "heavy")
# (the three added cases are small and time-homogeneous: the file stays under the size of gaussian_hmm_edges.npz)
CASES["b2_t12_h4_o3_outliers"] = (2, 12, 4, 3, "batched", "hom", "outliers")
OUTLIER_STEPS = (2, 6, 10)
NAMES = ("a", "b") + base.NAMES


def make_inputs(rng, B, T, h, o, lay, time, variant):
    out = base.make_inputs(rng, B, T, h, o, lay, time, "mvn")
    if variant == "scalar":
        out["a"], out["b"] = rng.uniform(1.0, 4.0, ()), rng.uniform(0.5, 3.0, ())
    elif variant == "heavy":
        out["a"], out["b"] = np.full((B,), 0.6), np.full((B,), 0.6)
    else:
        out["a"], out["b"] = rng.uniform(1.0, 4.0, (B,)), rng.uniform(0.5, 3.0, (B,))
    if variant == "outliers":
        out["x"][:, OUTLIER_STEPS, :] *= 10.0
    return out


def build(t):
    init = dist.MultivariateNormal(t["m0"], scale_tril=t["L0"].tril())
    trans = dist.MultivariateNormal(t["q"], scale_tril=t["Lq"].tril())
    obs = dist.MultivariateNormal(t["r"], scale_tril=t["Lr"].tril())
    return dist.GammaGaussianHMM(dist.Gamma(t["a"], t["b"]), init, t["F"], trans, t["H"], obs)


def main():
    rng = np.random.default_rng(20241101)
    flat = {}
    for name, (B, T, h, o, lay, time, variant) in CASES.items():
        arrays = make_inputs(rng, B, T, h, o, lay, time, variant)
        t = {k: torch.tensor(v, dtype=torch.float64, requires_grad=True) for k, v in arrays.items()}
        hmm = build(t)
        assert hmm.batch_shape == (B,), (name, hmm.batch_shape)
        lp = hmm.log_prob(t["x"])
        grads = torch.autograd.grad(lp.sum(), [t[k] for k in NAMES])
        with torch.no_grad():
            gamma, mvn = build({k: v.detach() for k, v in t.items()}).filter(t["x"].detach())
        for k in NAMES:
            flat[name + "/" + k] = arrays[k]
        for k, g in zip(NAMES, grads):
            flat[name + "/g_" + k] = g.numpy()
        flat[name + "/log_prob"] = lp.detach().numpy()
        flat[name + "/concentration"] = gamma.concentration.expand(B).numpy()
        flat[name + "/rate"] = gamma.rate.expand(B).numpy()
        flat[name + "/loc"] = mvn.loc.expand(B, h).numpy()
        flat[name + "/filter_precision"] = (mvn.scale_tril @ mvn.scale_tril.transpose(-1, -2)).expand(B, h, h).numpy()
        print(name, "log_prob", lp.detach().numpy())
    path = os.path.join(HERE, "gamma_gaussian_hmm.npz")
    np.savez_compressed(path, **flat)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
