"""Generate tests/golden/glm_families.npz from the UNMODIFIED reference (pyro-ppl/pyro 1.9.1), float64 on the CPU.

    python tests/golden/make_golden_glm_families.py

The reference is imported as the other generators import it (oracle/refshim stands in for opt_einsum).  Only the
data file depends on the reference; the tests read nothing else of it.

The four plated regression models of tests/glm_family_cases.py (make_model: the tests' own model text, written with
the reference's API) at N = 300, D = 5 with three vectorised particles: latents w [3, 1, 5], b [3, 1], sigma [3, 1],
nu [3, 1] fixed by poutine.condition, under pyro.plate("data", 1000, subsample_size=300) (scale 10/3) and a
poutine.mask that drops about a fifth of the rows; Binomial once with a per-row count and once with a scalar one.
Stored per model: the data, the latents, the per-particle log-probability sums of the observed site
("<model>/ll" [3]) and the reference's autograd gradients of their total with respect to every latent
("<model>/grad_<latent>").
"""
import os
import sys

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

import importlib.util  # noqa: E402

# (by path: the reference has a ``tests`` package of its own)
_spec = importlib.util.spec_from_file_location("glm_family_cases", os.path.join(ROOT, "tests", "glm_family_cases.py"))
cases = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(cases)

assert pyro.__version__ == "1.9.1"

N, D, P, PLATE = 300, 5, 3, 1000


def main():
    rng = np.random.default_rng(20261021)
    flat = {}
    for name in cases.GOLDEN_MODELS:
        family = cases.family_of(name)
        X = rng.standard_normal((N, D))
        w = 0.6 * rng.standard_normal((P, 1, D))
        b = 0.5 * rng.standard_normal((P, 1))
        sigma = rng.uniform(0.5, 2.0, (P, 1))
        nu = rng.uniform(2.0, 12.0, (P, 1))
        eta = (w[1, 0] @ X.T) + b[1]
        count = None
        if family == "normal":
            y = eta + rng.standard_normal(N)
        elif family == "student_t":
            y = eta + rng.standard_t(3.0, N)
        elif family == "poisson":
            y = rng.poisson(np.exp(eta)).astype(np.float64)
        else:
            n = rng.integers(1, 21, N) if name == "binomial_rows" else np.full(N, int(cases.SCALAR_COUNT))
            y = rng.binomial(n, 1.0 / (1.0 + np.exp(-eta))).astype(np.float64)
            count = n.astype(np.float64)
        mask = rng.random(N) > 0.2
        latents = {"w": w, "b": b}
        if family in ("normal", "student_t"):
            latents["sigma"] = sigma
        if family == "student_t":
            latents["nu"] = nu
        t = {k: torch.tensor(v, dtype=torch.float64, requires_grad=True) for k, v in latents.items()}
        Xt, yt, mt = torch.tensor(X), torch.tensor(y), torch.tensor(mask)
        ct = None
        if count is not None:
            ct = torch.tensor(count) if name == "binomial_rows" else cases.SCALAR_COUNT
        model = cases.make_model(pyro, dist, poutine, name)
        tr = poutine.trace(poutine.condition(model, data=t)).get_trace(Xt, yt, mt, PLATE, ct)
        tr.compute_log_prob()
        lp = tr.nodes["obs"]["log_prob"]
        assert lp.shape == (P, N), lp.shape
        for k in t:                                   # the flat priors contribute nothing
            assert float(tr.nodes[k]["log_prob"].abs().sum()) == 0.0
        ll = lp.sum(-1)
        grads = torch.autograd.grad(ll.sum(), list(t.values()))
        print(name, "ll", ll.tolist())
        flat[name + "/X"], flat[name + "/y"], flat[name + "/mask"] = X, y, mask
        flat[name + "/plate_size"] = np.array(PLATE)
        if count is not None:
            flat[name + "/count"] = count
        for k, v in latents.items():
            flat[name + "/" + k] = v
        flat[name + "/ll"] = ll.detach().numpy()
        for k, g in zip(t, grads):
            flat[name + "/grad_" + k] = g.numpy()
    path = os.path.join(HERE, "glm_families.npz")
    np.savez_compressed(path, **flat)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
