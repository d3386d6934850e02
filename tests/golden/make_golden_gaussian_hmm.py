"""Generate tests/golden/gaussian_hmm.npz from the UNMODIFIED reference (pyro-ppl/pyro 1.9.1): for every case the
inputs of a GaussianHMM, its log_prob, the autograd gradients of sum(log_prob) with respect to every input and the
moments of filter(), all float64 on the CPU.

    python tests/golden/make_golden_gaussian_hmm.py

The reference is imported as tests/golden/make_golden.py imports it (oracle/refshim stands in for opt_einsum).  Only
the data file depends on the reference; the tests read nothing else of it.

The noise is parametrised by ``scale_tril`` (``scale`` for the Independent(Normal) case) and the gradients are with
respect to those: that sidesteps the triangular-versus-symmetric convention of a covariance gradient.

Input recipe: F scaled to spectral norm 0.9, H = randn / sqrt(hidden), covariances A A^T / n + 0.5 I, locations
0.3 randn, x = 2 randn.  (With F = 0.5 randn -- spectral radius above 1 -- a float32 filter loses the positive
definiteness of the innovation covariance by T = 33 at hidden 8.)

Layouts (``lay``): "batched" parameters carry the batch axis, "shared" ones do not; "hom" parameters have a time
axis of 1 (or none), "het" ones of T.
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

assert pyro.__version__ == "1.9.1"

# name: (B, T, hidden, obs, batch layout, time layout, observation noise)
CASES = {
    "b3_t1_h2_o1": (3, 1, 2, 1, "batched", "hom", "mvn"),
    "b3_t7_h3_o2_shared": (3, 7, 3, 2, "shared", "hom", "mvn"),
    "b2_t9_h4_o3_het": (2, 9, 4, 3, "batched", "het", "mvn"),
    "b2_t33_h8_o5": (2, 33, 8, 5, "batched", "hom", "mvn"),
    "b2_t40_h16_o16": (2, 40, 16, 16, "batched", "hom", "mvn"),
    "b2_t17_h5_o16_het": (2, 17, 5, 16, "shared", "het", "mvn"),
    "b2_t12_h1_o1": (2, 12, 1, 1, "batched", "hom", "mvn"),
    # Independent(Normal) observation noise, a batch-shaped initial distribution over shared transitions
    "b3_t6_h3_o2_indep": (3, 6, 3, 2, "shared", "hom", "indep"),
}
NAMES = ("m0", "L0", "F", "q", "Lq", "H", "r", "Lr", "x")


def make_inputs(rng, B, T, h, o, lay, time, noise):
    lead = () if lay == "shared" else (B,)
    steps = (T,) if time == "het" else (() if lay == "shared" else (1,))
    pre = lead + steps

    def randn(*shape):
        return rng.standard_normal(shape)

    def tril(shape, n):
        A = randn(*(shape + (n, n)))
        cov = A @ np.swapaxes(A, -1, -2) / n + 0.5 * np.eye(n)
        return np.linalg.cholesky(cov)

    F = randn(*(pre + (h, h)))
    F = F * (0.9 / np.linalg.norm(F, ord=2, axis=(-2, -1)))[..., None, None]
    out = {"m0": 0.3 * randn(B, h), "L0": tril((B,), h), "F": F, "q": 0.3 * randn(*(pre + (h,))),
           "Lq": tril(pre, h), "H": randn(*(pre + (h, o))) / np.sqrt(h), "r": 0.3 * randn(*(pre + (o,))),
           "x": 2.0 * randn(B, T, o)}
    if noise == "indep":
        out["Lr"] = np.sqrt(np.abs(randn(*(pre + (o,)))) + 0.5)          # the Normal's scale
    else:
        out["Lr"] = tril(pre, o)
    return out


def build(t, noise):
    # (.tril(): the gradient stored for a scale_tril is the one of its lower triangle -- what autograd leaves in the
    # structurally zero upper triangle depends on how a library happens to use the matrix)
    init = dist.MultivariateNormal(t["m0"], scale_tril=t["L0"].tril())
    trans = dist.MultivariateNormal(t["q"], scale_tril=t["Lq"].tril())
    if noise == "indep":
        obs = dist.Normal(t["r"], t["Lr"]).to_event(1)
    else:
        obs = dist.MultivariateNormal(t["r"], scale_tril=t["Lr"].tril())
    return dist.GaussianHMM(init, t["F"], trans, t["H"], obs)


def main():
    rng = np.random.default_rng(20240917)
    flat = {}
    for name, (B, T, h, o, lay, time, noise) in CASES.items():
        arrays = make_inputs(rng, B, T, h, o, lay, time, noise)
        t = {k: torch.tensor(v, dtype=torch.float64, requires_grad=True) for k, v in arrays.items()}
        hmm = build(t, noise)
        assert hmm.batch_shape == (B,), (name, hmm.batch_shape)
        lp = hmm.log_prob(t["x"])
        grads = torch.autograd.grad(lp.sum(), [t[k] for k in NAMES])
        with torch.no_grad():
            post = build({k: v.detach() for k, v in t.items()}, noise).filter(t["x"].detach())
            fm = post.loc.expand(B, h)
            fP = post.covariance_matrix.expand(B, h, h)
        for k in NAMES:
            flat[name + "/" + k] = arrays[k]
        for k, g in zip(NAMES, grads):
            flat[name + "/g_" + k] = g.numpy()
        flat[name + "/log_prob"] = lp.detach().numpy()
        flat[name + "/filter_mean"] = fm.numpy()
        flat[name + "/filter_cov"] = fP.numpy()
        print(name, "log_prob", lp.detach().numpy())
    path = os.path.join(HERE, "gaussian_hmm.npz")
    np.savez_compressed(path, **flat)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
