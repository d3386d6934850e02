"""Generate tests/golden/gaussian_hmm_posterior.npz from the UNMODIFIED reference (pyro-ppl/pyro 1.9.1): for every
case of tests/golden/gaussian_hmm.npz (whose inputs are read back; there are no new inputs) the moments of the
posterior of the latent path z_1..z_T given x that GaussianHMM.rsample_posterior draws from, float64 on the CPU.

    python tests/golden/make_golden_gaussian_hmm_posterior.py

The reference's sampler is affine in its noise: with ``trans`` as rsample_posterior builds it,

    mean [B, T, h] = sequential_gaussian_filter_sample(init, trans, (), zeros)[..., 1:, :]

and the draws for the n = (T + 1) h unit vectors as noise, minus the mean, are the columns of the linear part A
[B, T h, n]; the covariance of the path is A A^T.  A Markov Gaussian is determined by its means, its marginal
covariances and its lag-one cross-covariances, so only those are stored:

    cov   [B, T, h, h]       the diagonal blocks
    cross [B, T - 1, h, h]   cross[t] = Cov(z_t, z_{t+1})

Only the data file depends on the reference; the tests read nothing else of it.
"""
import os

import numpy as np
import torch

from make_golden_gaussian_hmm import CASES, HERE, NAMES, build  # (puts the reference on the path and imports it)

from pyro.ops.gaussian import sequential_gaussian_filter_sample  # noqa: E402


def main():
    flat = {}
    with np.load(os.path.join(HERE, "gaussian_hmm.npz")) as z:
        inputs = {name: {k: z[name + "/" + k] for k in NAMES} for name in CASES}
    for name, (B, T, h, _o, _lay, _time, noise) in CASES.items():
        t = {k: torch.tensor(v, dtype=torch.float64) for k, v in inputs[name].items()}
        with torch.no_grad():
            hmm = build(t, noise)
            assert hmm.batch_shape == (B,), (name, hmm.batch_shape)
            trans = hmm._trans + hmm._obs.condition(t["x"]).event_pad(left=h)
            trans = trans.expand(trans.batch_shape)
            zeros = torch.zeros(B, T + 1, h, dtype=torch.float64)
            mean = sequential_gaussian_filter_sample(hmm._init, trans, (), zeros)[..., 1:, :]
            n = (T + 1) * h
            unit = torch.eye(n, dtype=torch.float64).reshape(n, 1, T + 1, h).expand(n, B, T + 1, h)
            draws = sequential_gaussian_filter_sample(hmm._init, trans, (n,), unit)[..., 1:, :]
            A = (draws - mean).reshape(n, B, T * h).permute(1, 2, 0)
            full = (A @ A.transpose(-1, -2)).reshape(B, T, h, T, h)
            cov = torch.stack([full[:, s, :, s, :] for s in range(T)], dim=1)
            cross = torch.stack([full[:, s, :, s + 1, :] for s in range(T - 1)], dim=1) if T > 1 \
                else torch.zeros(B, 0, h, h, dtype=torch.float64)
        flat[name + "/mean"] = mean.numpy()
        flat[name + "/cov"] = cov.numpy()
        flat[name + "/cross"] = cross.numpy()
        print(name, "mean", tuple(mean.shape), "cov", tuple(cov.shape), "cross", tuple(cross.shape))
    path = os.path.join(HERE, "gaussian_hmm_posterior.npz")
    np.savez_compressed(path, **flat)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
