"""Generate tests/golden/gaussian_hmm_prior.npz from the UNMODIFIED reference (pyro-ppl/pyro 1.9.1): for every case
of tests/golden/gaussian_hmm.npz (whose inputs are read back; there are no new inputs) the moments of what
GaussianHMM.rsample draws -- the latent path, the observations -- and of the latent path of a forecast, float64 on the
CPU, with ``duration = T`` where the case is time-homogeneous.

    python tests/golden/make_golden_gaussian_hmm_prior.py

Latent path (z_mean [B, T, h], z_cov [B, T, h, h], z_cross [B, T - 1, h, h] = Cov(z_t, z_{t+1})): the reference's
rsample draws it with sequential_gaussian_filter_sample(hmm._init, trans, ...), ``trans`` built exactly as there.  The
sampler is affine in its noise: zeros give the mean, the (T + 1) h unit vectors the columns of the linear part A, and
the covariance of the path is A A^T.  The path is Markov, so its means, marginal covariances and lag-one
cross-covariances determine its law; only those are stored.

Observations (x_mean [B, T, o], x_cov [B, T, o, o], x_cross [B, T - 1, o, o] = Cov(x_t, x_{t+1})): from the
reference's own log_prob, whose gradient in x is affine, grad log p(x) = -Lambda (x - mu).  One batched call
evaluates it at 0 and at the T o unit vectors: g(0) = Lambda mu, g(e_k) - g(0) = -Lambda e_k; Lambda is inverted in
float64 and only the blocks of mu and Lambda^-1 are stored.

Forecast (fc_z_mean, fc_z_cov, fc_z_cross, cases with T >= 2): the latent recipe again for
hmm.prefix_condition(x[:, :T // 2]), a model of the remaining T - T // 2 steps.

Only the data file depends on the reference; the tests read nothing else of it.
"""
import functools
import os

import numpy as np
import torch

from make_golden_gaussian_hmm import CASES, HERE, NAMES, build  # (puts the reference on the path and imports it)

import pyro.distributions as dist  # noqa: E402
from pyro.ops.gaussian import sequential_gaussian_filter_sample  # noqa: E402


def build_with_duration(t, noise, T):
    """``build`` of the first fixture's script with ``duration=T`` handed to the reference's constructor (it is what
    tells a time-homogeneous model how long a draw is)"""
    real = dist.GaussianHMM
    dist.GaussianHMM = functools.partial(real, duration=T)
    try:
        return build(t, noise)
    finally:
        dist.GaussianHMM = real


def blocks(full, T):
    """(diagonal blocks [B, T, n, n], lag-one blocks [B, T - 1, n, n]) of ``full`` [B, T, n, T, n]"""
    B, n = full.shape[0], full.shape[2]
    diag = torch.stack([full[:, s, :, s, :] for s in range(T)], dim=1)
    cross = torch.stack([full[:, s, :, s + 1, :] for s in range(T - 1)], dim=1) if T > 1 \
        else torch.zeros(B, 0, n, n, dtype=torch.float64)
    return diag, cross


def latent_moments(hmm, B, T, h):
    """the moments of the latent path that ``hmm.rsample`` draws, ``trans`` as the reference's rsample builds it"""
    trans = hmm._trans + hmm._obs.marginalize(right=hmm.obs_dim).event_pad(left=hmm.hidden_dim)
    trans = trans.expand(trans.batch_shape[:-1] + (T,))
    zeros = torch.zeros(B, T + 1, h, dtype=torch.float64)
    mean = sequential_gaussian_filter_sample(hmm._init, trans, (), zeros)[..., 1:, :]
    n = (T + 1) * h
    unit = torch.eye(n, dtype=torch.float64).reshape(n, 1, T + 1, h).expand(n, B, T + 1, h)
    draws = sequential_gaussian_filter_sample(hmm._init, trans, (n,), unit)[..., 1:, :]
    A = (draws - mean).reshape(n, B, T * h).permute(1, 2, 0)
    cov, cross = blocks((A @ A.transpose(-1, -2)).reshape(B, T, h, T, h), T)
    return mean.expand(B, T, h), cov, cross


def observation_moments(hmm, B, T, o):
    """the moments of x under ``hmm.log_prob``"""
    n = T * o
    pts = torch.cat([torch.zeros(1, n, dtype=torch.float64), torch.eye(n, dtype=torch.float64)])
    pts = pts.reshape(n + 1, 1, T, o).expand(n + 1, B, T, o).clone().requires_grad_(True)
    with torch.enable_grad():
        g, = torch.autograd.grad(hmm.log_prob(pts).sum(), pts)
    g = g.reshape(n + 1, B, n)
    Lam = -(g[1:] - g[:1]).permute(1, 2, 0)                      # column k: Lambda e_k
    Lam = 0.5 * (Lam + Lam.transpose(-1, -2))
    Sigma = torch.linalg.inv(Lam)
    mu = (Sigma @ g[0].unsqueeze(-1)).squeeze(-1)
    cov, cross = blocks(Sigma.reshape(B, T, o, T, o), T)
    return mu.reshape(B, T, o), cov, cross


def main():
    flat = {}
    with np.load(os.path.join(HERE, "gaussian_hmm.npz")) as z:
        inputs = {name: {k: z[name + "/" + k] for k in NAMES} for name in CASES}
    for name, (B, T, h, o, _lay, _time, noise) in CASES.items():
        t = {k: torch.tensor(v, dtype=torch.float64) for k, v in inputs[name].items()}
        with torch.no_grad():
            hmm = build_with_duration(t, noise, T)
            assert hmm.batch_shape == (B,) and hmm.duration == T, (name, hmm.batch_shape, hmm.duration)
            out = dict(zip(("z_mean", "z_cov", "z_cross"), latent_moments(hmm, B, T, h)))
            out.update(zip(("x_mean", "x_cov", "x_cross"), observation_moments(hmm, B, T, o)))
            if T >= 2:
                fc = hmm.prefix_condition(t["x"][:, :T // 2])
                assert fc.duration == T - T // 2 and fc.batch_shape == (B,)
                out.update(zip(("fc_z_mean", "fc_z_cov", "fc_z_cross"), latent_moments(fc, B, T - T // 2, h)))
        for k, v in out.items():
            flat[name + "/" + k] = v.numpy()
        print(name, {k: tuple(v.shape) for k, v in out.items()})
    path = os.path.join(HERE, "gaussian_hmm_prior.npz")
    np.savez_compressed(path, **flat)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
