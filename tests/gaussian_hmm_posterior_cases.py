"""The posterior-path fixtures of tests/golden/gaussian_hmm_posterior.npz (made by
tests/golden/make_golden_gaussian_hmm_posterior.py from the unmodified reference, float64) for the cases of
tests/gaussian_hmm_cases.py, and what the host and device tests of rsample_posterior share: loaded once, never
modified."""
import os

import numpy as np
import torch

from tests import gaussian_hmm_cases as gc

KINDS = ("mean", "cov", "cross")
_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gaussian_hmm_posterior.npz")
_CACHE = {}


def golden(case):
    """{"mean" [B, T, h], "cov" [B, T, h, h], "cross" [B, T - 1, h, h] = Cov(z_t, z_{t+1})} of one case."""
    if not _CACHE:
        with np.load(_PATH) as z:
            for key in z.files:
                c, name = key.split("/")
                _CACHE.setdefault(c, {})[name] = z[key]
        for c in _CACHE.values():
            for a in c.values():
                a.setflags(write=False)
    return _CACHE[case]


def moments(c, G, L):
    """The moments of the chain z_T = c_T + L_T eps_T, z_t = c_t + G_t z_{t+1} + L_t eps_t rebuilt from its maps
    (tensors [B, T, ...] of any dtype and device; the recursion runs in float64 on the CPU):
        mu_T = c_T, V_T = L_T L_T^T;  mu_t = c_t + G_t mu_{t+1};  V_t = G_t V_{t+1} G_t^T + L_t L_t^T;
        X_t = Cov(z_t, z_{t+1}) = G_t V_{t+1}
    -> {"mean", "cov", "cross"} as float64 numpy arrays."""
    c, G, L = (v.detach().cpu().double() for v in (c, G, L))
    T = c.shape[1]
    mu, V = c[:, T - 1], L[:, T - 1] @ L[:, T - 1].transpose(-1, -2)
    mus, Vs, Xs = [mu], [V], []
    for t in range(T - 2, -1, -1):
        Xs.append(G[:, t] @ V)
        mu = c[:, t] + (G[:, t] @ mu.unsqueeze(-1)).squeeze(-1)
        V = G[:, t] @ V @ G[:, t].transpose(-1, -2) + L[:, t] @ L[:, t].transpose(-1, -2)
        mus.append(mu)
        Vs.append(V)
    h = c.shape[-1]
    cross = torch.stack(Xs[::-1], dim=1) if Xs else torch.zeros(c.shape[0], 0, h, h, dtype=torch.float64)
    return {"mean": torch.stack(mus[::-1], dim=1).numpy(), "cov": torch.stack(Vs[::-1], dim=1).numpy(),
            "cross": cross.numpy()}


def moment_errors(c, G, L, case):
    """{kind: gc.rel_err of the moments rebuilt from the maps against the fixture}"""
    got, want = moments(c, G, L), golden(case)
    return {k: gc.rel_err(got[k], want[k]) for k in KINDS}


def fixed_noise(case, S, dtype=torch.float64):
    """[S, B, T, h] standard normal from a generator seeded by the case (float64 draws, then cast)"""
    g = gc.golden(case)
    B, T = g["x"].shape[:2]
    seed = 1000 + gc.CASES.index(case) if case in gc.CASES else 999
    gen = torch.Generator().manual_seed(seed)
    return torch.randn(S, B, T, g["m0"].shape[-1], generator=gen, dtype=torch.float64).to(dtype)
