"""The forward-draw fixtures of tests/golden/gaussian_hmm_prior.npz (made by
tests/golden/make_golden_gaussian_hmm_prior.py from the unmodified reference, float64) for the cases of
tests/gaussian_hmm_cases.py, and what the host and device tests of GaussianHMM.rsample share: the model of a case as
plain arrays, a float64 numpy restatement of the generative equations, and the affine map from noise to draws.
Loaded once, never modified."""
import os

import numpy as np
import torch

from tests import gaussian_hmm_cases as gc

_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gaussian_hmm_prior.npz")
_CACHE = {}
TOL64 = 1e-12        # the existing fixtures agree with the reference at 1e-14 to 3e-15: two orders of magnitude
FLOOR32 = 4 * 2.0 ** -23      # four float32 roundings


def golden(case):
    """{"z_mean" [B, T, h], "z_cov" [B, T, h, h], "z_cross" [B, T - 1, h, h] = Cov(z_t, z_{t+1}), "x_mean", "x_cov",
    "x_cross" likewise over obs, and for T >= 2 "fc_z_mean", "fc_z_cov", "fc_z_cross" of the forecast's T - T // 2
    latent states} of one case."""
    if not _CACHE:
        with np.load(_PATH) as z:
            for key in z.files:
                c, name = key.split("/")
                _CACHE.setdefault(c, {})[name] = z[key]
        for c in _CACHE.values():
            for a in c.values():
                a.setflags(write=False)
    return _CACHE[case]


def model(case):
    """The case's model as float64 numpy arrays expanded to every series and step: m0 [B, h], P0 [B, h, h],
    F, Q [B, T, h, h], q [B, T, h], H [B, T, h, o], r [B, T, o], R [B, T, o, o] -- the covariances formed from the
    fixture's scale factors here, not by the package."""
    g = gc.golden(case)
    B, T, o = g["x"].shape

    def full(a, nd):                       # no leading dims: shared and time-homogeneous; one: shared, per step
        a = a.reshape((1,) * (2 - (a.ndim - nd)) + a.shape)
        return np.broadcast_to(a, (B, T) + a.shape[2:])

    def cov(L):
        L = np.tril(L)
        return L @ np.swapaxes(L, -1, -2)
    if case.endswith("indep"):
        R = full(g["Lr"], 1)[..., None] * np.eye(o) * full(g["Lr"], 1)[..., None, :]
    else:
        R = full(cov(g["Lr"]), 2)
    return {"m0": g["m0"], "P0": cov(g["L0"]), "F": full(g["F"], 2), "q": full(g["q"], 1), "Q": full(cov(g["Lq"]), 2),
            "H": full(g["H"], 2), "r": full(g["r"], 1), "R": R}


def restate(m, eps0, eps_z, eps_x):
    """The three equations in float64 numpy for a model of ``model``'s layout (every parameter per series and per
    step) and noise [S, B, h], [S, B, T, h], [S, B, T, o]:
        z_0 = m0 + L_0 e_0,   z_t = z_{t-1} F_t + q_t + L_{Q,t} e_t,   x_t = z_t H_t + r_t + L_{R,t} e'_t
    -> (x [S, B, T, o], z [S, B, T, h])"""
    eps0, eps_z, eps_x = (np.asarray(e, dtype=np.float64) for e in (eps0, eps_z, eps_x))
    T = eps_z.shape[2]
    chol = np.linalg.cholesky
    z = m["m0"] + np.einsum("bij,sbj->sbi", chol(m["P0"]), eps0)
    xs, zs = [], []
    for t in range(T):
        z = np.einsum("sbi,bij->sbj", z, m["F"][:, t]) + m["q"][:, t] \
            + np.einsum("bij,sbj->sbi", chol(m["Q"][:, t]), eps_z[:, :, t])
        x = np.einsum("sbi,bij->sbj", z, m["H"][:, t]) + m["r"][:, t] \
            + np.einsum("bij,sbj->sbi", chol(m["R"][:, t]), eps_x[:, :, t])
        zs.append(z)
        xs.append(x)
    return np.stack(xs, axis=2), np.stack(zs, axis=2)


def unit_noise(B, T, h, o, dtype=torch.float64):
    """The noise of the affine map: n + 1 draws for n = h + T (h + o), the first with zero noise, draw 1 + k with the
    k-th unit vector of (e_0, e, e') in every series -> (eps0 [n + 1, B, h], eps_z [n + 1, B, T, h],
    eps_x [n + 1, B, T, o])"""
    n = h + T * (h + o)
    eye = torch.cat([torch.zeros(1, n, dtype=torch.float64), torch.eye(n, dtype=torch.float64)])
    e0, ez, ex = eye.split([h, T * h, T * o], dim=1)
    wide = lambda e, *tail: e.reshape(n + 1, 1, *tail).expand(n + 1, B, *tail).contiguous().to(dtype)   # noqa: E731
    return wide(e0, h), wide(ez, T, h), wide(ex, T, o)


def seeded_noise(case, S, B, T, h, o, dtype=torch.float64):
    """S draws of standard normal noise from a generator seeded by the case (float64 draws, then cast)"""
    seed = 2000 + gc.CASES.index(case) if case in gc.CASES else 1999
    gen = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64).to(dtype)        # noqa: E731
    return r(S, B, h), r(S, B, T, h), r(S, B, T, o)


def affine(y):
    """Draws ``y`` [n + 1, B, T, d] for ``unit_noise`` -> (the mean a [B, T, d], the linear part M [B, T d, n]) as
    float64 numpy arrays"""
    y = np.asarray(y.detach().cpu().double().numpy() if isinstance(y, torch.Tensor) else y, dtype=np.float64)
    n, B = y.shape[0] - 1, y.shape[1]
    return y[0], np.transpose((y[1:] - y[:1]).reshape(n, B, -1), (1, 2, 0))


def blocks(full, T):
    """(diagonal blocks [B, T, d, e], lag-one blocks [B, T - 1, d, e]) of ``full`` [B, T d, T e]"""
    B = full.shape[0]
    d, e = full.shape[1] // T, full.shape[2] // T
    full = full.reshape(B, T, d, T, e)
    diag = np.stack([full[:, s, :, s, :] for s in range(T)], axis=1)
    cross = np.stack([full[:, s, :, s + 1, :] for s in range(T - 1)], axis=1) if T > 1 else np.zeros((B, 0, d, e))
    return diag, cross


def moments(y):
    """{"mean", "cov", "cross"} of the affine map of the draws ``y`` for ``unit_noise``"""
    a, M = affine(y)
    cov, cross = blocks(M @ np.swapaxes(M, -1, -2), y.shape[2])
    return {"mean": a, "cov": cov, "cross": cross}


def moment_errors(y, want, prefix):
    """{kind: gc.rel_err of ``moments(y)`` against want[prefix + kind]}"""
    got = moments(y)
    return {k: gc.rel_err(got[k], want[prefix + k]) for k in ("mean", "cov", "cross")}


def push_through(zm, m, t0):
    """The moments of x_t = z_t H_t + r_t + N(0, R_t) over the steps t0.. of ``model`` ``m`` from those of the latent
    path ``zm`` = {"mean", "cov", "cross"} -> {"x_mean", "x_cov", "x_cross"}"""
    H, r, R = m["H"][:, t0:], m["r"][:, t0:], m["R"][:, t0:]
    Ht = np.swapaxes(H, -1, -2)
    return {"x_mean": np.einsum("bti,btij->btj", zm["mean"], H) + r, "x_cov": Ht @ zm["cov"] @ H + R,
            "x_cross": Ht[:, :-1] @ zm["cross"] @ H[:, 1:]}
