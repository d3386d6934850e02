"""Cases shared by the Periodic tests and by tests/golden/make_golden_gp_periodic.py: the float64 restatement of the
periodic covariance and its five gradients by the closed forms (the same code run in float32 is its twin), the
conditioning terms of a case, and the kernel and model tables of the reference fixture.

Everything that builds a kernel or a model takes the ``gp`` package as an argument, so that the same table runs on the
reference (the fixture's maker) and on this package (the tests).  The module imports nothing of the tests' package: the
maker loads it by its path."""
import math
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gp_periodic.npz")
MODES = [(al, ap) for al in (False, True) for ap in (False, True)]      # (ARD lengthscale, ARD period)


def restate(x, z, lengthscale, period, variance, G):
    """K and the five gradients given G = dL/dK, in the dtype of the arguments (CPU); with z None gx carries both
    roles.  ``S_*``: the sums of the absolute summands of the reduced gradients.  ``C`` = max_ij sum_k (2 / l_k^2)
    |theta sin 2 theta|, the first-order sensitivity of log K to a relative rounding of the angles; ``Theta`` = max |theta|."""
    both = z is None
    z = x if both else z
    D = x.shape[1]
    l, p, var = lengthscale.reshape(-1).expand(D), period.reshape(-1).expand(D), variance.reshape(())
    theta = math.pi * (x[:, None, :] - z[None, :, :]) / p                 # [N, M, D]
    s, s2t = torch.sin(theta), torch.sin(2 * theta)
    f = torch.exp(-2 * (s / l).pow(2).sum(-1))
    W = (G * var * f)[:, :, None]
    out = {"K": var * f}
    gx = -(2 * math.pi / (p * l * l)) * (W * s2t).sum(1)
    gz = (2 * math.pi / (p * l * l)) * (W * s2t).sum(0)
    out["gx"], out["gz"] = (gx + gz, None) if both else (gx, gz)
    terms = {"ls": (4 / l.pow(3)) * W * s * s, "period": (2 / (p * l * l)) * W * theta * s2t}
    for name, par in (("ls", lengthscale), ("period", period)):
        t = terms[name]
        if par.numel() == 1:
            out["g_" + name], out["S_" + name] = t.sum().reshape(1), t.abs().sum().reshape(1)
        else:
            out["g_" + name], out["S_" + name] = t.sum((0, 1)), t.abs().sum((0, 1))
    out["g_var"], out["S_var"] = (G * f).sum().reshape(1), (G * f).abs().sum().reshape(1)
    out["C"] = ((2 / (l * l)) * (theta * s2t).abs()).sum(-1).max().item() if theta.numel() else 0.0
    out["Theta"] = theta.abs().max().item() if theta.numel() else 0.0
    return out


def parameters(seed, D, ard_ls, ard_period, dtype=torch.float64):
    """lengthscales in [0.5, 2], periods in [0.7, 3], variance in [0.5, 2]"""
    g = np.random.default_rng(2000 + seed)
    ls = torch.as_tensor(g.uniform(0.5, 2.0, size=D if ard_ls else 1), dtype=dtype)
    period = torch.as_tensor(g.uniform(0.7, 3.0, size=D if ard_period else 1), dtype=dtype)
    return ls, period, torch.as_tensor(g.uniform(0.5, 2.0, size=1), dtype=dtype)


def build(gp, D, ls, period, var, active_dims=None):
    one = lambda t: t.clone() if t.numel() > 1 else t.reshape(()).clone()      # noqa: E731
    return gp.kernels.Periodic(D, variance=one(var), lengthscale=one(ls), period=one(period), active_dims=active_dims)


# ---- the fixture's tables (the data are gp_cases.fixture_data's: three features) -----------------------------------
def _t(*v, **kw):
    return torch.tensor(v if len(v) > 1 else v[0], dtype=kw.get("dtype", torch.float64), device=kw.get("device", "cpu"))


def product_kernel(gp, dtype=torch.float64, device="cpu"):
    t = lambda *v: _t(*v, dtype=dtype, device=device)      # noqa: E731
    k = gp.kernels
    return k.Product(k.Periodic(3, variance=t(1.2), lengthscale=t(0.9, 1.6, 0.7), period=t(2.3, 1.1, 2.9)),
                     k.RBF(3, variance=t(1.0), lengthscale=t(1.5)))


def kernel_table(gp):
    k = gp.kernels
    return {"scalar": k.Periodic(3, variance=_t(1.3), lengthscale=_t(0.8), period=_t(1.7)),
            "ard": k.Periodic(3, variance=_t(0.6), lengthscale=_t(0.5, 1.1, 1.9), period=_t(0.7, 2.2, 1.3)),
            "active": k.Periodic(2, variance=_t(1.1), lengthscale=_t(0.7, 1.4), period=_t(0.9), active_dims=[0, 2]),
            "product": product_kernel(gp)}


def build_model(gp, data, y=None, dtype=torch.float64, device="cpu"):
    c = lambda a: a.to(dtype=dtype, device=device)      # noqa: E731
    return gp.models.GPRegression(c(data["X"]), c(data["y"] if y is None else y), product_kernel(gp, dtype, device),
                                  noise=_t(0.2, dtype=dtype, device=device))


def check_model(gp, gc, elbo, device="cpu"):
    """GPRegression over Product(Periodic, RBF) in float64 against the fixture, within ten times its recorded sensitivity."""
    g = dict(np.load(GOLDEN))
    loss, grads = gc.loss_and_grads(build_model(gp, gc.fixture_data(), device=device), elbo)
    assert abs(loss - g["model/loss"]) <= gc.allowed(g["model/loss"], g["model/p_loss"])
    assert sorted(grads) == sorted(k[len("model/grad_"):] for k in g if k.startswith("model/grad_"))
    for name, got in grads.items():
        assert (np.abs(got - g["model/grad_" + name]) <= gc.allowed(g["model/grad_" + name], g["model/p_grad_" + name])).all(), name
