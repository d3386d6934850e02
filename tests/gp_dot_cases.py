"""Cases shared by the Polynomial / Coregionalize tests and by tests/golden/make_golden_gp_dot.py: the kernel and model
tables of the reference fixture and what is recorded of each kernel.  Everything takes the ``gp`` package as an argument,
so that the same table runs on the reference (the fixture's maker) and on this package (the tests).  The module imports
nothing of the tests' package: the maker loads it by its path."""
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gp_dot.npz")


def _t(*v, **kw):
    return torch.tensor(v if len(v) > 1 else v[0], dtype=kw.get("dtype", torch.float64), device=kw.get("device", "cpu"))


def kernel_table(gp):
    """id -> kernel over the three features of gp_cases.fixture_data."""
    k = gp.kernels
    C = torch.as_tensor(np.random.default_rng(5).standard_normal((3, 3)) * 0.6)
    return {"poly1": k.Polynomial(3, variance=_t(1.3), bias=_t(0.7), degree=1),
            "poly2_active": k.Polynomial(2, variance=_t(0.6), bias=_t(1.4), degree=2, active_dims=[0, 2]),
            "poly3": k.Polynomial(3, variance=_t(0.9), bias=_t(0.5), degree=3),
            "coreg_low": k.Coregionalize(3, components=C[:, :2].clone(), diagonal=_t(0.4, 1.1, 0.8)),
            "coreg_full": k.Coregionalize(3, components=C.clone(), diagonal=_t(0.3, 0.6, 1.2))}


def record(kern, X, Z):
    """K(X), K(X, Z), the diagonal, and the gradients of K(X, Z).sum() + K(X).sum() with respect to X, Z and every
    parameter of ``kern`` (by its name), as numpy arrays."""
    X, Z = X.clone().requires_grad_(), Z.clone().requires_grad_()
    for p in kern.parameters():
        p.grad = None
    K, KZ = kern(X), kern(X, Z)
    (KZ.sum() + K.sum()).backward()
    out = {"K": K, "KZ": KZ, "diag": kern(X, diag=True), "gX": X.grad, "gZ": Z.grad}
    out.update({"g_" + n: p.grad for n, p in kern.named_parameters()})
    return {n: v.detach().cpu().numpy() for n, v in out.items()}


def build_model(gp, data, y=None, dtype=torch.float64, device="cpu"):
    """GPRegression over Sum(Polynomial(degree 2), WhiteNoise)."""
    t = lambda *v: _t(*v, dtype=dtype, device=device)      # noqa: E731
    c = lambda a: a.to(dtype=dtype, device=device)      # noqa: E731
    k = gp.kernels
    kernel = k.Sum(k.Polynomial(3, variance=t(0.8), bias=t(0.6), degree=2), k.WhiteNoise(3, variance=t(0.05)))
    return gp.models.GPRegression(c(data["X"]), c(data["y"] if y is None else y), kernel, noise=t(0.2))


def check_model(gp, gc, elbo, device="cpu"):
    """The model's loss in float64 against the fixture, within ten times its recorded sensitivity."""
    g = dict(np.load(GOLDEN))
    loss, grads = gc.loss_and_grads(build_model(gp, gc.fixture_data(), device=device), elbo)
    assert abs(loss - g["model/loss"]) <= gc.allowed(g["model/loss"], g["model/p_loss"])
    assert all(np.isfinite(v).all() for v in grads.values()) and len(grads) == 4
