"""Cases shared by the Cosine / Brownian / Exponent / VerticalScaling / Warping tests and by
tests/golden/make_golden_gp_wrap.py: the kernel table of the reference fixture and what is recorded of each kernel.
Everything takes the ``gp`` package as an argument, so that the same table runs on the reference (the fixture's maker)
and on this package (the tests).  The module imports nothing of the tests' package: the maker loads it by its path."""
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gp_wrap.npz")
KERNELS = ("cosine", "cosine_ard", "brownian", "exponent_rbf", "warping_matern52", "warping_input_only", "vscaling_rbf",
           "vscaling_exponent_rbf", "vscaling_warping_rq", "exponent_exponent", "exponent_sum")


def weights(dtype=torch.float64, device="cpu"):
    """The Linear(3, 2)-style input warping (W, c) and the vertical scaling's v, as leaves."""
    g = np.random.default_rng(11)
    w = {"W": g.standard_normal((3, 2)) * 0.7, "c": g.standard_normal(2) * 0.3, "v": g.standard_normal(3) * 0.4}
    return {n: torch.as_tensor(a).to(dtype=dtype, device=device).requires_grad_() for n, a in w.items()}


def kernel_table(gp, w):
    """id -> kernel over the three features of gp_cases.fixture_data; ``w``: weights(), or the fixture's."""
    k = gp.kernels
    t = lambda *v: torch.tensor(v if len(v) > 1 else v[0], dtype=w["W"].dtype, device=w["W"].device)      # noqa: E731
    warp = lambda x: x @ w["W"] + w["c"]                        # noqa: E731
    scale = lambda x: 1.0 + 0.5 * torch.tanh(x @ w["v"])        # noqa: E731
    rbf = lambda: k.RBF(3, variance=t(0.8), lengthscale=t(0.9, 1.4, 0.7))      # noqa: E731
    return {
        "cosine": k.Cosine(3, variance=t(1.3), lengthscale=t(0.8)),
        "cosine_ard": k.Cosine(2, variance=t(0.6), lengthscale=t(0.5, 1.9), active_dims=[0, 2]),
        "brownian": k.Brownian(1, variance=t(0.7), active_dims=[1]),
        "exponent_rbf": k.Exponent(rbf()),
        "warping_matern52": k.Warping(k.Matern52(2, variance=t(1.1), lengthscale=t(1.2, 0.8)), warp, [1, 0, 2]),
        "warping_input_only": k.Warping(k.RBF(2, variance=t(1.2), lengthscale=t(1.5)), warp),
        "vscaling_rbf": k.VerticalScaling(rbf(), scale),
        "vscaling_exponent_rbf": k.VerticalScaling(k.Exponent(rbf()), scale),
        "vscaling_warping_rq": k.VerticalScaling(k.Warping(k.RationalQuadratic(
            3, variance=t(0.9), lengthscale=t(1.1), scale_mixture=t(0.7)), None, [0, 1, 0, 2]), scale),
        "exponent_exponent": k.Exponent(k.Exponent(k.RBF(3, variance=t(0.3), lengthscale=t(1.3)))),
        "exponent_sum": k.Exponent(k.Sum(k.RBF(3, variance=t(0.5), lengthscale=t(1.6)), k.Linear(3, variance=t(0.1)))),
    }


def record(kern, X, Z, w):
    """K(X), K(X, Z), the diagonal, and the gradients of sum(K(X) G) + sum(K(X, Z) H) for fixed G and H with respect to
    X, Z, every parameter of ``kern`` (by its name) and the weights, as numpy arrays."""
    g = np.random.default_rng(12)
    G, H = (torch.as_tensor(g.standard_normal(s)).to(X) for s in ((X.shape[0],) * 2, (X.shape[0], Z.shape[0])))
    X, Z = X.clone().requires_grad_(), Z.clone().requires_grad_()
    for p in list(kern.parameters()) + list(w.values()):
        p.grad = None
    K, KZ = kern(X), kern(X, Z)
    ((K * G).sum() + (KZ * H).sum()).backward()
    out = {"K": K, "KZ": KZ, "diag": kern(X, diag=True), "gX": X.grad, "gZ": Z.grad}
    out.update({"g_" + n: p.grad for n, p in kern.named_parameters()})
    out.update({"g_" + n: p.grad for n, p in w.items() if p.grad is not None})
    return {n: v.detach().cpu().numpy() for n, v in out.items()}
