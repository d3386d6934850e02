"""Cases shared by the Gaussian-process tests and by tests/golden/make_golden_gp.py: the float64 restatement of the
stationary covariance kernels by DIRECT DIFFERENCES (and its float32 twin: the same code in another dtype), the kernel
and model tables of the reference fixture, and the bounds.

Everything that builds a kernel or a model takes the ``gp`` package as an argument, so that the same table runs on the
reference (the fixture's maker) and on this package (the tests)."""
import math
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "gp.npz")
FAMILIES = ("rbf", "rational_quadratic", "exponential", "matern32", "matern52")
CLASS_OF = {"rbf": "RBF", "rational_quadratic": "RationalQuadratic", "exponential": "Exponential",
            "matern32": "Matern32", "matern52": "Matern52"}
EPS64, EPS32 = 2.0 ** -52, 2.0 ** -23
_golden = {}


def golden():
    if "g" not in _golden:
        _golden["g"] = dict(np.load(GOLDEN))
    return _golden["g"]


# ---- the restatement ---------------------------------------------------------------------------------------------------
def f_and_derivative(family, r2, alpha=None):
    """(f(r2), df/d(r2), df/d(alpha) or None), r = sqrt(r2 + 1e-12): the reference's guard is part of the function."""
    r = (r2 + 1e-12).sqrt()
    if family == "rbf":
        f = torch.exp(-0.5 * r2)
        return f, -0.5 * f, None
    if family == "rational_quadratic":
        u = r2 / (2 * alpha)
        f = torch.exp(-alpha * torch.log1p(u))
        return f, -0.5 * f / (1 + u), f * (u / (1 + u) - torch.log1p(u))
    if family == "exponential":
        f = torch.exp(-r)
        return f, -0.5 * f / r, None
    if family == "matern32":
        e = torch.exp(-math.sqrt(3.0) * r)
        return (1 + math.sqrt(3.0) * r) * e, -1.5 * e, None
    if family == "matern52":
        e = torch.exp(-math.sqrt(5.0) * r)
        return (1 + math.sqrt(5.0) * r + (5.0 / 3.0) * r2) * e, e * (-5.0 / 6.0 - (5.0 * math.sqrt(5.0) / 6.0) * r2 / r), None
    raise ValueError(family)


def scaled_differences(x, z, lengthscale):
    """d [N, M, D] = (x_i - z_j) / l, the difference first."""
    return (x[:, None, :] - z[None, :, :]) / lengthscale.reshape(-1)


def restate_K(family, x, z, lengthscale, variance, alpha=None):
    z = x if z is None else z
    r2 = scaled_differences(x, z, lengthscale).pow(2).sum(-1)
    return variance.reshape(()) * f_and_derivative(family, r2, None if alpha is None else alpha.reshape(()))[0]


def restate(family, x, z, lengthscale, variance, alpha, G):
    """K and the five gradients given G = dL/dK, in the dtype of the arguments (CPU), by the closed forms; with z None
    gX carries both roles.  ``S_*``: the sums of the absolute summands of the reduced gradients."""
    both = z is None
    z = x if both else z
    l = lengthscale.reshape(-1)
    var = variance.reshape(())
    a = None if alpha is None else alpha.reshape(())
    d = scaled_differences(x, z, l)
    r2 = d.pow(2).sum(-1)
    f, df, da = f_and_derivative(family, r2, a)
    W = G * var * df
    out = {"K": var * f}
    gx = (2.0 / l) * (W[:, :, None] * d).sum(1)
    gz = -(2.0 / l) * (W[:, :, None] * d).sum(0)
    out["gx"], out["gz"] = (gx + gz, None) if both else (gx, gz)
    terms = -(2.0 / l) * W[:, :, None] * d.pow(2)                     # [N, M, D]
    if l.numel() == 1:
        out["g_ls"], out["S_ls"] = terms.sum().reshape(1), terms.sum(-1).abs().sum().reshape(1)
    else:
        out["g_ls"], out["S_ls"] = terms.sum((0, 1)), terms.abs().sum((0, 1))
    out["g_var"], out["S_var"] = (G * f).sum().reshape(1), (G * f).abs().sum().reshape(1)
    if da is not None:
        out["g_alpha"], out["S_alpha"] = (var * G * da).sum().reshape(1), (var * G * da).abs().sum().reshape(1)
    else:
        out["g_alpha"] = out["S_alpha"] = None
    return out


def conditioning_bound(family, x, z, lengthscale, variance, alpha=None):
    """Per entry: how far the float64 EXPANSION r2 = X2 - 2 X Z^T + Z2 may lie from the restatement, to first order:
    2^-52 (D + 8) (|x / l|^2 + |z / l|^2) |variance f'(r2)| + 1e-15."""
    z = x if z is None else z
    l = lengthscale.reshape(-1)
    D = x.shape[1]
    r2 = scaled_differences(x, z, l).pow(2).sum(-1)
    df = f_and_derivative(family, r2, None if alpha is None else alpha.reshape(()))[1]
    norms = (x / l).pow(2).sum(-1)[:, None] + (z / l).pow(2).sum(-1)[None, :]
    return EPS64 * (D + 8) * norms * (variance.reshape(()) * df).abs() + 1e-15


def points(seed, n, D, shift=0.0, near=True, dtype=torch.float64):
    """n points ~ N(0, 1) + shift; with ``near`` (n >= 4) point 1 duplicates point 0 and point 3 lies 1e-4 from 2."""
    g = np.random.default_rng(seed)
    x = g.standard_normal((n, D))
    if near and n >= 4:
        x[1] = x[0]
        x[3] = x[2] + 1e-4 * g.standard_normal(D) / math.sqrt(D)
    return torch.as_tensor(x + shift, dtype=dtype)


def parameters(seed, D, ard, family, dtype=torch.float64):
    g = np.random.default_rng(1000 + seed)
    ls = torch.as_tensor(g.uniform(0.5, 2.0, size=D if ard else 1), dtype=dtype)
    var = torch.as_tensor(g.uniform(0.5, 2.0, size=1), dtype=dtype)
    alpha = torch.as_tensor(g.uniform(0.5, 2.0, size=1), dtype=dtype) if family == "rational_quadratic" else None
    return ls, var, alpha


def build_stationary(gp, family, D, ls, var, alpha, active_dims=None):
    cls = getattr(gp.kernels, CLASS_OF[family])
    kwargs = {"variance": var.reshape(()).clone(), "lengthscale": ls.clone() if ls.numel() > 1 else ls.reshape(()).clone()}
    if alpha is not None:
        kwargs["scale_mixture"] = alpha.reshape(()).clone()
    return cls(D, active_dims=active_dims, **kwargs)


# ---- the fixture's tables ------------------------------------------------------------------------------------------
N_FIX, D_FIX, M_FIX, U_FIX = 30, 3, 7, 5


def fixture_data():
    g = np.random.default_rng(2024)
    X = g.standard_normal((N_FIX, D_FIX))
    X[1] = X[0] + 1e-4
    y = np.sin(X[:, 0]) + 0.5 * X[:, 1] + 0.1 * g.standard_normal(N_FIX)
    t = lambda a: torch.as_tensor(a, dtype=torch.float64)      # noqa: E731
    return {"X": t(X), "y": t(y), "Xnew": t(g.standard_normal((M_FIX, D_FIX))), "Xu": t(X[::6][:U_FIX].copy() + 0.05),
            "f_loc": t(g.standard_normal((2, N_FIX))), "f_scale_tril": t(np.tril(g.standard_normal((2, N_FIX, N_FIX))) * 0.3)}


def _t(*v):
    return torch.tensor(v if len(v) > 1 else v[0], dtype=torch.float64)


def kernel_table(gp):
    """id -> kernel over D_FIX features."""
    k = gp.kernels
    table = {}
    for family in FAMILIES:
        extra = {"scale_mixture": _t(0.7)} if family == "rational_quadratic" else {}
        cls = getattr(k, CLASS_OF[family])
        table[family + "_scalar"] = cls(D_FIX, variance=_t(1.3), lengthscale=_t(0.8), **extra)
        table[family + "_ard"] = cls(D_FIX, variance=_t(0.6), lengthscale=_t(0.5, 1.1, 1.9), **extra)
    table["rbf_active"] = k.RBF(2, variance=_t(1.1), lengthscale=_t(0.7, 1.4), active_dims=[0, 2])
    table["constant"] = k.Constant(D_FIX, variance=_t(0.4))
    table["whitenoise"] = k.WhiteNoise(D_FIX, variance=_t(0.3))
    table["linear"] = k.Linear(D_FIX, variance=_t(0.9))
    table["sum_rbf_white"] = k.Sum(k.RBF(D_FIX, lengthscale=_t(1.2)), k.WhiteNoise(D_FIX, variance=_t(0.2)))
    table["sum_matern_number"] = k.Sum(k.Matern32(D_FIX, lengthscale=_t(0.9)), 0.5)
    table["product_matern_rbf_active"] = k.Product(k.Matern32(D_FIX, lengthscale=_t(1.5)),
                                                   k.RBF(1, lengthscale=_t(0.6), active_dims=[1]))
    table["product_of_sum_number"] = k.Product(k.Sum(k.RBF(D_FIX, variance=_t(0.5)), k.Linear(D_FIX, variance=_t(0.1))), 2.0)
    return table


CONDITIONAL_CASES = [(s, w, c) for s in (False, True) for w in (False, True) for c in (False, True)]
MODELS = ("gpr", "sgpr_DTC", "sgpr_FITC", "sgpr_VFE")
FORWARD_CASES = [(c, n) for c in (False, True) for n in (False, True)]
TRAIN_STEPS = 10
LENGTHSCALE_AT = (0.9, 1.2, 0.7)          # where the lengthscale's latent is fixed under the LogNormal prior


def model_kernel(gp, dtype=torch.float64, device="cpu", which="rbf"):
    t = lambda *v: torch.tensor(v if len(v) > 1 else v[0], dtype=dtype, device=device)      # noqa: E731
    k = gp.kernels
    if which == "rbf":
        return k.RBF(D_FIX, variance=t(1.3), lengthscale=t(0.8, 1.3, 0.6))
    if which == "sum":
        return k.Sum(k.RBF(D_FIX, variance=t(1.3), lengthscale=t(0.8, 1.3, 0.6)), k.WhiteNoise(D_FIX, variance=t(0.05)))
    if which == "product":
        return k.Product(k.Matern32(D_FIX, variance=t(1.1), lengthscale=t(1.4)),
                         k.RBF(2, lengthscale=t(0.9, 1.7), active_dims=[0, 2]))
    raise ValueError(which)


def build_model(gp, name, data, prior=None, dtype=torch.float64, device="cpu", which="rbf", y=None):
    """``prior``: (PyroSample, dist) puts LogNormal(0, 1) on the lengthscale and fixes its latent at LENGTHSCALE_AT."""
    c = lambda a: a.to(dtype=dtype, device=device)      # noqa: E731
    kernel = model_kernel(gp, dtype, device, which)
    X, y = c(data["X"]), c(data["y"] if y is None else y)
    noise = torch.tensor(0.2, dtype=dtype, device=device)
    if name == "gpr":
        model = gp.models.GPRegression(X, y, kernel, noise=noise)
    else:
        model = gp.models.SparseGPRegression(X, y, kernel, c(data["Xu"]).clone(), noise=noise, approx=name.split("_")[1])
    if prior is not None:
        PyroSample, dist = prior
        zero, one = torch.zeros(D_FIX, dtype=dtype, device=device), torch.ones(D_FIX, dtype=dtype, device=device)
        torch.manual_seed(0)
        model.kernel.lengthscale = PyroSample(dist.LogNormal(zero, one).to_event())
        leaf = dict(model.named_parameters())["kernel.lengthscale_map_unconstrained"]
        leaf.data = torch.tensor(LENGTHSCALE_AT, dtype=dtype, device=device).log()
    return model


def loss_and_grads(model, elbo):
    for p in model.parameters():
        p.grad = None
    loss = elbo.differentiable_loss(model.model, model.guide)
    loss.backward()
    grads = {n: p.grad.detach().cpu().numpy().copy() for n, p in model.named_parameters() if p.grad is not None}
    return float(loss.detach()), grads


def perturbed_y(data):
    g = np.random.default_rng(7)
    return data["y"] * (1 + 1e-13 * torch.as_tensor(g.choice([-1.0, 1.0], size=N_FIX)))


def perturbed_inputs(data):
    """X, Xnew, f_loc and f_scale_tril perturbed by 1e-13 relative (the sensitivity of ``conditional``)."""
    g = np.random.default_rng(8)
    return {k: data[k] * (1 + 1e-13 * torch.as_tensor(g.choice([-1.0, 1.0], size=tuple(data[k].shape))))
            for k in ("X", "Xnew", "f_loc", "f_scale_tril")}


def allowed(want, perturbed):
    """Ten times the deviation the reference shows against itself under the 1e-13 perturbation of y, entry by entry;
    where that rounds to zero in an entry, the largest deviation of the same array stands in (the rule of
    tests/test_forecast_host.py)."""
    want = np.asarray(want, dtype=np.float64)
    own = np.abs(want - np.asarray(perturbed))
    # (a lone scalar has no array to borrow from: one spacing of float64 at its own magnitude is the least a
    # different order of the same additions can cost)
    return np.maximum(np.maximum(10 * own, own.max()), np.spacing(np.abs(want)))
