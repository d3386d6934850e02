"""The composite covariance kernel (csrc/gp_compose.hip) per element on the device, f32 and f64, and the routing of
``Sum`` / ``Product`` onto it.

Truth: the composition as a plain float64 torch expression on the CPU -- direct differences, the reference's formula
per leaf -- on the inputs AS THE KERNEL SEES THEM (f32 inputs cast up); autograd gives gx and gz, a forward-mode Jacobian
of K the parameter gradients and the sums S of their absolute summands.  Bounds, the rule of tests/test_gp_kernel_gpu.py
and tests/test_gp_periodic_gpu.py with the union's width U for D (derivations, not measurements):
    f64  K, gx, gz          2^-52 * 16 (U + 8) * (1 + A) * F * P,   A the largest magnitude of that output
    f64  parameter sums     2^-52 (N M + 16 U) * S * F * P
    F the number of factors of the largest term (a product of F values carries F relative errors); P = 1 + C + 2 Theta
    where a Periodic factor is present, else 1: C = max_ij of the sum over the Periodic factors of ONE term of
    sum_k (2 / l_k^2) |theta sin 2 theta| (the sensitivities of log K add over the factors of a product), Theta = max |theta|
    f32  four times the error of the same expression in float32, floor 4 * 2^-23 (1 + A), or 4 * 2^-23 S"""
import math

import numpy as np
import pytest
import torch

from . import gp_cases as gc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = {"f32": torch.float32, "f64": torch.float64}


@pytest.fixture(scope="module")
def kernels():
    from pyro_amd import kernels as k
    return k


def _phi(kind, d, ls, aux):
    if kind == "periodic":
        return torch.exp(-2 * (torch.sin(math.pi * d / aux) / ls).pow(2).sum(-1))
    return gc.f_and_derivative(kind, (d / ls).pow(2).sum(-1), aux)[0]


def _K(spec, x, z, params):
    bias, terms = spec
    K, it = bias, iter(params)
    for coef, factors in terms:
        term = coef
        for kind, cols in factors:
            var, ls, aux = next(it)
            term = term * var * _phi(kind, x[:, None, list(cols)] - z[None, :, list(cols)], ls, aux)
        K = K + term
    return K


def _restate(spec, x, z, params, G):
    """name -> (value, S or None) in the dtype of the arguments; with z None gx carries both roles."""
    flat = [p for ps in params for p in ps if p is not None]
    x, zz = x.clone().requires_grad_(), None if z is None else z.clone().requires_grad_()

    def of(*ps):
        return _K(spec, x, x if zz is None else zz, _unflatten(params, ps))
    K = of(*flat)
    grads = torch.autograd.grad((K * G).sum(), [x] + ([] if zz is None else [zz]))
    out = {"K": (K.detach(), None), "gx": (grads[0], None), "gz": (None if zz is None else grads[1], None)}
    names = [(f, n) for f, ps in enumerate(params) for n, p in zip(("var", "ls", "aux"), ps) if p is not None]
    for i, (f, n) in enumerate(names):
        with torch.no_grad():      # one parameter at a time: [N, M, numel]
            summands = G[:, :, None] * torch.func.jacfwd(lambda p: of(*flat[:i], p, *flat[i + 1:]))(flat[i])
        out["%s%d" % (n, f)] = (summands.sum((0, 1)), summands.abs().sum((0, 1)))
    return out


def _unflatten(params, flat):
    it = iter(flat)
    return [tuple(None if p is None else next(it) for p in ps) for ps in params]


def _periodic_conditioning(spec, x, z, params):
    it, C, Theta = iter(params), 0.0, 0.0
    for _, factors in spec[1]:
        c = 0.0
        for kind, cols in factors:
            _, ls, aux = next(it)
            if kind == "periodic":
                theta = math.pi * (x[:, None, list(cols)] - z[None, :, list(cols)]) / aux
                c = c + ((2 / (ls * ls)) * (theta * torch.sin(2 * theta)).abs()).sum(-1)
                Theta = max(Theta, theta.abs().max().item())
        C = max(C, c.max().item() if torch.is_tensor(c) else 0.0)
    return 1 + C + 2 * Theta if Theta else 1.0


def _compare(got, spec, x, z, params, G, label=""):
    dtype, (N, U) = x.dtype, x.shape
    M = N if z is None else z.shape[0]
    up = lambda t: None if t is None else t.double()      # noqa: E731
    params64 = [tuple(up(p) for p in ps) for ps in params]
    truth = _restate(spec, up(x), up(z), params64, up(G))
    twin = _restate(spec, x, z, params, G) if dtype == torch.float32 else truth
    scale = max(len(fs) for _, fs in spec[1]) * _periodic_conditioning(spec, up(x), up(x if z is None else z), params64)
    worst = 0.0
    for name, value in got.items():
        t, S = truth[name]
        if t is None:
            assert value is None, (label, name)
            continue
        assert value.shape == t.shape and value.dtype == dtype and torch.isfinite(value).all(), (label, name)
        A, own = t.abs().max().item(), (twin[name][0].double() - t).abs()
        if dtype == torch.float64:
            bound = torch.as_tensor(gc.EPS64 * scale * (16 * (U + 8) * (1 + A) if S is None else (N * M + 16 * U) * S))
        else:
            bound = torch.maximum(4 * own, torch.as_tensor(4 * gc.EPS32 * ((1 + A) if S is None else S), dtype=torch.float64))
        err = (value.cpu().double() - t).abs()
        ratio = (err / bound.clamp(min=1e-300)).max().item()
        worst = max(worst, ratio)
        assert (err <= bound).all(), "%s %s N=%d M=%d U=%d: error / bound %.3g (error %.3g)" % (
            label, name, N, M, U, ratio, err.max().item())
    return worst


def _parameters(spec, seed, U, **fixed):
    """per factor (variance, lengthscale, aux): lengthscales in [0.5, 2] sqrt(U), periods in [0.7, 3], the rest in [0.5, 2]"""
    g, out = np.random.default_rng(3000 + seed), []
    t = lambda a: torch.as_tensor(a, dtype=torch.float64)      # noqa: E731
    for f, (kind, cols, ard_ls, ard_aux) in enumerate(spec):
        ls = t(g.uniform(0.5, 2.0, size=len(cols) if ard_ls else 1) * math.sqrt(U))
        aux = {"periodic": t(g.uniform(0.7, 3.0, size=len(cols) if ard_aux else 1)),
               "rational_quadratic": t(g.uniform(0.5, 2.0, size=1))}.get(kind)
        out.append((t(g.uniform(0.5, 2.0, size=1)), t([fixed["ls%d" % f]]) if "ls%d" % f in fixed else ls, aux))
    return out


ALL5, ALL64 = tuple(range(5)), tuple(range(64))
# name -> (U, bias, terms); a term (coef, factors), a factor (kind, cols, ARD lengthscale, ARD period)
COMPOSITIONS = {
    "rbf_periodic": (1, 0.0, ((1.0, (("rbf", (0,), False, False), ("periodic", (0,), False, False))),)),
    "matern_rbf_rq": (5, 0.0, ((1.0, (("matern32", ALL5, True, False), ("rbf", (1, 3), False, False))),
                               (1.0, (("rational_quadratic", ALL5, False, False),)))),
    "three_factors": (5, 0.3, ((0.7, (("exponential", (0, 2), False, False), ("matern52", ALL5, True, False),
                                      ("periodic", (4, 1), True, True))),
                               (2.0, (("rbf", ALL5, True, False),)), (1.0, (("rational_quadratic", (3,), False, False),)))),
    "full_width": (64, 0.0, ((1.0, (("periodic", ALL64, True, False), ("rbf", ALL64, False, False))),
                             (1.0, (("matern32", ALL64, True, False),)))),
}
# (N, M, z, forced_splits): the tile and split seams; z given, None, and the same tensor
SHAPES = [(1, 1, "null", 0), (63, 65, "given", 1), (65, 63, "given", 2), (130, 64, "given", 7), (65, 65, "same", 0),
          (130, 130, "null", 2)]


def _run(kernels, name, N, M, zmode, forced, dtype, seed=0, **fixed):
    U, bias, terms = COMPOSITIONS[name]
    spec = (bias, tuple((coef, tuple((kind, cols) for kind, cols, _, _ in fs)) for coef, fs in terms))
    params = [tuple(None if p is None else p.to(dtype) for p in ps)
              for ps in _parameters([f for _, fs in terms for f in fs], seed, U, **fixed)]
    x = gc.points(seed, N, U).to(dtype)
    z = None if zmode == "null" else (x if zmode == "same" else gc.points(seed + 50, M, U).to(dtype))
    if zmode == "given" and N >= 5 and M >= 6:
        z[5] = x[4]                                         # an exact duplicate off the diagonal
    G = torch.as_tensor(np.random.default_rng(seed + 7).standard_normal((N, N if z is None else M))).to(dtype)
    dev = lambda t: None if t is None else t.to(DEV)      # noqa: E731
    xd, pd = dev(x), [tuple(dev(p) for p in ps) for ps in params]
    zd = xd if zmode == "same" else dev(z)
    got = {"K": kernels.gp_compose_fwd(xd, zd, spec, pd)}
    got["gx"], got["gz"], grads = kernels.gp_compose_bwd(xd, zd, spec, pd, dev(G), None, forced)
    for f, gs in enumerate(grads):
        got.update({"%s%d" % (n, f): g for n, g, p in zip(("var", "ls", "aux"), gs, params[f]) if p is not None})
    return _compare(got, spec, x, z, params, G, "%s %s" % (name, (N, M, zmode, forced)))


@pytest.mark.parametrize("dt", sorted(DTYPES))
@pytest.mark.parametrize("name", sorted(COMPOSITIONS))
def test_per_element(kernels, name, dt):
    shapes = [SHAPES[2], SHAPES[4]] if name == "full_width" else SHAPES
    worst = max(_run(kernels, name, *shape, DTYPES[dt], seed=n) for n, shape in enumerate(shapes))
    print("%s %s: worst error / bound %.3f" % (name, dt, worst))


@pytest.mark.parametrize("dt", sorted(DTYPES))
def test_a_factor_that_underflows_to_zero(kernels, dt):
    """The first factor's lengthscale is 1e-3: its value is exactly 0 for every pair but the duplicates, and the weight of
    the OTHER factor of its term is that zero -- a product, never the term divided by a factor."""
    _run(kernels, "matern_rbf_rq", 40, 33, "given", 2, DTYPES[dt], ls0=1e-3)
    _run(kernels, "three_factors", 40, 40, "null", 0, DTYPES[dt], ls1=1e-3)


def _tree(gp, params, dtype):
    """Product(RBF ARD, Periodic on columns 0 and 2) + RationalQuadratic * 2.0 + 0.5, on the device"""
    k = gp.kernels
    one = lambda t: (t.clone() if t.numel() > 1 else t.reshape(()).clone()).to(dtype)      # noqa: E731
    (v0, l0, _), (v1, l1, p1), (v2, l2, a2) = params
    tree = k.Sum(k.Product(k.RBF(5, variance=one(v0), lengthscale=one(l0)),
                           k.Periodic(2, variance=one(v1), lengthscale=one(l1), period=one(p1), active_dims=[0, 2])),
                 k.Sum(k.Product(k.RationalQuadratic(5, variance=one(v2), lengthscale=one(l2), scale_mixture=one(a2)), 2.0), 0.5))
    return tree.to(DEV)


TREE = [("rbf", ALL5, True, False), ("periodic", (0, 2), False, True), ("rational_quadratic", ALL5, False, False)]
TREE_SPEC = (0.5, ((1.0, (("rbf", ALL5), ("periodic", (0, 2)))), (2.0, (("rational_quadratic", ALL5),))))


@pytest.mark.parametrize("dt", sorted(DTYPES))
def test_routing_of_sum_and_product(kernels, dt, monkeypatch):
    import pyro_amd.contrib.gp as gp
    dtype, calls = DTYPES[dt], []
    monkeypatch.setattr(gp.kernels, "FUSED_GP_COMPOSE", True)
    for name in ("gp_compose_fwd", "gp_compose_bwd", "gp_kernel_fwd", "gp_periodic_fwd"):
        real = getattr(kernels, name)
        monkeypatch.setattr(kernels, name, lambda *a, _real=real, _name=name, **k: calls.append(_name) or _real(*a, **k))
    params = _parameters(TREE, 0, 5)
    x, z = gc.points(0, 70, 5).to(dtype), gc.points(50, 33, 5).to(dtype)
    G = torch.as_tensor(np.random.default_rng(7).standard_normal((70, 33))).to(dtype)
    tree = _tree(gp, params, dtype)
    X, Z = x.to(DEV).requires_grad_(), z.to(DEV).requires_grad_()
    K = tree(X, Z)
    (K * G.to(DEV)).sum().backward()
    assert calls == ["gp_compose_fwd", "gp_compose_bwd"]
    rbf, per, rq = tree.kern0.kern0, tree.kern0.kern1, tree.kern1.kern0.kern0      # the parameters as the modules hold them
    pd = [tuple(None if p is None else p.detach().reshape(-1) for p in ps) for ps in (
        (rbf.variance, rbf.lengthscale, None), (per.variance, per.lengthscale, per.period),
        (rq.variance, rq.lengthscale, rq.scale_mixture))]
    direct = kernels.gp_compose_bwd(x.to(DEV), z.to(DEV), TREE_SPEC, pd, G.to(DEV))
    assert torch.equal(K.detach(), kernels.gp_compose_fwd(x.to(DEV), z.to(DEV), TREE_SPEC, pd))
    assert torch.equal(X.grad, direct[0]) and torch.equal(Z.grad, direct[1])
    assert tree.kern0.kern1.period_unconstrained.grad.shape == direct[2][1][2].shape
    del calls[:]
    # a Linear and a WhiteNoise term beside the tree: the tree still takes one launch, the result matches the truth
    if dtype == torch.float64:
        lin = gp.kernels.Linear(5, variance=torch.tensor(0.4, dtype=dtype)).to(DEV)
        both = gp.kernels.Sum(gp.kernels.Sum(tree, lin), gp.kernels.WhiteNoise(5, variance=torch.tensor(0.3, dtype=dtype)).to(DEV))
        X.grad = None
        Kb = both(X)
        Kb.sum().backward()
        assert calls == ["gp_compose_fwd", "gp_compose_bwd"]
        xr = x.clone().requires_grad_()
        want = _K(TREE_SPEC, xr, xr, params) + 0.4 * xr @ xr.t() + 0.3 * torch.eye(70, dtype=dtype)
        want.sum().backward()
        bound = gc.EPS64 * 16 * (5 + 8) * 2 * _periodic_conditioning(TREE_SPEC, x, x, params)
        assert ((Kb.detach().cpu() - want.detach()).abs() <= bound * (1 + want.abs().max())).all()
        assert ((X.grad.cpu() - xr.grad).abs() <= bound * (1 + xr.grad.abs().max())).all()
        del calls[:]
    # the switch off, CPU tensors, a batched lengthscale, a single leaf beside a WhiteNoise: no composite call
    monkeypatch.setattr(gp.kernels, "FUSED_GP_COMPOSE", False)
    off = tree(X, Z)
    monkeypatch.setattr(gp.kernels, "FUSED_GP_COMPOSE", True)
    assert "gp_compose_fwd" not in calls and (off - K).abs().max() <= 1e-4 * (1 + K.abs().max())
    _tree(gp, params, dtype).cpu()(x, z)
    k = gp.kernels
    k.Product(k.RBF(5, lengthscale=torch.ones(2, 5, dtype=dtype)), k.RBF(5, lengthscale=torch.ones(5, dtype=dtype))).to(DEV)(X[:2])
    k.Sum(k.RBF(5).to(DEV, dtype), k.WhiteNoise(5).to(DEV, dtype))(X)
    assert "gp_compose_fwd" not in calls
    del calls[:]
    assert tree(X, diag=True).shape == (70,) and calls == []


def test_peak_memory_stays_below_four_matrices(monkeypatch):
    import pyro_amd.contrib.gp as gp
    monkeypatch.setattr(gp.kernels, "FUSED_GP_COMPOSE", True)
    N = M = 512
    k, one = gp.kernels, torch.ones(16)
    kern = k.Sum(k.Product(k.RBF(16, lengthscale=4 * one), k.Periodic(16, lengthscale=4 * one, period=2 * one)),
                 k.Matern32(16, lengthscale=4 * one)).to(DEV)
    X, Z = gc.points(0, N, 16).float().to(DEV).requires_grad_(), gc.points(1, M, 16).float().to(DEV)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    kern(X, Z).sum().backward()
    torch.cuda.synchronize()
    assert X.grad is not None and kern.kern0.kern1.period_unconstrained.grad is not None
    assert torch.cuda.max_memory_allocated() - before < 4 * N * M * 4      # leaf by leaf: five matrices or more
