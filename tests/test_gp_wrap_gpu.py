"""The wrapped covariance kernel (csrc/gp_wrap.hip) per element on the device, f32 and f64, and the routing of
gp.kernels.Cosine / Exponent / Warping / VerticalScaling onto it.

Truth: K = a_i q(k0_ij) b_j and its gradients by the closed forms in float64 on the CPU, on the inputs AS THE KERNEL
SEES THEM (f32 inputs cast up).  k0 = variance f(r2) and everything that flows through it are gp_cases.restate's, run on
G' = G a b q'(k0); q, a, b and their derivatives are applied to it here.  Bounds (derived, not measured), with u the
spacing of the dtype (2^-23 / 2^-52) and "the rule" that of tests/test_gp_kernel_gpu.py -- f64 2^-52 16 (D + 8) (1 + A),
f32 four times the error of the float32 twin of the restatement with floor 4 u (1 + A), A the largest magnitude:
    K                        the rule's bound of k0 times |a_i b_j q'(k0_ij)| (first-order amplification through q)
                             plus u |K_ij| for the transform's own rounding
    gX, gZ, g_a, g_b         the rule, on the output itself
    lengthscale / variance / alpha gradients    f64 2^-52 (N M + 16 D) S, f32 the twin's error times four with floor
                             4 u S, S the sum of the absolute summands
<f64, polynomial, scaled> is not built (its backward does not fit the registers): the launcher raises Unsupported."""
import itertools

import numpy as np
import pytest
import torch

from pyro_amd import kernels

from . import gp_cases as gc
from . import gp_wrap_cases as wc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = {"f32": torch.float32, "f64": torch.float64}
QS = {"identity": None, "exp": "exp", "poly": (0, 1, 0, 2)}
NAMES = ("gx", "gz", "g_ls", "g_var", "g_alpha", "g_a", "g_b")
SUMS = {"g_ls": "S_ls", "g_var": "S_var", "g_alpha": "S_alpha"}
SHAPES = [(1, 1, 1, 0), (63, 65, 5, 0), (65, 63, 8, 2), (130, 64, 64, 0), (3, 5000, 3, 0), (3, 5000, 3, 7), (0, 5, 3, 0)]
_stationary = gc.f_and_derivative


def _f_and_derivative(family, r2, alpha=None):
    if family != "cosine":
        return _stationary(family, r2, alpha)
    r = (r2 + 1e-12).sqrt()
    return torch.cos(r), -0.5 * torch.sin(r) / r, None


@pytest.fixture(autouse=True)
def cosine_in_the_restatement(monkeypatch):
    monkeypatch.setattr(gc, "f_and_derivative", _f_and_derivative)


def _q(q, k0):
    if q is None:
        return k0, torch.ones_like(k0)
    if q == "exp":
        return k0.exp(), k0.exp()
    return (sum(c * k0 ** n for n, c in enumerate(q)), sum(n * c * k0 ** (n - 1) for n, c in enumerate(q) if n))


def _restate(family, x, z, ls, var, al, G, q, a, b):
    """The outputs in the dtype of the arguments, and (k0, dK / dk0); with z None gx and g_a carry both roles."""
    k0 = gc.restate(family, x, z, ls, var, al, G)["K"]
    qv, dq = _q(q, k0)
    ai = torch.ones_like(k0[:, 0]) if a is None else a
    bj = ai if z is None else (torch.ones_like(k0[0]) if b is None else b)
    e = ai[:, None] * bj[None, :] * dq
    out = gc.restate(family, x, z, ls, var, al, G * e)
    out["K"] = ai[:, None] * qv * bj[None, :]
    ga, gb = (G * qv * bj[None, :]).sum(1), (G * qv * ai[:, None]).sum(0)
    out["g_a"], out["g_b"] = (None, None) if a is None else ((ga + gb, None) if z is None else (ga, gb))
    return out, k0, e


def _rule(truth, twin, S, N, M, D, dtype):
    A = truth.abs().max().item()
    if dtype == torch.float64:
        return torch.full_like(truth, gc.EPS64 * 16 * (D + 8) * (1 + A)) if S is None else gc.EPS64 * (N * M + 16 * D) * S
    floor = 4 * gc.EPS32 * (1 + A) if S is None else 4 * gc.EPS32 * S
    return torch.maximum(4 * (twin.double() - truth).abs(), floor + torch.zeros_like(truth))


def _inputs(family, N, M, D, dtype, scaling, seed=0):
    g = np.random.default_rng(seed + 7)
    x = gc.points(seed, N, D).to(dtype)
    z = None if scaling == "shared" else gc.points(seed + 50, M, D).to(dtype)
    ls, var, al = (None if t is None else t.to(dtype) for t in gc.parameters(seed, D, seed % 2 == 1, family))
    cols = N if z is None else M
    a = None if scaling == "none" else torch.as_tensor(g.uniform(0.5, 1.5, N) * g.choice([-1.0, 1.0], N)).to(dtype)
    b = torch.as_tensor(g.uniform(0.5, 1.5, cols)).to(dtype) if scaling == "given" else None
    return x, z, ls, var, al, torch.as_tensor(g.standard_normal((N, cols))).to(dtype), a, b


def _check(family, N, M, D, dtype, q, scaling, forced=0, wants=((True,) * 7,), seed=0):
    x, z, ls, var, al, G, a, b = cpu = _inputs(family, N, M, D, dtype, scaling, seed)
    dx, dz, dls, dvar, dal, dG, da, db = (None if t is None else t.to(DEV) for t in cpu)
    if isinstance(q, tuple) and a is not None and dtype == torch.float64:
        with pytest.raises(kernels.Unsupported):
            kernels.gp_wrap_fwd(dx, dz, dls, dvar, dal, family, q, da, db)
        return 0.0
    K = kernels.gp_wrap_fwd(dx, dz, dls, dvar, dal, family, q, da, db)
    cols = N if z is None else M
    if N == 0 or cols == 0:
        grads = kernels.gp_wrap_bwd(dx, dz, dls, dvar, dal, dG, family, q, da, db)
        assert K.shape == (N, cols) and all(g is None or not g.any() for g in grads)
        return 0.0
    truth, k0, e = _restate(family, *(None if t is None else t.double() for t in cpu[:6]), q,
                            *(None if t is None else t.double() for t in (a, b)))
    twin, k0_twin, _ = _restate(family, x, z, ls, var, al, G, q, a, b) if dtype == torch.float32 else (truth, k0, e)
    u = gc.EPS32 if dtype == torch.float32 else gc.EPS64
    bounds = {"K": _rule(k0, k0_twin, None, N, cols, D, dtype) * e.abs() + u * truth["K"].abs()}
    for name in NAMES:
        if truth[name] is not None:
            bounds[name] = _rule(truth[name], twin[name], truth[SUMS[name]] if name in SUMS else None, N, cols, D, dtype)
    worst = 0.0
    for want in wants:
        got = dict(zip(NAMES, kernels.gp_wrap_bwd(dx, dz, dls, dvar, dal, dG, family, q, da, db, want, forced)), K=K)
        for name, value in got.items():
            if name != "K" and not (want[NAMES.index(name)] and truth[name] is not None):
                assert value is None, (name, want)
                continue
            assert value.shape == truth[name].shape and value.dtype == dtype and torch.isfinite(value).all(), name
            err = (value.cpu().double() - truth[name]).abs()
            ratio = (err / bounds[name].clamp(min=1e-300)).max().item()
            worst = max(worst, ratio)
            assert ratio <= 1, "%s %s %s %s N=%d M=%d D=%d want=%s: error / bound %.3g (error %.3g)" % (
                family, q, scaling, name, N, cols, D, want, ratio, err.max().item())
    return worst


CASES = [(dt, q, s, "cosine") for dt in sorted(DTYPES) for q in QS for s in ("none", "given", "shared")]
CASES += [("f64", "exp", "shared", "matern52"), ("f32", "poly", "given", "rational_quadratic")]


@pytest.mark.parametrize("dt,q,scaling,family", CASES)
def test_tile_seams_pads_and_splits(dt, q, scaling, family):
    worst = 0.0
    for n, (N, M, D, forced) in enumerate(SHAPES):
        if scaling == "shared" and M > 1000:
            N = 300                                       # (z = x: five column tiles under the same splits)
        worst = max(worst, _check(family, N, M, D, DTYPES[dt], QS[q], scaling, forced, seed=n))
    print("%s %s %s %s: worst error / bound %.3f" % (family, dt, q, scaling, worst))


@pytest.mark.parametrize("dt,scaling", [("f32", "given"), ("f64", "given"), ("f32", "shared"), ("f64", "shared")])
def test_every_combination_of_wanted_gradients(dt, scaling):
    free = [0, 1, 2, 3, 4, 5, 6] if scaling == "given" else [0, 2, 3, 4, 5]
    wants = [tuple(i in free and bits[free.index(i)] for i in range(7))
             for bits in itertools.product([False, True], repeat=len(free))]
    _check("rational_quadratic", 65, 65, 33, DTYPES[dt], "exp", scaling, forced=2, wants=wants, seed=1)


@pytest.mark.parametrize("dt", sorted(DTYPES))
def test_two_backward_calls_are_bit_equal(dt):
    x, z, ls, var, al, G, a, b = (t.to(DEV) for t in _inputs("rational_quadratic", 300, 130, 7, DTYPES[dt], "given", 1))
    first = kernels.gp_wrap_bwd(x, z, ls, var, al, G, "rational_quadratic", "exp", a, b)
    again = kernels.gp_wrap_bwd(x, z, ls, var, al, G, "rational_quadratic", "exp", a, b)
    assert all(torch.equal(f, s) for f, s in zip(first, again))


def test_routing_of_the_classes(monkeypatch):
    import pyro_amd as pyro
    import pyro_amd.contrib.gp as gp
    k, calls, dtype = gp.kernels, [], torch.float64
    real_fwd, real_bwd = kernels.gp_wrap_fwd, kernels.gp_wrap_bwd
    monkeypatch.setattr(kernels, "gp_wrap_fwd", lambda *a, **kw: calls.append("fwd") or real_fwd(*a, **kw))
    monkeypatch.setattr(kernels, "gp_wrap_bwd", lambda *a, **kw: calls.append("bwd") or real_bwd(*a, **kw))
    X, Z = gc.points(0, 70, 3), gc.points(1, 33, 3)
    fused_ids = ("cosine", "cosine_ard", "exponent_rbf", "warping_matern52", "vscaling_rbf", "vscaling_exponent_rbf")

    def run(kid, device, fused):
        pyro.clear_param_store()
        monkeypatch.setattr(k, "FUSED_GP_WRAP", fused)
        w = wc.weights(dtype, device)
        kern = wc.kernel_table(gp, w)[kid].to(device)
        return wc.record(kern, X.to(device), Z.to(device), w)

    for kid in wc.KERNELS:
        del calls[:]
        fused = run(kid, DEV, True)
        # K(X), K(X, Z): one launch each and one backward pass each; the diagonal none
        assert calls == (["fwd", "fwd", "bwd", "bwd"] if kid in fused_ids else []), (kid, calls)
        del calls[:]
        want, off = run(kid, "cpu", False), run(kid, DEV, False)
        assert calls == [], kid
        for name in want:
            scale = 1e-10 * (1 + np.abs(want[name]).max())
            assert np.abs(fused[name] - want[name]).max() <= scale and np.abs(off[name] - want[name]).max() <= scale, (kid, name)
    # nine coefficients: the torch route, silently; the launcher itself refuses them and D = 65
    monkeypatch.setattr(k, "FUSED_GP_WRAP", True)
    del calls[:]
    rbf = k.RBF(3).to(DEV, dtype)
    k.Warping(rbf, owarping_coef=[1] * 9)(X.to(DEV))
    assert calls == []
    one = torch.ones(1, device=DEV)
    for D, q in ((3, (1,) * 9), (65, "exp")):
        with pytest.raises(kernels.Unsupported):
            real_fwd(torch.zeros(4, D, device=DEV), None, one, one, None, "rbf", q)
    # the diagonal is updated in place before the backward: K is recomputed, not saved
    Xd, Xc = X.to(DEV).requires_grad_(), X.clone().requires_grad_()
    K = k.Exponent(rbf)(Xd)
    K.view(-1)[::71] += 5.0
    K.pow(2).sum().backward()
    assert calls == ["fwd", "bwd"]
    (k.Exponent(k.RBF(3).to(dtype=dtype))(Xc) + 5.0 * torch.eye(70, dtype=dtype)).pow(2).sum().backward()
    assert (Xd.grad.cpu() - Xc.grad).abs().max() <= 1e-10 * Xc.grad.abs().max()


def test_fake_of_the_dispatcher_op():
    import pyro_amd.contrib.gp as gp
    from pyro_amd.ops import torch_library as tl
    from torch._subclasses.fake_tensor import FakeTensorMode
    x, z, ls, var, al, _, a, b = (None if t is None else t.to(DEV) for t in _inputs("cosine", 9, 6, 4, torch.float64, "given"))
    sid, tensors = tl._spec_of("gp_wrap", gp.kernels._WrappedCovariance, (x, z, ls, var, al, a, b, "cosine", "exp"))
    with FakeTensorMode() as mode:
        out = torch.ops.pyro_amd.fn_gp_wrap([mode.from_tensor(t) for t in tensors], sid)
    assert tuple(out[0].shape) == (9, 6) and out[0].dtype == torch.float64
