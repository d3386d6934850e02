"""The dot-product covariance kernel (csrc/gp_dot.hip) per element on the device, f32 and f64, and the routing of
gp.kernels.Polynomial / Coregionalize onto it.

Truth: the closed forms in float64 on the CPU, on the inputs AS THE KERNEL SEES THEM (f32 inputs cast up).  Bounds
(derived, not measured), with u = 2^-24 (f32) / 2^-53 (f64), m_ij = |bias| + sum_k |x_ik| |z_jk| and L = GP_DOT_FLUSH:
    K               u (D + 2 degree + 8) variance m_ij^degree
    a gradient      u (min(n, L) + D + 2 degree + 8) times the same sum over the absolute values of its terms, n the
                    number of terms summed in the tensor's dtype (the float64 finalize adds nothing visible)
both doubled in f64 for the truth's own rounding."""
import itertools

import numpy as np
import pytest
import torch

from pyro_amd import kernels

from . import gp_cases as gc
from . import gp_dot_cases as dc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = {"f32": torch.float32, "f64": torch.float64}
NAMES = ("gx", "gz", "g_var", "g_bias")
SHAPES = [(1, 1), (31, 33), (32, 32), (33, 65), (64, 64), (65, 31), (3, 5000), (5000, 3), (0, 5)]
DS, DEGREES = [1, 2, 3, 7, 8, 33, 64], [1, 2, 3, 5]


def _truth(x, z, var, bias, degree, G):
    """name -> (value, majorant, n) in float64; with z None gx carries both roles."""
    both, z = z is None, x if z is None else z
    var, b = (1.0 if var is None else var.item()), (0.0 if bias is None else bias.item())
    t, m = b + x @ z.T, abs(b) + x.abs() @ z.abs().T
    W, Wa = G * var * degree * t ** (degree - 1), G.abs() * var * degree * m ** (degree - 1)
    (N, D), M = x.shape, z.shape[0]
    out = {"K": (var * t ** degree, var * m ** degree, 0),
           "gx": (W @ z, Wa @ z.abs(), M), "gz": (W.T @ x, Wa.T @ x.abs(), N),
           "g_var": ((G * t ** degree).sum().reshape(1), (G.abs() * m ** degree).sum().reshape(1), N * M),
           "g_bias": (W.sum().reshape(1), Wa.sum().reshape(1), N * M)}
    if both:
        out["gx"] = (out["gx"][0] + out["gz"][0], out["gx"][1] + out["gz"][1], N + M)
    return out


def _compare(got, x, z, var, bias, degree, G, label=""):
    dtype, D = x.dtype, x.shape[1]
    up = lambda t: None if t is None else t.double()      # noqa: E731
    truth = _truth(up(x), up(z), up(var), up(bias), degree, up(G))
    u = 2.0 ** -24 if dtype == torch.float32 else 2.0 ** -52      # (f64: 2^-53 doubled)
    for name, value in got.items():
        if value is None:
            continue
        want, major, n = truth[name]
        assert value.shape == want.shape and value.dtype == dtype, (label, name)
        err, bound = (value.cpu().double() - want).abs(), u * (min(n, kernels.GP_DOT_FLUSH) + D + 2 * degree + 8) * major
        if err.numel():
            print("%s %s: worst error / bound %.3f" % (label, name, (err / bound.clamp(min=1e-300)).max().item()))
        assert (err <= bound).all(), (label, name, err.max().item())


def _inputs(N, M, D, dtype, seed=0, zmode="given", params=True):
    g = np.random.default_rng(seed)
    x = gc.points(seed, N, D).to(dtype)
    z = None if zmode == "null" else gc.points(seed + 50, M, D).to(dtype)
    var, bias = (torch.as_tensor(g.uniform(0.5, 2.0, size=1)).to(dtype) if params else None for _ in range(2))
    return x, z, var, bias, torch.as_tensor(g.standard_normal((N, N if z is None else M))).to(dtype)


def _check(N, M, D, dtype, degree, want=(True,) * 4, forced=0, **kw):
    x, z, var, bias, G = cpu = _inputs(N, M, D, dtype, **kw)
    xd, zd, vd, bd, Gd = (None if t is None else t.to(DEV) for t in cpu)
    got = {"K": kernels.gp_dot_fwd(xd, zd, vd, bd, degree)}
    for name, w, value in zip(NAMES, want, kernels.gp_dot_bwd(xd, zd, vd, bd, degree, Gd, want, forced)):
        assert (value is not None) == bool(w and (name != "gz" or z is not None) and (name in ("gx", "gz") or var is not None))
        got[name] = value
    again = kernels.gp_dot_bwd(xd, zd, vd, bd, degree, Gd, want, forced)
    assert all(a is None or torch.equal(a, v) for a, v in zip(again, [got[n] for n in NAMES])), "not bit-reproducible"
    _compare(got, x, z, var, bias, degree, G, str((N, M, D, degree, forced, kw)))


@pytest.mark.parametrize("dt", sorted(DTYPES))
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_tile_seams_pads_and_splits(shape, dt):
    for n, D in enumerate(DS):
        degree, forced = DEGREES[(n + sum(shape)) % 4], [0, 1, 2, 7][n % 4]
        _check(*shape, D, DTYPES[dt], degree, forced=forced, seed=n)
        if n % 2 == 0 and 0 < shape[0] <= 65:
            _check(shape[0], shape[0], D, DTYPES[dt], degree, forced=forced, seed=n, zmode="null")


@pytest.mark.parametrize("dt", sorted(DTYPES))
@pytest.mark.parametrize("degree", DEGREES)
def test_every_degree_at_both_blocks_of_gx_and_without_parameters(degree, dt):
    _check(70, 40, 64, DTYPES[dt], degree)
    _check(40, 70, 33, DTYPES[dt], degree, params=False)
    _check(130, 130, 5, DTYPES[dt], degree, zmode="null", forced=2)


@pytest.mark.parametrize("dt", sorted(DTYPES))
@pytest.mark.parametrize("zmode", ["given", "null"])
def test_every_combination_of_wanted_gradients(zmode, dt):
    for want in itertools.product([False, True], repeat=4):
        _check(65, 65, 33, DTYPES[dt], 3, want=want, forced=2, zmode=zmode)


@pytest.mark.parametrize("dt", sorted(DTYPES))
def test_columns_just_over_the_flush_length(dt):
    _check(40, kernels.GP_DOT_FLUSH + 70, 8, DTYPES[dt], 2, forced=1)


@pytest.mark.parametrize("dt", sorted(DTYPES))
def test_routing_of_the_classes(dt, monkeypatch):
    import pyro_amd as pyro
    import pyro_amd.contrib.gp as gp
    dtype, calls, k = DTYPES[dt], [], gp.kernels
    real_fwd, real_bwd = kernels.gp_dot_fwd, kernels.gp_dot_bwd
    monkeypatch.setattr(kernels, "gp_dot_fwd", lambda *a, **kw: calls.append("fwd") or real_fwd(*a, **kw))
    monkeypatch.setattr(kernels, "gp_dot_bwd", lambda *a, **kw: calls.append("bwd") or real_bwd(*a, **kw))
    wide = gc.points(0, 70, 7).to(dtype)
    X, Z = wide[:, ::2], gc.points(1, 33, 4).to(dtype)
    t = lambda *v: torch.tensor(v if len(v) > 1 else v[0], dtype=dtype)      # noqa: E731
    C = torch.as_tensor(np.random.default_rng(3).standard_normal((3, 2))).to(dtype)
    make = {"poly": lambda: k.Polynomial(3, variance=t(1.3), bias=t(0.7), degree=3, active_dims=[0, 1, 3]),
            "coreg": lambda: k.Coregionalize(3, components=C.clone(), diagonal=t(0.4, 1.1, 0.8), active_dims=[0, 1, 3])}

    def run(kid, device, fused):
        pyro.clear_param_store()
        monkeypatch.setattr(k, "FUSED_GP_DOT", fused)
        kern = make[kid]().to(device)
        return kern, dc.record(kern, X.to(device), Z.to(device))

    for kid in make:
        del calls[:]
        kern, fused = run(kid, DEV, True)
        assert calls == ["fwd", "fwd", "bwd", "bwd"], calls          # K(X), K(X, Z): one launch each; diag none
        want = run(kid, "cpu", False)[1]
        off = run(kid, DEV, False)[1]
        assert calls == ["fwd", "fwd", "bwd", "bwd"]
        tol = 1e-4 if dtype == torch.float32 else 1e-11
        for name in want:
            scale = 1 + np.abs(want[name]).max()
            assert np.abs(fused[name] - want[name]).max() <= tol * scale, (kid, name)
            assert np.abs(off[name] - want[name]).max() <= tol * scale, (kid, name)
    # the diagonal is updated in place before the backward: K is recomputed, not saved
    monkeypatch.setattr(k, "FUSED_GP_DOT", True)
    kern, Xd = make["poly"]().to(DEV), wide.to(DEV)[:, ::2].detach().requires_grad_()      # (not contiguous)
    K = kern(Xd)
    K.view(-1)[::71] += 5.0
    K.pow(2).sum().backward()
    Xc = X.clone().requires_grad_()
    Kc = make["poly"]()(Xc) + 5.0 * torch.eye(70, dtype=dtype)
    Kc.pow(2).sum().backward()
    assert (Xd.grad.cpu() - Xc.grad).abs().max() <= (1e-3 if dtype == torch.float32 else 1e-10) * Xc.grad.abs().max()
    # over the caps: the torch route, silently
    del calls[:]
    pyro.clear_param_store()
    k.Polynomial(65).to(DEV, dtype)(torch.zeros(3, 65, device=DEV, dtype=dtype))
    k.Polynomial(3, degree=17).to(DEV, dtype)(Xd[:, :3])
    k.Coregionalize(33, rank=32).to(DEV, dtype)(torch.zeros(3, 33, device=DEV, dtype=dtype))
    assert calls == []
    for D, degree in ((65, 1), (3, 17)):      # the launcher itself refuses them
        with pytest.raises(kernels.Unsupported):
            real_fwd(torch.zeros(4, D, device=DEV), None, None, None, degree)


def test_regression_over_sum_polynomial_whitenoise_within_the_reference_sensitivity(monkeypatch):
    import pyro_amd as pyro
    import pyro_amd.contrib.gp as gp
    from pyro_amd.infer import Trace_ELBO
    pyro.clear_param_store()
    monkeypatch.setattr(gp.kernels, "FUSED_GP_DOT", True)
    dc.check_model(gp, gc, Trace_ELBO(), DEV)


def test_fake_of_the_dispatcher_op():
    import pyro_amd.contrib.gp as gp
    from pyro_amd.ops import torch_library as tl
    from torch._subclasses.fake_tensor import FakeTensorMode
    x, z, var, bias, _ = (t.to(DEV) for t in _inputs(9, 6, 4, torch.float64))
    sid, tensors = tl._spec_of("gp_dot", gp.kernels._DotCovariance, (x, z, var, bias, 3))
    with FakeTensorMode() as mode:
        out = torch.ops.pyro_amd.fn_gp_dot([mode.from_tensor(t) for t in tensors], sid)
    assert tuple(out[0].shape) == (9, 6) and out[0].dtype == torch.float64
