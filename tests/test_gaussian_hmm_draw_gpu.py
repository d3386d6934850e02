"""csrc/gaussian_hmm_draw.hip on the device: the factors kernel (one wave per distinct covariance) and the draw kernel
(one lane per sample path), through kernels.gaussian_hmm_draw, the dispatcher op and GaussianHMM.rsample, against the
fixtures of the unmodified reference (tests/golden/gaussian_hmm_prior.npz, float64) and the float64 numpy restatement
of the three equations (tests/gaussian_hmm_prior_cases.restate).

One call per case carries, as its sample dimension, zero noise, the h + T (h + o) unit vectors and three seeded draws:
the first 1 + h + T (h + o) give the affine map (mean and linear part M) of x and of z, all of them are compared as
draws.  Errors are gaussian_hmm_cases.rel_err = max |got - want| / (1 + max |want|).

float64: 1e-12 (the existing fixtures agree with the reference at 1e-14 to 3e-15).

float32: the kernel orders its operations differently from torch, so it gets FOUR times the error of the float32 torch
route run on the CPU on the same float32 inputs and noise (the factor the sampler's tests use), per case and kind, with
a floor of 4 * 2^-23, four float32 roundings.  The torch route's error is measured when the test runs, never the
kernel's; the torch route's z is its x under an identity observation matrix without observation noise.

The eight cases reach all four instantiations of both kernels (<float | double, padded dimension 8 | 16>, the padding
chosen by max(hidden, obs)), h = o = 1, o > 8 with h <= 8, shared / per-series and time-homogeneous / per-step
parameters.
"""
import functools

import numpy as np
import pytest
import torch

import pyro_amd.distributions as dist
from pyro_amd import kernels
from pyro_amd.distributions import hmm
from tests import gaussian_hmm_cases as gc
from tests import gaussian_hmm_prior_cases as pr

pytestmark = pytest.mark.gpu
CPU = torch.device("cpu")
F32, F64 = torch.float32, torch.float64
SEEDED = 3


def _long_chain():
    """one series, T = 2000, hidden 4, obs 2, shared time-homogeneous parameters, F of spectral norm 0.9"""
    gen = torch.Generator().manual_seed(7)
    h, o = 4, 2
    r = lambda *s: torch.randn(*s, generator=gen, dtype=F64)                              # noqa: E731

    def cov(n):
        A = r(n, n)
        return A @ A.T / n + 0.5 * torch.eye(n, dtype=F64)
    F = r(h, h)
    F = F * (0.9 / torch.linalg.matrix_norm(F, ord=2))
    return (0.3 * r(1, h), cov(h)[None], F[None, None], 0.3 * r(1, 1, h), cov(h)[None, None],
            (r(h, o) / h ** 0.5)[None, None], 0.3 * r(1, 1, o), cov(o)[None, None])


LONG_T, LONG_S = 2000, 64


@functools.lru_cache(maxsize=None)
def _case(case):
    """(the eight parts in the layouts of kernels.gaussian_hmm_draw as float64 CPU tensors, T, the model for
    ``restate``, the noise triple as float64 CPU tensors, how many leading draws are the affine map's): made once,
    never modified"""
    if case == "long":
        parts, T = _long_chain(), LONG_T
        names = ("m0", "P0", "F", "q", "Q", "H", "r", "R")
        m = {k: np.broadcast_to(p.numpy(), (1, T) + tuple(p.shape[2:])) if p.dim() > 2 and k not in ("m0", "P0")
             else p.numpy() for k, p in zip(names, parts)}
        return parts, T, m, pr.seeded_noise(case, LONG_S, 1, T, 4, 2), 0
    t = gc.leaves(case, F64, CPU, requires_grad=False)
    d = gc.build(t, case, dist)
    B, T, o = t["x"].shape
    h = d.hidden_dim
    unit, seeded = pr.unit_noise(B, T, h, o), pr.seeded_noise(case, SEEDED, B, T, h, o)
    noise = tuple(torch.cat([u, s]) for u, s in zip(unit, seeded))
    return tuple(d._kernel_parts(d.batch_shape)), T, pr.model(case), noise, unit[0].shape[0]


@functools.lru_cache(maxsize=None)
def _want(case):
    """(x, z) of the float64 restatement for the case's noise"""
    _, _, m, noise, _ = _case(case)
    return pr.restate(m, *(e.numpy() for e in noise))


def _on(case, dtype, device):
    parts, T, _, noise, n_map = _case(case)
    return [p.to(dtype).to(device) for p in parts], T, [e.to(dtype).to(device) for e in noise], n_map


def _errors(case, x, z):
    wx, wz = _want(case)
    return {"x": gc.rel_err(x.detach().cpu().double().numpy(), wx), "z": gc.rel_err(z.detach().cpu().double().numpy(), wz)}


@functools.lru_cache(maxsize=None)
def _torch_f32_errors(case):
    """the float32 torch route on the CPU against the float64 restatement (measured once per case)"""
    parts, T, noise, _ = _on(case, F32, CPU)
    m0, P0, F, q, Q, H, r, R = parts
    S, B, h = noise[0].shape
    x = dist.GaussianHMM._from_parts(tuple(parts), T, None).rsample((S,), noise=noise)
    eye = torch.eye(h, dtype=F32)
    ident = (m0, P0, F, q, Q, eye[None, None], torch.zeros(1, 1, h), eye[None, None])
    z = dist.GaussianHMM._from_parts(ident, T, None).rsample((S,), noise=(noise[0], noise[1], torch.zeros_like(noise[1])))
    return _errors(case, x.reshape(S, B, T, -1), z.reshape(S, B, T, h))


def _fmt(err):
    return {k: "%.1e" % v for k, v in err.items()}


def _spy(monkeypatch):
    calls = []
    real = kernels.gaussian_hmm_draw

    def spy(*a, **kw):
        calls.append(kw)
        return real(*a, **kw)
    monkeypatch.setattr(kernels, "gaussian_hmm_draw", spy)
    return calls


@pytest.mark.parametrize("case", gc.CASES)
def test_fixtures_float64(case, gpu):
    parts, T, noise, n = _on(case, F64, gpu)
    x, z = kernels.gaussian_hmm_draw(*parts, T, *noise, need_states=True)
    g = pr.golden(case)
    err = {"z_" + k: v for k, v in pr.moment_errors(z[:n], g, "z_").items()}
    err.update({"x_" + k: v for k, v in pr.moment_errors(x[:n], g, "x_").items()})
    # the whole of M M^T of x, and Cov(z_t, x_t), against the restatement's
    wx, wz = _want(case)
    (_, Mx), (_, Mz), (_, Wx), (_, Wz) = pr.affine(x[:n]), pr.affine(z[:n]), pr.affine(wx[:n]), pr.affine(wz[:n])
    err["x_full_cov"] = gc.rel_err(Mx @ np.swapaxes(Mx, -1, -2), Wx @ np.swapaxes(Wx, -1, -2))
    err["cov_z_x"] = gc.rel_err(pr.blocks(Mz @ np.swapaxes(Mx, -1, -2), T)[0], pr.blocks(Wz @ np.swapaxes(Wx, -1, -2), T)[0])
    err.update(_errors(case, x, z))
    print(case, "f64 kernel", _fmt(err))
    assert max(err.values()) <= pr.TOL64, err
    # without the states: the same bits
    x2, none = kernels.gaussian_hmm_draw(*parts, T, *noise)
    assert none is None and torch.equal(x, x2)


@pytest.mark.parametrize("case", gc.CASES)
def test_fixtures_float32(case, gpu):
    base = _torch_f32_errors(case)
    parts, T, noise, _ = _on(case, F32, gpu)
    x, z = kernels.gaussian_hmm_draw(*parts, T, *noise, need_states=True)
    err = _errors(case, x, z)
    print(case, "f32 kernel", _fmt(err), "torch route on the CPU", _fmt(base))
    for kind in err:
        assert err[kind] <= max(4 * base[kind], pr.FLOOR32), (kind, err, base)


def test_long_stable_chain_float32(gpu):
    """one series, T = 2000, hidden 4, obs 2, S = 64 in float32 against the float64 restatement; the same bound"""
    base = _torch_f32_errors("long")
    parts, T, noise, _ = _on("long", F32, gpu)
    x, z = kernels.gaussian_hmm_draw(*parts, T, *noise, need_states=True)
    err = _errors("long", x, z)
    print("long chain: f32 kernel", _fmt(err), "torch route on the CPU", _fmt(base))
    assert x.shape == (LONG_S, 1, LONG_T, 2) and torch.isfinite(x).all() and torch.isfinite(z).all()
    for kind in err:
        assert err[kind] <= max(4 * base[kind], pr.FLOOR32), (kind, err, base)


@pytest.mark.parametrize("T", [1, 2, 3])
@pytest.mark.parametrize("dtype", [F32, F64])
def test_chunk_edges(T, dtype, gpu):
    """one lane per draw, 64 draws per block: a draw does not depend on S, on its lane or on the other series"""
    case = "b2_t9_h4_o3_het"
    parts, _, _, _ = _on(case, dtype, gpu)
    parts = parts[:2] + [p[:, :T].contiguous() for p in parts[2:]]         # per series, per step: the first T steps
    B, h, o = 2, 4, 3
    assert all(p.shape[0] == B for p in parts) and all(p.shape[1] == T for p in parts[2:])
    noise = [e.to(dtype).to(gpu) for e in pr.seeded_noise("edges", 130, B, T, h, o)]
    x130, z130 = kernels.gaussian_hmm_draw(*parts, T, *noise, need_states=True)
    m = {k: p.cpu().double().numpy() for k, p in zip(("m0", "P0", "F", "q", "Q", "H", "r", "R"), parts)}
    wx, wz = pr.restate(m, *(e.cpu().double().numpy() for e in noise))
    tol = pr.TOL64 if dtype == F64 else 1e-5
    assert gc.rel_err(x130.cpu().numpy(), wx) < tol and gc.rel_err(z130.cpu().numpy(), wz) < tol
    for S in (1, 63, 64, 65):
        x, z = kernels.gaussian_hmm_draw(*parts, T, *(e[:S].contiguous() for e in noise), need_states=True)
        assert x.shape == (S, B, T, o) and z.shape == (S, B, T, h), S
        assert torch.equal(x, x130[:S]) and torch.equal(z, z130[:S]), S
    for b in range(B):                                                     # series b alone
        x, z = kernels.gaussian_hmm_draw(*(p[b:b + 1].contiguous() for p in parts), T,
                                         *(e[:, b:b + 1].contiguous() for e in noise), need_states=True)
        assert torch.equal(x, x130[:, b:b + 1]) and torch.equal(z, z130[:, b:b + 1]), b
    # S = 0 and B = 0
    x0, z0 = kernels.gaussian_hmm_draw(*parts, T, *(e[:0].contiguous() for e in noise), need_states=True)
    assert x0.shape == (0, B, T, o) and z0.shape == (0, B, T, h)
    xe, _ = kernels.gaussian_hmm_draw(*(p[:0].contiguous() for p in parts), T, *(e[:5, :0].contiguous() for e in noise))
    assert xe.shape == (5, 0, T, o)


@pytest.mark.parametrize("dtype", [F32, F64])
def test_stride_zero_equals_expanded(dtype, gpu):
    """shared, time-homogeneous parameters passed with stride 0 (each covariance factored once) and the same values
    expanded per series and per step (factored B T times): identical bits"""
    parts, T, noise, _ = _on("b3_t7_h3_o2_shared", dtype, gpu)
    B = noise[0].shape[1]
    assert all(p.shape[0] == 1 and p.shape[1] == 1 for p in parts[2:])
    x0, z0 = kernels.gaussian_hmm_draw(*parts, T, *noise, need_states=True)
    wide = parts[:2] + [p.expand(B, T, *p.shape[2:]).contiguous() for p in parts[2:]]
    x1, z1 = kernels.gaussian_hmm_draw(*wide, T, *noise, need_states=True)
    assert torch.isfinite(x0).all() and torch.equal(x0, x1) and torch.equal(z0, z1)
    steps = parts[:2] + [p.expand(1, T, *p.shape[2:]).contiguous() for p in parts[2:]]     # shared, per step
    x2, z2 = kernels.gaussian_hmm_draw(*steps, T, *noise, need_states=True)
    assert torch.equal(x0, x2) and torch.equal(z0, z2)


@pytest.mark.parametrize("case", ["b2_t33_h8_o5", "b2_t17_h5_o16_het"])
@pytest.mark.parametrize("dtype", [F32, F64])
def test_reproducible(case, dtype, gpu):
    parts, T, noise, _ = _on(case, dtype, gpu)
    a = kernels.gaussian_hmm_draw(*parts, T, *noise, need_states=True)
    b = kernels.gaussian_hmm_draw(*parts, T, *noise, need_states=True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_a_bad_series_is_nan_and_alone(gpu):
    """one series of three with a Q that has a negative diagonal entry, then with one bad step of a per-step R: NaN
    x and z there, the other two bit for bit what a run without it gives"""
    parts, T, noise, _ = _on("b3_t7_h3_o2_shared", F32, gpu)
    m0, P0, F, q, Q, H, r, R = parts
    B = 3
    Q3 = Q.expand(B, 1, *Q.shape[2:]).contiguous()
    R3 = R.expand(B, T, *R.shape[2:]).contiguous()
    gx, gz = kernels.gaussian_hmm_draw(m0, P0, F, q, Q3, H, r, R3, T, *noise, need_states=True)
    assert torch.isfinite(gx).all() and torch.isfinite(gz).all()
    Qb = Q3.clone()
    Qb[1, 0, 1, 1] = -1.0
    Rb = R3.clone()
    Rb[1, T - 2, 0, 0] = -1.0
    for Qx, Rx in ((Qb, R3), (Q3, Rb)):
        bx, bz = kernels.gaussian_hmm_draw(m0, P0, F, q, Qx, H, r, Rx, T, *noise, need_states=True)
        assert torch.isnan(bx[:, 1]).all() and torch.isnan(bz[:, 1]).all()
        for b in (0, 2):
            assert torch.equal(gx[:, b], bx[:, b]) and torch.equal(gz[:, b], bz[:, b])
    # a bad parameter that every series shares: NaN everywhere
    Qs = Q.clone()
    Qs[0, 0, 0, 0] = -1.0
    sx, _ = kernels.gaussian_hmm_draw(m0, P0, F, q, Qs, H, r, R, T, *noise)
    assert torch.isnan(sx).all()


def test_over_the_dimension_limits(gpu, monkeypatch):
    z = lambda *s: torch.zeros(*s, device=gpu)                                            # noqa: E731
    eye = lambda n: torch.eye(n, device=gpu)                                              # noqa: E731
    for h, o in ((kernels.GAUSSIAN_HMM_MAX_HIDDEN + 1, 2), (2, kernels.GAUSSIAN_HMM_MAX_OBS + 1)):
        args = (z(1, h), eye(h)[None], 0.5 * eye(h)[None, None], z(1, 1, h), eye(h)[None, None],
                torch.ones(1, 1, h, o, device=gpu) / h, z(1, 1, o), eye(o)[None, None], 3, z(4, 2, h), z(4, 2, 3, h),
                z(4, 2, 3, o))
        with pytest.raises(kernels.Unsupported):
            kernels.gaussian_hmm_draw(*args)
        calls = _spy(monkeypatch)                     # the class takes its torch route
        d = dist.GaussianHMM(dist.MultivariateNormal(z(h), eye(h)), 0.5 * eye(h), dist.MultivariateNormal(z(h), eye(h)),
                             torch.ones(h, o, device=gpu) / h, dist.MultivariateNormal(z(o), eye(o)), duration=3)
        x = d.rsample((4,))
        assert x.shape == (4, 3, o) and torch.isfinite(x).all() and not calls
        monkeypatch.undo()


@pytest.mark.parametrize("case", ["b2_t9_h4_o3_het", "b2_t33_h8_o5"])
def test_forecast_float64(case, gpu, monkeypatch):
    """prefix_condition(data).rsample(noise=...) on the device: the filter's launch, then the two of the draw; its
    affine map against the reference's forecast moments pushed through H, R of the remaining steps"""
    calls = _spy(monkeypatch)
    t = gc.leaves(case, F64, gpu, requires_grad=False)
    d = gc.build(t, case, dist)
    B, T, o = t["x"].shape
    h, t0, f = d.hidden_dim, T // 2, T - T // 2
    if d.duration is None:
        d = dist.GaussianHMM._from_parts(d._parts, T, None)
    fc = d.prefix_condition(t["x"][:, :t0])
    noise = [e.to(gpu) for e in pr.unit_noise(B, f, h, o)]
    x = fc.rsample((noise[0].shape[0],), noise=noise)
    assert len(calls) == 1 and x.shape == (noise[0].shape[0], B, f, o)
    g = pr.golden(case)
    want = pr.push_through({k: g["fc_z_" + k] for k in ("mean", "cov", "cross")}, pr.model(case), t0)
    err = pr.moment_errors(x, want, "x_")
    print(case, "forecast f64 kernel against the reference", _fmt(err))
    assert max(err.values()) <= pr.TOL64, err


def test_routing(gpu, monkeypatch):
    case = "b2_t9_h4_o3_het"
    calls = _spy(monkeypatch)
    parts, T, noise, _ = _on(case, F64, gpu)
    noise = [e[-SEEDED:].contiguous() for e in noise]
    want = _want(case)[0][-SEEDED:]
    t = gc.leaves(case, F64, gpu, requires_grad=False)
    # nothing needs a gradient: one kernel call, a detached result
    x = gc.build(t, case, dist).rsample((SEEDED,), noise=noise)
    assert len(calls) == 1 and not x.requires_grad and x.shape == (SEEDED, 2, 9, 3)
    assert gc.rel_err(x.cpu().numpy(), want) <= pr.TOL64
    tg = gc.leaves(case, F64, gpu, requires_grad=True)
    with torch.no_grad():
        xn = gc.build(tg, case, dist).rsample((SEEDED,), noise=noise)
    assert len(calls) == 2 and not xn.requires_grad and torch.equal(x, xn)
    # a part requires a gradient: the loop, and backward reaches m0
    xg = gc.build(tg, case, dist).rsample((SEEDED,), noise=noise)
    assert len(calls) == 2 and xg.requires_grad
    xg.sum().backward()
    assert tg["m0"].grad is not None and tg["m0"].grad.abs().max() > 0
    assert gc.rel_err(xg.detach().cpu().numpy(), want) <= pr.TOL64                 # both routes, one noise
    # CPU tensors: the loop
    tc = gc.leaves(case, F64, CPU, requires_grad=False)
    xc = gc.build(tc, case, dist).rsample((SEEDED,), noise=[e.cpu() for e in noise])
    assert len(calls) == 2 and gc.rel_err(xc.numpy(), want) <= pr.TOL64
    # the switch: the loop on the device
    monkeypatch.setattr(hmm, "FUSED_GAUSSIAN_HMM", False)
    xs = gc.build(t, case, dist).rsample((SEEDED,), noise=noise)
    assert len(calls) == 2 and gc.rel_err(xs.cpu().numpy(), want) <= pr.TOL64
    monkeypatch.setattr(hmm, "FUSED_GAUSSIAN_HMM", True)
    # sample shapes and drawn noise, on the kernel: torch.manual_seed reproduces a call
    d = gc.build(t, case, dist)
    assert d.rsample().shape == (2, 9, 3) and len(calls) == 3
    torch.manual_seed(3)
    a = d.rsample((2, 5))
    torch.manual_seed(3)
    flat = torch.randn(10 * 2 * (4 + 9 * 7), dtype=F64, device=gpu)
    e0, ez, ex = flat.split([10 * 2 * 4, 10 * 2 * 9 * 4, 10 * 2 * 9 * 3])
    b = d.rsample((2, 5), noise=(e0.reshape(2, 5, 2, 4), ez.reshape(2, 5, 2, 9, 4), ex.reshape(2, 5, 2, 9, 3)))
    assert a.shape == (2, 5, 2, 9, 3) and torch.equal(a, b) and len(calls) == 5 and torch.isfinite(a).all()
    # a scalar batch shape
    one = dist.GaussianHMM._from_parts(tuple(p[0] for p in d._parts), 9, None)
    assert one.batch_shape == () and one.rsample((4,)).shape == (4, 9, 3) and len(calls) == 6


@pytest.mark.parametrize("case", ["b3_t7_h3_o2_shared", "b2_t17_h5_o16_het"])
@pytest.mark.parametrize("dtype", [F32, F64])
def test_dispatcher_op(case, dtype, gpu):
    from pyro_amd.ops import torch_library
    assert torch_library.available()
    parts, T, noise, _ = _on(case, dtype, gpu)
    x, z = kernels.gaussian_hmm_draw(*parts, T, *noise, need_states=True)
    x2, states = torch.ops.pyro_amd.gaussian_hmm_draw(*parts, T, *noise, True)
    assert torch.equal(x, x2) and len(states) == 1 and torch.equal(z, states[0])
    x3, none = torch.ops.pyro_amd.gaussian_hmm_draw(*parts, T, *noise, False)
    assert torch.equal(x, x3) and len(none) == 0
