"""csrc/gaussian_hmm_sample.hip on the device: the maps kernel (Kalman filter, then the backward sweep that writes the
maps (c, G, L) of the path's posterior) and the paths kernel (one lane per draw), through
kernels.gaussian_hmm_sample and through GaussianHMM.rsample_posterior, against the fixtures of the unmodified
reference (tests/golden/gaussian_hmm_posterior.npz, float64) and the float64 torch route of distributions/hmm.py.

Kinds of error, each gaussian_hmm_cases.rel_err = max |got - want| / (1 + max |want|): the path's ``mean``, marginal
``cov`` and lag-one ``cross`` covariances rebuilt from the kernel's maps (gaussian_hmm_posterior_cases.moments)
against the fixture, and the ``draws`` for a fixed eps (S = 3, a generator seeded per case) against the float64
torch route on the CPU with the same eps.

float64: 1e-9, the project's golden tolerance.

float32: the kernel orders its operations differently from torch, so it gets FOUR times the error of the float32
torch route run on the CPU on the same float32 inputs and eps, per case and kind.  The torch route's error is
measured when the test runs (never the kernel's); on the machine the fixtures were made on it was

    case                        mean       cov        cross      draws
    b3_t1_h2_o1                 5.4e-08    6.9e-08    -          7.0e-08
    b3_t7_h3_o2_shared          1.1e-07    1.6e-07    6.0e-08    2.5e-07
    b2_t9_h4_o3_het             1.5e-07    1.8e-07    2.5e-07    1.9e-07
    b2_t33_h8_o5                1.8e-07    1.3e-07    1.8e-07    1.9e-07
    b2_t40_h16_o16              2.9e-07    2.8e-07    1.2e-07    2.7e-07
    b2_t17_h5_o16_het           2.7e-07    3.2e-07    6.2e-08    3.3e-07
    b2_t12_h1_o1                1.6e-07    1.2e-07    1.1e-07    1.7e-07
    b3_t6_h3_o2_indep           1.8e-07    1.6e-07    1.5e-07    1.7e-07
    long chain (T = 2000)       2.6e-07    2.4e-07    2.4e-07    2.4e-07
    near-singular Q             9.5e-05    1.5e-05    4.9e-06    1.4e-04

The eight cases reach all four instantiations of both kernels (<float | double, padded dimension 8 | 16>; the maps
kernel pads to max(hidden, obs), the paths kernel to hidden), padded and unpadded dimensions, shared / per-series
and time-homogeneous / per-step parameters.
"""
import functools

import numpy as np
import pytest
import torch

import pyro_amd.distributions as dist
from pyro_amd import kernels
from pyro_amd.distributions import hmm
from tests import gaussian_hmm_cases as gc
from tests import gaussian_hmm_posterior_cases as pc

pytestmark = pytest.mark.gpu
TOL64 = 1e-9
CPU = torch.device("cpu")
F32, F64 = torch.float32, torch.float64
KINDS = pc.KINDS + ("draws",)


# ---- the extra cases: no fixture, the float64 torch route on the CPU is the target --------------------------------
def _long_chain():
    """B = 2, T = 2000, hidden 4, obs 2: the recipe of test_gaussian_hmm_gpu.py's long chain"""
    gen = torch.Generator().manual_seed(7)
    B, T, h, o = 2, 2000, 4, 2
    r = lambda *s: torch.randn(*s, generator=gen, dtype=F64)                              # noqa: E731

    def tril(n):
        A = r(B, 1, n, n)
        return torch.linalg.cholesky(A @ A.transpose(-1, -2) / n + 0.5 * torch.eye(n, dtype=F64))
    F = r(B, 1, h, h)
    F = F * (0.9 / torch.linalg.matrix_norm(F, ord=2))[..., None, None]
    return {"m0": 0.3 * r(B, h), "L0": tril(h)[:, 0], "F": F, "q": 0.3 * r(B, 1, h), "Lq": tril(h),
            "H": r(B, 1, h, o) / h ** 0.5, "r": 0.3 * r(B, 1, o), "Lr": tril(o), "x": 2.0 * r(B, T, o)}


NEAR_SINGULAR_Q_SCALE = 1e-8


def _near_singular():
    """The fixtures' recipe (tests/golden/make_golden_gaussian_hmm.py, per-series time-homogeneous parameters) with
    B = 2, T = 33, hidden 8, obs 2 and numpy.random.default_rng(9), Q scaled by NEAR_SINGULAR_Q_SCALE"""
    rng = np.random.default_rng(9)
    B, T, h, o = 2, 33, 8, 2
    pre = (B, 1)

    def randn(*shape):
        return rng.standard_normal(shape)

    def tril(shape, n):
        A = randn(*(shape + (n, n)))
        return np.linalg.cholesky(A @ np.swapaxes(A, -1, -2) / n + 0.5 * np.eye(n))

    F = randn(*(pre + (h, h)))
    F = F * (0.9 / np.linalg.norm(F, ord=2, axis=(-2, -1)))[..., None, None]
    out = {"m0": 0.3 * randn(B, h), "L0": tril((B,), h), "F": F, "q": 0.3 * randn(*(pre + (h,))),
           "Lq": tril(pre, h), "H": randn(*(pre + (h, o))) / np.sqrt(h), "r": 0.3 * randn(*(pre + (o,))),
           "x": 2.0 * randn(B, T, o)}
    out["Lr"] = tril(pre, o)
    out["Lq"] = out["Lq"] * np.sqrt(NEAR_SINGULAR_Q_SCALE)
    return {k: torch.tensor(v, dtype=F64) for k, v in out.items()}


EXTRA = {"long": (_long_chain, 2), "near_singular": (_near_singular, 4)}


@functools.lru_cache(maxsize=None)
def _inputs(case):
    """({name: float64 CPU tensor} of the case, eps [S, B, T, h] float64): made once, never modified"""
    if case in EXTRA:
        make, S = EXTRA[case]
        t = make()
        B, T = t["x"].shape[:2]
        gen = torch.Generator().manual_seed(999)
        return t, torch.randn(S, B, T, t["m0"].shape[-1], generator=gen, dtype=F64)
    return {k: torch.tensor(gc.golden(case)[k]) for k in gc.NAMES}, pc.fixed_noise(case, 3)


def _leaves(case, dtype, device, requires_grad=False):
    t, eps = _inputs(case)
    return {k: v.to(dtype).to(device).requires_grad_(requires_grad) for k, v in t.items()}, eps.to(dtype).to(device)


def _torch_route(case, dtype):
    """(maps, draws) of the torch route on the CPU"""
    t, eps = _leaves(case, dtype, CPU)
    d = gc.build(t, case, dist)
    maps = hmm._backward_sample_maps(*d._parts, t["x"])
    return maps, hmm._backward_sample(*maps, eps)


@functools.lru_cache(maxsize=None)
def _want(case):
    """the float64 target: the fixture's moments (an extra case: those of the float64 torch route) and its draws"""
    maps, draws = _torch_route(case, F64)
    return (pc.moments(*maps) if case in EXTRA else pc.golden(case)), draws.numpy()


def _errors(case, maps, draws):
    moments, want_draws = _want(case)
    got = pc.moments(*maps)
    err = {k: gc.rel_err(got[k], moments[k]) for k in pc.KINDS}
    err["draws"] = gc.rel_err(draws.detach().cpu().double().numpy(), want_draws)
    return err


@functools.lru_cache(maxsize=None)
def _torch_f32_errors(case):
    """the float32 torch route on the CPU against the float64 target (measured once per case)"""
    return _errors(case, *_torch_route(case, F32))


def _raw(case, dtype, gpu):
    """the case in the layouts of kernels.gaussian_hmm_sample (detached) and its eps"""
    t, eps = _leaves(case, dtype, gpu)
    d = gc.build(t, case, dist)
    batch, T = d._check_value(t["x"])
    return [a.detach() for a in d._kernel_inputs(t["x"], batch, T)], eps


def _spy(monkeypatch):
    calls = []
    real = kernels.gaussian_hmm_sample

    def spy(*a, **kw):
        calls.append(kw)
        return real(*a, **kw)
    monkeypatch.setattr(kernels, "gaussian_hmm_sample", spy)
    return calls


def _fmt(err):
    return {k: "%.1e" % v for k, v in err.items()}


@pytest.mark.parametrize("case", gc.CASES)
def test_fixtures_float64(case, gpu):
    raw, eps = _raw(case, F64, gpu)
    z, maps = kernels.gaussian_hmm_sample(*raw, eps, need_maps=True)
    c, G, L = maps
    assert not G[:, -1].any() and torch.equal(L, L.tril())
    err = _errors(case, maps, z)
    print(case, "f64 kernel", _fmt(err))
    assert max(err.values()) < TOL64, err
    # without the maps (they then live in the workspace) and through the typed dispatcher op: the same bits
    z2, none = kernels.gaussian_hmm_sample(*raw, eps)
    assert none is None and torch.equal(z, z2)
    from pyro_amd.ops import torch_library
    assert torch_library.available()
    z3, maps3 = torch.ops.pyro_amd.gaussian_hmm_sample(*raw, eps, True)
    assert torch.equal(z, z3) and all(torch.equal(a, b) for a, b in zip(maps, maps3))


@pytest.mark.parametrize("case", gc.CASES)
def test_fixtures_float32(case, gpu):
    base = _torch_f32_errors(case)
    raw, eps = _raw(case, F32, gpu)
    z, maps = kernels.gaussian_hmm_sample(*raw, eps, need_maps=True)
    err = _errors(case, maps, z)
    print(case, "f32 kernel", _fmt(err), "torch route on the CPU", _fmt(base))
    for kind in KINDS:
        assert err[kind] <= 4 * base[kind], (kind, err, base)


def test_long_stable_chain_float32(gpu):
    """B = 2, T = 2000, hidden 4, obs 2 in float32 against the float64 torch route, S = 2; the same 4x rule"""
    base = _torch_f32_errors("long")
    raw, eps = _raw("long", F32, gpu)
    z, maps = kernels.gaussian_hmm_sample(*raw, eps, need_maps=True)
    err = _errors("long", maps, z)
    print("long chain: f32 kernel", _fmt(err), "torch route on the CPU", _fmt(base))
    assert torch.isfinite(z).all()
    for kind in KINDS:
        assert err[kind] <= 4 * base[kind], (kind, err, base)


def test_near_singular_process_noise_float32(gpu):
    """Q scaled by 1e-8 (NEAR_SINGULAR_Q_SCALE) at hidden 8, T = 33, S = 4, float32: the conditional covariances are
    nearly singular, and the draws stay finite and within the 4x rule only because they are formed in Joseph form.
    On the CPU, float32, at this scale: the torch route (Joseph form) is finite, its smallest Cholesky pivot of a
    conditional covariance is 8.74e-05 (float64: 8.74e-05; the pivots of P^p and P_T: 9.62e-05 in both, so the
    filter is not marginal), its draws are within 1.6e-04 of float64; the subtraction form P - G P^p G^T fed the
    same float32 filter has a non-positive pivot.  (It also fails at 1e-7 and holds from 1e-6 on.)  Both facts are
    checked here before the kernel is."""
    case = "near_singular"
    t, _ = _leaves(case, F32, CPU)
    d = gc.build(t, case, dist)
    (c, G, L), draws = _torch_route(case, F32)
    pivot = float(L.diagonal(dim1=-2, dim2=-1).min())
    print("near-singular: smallest pivot of the float32 torch route", pivot)
    assert torch.isfinite(draws).all() and 8.0e-5 < pivot < 9.5e-5
    kept = []
    hmm._kalman_filter(*d._parts, t["x"], keep=kept)
    F, Q = d._parts[2][:, 0], d._parts[4][:, 0]
    fails = False
    for m, P in kept[:-1]:
        FtP = F.transpose(-1, -2) @ P
        Pp = FtP @ F + Q
        Pp = 0.5 * (Pp + Pp.transpose(-1, -2))
        Gt = torch.cholesky_solve(FtP, torch.linalg.cholesky(Pp)).transpose(-1, -2)
        C = P - Gt @ Pp @ Gt.transpose(-1, -2)
        fails |= bool((torch.linalg.cholesky_ex(0.5 * (C + C.transpose(-1, -2)))[1] > 0).any())
    assert fails, "the subtraction form no longer fails here: the case does not pin the Joseph form"
    base = _torch_f32_errors(case)
    raw, eps = _raw(case, F32, gpu)
    z, maps = kernels.gaussian_hmm_sample(*raw, eps, need_maps=True)
    err = _errors(case, maps, z)
    print("near-singular: f32 kernel", _fmt(err), "torch route on the CPU", _fmt(base))
    assert torch.isfinite(z).all() and all(torch.isfinite(v).all() for v in maps)
    assert err["draws"] <= 4 * base["draws"], (err, base)


@pytest.mark.parametrize("case", ["b3_t1_h2_o1", "b2_t9_h4_o3_het", "b2_t40_h16_o16", "b2_t17_h5_o16_het"])
@pytest.mark.parametrize("dtype", [F32, F64])
def test_both_kernels_run_the_same_filter(case, dtype, gpu):
    """The maps kernel and gaussian_hmm_kernel share one filter (csrc/gaussian_hmm.h): the maps kernel's c_T is its
    filtered m_T stored untouched, so it equals the other kernel's filter mean BIT FOR BIT, and L_T L_T^T is
    sym(P_T) of that kernel up to the Cholesky's rounding (float64: 1e-9; float32: the file's rule, four times the
    ``cov`` error of the float32 torch route on the case).  T = 1, per-step parameters, both padded widths, and
    hidden != obs with the width chosen by obs: all four instantiations of both kernels."""
    raw, eps = _raw(case, dtype, gpu)
    _, (fm, fP), _ = kernels.gaussian_hmm_fwd_bwd(*raw, need_grads=False, need_filter=True)
    _, (c, _G, L) = kernels.gaussian_hmm_sample(*raw, eps[:0].contiguous(), need_maps=True)
    assert torch.isfinite(fm).all() and torch.equal(c[:, -1], fm)
    LT = L[:, -1].double().cpu()
    want = fP.double().cpu()
    err = gc.rel_err((LT @ LT.transpose(-1, -2)).numpy(), (0.5 * (want + want.transpose(-1, -2))).numpy())
    tol = TOL64 if dtype == F64 else 4 * _torch_f32_errors(case)["cov"]
    print(case, dtype, "L_T L_T^T against sym(P_T): %.1e, allowed %.1e" % (err, tol))
    assert err <= tol, (err, tol)


@pytest.mark.parametrize("dtype", [F32, F64])
def test_sample_chunk_edges(dtype, gpu):
    """one lane per draw, 64 draws per block: a draw does not depend on S, on its lane or on the other series"""
    case = "b2_t9_h4_o3_het"
    raw, _ = _raw(case, dtype, gpu)
    B, T, _o = raw[-1].shape
    gen = torch.Generator().manual_seed(5)
    eps = torch.randn(130, B, T, 4, generator=gen, dtype=F64).to(dtype).to(gpu)
    z130, maps = kernels.gaussian_hmm_sample(*raw, eps, need_maps=True)
    assert torch.isfinite(z130).all()
    want = hmm._backward_sample(*(v.cpu().double() for v in maps), eps.cpu().double())
    assert gc.rel_err(z130.cpu().double().numpy(), want.numpy()) < (TOL64 if dtype == F64 else 1e-5)
    for S in (1, 63, 64, 65):
        z, _ = kernels.gaussian_hmm_sample(*raw, eps[:S].contiguous())
        assert z.shape == (S, B, T, 4) and torch.equal(z, z130[:S]), S
    one = [a[:1].contiguous() for a in raw]                       # B = 1 (every parameter of this case is per series)
    assert all(a.shape[0] == B for a in raw)
    z1, maps1 = kernels.gaussian_hmm_sample(*one, eps[:, :1].contiguous(), need_maps=True)
    assert torch.equal(z1, z130[:, :1]) and all(torch.equal(a, b[:1]) for a, b in zip(maps1, maps))
    # S = 0 (the maps are still made) and B = 0
    z0, maps0 = kernels.gaussian_hmm_sample(*raw, eps[:0].contiguous(), need_maps=True)
    assert z0.shape == (0, B, T, 4) and all(torch.equal(a, b) for a, b in zip(maps0, maps))
    assert kernels.gaussian_hmm_sample(*raw, eps[:0].contiguous())[0].shape == (0, B, T, 4)
    none = [a[:0].contiguous() for a in raw]
    ze, mapse = kernels.gaussian_hmm_sample(*none, eps[:5, :0].contiguous(), need_maps=True)
    assert ze.shape == (5, 0, T, 4) and [tuple(v.shape) for v in mapse] == [(0, T, 4), (0, T, 4, 4), (0, T, 4, 4)]


@pytest.mark.parametrize("case", ["b2_t33_h8_o5", "b2_t17_h5_o16_het"])
@pytest.mark.parametrize("dtype", [F32, F64])
def test_reproducible(case, dtype, gpu):
    raw, eps = _raw(case, dtype, gpu)
    a = kernels.gaussian_hmm_sample(*raw, eps, need_maps=True)
    b = kernels.gaussian_hmm_sample(*raw, eps, need_maps=True)
    assert torch.equal(a[0], b[0]) and all(torch.equal(u, v) for u, v in zip(a[1], b[1]))


@pytest.mark.parametrize("dtype", [F32, F64])
def test_stride_zero_equals_expanded(dtype, gpu):
    """shared, time-homogeneous parameters passed with stride 0 and the same values expanded per series and per
    step: identical bits for the maps and the draws"""
    raw, eps = _raw("b3_t7_h3_o2_shared", dtype, gpu)
    B, T, _o = raw[-1].shape
    assert all(a.shape[0] == 1 and a.shape[1] == 1 for a in raw[2:8])
    z0, maps0 = kernels.gaussian_hmm_sample(*raw, eps, need_maps=True)
    wide = [raw[0], raw[1]] + [a.expand(B, T, *a.shape[2:]).contiguous() for a in raw[2:8]] + [raw[8]]
    z1, maps1 = kernels.gaussian_hmm_sample(*wide, eps, need_maps=True)
    assert torch.isfinite(z0).all()
    assert torch.equal(z0, z1) and all(torch.equal(a, b) for a, b in zip(maps0, maps1))


def test_a_bad_series_is_nan_and_alone(gpu):
    """one series of three with an R that is not positive definite: NaN maps and paths there, the other two bit for
    bit what a run without it gives"""
    raw, eps = _raw("b3_t7_h3_o2_shared", F32, gpu)
    m0, P0, F, q, Q, H, r, R, x = raw
    R3 = R.expand(3, *R.shape[1:]).contiguous()
    good = kernels.gaussian_hmm_sample(m0, P0, F, q, Q, H, r, R3, x, eps, need_maps=True)
    Rb = R3.clone()
    Rb[1] = -40.0 * torch.eye(R.shape[-1], device=gpu)          # S = H^T P^p H + R loses its first pivot
    bad = kernels.gaussian_hmm_sample(m0, P0, F, q, Q, H, r, Rb, x, eps, need_maps=True)
    for a, b in zip(good[1], bad[1]):
        assert a.shape[0] == 3 and torch.isfinite(a).all() and torch.isnan(b[1]).all()
        assert torch.equal(a[0], b[0]) and torch.equal(a[2], b[2])
    a, b = good[0], bad[0]
    assert torch.isfinite(a).all() and torch.isnan(b[:, 1]).all()
    assert torch.equal(a[:, 0], b[:, 0]) and torch.equal(a[:, 2], b[:, 2])


def test_over_the_dimension_limits(gpu, monkeypatch):
    z = lambda *s: torch.zeros(*s, device=gpu)                                            # noqa: E731
    eye = lambda n: torch.eye(n, device=gpu)                                              # noqa: E731
    for h, o in ((kernels.GAUSSIAN_HMM_MAX_HIDDEN + 1, 2), (2, kernels.GAUSSIAN_HMM_MAX_OBS + 1)):
        args = (z(1, h), eye(h)[None], 0.5 * eye(h)[None, None], z(1, 1, h), eye(h)[None, None],
                torch.ones(1, 1, h, o, device=gpu) / h, z(1, 1, o), eye(o)[None, None], z(2, 3, o), z(4, 2, 3, h))
        with pytest.raises(kernels.Unsupported):
            kernels.gaussian_hmm_sample(*args)
        calls = _spy(monkeypatch)                     # the class takes its torch route
        d = dist.GaussianHMM(dist.MultivariateNormal(z(h), eye(h)), 0.5 * eye(h), dist.MultivariateNormal(z(h), eye(h)),
                             torch.ones(h, o, device=gpu) / h, dist.MultivariateNormal(z(o), eye(o)))
        paths = d.rsample_posterior(z(2, 3, o), (4,))
        assert paths.shape == (4, 2, 3, h) and torch.isfinite(paths).all() and not calls
        monkeypatch.undo()


def test_routing(gpu, monkeypatch):
    case = "b2_t9_h4_o3_het"
    calls = _spy(monkeypatch)
    t, eps = _leaves(case, F64, gpu)
    want = _want(case)[1]
    # nothing needs a gradient: one kernel call, a detached result
    z = gc.build(t, case, dist).rsample_posterior(t["x"], (3,), noise=eps)
    assert len(calls) == 1 and not z.requires_grad and z.shape == (3, 2, 9, 4)
    assert gc.rel_err(z.cpu().numpy(), want) < TOL64
    tg, _ = _leaves(case, F64, gpu, requires_grad=True)
    with torch.no_grad():
        zn = gc.build(tg, case, dist).rsample_posterior(tg["x"], (3,), noise=eps)
    assert len(calls) == 2 and not zn.requires_grad and torch.equal(z, zn)
    # a leaf requires a gradient: the torch route, and backward reaches m0
    zg = gc.build(tg, case, dist).rsample_posterior(tg["x"], (3,), noise=eps)
    assert len(calls) == 2 and zg.requires_grad
    zg.sum().backward()
    assert tg["m0"].grad is not None and tg["m0"].grad.abs().max() > 0
    # ... both routes agree for the one noise tensor
    assert gc.rel_err(zg.detach().cpu().numpy(), z.cpu().numpy()) < TOL64
    # the switch: the torch route on the device
    monkeypatch.setattr(hmm, "FUSED_GAUSSIAN_HMM", False)
    zs = gc.build(t, case, dist).rsample_posterior(t["x"], (3,), noise=eps)
    assert len(calls) == 2 and gc.rel_err(zs.cpu().numpy(), want) < TOL64
    monkeypatch.setattr(hmm, "FUSED_GAUSSIAN_HMM", True)
    # sample shapes, a leading batch dim on the value and drawn noise, on the kernel
    d = gc.build(t, case, dist)
    assert d.rsample_posterior(t["x"]).shape == (2, 9, 4)
    x2 = torch.stack([t["x"], t["x"] + 1.0, t["x"] - 1.0])
    torch.manual_seed(3)
    a = d.rsample_posterior(x2, (2, 5))
    torch.manual_seed(3)
    noise = torch.randn(2, 5, 3, 2, 9, 4, dtype=F64, device=gpu)
    b = d.rsample_posterior(x2, (2, 5), noise=noise)
    assert a.shape == (2, 5, 3, 2, 9, 4) and torch.equal(a, b) and len(calls) == 5
    # ... and a series' draws do not depend on what else is in the batch
    assert torch.equal(a[:, :, 1], d.rsample_posterior(x2[1], (2, 5), noise=noise[:, :, 1]))
