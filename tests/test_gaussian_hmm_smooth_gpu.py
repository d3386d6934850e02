"""csrc/gaussian_hmm_smooth.hip on the device: the smoothed marginals (Kalman filter, then the Rauch-Tung-Striebel sweep
with the covariance in subtraction form) through kernels.gaussian_hmm_smooth, torch.ops.pyro_amd.gaussian_hmm_smooth and
GaussianHMM.smooth.

The targets are never the kernel's own output: the fixtures of the unmodified reference
(tests/golden/gaussian_hmm_posterior.npz, float64) where they exist, otherwise the float64 torch route of
distributions/hmm.py on the CPU, which tests/test_gaussian_hmm_smooth_host.py ties to the fixtures and to dense
conditioning of the joint Gaussian.  Errors are gaussian_hmm_cases.rel_err = max |got - want| / (1 + max |want|) per
array; the kinds are ``mean``, ``cov`` and ``cross``.

float64: 1e-9.

float32: the kernel orders its sums differently from torch, so it gets max(FOUR times the error of the float32 torch
route run on the CPU on the same inputs, 4 * 2^-23), per case and kind (the margin and the floor of
tests/test_gaussian_hmm_edges_gpu.py).  The torch route's error is measured when the test runs.  In group D (the
ill-conditioned inputs of tests/gaussian_hmm_edge_cases.py) the base of a recipe x shape x kind is the worst of the
eight seeds, the float32 kernel stays within 4 x base on every seed and the float64 kernel within
max(1e-9, 4 x base x 2^-29).

The worst figures over each group as the tests print them on an MI355X (kernel / float32 torch route on the CPU):

    worst of the group                         mean      cov       cross
    fixtures, 8 cases        f64 kernel        2.4e-15   2.6e-15   2.9e-15
                             f32 kernel        4.3e-07   3.6e-07   2.2e-07
                             f32 torch         4.8e-07   2.7e-07   2.6e-07
    A (3, 2), 26 layouts     f64 kernel        7.1e-16   5.5e-16   4.7e-16
                             f32 kernel        2.0e-07   1.5e-07   2.1e-07
                             f32 torch         3.9e-07   2.0e-07   1.6e-07
    A (9, 2), 26 layouts     f64 kernel        8.6e-16   5.7e-16   5.8e-16
                             f32 kernel        3.6e-07   2.5e-07   2.4e-07
                             f32 torch         2.5e-07   1.3e-07   1.9e-07
    B, 40 shapes x lengths   f64 kernel        1.2e-15   1.5e-15   4.1e-16
                             f32 kernel        7.5e-07   3.1e-07   2.1e-07
                             f32 torch         8.0e-07   1.2e-06   1.2e-07
    long chain (T = 2000)    f32 kernel        2.3e-07   2.1e-07   1.2e-07
                             f32 torch         3.3e-07   1.4e-07   1.7e-07
    near-singular Q          f32 kernel        4.9e-05   1.1e-05   3.2e-06
                             f32 torch         3.0e-05   2.9e-06   8.7e-07

    D: base = worst torch of 8 seeds           mean      cov       cross
    noiseless (4, 4)         base              6.3e-04   1.5e-04   3.1e-05
                             f32 kernel        4.8e-04   8.7e-05   2.6e-05
    noiseless (9, 2)         base              3.2e-07   3.2e-07   2.3e-07
                             f32 kernel        3.3e-07   2.8e-07   2.8e-07
    noiseless (16, 16)       base              3.9e-04   7.6e-05   1.8e-05
                             f32 kernel        6.8e-04   8.9e-05   1.5e-05
    shifted (4, 4)           base              1.6e-05   2.3e-07   1.5e-07
                             f32 kernel        1.1e-05   2.7e-07   1.4e-07
    shifted (9, 2)           base              1.6e-05   1.6e-07   1.9e-07
                             f32 kernel        1.0e-05   2.9e-07   2.2e-07
    shifted (16, 16)         base              1.4e-05   2.3e-07   1.4e-07
                             f32 kernel        1.1e-05   3.4e-07   2.6e-07
    diffuse (4, 4)           base              4.3e-04   3.4e-04   2.7e-04
                             f32 kernel        2.9e-04   2.7e-04   2.3e-04
    diffuse (9, 2)           base              7.4e-06   7.4e-06   8.6e-06
                             f32 kernel        8.8e-06   5.2e-06   4.4e-06
    diffuse (16, 16)         base              4.1e-04   2.9e-04   1.5e-04
                             f32 kernel        4.0e-04   2.1e-04   2.0e-04
    (float64 kernel in D: at most 2.3e-12)
"""
import functools

import numpy as np
import pytest
import torch

import pyro_amd.distributions as dist
from pyro_amd import kernels
from pyro_amd.distributions import hmm
from tests import gaussian_hmm_cases as gc
from tests import gaussian_hmm_edge_cases as ec
from tests import gaussian_hmm_posterior_cases as pc
from tests.test_gaussian_hmm_sample_gpu import _long_chain, _near_singular

pytestmark = pytest.mark.gpu
TOL64 = 1e-9
F32, F64, CPU = ec.F32, ec.F64, ec.CPU
DTYPES = [F32, F64]
KINDS = pc.KINDS
EXTRA = {"long": _long_chain, "near_singular": _near_singular}
_id = lambda v: "_".join(str(x) for x in v) if isinstance(v, tuple) else str(v).replace("torch.", "")   # noqa: E731


def _np(v):
    return v.detach().cpu().double().numpy()


def _arrays(out):
    return {k: _np(v) for k, v in zip(KINDS, out)}


def _errors(got, want):
    err = {k: gc.rel_err(got[k], want[k]) for k in KINDS}
    return {k: (v if np.isfinite(v) else float("inf")) for k, v in err.items()}


def _fmt(err):
    return " ".join("%s %.1e" % kv for kv in err.items())


def _within_4x(err, base, what):
    for kind in KINDS:
        assert err[kind] <= max(4 * base[kind], ec.FLOOR32), (what, kind, err, base)


# ---- the cases with a fixture, and the two extra ones ---------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _inputs(case):
    """{name: float64 CPU tensor} of the case: made once, never modified"""
    if case in EXTRA:
        return EXTRA[case]()
    return {k: torch.tensor(gc.golden(case)[k]) for k in gc.NAMES}


def _leaves(case, dtype, device, requires_grad=False):
    return {k: v.to(dtype).to(device).requires_grad_(requires_grad) for k, v in _inputs(case).items()}


@functools.lru_cache(maxsize=None)
def _torch_route(case, dtype):
    """the torch route on the CPU (CPU tensors never reach a kernel)"""
    t = _leaves(case, dtype, CPU)
    return _arrays(gc.build(t, case, dist).smooth(t["x"], cross=True))


def _want(case):
    return _torch_route(case, F64) if case in EXTRA else pc.golden(case)


@functools.lru_cache(maxsize=None)
def _base(case):
    """the float32 torch route on the CPU against the float64 target (measured once per case)"""
    return _errors(_torch_route(case, F32), _want(case))


def _raw(case, dtype, gpu):
    """the case in the layouts of kernels.gaussian_hmm_smooth (detached)"""
    t = _leaves(case, dtype, gpu)
    d = gc.build(t, case, dist)
    batch, T = d._check_value(t["x"])
    return [a.detach() for a in d._kernel_inputs(t["x"], batch, T)]


def _spy(monkeypatch):
    calls = []
    real = kernels.gaussian_hmm_smooth

    def spy(*a, **kw):
        calls.append(kw)
        return real(*a, **kw)
    monkeypatch.setattr(kernels, "gaussian_hmm_smooth", spy)
    return calls


@pytest.mark.parametrize("case", gc.CASES)
def test_fixtures_float64(case, gpu):
    raw = _raw(case, F64, gpu)
    out = kernels.gaussian_hmm_smooth(*raw, need_cross=True)
    B, T, _ = raw[-1].shape
    h = raw[0].shape[-1]
    assert [tuple(v.shape) for v in out] == [(B, T, h), (B, T, h, h), (B, T - 1, h, h)]
    err = _errors(_arrays(out), pc.golden(case))
    print(case, "f64 kernel", _fmt(err))
    assert max(err.values()) < TOL64, err
    assert torch.equal(out[1], out[1].transpose(-1, -2))
    # without the cross covariances and through the typed dispatcher op: the same bits
    mean, cov, none = kernels.gaussian_hmm_smooth(*raw)
    assert none is None and torch.equal(mean, out[0]) and torch.equal(cov, out[1])
    from pyro_amd.ops import torch_library
    assert torch_library.available()
    m3, c3, x3 = torch.ops.pyro_amd.gaussian_hmm_smooth(*raw, True)
    assert len(x3) == 1 and torch.equal(m3, out[0]) and torch.equal(c3, out[1]) and torch.equal(x3[0], out[2])
    m4, c4, x4 = torch.ops.pyro_amd.gaussian_hmm_smooth(*raw, False)
    assert x4 == [] and torch.equal(m4, out[0]) and torch.equal(c4, out[1])


@pytest.mark.parametrize("case", gc.CASES)
def test_fixtures_float32(case, gpu):
    base = _base(case)
    out = kernels.gaussian_hmm_smooth(*_raw(case, F32, gpu), need_cross=True)
    err = _errors(_arrays(out), pc.golden(case))
    print(case, "f32 kernel", _fmt(err), "| torch route on the CPU", _fmt(base))
    _within_4x(err, base, case)


def test_long_stable_chain_float32(gpu):
    """B = 2, T = 2000, hidden 4, obs 2 in float32 against the float64 torch route; the same 4x rule"""
    base = _base("long")
    out = kernels.gaussian_hmm_smooth(*_raw("long", F32, gpu), need_cross=True)
    err = _errors(_arrays(out), _want("long"))
    print("long chain: f32 kernel", _fmt(err), "| torch route on the CPU", _fmt(base))
    assert all(torch.isfinite(v).all() for v in out)
    _within_4x(err, base, "long")


def test_near_singular_process_noise_float32(gpu):
    """Q scaled by 1e-8 at hidden 8, T = 33, float32: the case that made the backward sampler take the Joseph form.
    Nothing is factorised from the smoothed covariance, so the subtraction form stays finite here and within the 4x
    rule: an accuracy case, not a pin on a formula"""
    case = "near_singular"
    base = _base(case)
    out = kernels.gaussian_hmm_smooth(*_raw(case, F32, gpu), need_cross=True)
    err = _errors(_arrays(out), _want(case))
    print("near-singular: f32 kernel", _fmt(err), "| torch route on the CPU", _fmt(base))
    assert all(torch.isfinite(v).all() for v in out)
    _within_4x(err, base, case)


@pytest.mark.parametrize("case", ["b3_t1_h2_o1", "b2_t9_h4_o3_het", "b2_t40_h16_o16", "b2_t17_h5_o16_het"])
@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
def test_one_filter(case, dtype, gpu):
    """The smoother and gaussian_hmm_kernel share one filter (csrc/gaussian_hmm.h): the last smoothed marginal is the
    filtered one, m_T stored untouched and sym(P_T), BIT FOR BIT.  T = 1, per-step parameters, both padded widths,
    and hidden != obs with the width chosen by obs: all four instantiations"""
    raw = _raw(case, dtype, gpu)
    _, (fm, fP), _ = kernels.gaussian_hmm_fwd_bwd(*raw, need_grads=False, need_filter=True)
    mean, cov, _ = kernels.gaussian_hmm_smooth(*raw)
    assert torch.isfinite(fm).all() and torch.isfinite(fP).all()
    assert torch.equal(mean[:, -1], fm) and torch.equal(cov[:, -1], 0.5 * (fP + fP.transpose(-1, -2)))


@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
def test_reproducible_and_isolated(dtype, gpu):
    for case in ("b2_t33_h8_o5", "b2_t17_h5_o16_het"):
        raw = _raw(case, dtype, gpu)
        a = kernels.gaussian_hmm_smooth(*raw, need_cross=True)
        b = kernels.gaussian_hmm_smooth(*raw, need_cross=True)
        assert all(torch.isfinite(u).all() and torch.equal(u, v) for u, v in zip(a, b)), case
    raw = _raw("b2_t9_h4_o3_het", dtype, gpu)                     # every parameter of this case is per series
    B, T, _o = raw[-1].shape
    assert all(a.shape[0] == B for a in raw)
    full = kernels.gaussian_hmm_smooth(*raw, need_cross=True)
    for b in range(B):
        one = kernels.gaussian_hmm_smooth(*[a[b:b + 1].contiguous() for a in raw], need_cross=True)
        assert all(torch.equal(u, v[b:b + 1]) for u, v in zip(one, full)), b
    empty = kernels.gaussian_hmm_smooth(*[a[:0].contiguous() for a in raw], need_cross=True)
    assert [tuple(v.shape) for v in empty] == [(0, T, 4), (0, T, 4, 4), (0, T - 1, 4, 4)]
    empty = kernels.gaussian_hmm_smooth(*[a[:0].contiguous() for a in raw])
    assert empty[2] is None and empty[0].shape == (0, T, 4)


# ---- the edge cases of tests/gaussian_hmm_edge_cases.py -------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _edge_route(key, dtype):
    """the torch route of an edge case on the CPU: float64 is the target, float32 the base of the 4x rule"""
    t = ec.leaves(key, dtype, CPU)
    B, T, _ = t["x"].shape
    return _arrays(ec.model(ec.parts(t), T, B).smooth(t["x"], cross=True))


def _edge_raw(key, dtype, gpu):
    t = ec.leaves(key, dtype, gpu)
    return [a.detach().contiguous() for a in (*ec.parts(t), t["x"])]


def _edge_check(key, dtype, out):
    err = _errors(_arrays(out), _edge_route(key, F64))
    if dtype == F64:
        print(_id(key), "f64 kernel", _fmt(err))
        assert max(err.values()) < TOL64, (key, err)
        return
    base = _errors(_edge_route(key, F32), _edge_route(key, F64))
    print(_id(key), "f32 kernel", _fmt(err), "| torch route on the CPU", _fmt(base))
    _within_4x(err, base, key)


@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
@pytest.mark.parametrize("key", ec.A_KEYS, ids=_id)
def test_layout_matrix(key, dtype, gpu):
    raw = _edge_raw(key, dtype, gpu)
    out = kernels.gaussian_hmm_smooth(*raw, need_cross=True)
    _edge_check(key, dtype, out)
    # every stride-0 axis expanded and made contiguous: the same bits
    B, T, _ = raw[-1].shape
    wide = [a.expand(B, *a.shape[1:]).contiguous() for a in raw[:2]]
    wide += [a.expand(B, T, *a.shape[2:]).contiguous() for a in raw[2:8]] + [raw[8]]
    assert any(w.shape != a.shape for w, a in zip(wide, raw))
    for a, b in zip(out, kernels.gaussian_hmm_smooth(*wide, need_cross=True)):
        assert torch.isfinite(a).all() and torch.equal(a, b)


def _border_keys(shape):
    keys = [("B",) + shape + (T, False) for T in ec.B_TS]
    if shape in ec.B_PER_STEP:
        keys += [("B",) + shape + (T, True) for T in ec.B_TS if T > 1]
    return keys


@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
@pytest.mark.parametrize("shape", ec.B_SHAPES, ids=_id)
def test_width_border_and_short_chains(shape, dtype, gpu):
    for key in _border_keys(shape):
        raw = _edge_raw(key, dtype, gpu)
        out = kernels.gaussian_hmm_smooth(*raw, need_cross=True)
        assert out[2].shape[1] == key[3] - 1
        _edge_check(key, dtype, out)
        mean, cov, none = kernels.gaussian_hmm_smooth(*raw)
        assert none is None and torch.equal(mean, out[0]) and torch.equal(cov, out[1])


@pytest.mark.parametrize("shape", ec.D_SHAPES, ids=_id)
@pytest.mark.parametrize("recipe", ec.RECIPES)
def test_ill_conditioned(recipe, shape, gpu):
    """near-noiseless observations, data far from zero, a diffuse prior; eight seeds, float32 and float64"""
    keys = ec.d_keys(recipe, shape)
    base = dict.fromkeys(KINDS, 0.0)
    for key in keys:
        b = _errors(_edge_route(key, F32), _edge_route(key, F64))
        assert all(np.isfinite(b[k]) for k in KINDS), (key, b)
        base = {k: max(base[k], b[k]) for k in KINDS}
    worst = {F32: dict.fromkeys(KINDS, 0.0), F64: dict.fromkeys(KINDS, 0.0)}
    fails = []
    for key in keys:
        for dtype in DTYPES:
            out = kernels.gaussian_hmm_smooth(*_edge_raw(key, dtype, gpu), need_cross=True)
            err = _errors(_arrays(out), _edge_route(key, F64))
            for k in KINDS:
                bound = max(4 * base[k], ec.FLOOR32) if dtype == F32 else max(TOL64, 4 * base[k] * 2.0 ** -29)
                worst[dtype][k] = max(worst[dtype][k], err[k])
                if not err[k] <= bound:
                    fails.append("%s %s %s: %.1e over %.1e" % (_id(key), _id(dtype), k, err[k], bound))
    print(recipe, _id(shape), "base (worst f32 torch route of the seeds)", _fmt(base), "| f32 kernel",
          _fmt(worst[F32]), "| f64 kernel", _fmt(worst[F64]))
    assert not fails, fails


# ---- bad series -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
@pytest.mark.parametrize("key", ec.E_KEYS, ids=_id)
def test_a_bad_q_marks_its_series(key, dtype, gpu):
    """Series 1 of three with a Q that is not positive definite while every innovation covariance is: NaN in all
    three outputs for that series.  Only hom_q (3, 2) has a P^p = sym(F^T P_{t-1} F + Q) that is not positive definite
    (smallest eigenvalue -0.011; the others +0.480, +0.188, +0.013: tests/test_gaussian_hmm_smooth_host.py); on the
    other keys it is the kernel's check of Q's own pivots that marks the series -- once before the sweep in step_q
    (Q time-homogeneous), in every step of it in hom_q."""
    p, x = ec.bad_pivot_parts(key, "Q", dtype, gpu)
    bad = kernels.gaussian_hmm_smooth(*p, x, need_cross=True)
    print(_id(key), _id(dtype), "NaN in series 1 of mean, cov, cross:", [bool(torch.isnan(b[1]).all()) for b in bad])
    for b in bad:
        assert torch.isnan(b[1]).all()


@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
@pytest.mark.parametrize("key", ec.E_KEYS, ids=_id)
def test_a_bad_q_or_p0_leaves_the_other_series_alone(key, dtype, gpu):
    """with series 1's Q not positive definite the other two are bit for bit unchanged; with a P0 that is not
    positive definite (never factorised here, and the first P^p still is) every series stays finite"""
    p, x = ec.bad_pivot_parts(key, None, dtype, gpu)
    good = kernels.gaussian_hmm_smooth(*p, x, need_cross=True)
    p, x = ec.bad_pivot_parts(key, "Q", dtype, gpu)
    bad = kernels.gaussian_hmm_smooth(*p, x, need_cross=True)
    for a, b in zip(good, bad):
        assert a.shape[0] == 3 and torch.isfinite(a).all()
        assert torch.equal(a[0], b[0]) and torch.equal(a[2], b[2])
    p, x = ec.bad_pivot_parts(key, "P0", dtype, gpu)
    odd = kernels.gaussian_hmm_smooth(*p, x, need_cross=True)
    for a, b in zip(good, odd):
        assert torch.isfinite(b).all() and torch.equal(a[0], b[0]) and torch.equal(a[2], b[2])


@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
def test_a_bad_series_in_the_filter_is_nan_and_alone(dtype, gpu):
    """one series of three with an R that is not positive definite: the filter's own pivot fails"""
    m0, P0, F, q, Q, H, r, R, x = _raw("b3_t7_h3_o2_shared", dtype, gpu)
    R3 = R.expand(3, *R.shape[1:]).contiguous()
    good = kernels.gaussian_hmm_smooth(m0, P0, F, q, Q, H, r, R3, x, need_cross=True)
    Rb = R3.clone()
    Rb[1] = -40.0 * torch.eye(R.shape[-1], dtype=dtype, device=gpu)          # S = H^T P^p H + R loses its first pivot
    bad = kernels.gaussian_hmm_smooth(m0, P0, F, q, Q, H, r, Rb, x, need_cross=True)
    for a, b in zip(good, bad):
        assert a.shape[0] == 3 and torch.isfinite(a).all() and torch.isnan(b[1]).all()
        assert torch.equal(a[0], b[0]) and torch.equal(a[2], b[2])


# ---- the class ------------------------------------------------------------------------------------------------------
def test_over_the_dimension_limits(gpu, monkeypatch):
    z = lambda *s: torch.zeros(*s, device=gpu)                                            # noqa: E731
    eye = lambda n: torch.eye(n, device=gpu)                                              # noqa: E731
    for h, o in ((kernels.GAUSSIAN_HMM_MAX_HIDDEN + 1, 2), (2, kernels.GAUSSIAN_HMM_MAX_OBS + 1)):
        args = (z(1, h), eye(h)[None], 0.5 * eye(h)[None, None], z(1, 1, h), eye(h)[None, None],
                torch.ones(1, 1, h, o, device=gpu) / h, z(1, 1, o), eye(o)[None, None], z(2, 3, o))
        with pytest.raises(kernels.Unsupported):
            kernels.gaussian_hmm_smooth(*args)
        calls = _spy(monkeypatch)                     # the class takes its torch route
        d = dist.GaussianHMM(dist.MultivariateNormal(z(h), eye(h)), 0.5 * eye(h), dist.MultivariateNormal(z(h), eye(h)),
                             torch.ones(h, o, device=gpu) / h, dist.MultivariateNormal(z(o), eye(o)))
        out = d.smooth(z(2, 3, o), cross=True)
        assert [tuple(v.shape) for v in out] == [(2, 3, h), (2, 3, h, h), (2, 2, h, h)]
        assert all(torch.isfinite(v).all() for v in out) and not calls
        monkeypatch.undo()


def test_routing(gpu, monkeypatch):
    case = "b2_t9_h4_o3_het"
    calls = _spy(monkeypatch)
    t = _leaves(case, F64, gpu)
    want = pc.golden(case)
    # nothing needs a gradient: one kernel call, a detached result
    out = gc.build(t, case, dist).smooth(t["x"], cross=True)
    assert len(calls) == 1 and calls[0] == {"need_cross": True} and not any(v.requires_grad for v in out)
    assert [tuple(v.shape) for v in out] == [(2, 9, 4), (2, 9, 4, 4), (2, 8, 4, 4)]
    assert max(_errors(_arrays(out), want).values()) < TOL64
    two = gc.build(t, case, dist).smooth(t["x"])
    assert len(calls) == 2 and calls[1] == {"need_cross": False} and len(two) == 2 and torch.equal(two[1], out[1])
    tg = _leaves(case, F64, gpu, requires_grad=True)
    with torch.no_grad():
        outn = gc.build(tg, case, dist).smooth(tg["x"], cross=True)
    assert len(calls) == 3 and all(not v.requires_grad and torch.equal(v, w) for v, w in zip(outn, out))
    # a leaf requires a gradient: the torch route, and backward reaches m0
    outg = gc.build(tg, case, dist).smooth(tg["x"], cross=True)
    assert len(calls) == 3 and all(v.requires_grad for v in outg)
    sum(v.sum() for v in outg).backward()
    assert tg["m0"].grad is not None and tg["m0"].grad.abs().max() > 0
    # ... both routes agree
    assert max(_errors(_arrays(outg), _arrays(out)).values()) < TOL64
    # the switch: the torch route on the device
    monkeypatch.setattr(hmm, "FUSED_GAUSSIAN_HMM", False)
    outs = gc.build(t, case, dist).smooth(t["x"], cross=True)
    assert len(calls) == 3 and max(_errors(_arrays(outs), want).values()) < TOL64
    monkeypatch.setattr(hmm, "FUSED_GAUSSIAN_HMM", True)
    # a leading batch dim on the value: a series' result does not depend on what else is in the batch
    d = gc.build(t, case, dist)
    x2 = torch.stack([t["x"], t["x"] + 1.0, t["x"] - 1.0])
    a = d.smooth(x2, cross=True)
    assert [tuple(v.shape) for v in a] == [(3, 2, 9, 4), (3, 2, 9, 4, 4), (3, 2, 8, 4, 4)] and len(calls) == 4
    assert all(torch.equal(u[1], v) for u, v in zip(a, d.smooth(x2[1], cross=True)))
    assert all(torch.equal(u[0], v) for u, v in zip(a, out))
