"""The Student-t variant of csrc/gaussian_hmm.hip on the device: through kernels.gamma_gaussian_hmm_fwd_bwd, the typed op
pyro_amd::gamma_gaussian_hmm and pyro_amd.distributions.GammaGaussianHMM, in float32 and float64, against the fixtures
of the unmodified reference (tests/golden/gamma_gaussian_hmm.npz, float64) and the float64 torch route of
distributions/hmm.py on the CPU -- never the kernel's own output.

Errors are gaussian_hmm_cases.rel_err = max |got - want| / (1 + max |want|) per array (log_prob: per element), and a
kind's error is the worst of its arrays.  The kinds: log_prob, grads (the nine gradients of the model's leaves), grad_a,
grad_b, rate (the Gamma posterior's) and filter (its concentration, the normal's loc and covariance -- against the
fixture the INVERSE of the covariance, which is what the reference's normal holds).

float64: 1e-9 per array.

float32: at most max(FOUR times the error of the float32 torch route on the CPU on the same inputs, FLOOR32 = 4 * 2^-23),
per case and kind -- the rule of tests/test_gaussian_hmm_edges_gpu.py, the base measured when the test runs.

The worst figures over the tests that print them, on an MI355X (the ten fixtures, the border shapes, the layouts, the
shared Gamma, the extreme weights):

                                 log_prob  grads     grad_a    grad_b    rate      filter
    float64 kernel               6.2e-16   1.4e-14   1.0e-15   4.3e-16   9.0e-16   1.7e-15
    float32 kernel               2.3e-07   5.9e-06   5.1e-07   3.0e-07   2.0e-07   1.1e-06
    float32 torch route, CPU     1.7e-07   3.8e-06   6.4e-07   2.1e-07   2.5e-07   7.6e-07

(the 5.9e-06 / 3.8e-06 are the case with weights near 200).  Mutations of the sweep's scaling, each failing on the
``grads`` kind: w fixed at 1 -- 41 of the 67 tests fail; the 1 / w on the outgoing covariance gradients dropped -- 41; the
batch stride of ``a`` ignored -- 35 (the cases with one value of ``a`` pass).
"""
import functools

import numpy as np
import pytest
import torch

import pyro_amd.distributions as dist
from pyro_amd import kernels
from pyro_amd.distributions import hmm
from pyro_amd.ops.contract import _GammaGaussianHMM
from tests import gamma_gaussian_hmm_cases as ggc
from tests import gaussian_hmm_cases as gc
from tests import gaussian_hmm_edge_cases as ec

pytestmark = pytest.mark.gpu
TOL64 = 1e-9
F32, F64, CPU = ec.F32, ec.F64, ec.CPU
DTYPES = [F32, F64]
KINDS = ("log_prob", "grads", "grad_a", "grad_b", "rate", "filter")
NAMES = ("a", "b") + ec.NAMES
_id = lambda v: "_".join(str(x) for x in v) if isinstance(v, tuple) else str(v).replace("torch.", "")   # noqa: E731


def _np(v):
    return v.detach().cpu().double().numpy()


def _bound(dtype, err, base):
    for kind in KINDS:
        if dtype == F64:
            assert err[kind] < TOL64, (kind, err)
        else:
            assert err[kind] <= max(4 * base[kind], ec.FLOOR32), (kind, err, base)


def _spy(monkeypatch):
    calls = []
    real = kernels.gamma_gaussian_hmm_fwd_bwd

    def spy(*a, **kw):
        calls.append(kw)
        return real(*a, **kw)
    monkeypatch.setattr(kernels, "gamma_gaussian_hmm_fwd_bwd", spy)
    return calls


# ---- the fixtures of the reference, through the class --------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _torch_f32_errors(case):
    """the float32 torch route on the CPU against the float64 fixture (measured once per case)"""
    return ggc.errors(ggc.leaves(case, F32, CPU), case, dist)[0]


@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
@pytest.mark.parametrize("case", ggc.CASES)
def test_fixtures(case, dtype, gpu, monkeypatch):
    calls = _spy(monkeypatch)
    err, per = ggc.errors(ggc.leaves(case, dtype, gpu), case, dist)
    base = _torch_f32_errors(case) if dtype == F32 else None
    print(case, _id(dtype), "kernel", ec.fmt(err), "| f32 torch route on the CPU", base and ec.fmt(base),
          {k: "%.1e" % v for k, v in per.items()})
    assert len(calls) == 2 and calls[0].get("need_grads", True)          # log_prob with its gradients, filter
    _bound(dtype, err, base)


# ---- the kernel's own layouts against the float64 torch route ------------------------------------------------------
def _leaves(arrays, dtype, device):
    return {k: torch.tensor(v, dtype=dtype, device=device, requires_grad=True) for k, v in arrays.items()}


def _route(t, kernel):
    """Everything the entry point computes, from leaves in the layouts of tests/gaussian_hmm_edge_cases.py plus ``a``,
    ``b`` [B | 1]: by the autograd Function and the wrapper (``kernel``) or by the torch route on the leaves' device ->
    ({name: float64 array}, the wrapper's raw outputs or None)"""
    p, x = ec.parts(t), t["x"]
    n = x.shape[1] * x.shape[2]
    raw = None
    if kernel:
        args = [t["a"], t["b"]] + [v.contiguous() for v in p] + [x]
        lp = _GammaGaussianHMM.invoke(*args)
        raw = kernels.gamma_gaussian_hmm_fwd_bwd(*[v.detach() for v in args], need_grads=True, need_filter=True)
        quad, _, (m, P), _ = raw
        assert torch.equal(lp.detach(), hmm._student_log_prob(t["a"].detach(), t["b"].detach(), raw[0], raw[1], n))
    else:
        quad, logdet, m, P = hmm._kalman_terms(*p, x)
        lp = hmm._student_log_prob(t["a"], t["b"], quad, logdet, n)
        m, P = m.expand(x.shape[0], -1), P.expand(x.shape[0], -1, -1)
    out = {"log_prob": _np(lp), "rate": _np(t["b"] + 0.5 * quad), "loc": _np(m), "cov": _np(P)}
    for k, g in zip(NAMES, torch.autograd.grad(lp.sum(), [t[k] for k in NAMES])):
        assert g.shape == t[k].shape, k
        out["g_" + k] = _np(g)
    return out, raw


def _errors(got, want):
    err = {"log_prob": ec.lp_err(got["log_prob"], want["log_prob"]),
           "grads": max(gc.rel_err(got["g_" + k], want["g_" + k]) for k in ec.NAMES),
           "grad_a": gc.rel_err(got["g_a"], want["g_a"]), "grad_b": gc.rel_err(got["g_b"], want["g_b"]),
           "rate": gc.rel_err(got["rate"], want["rate"]),
           "filter": max(gc.rel_err(got["loc"], want["loc"]), gc.rel_err(got["cov"], want["cov"]))}
    return {k: (v if np.isfinite(v) else float("inf")) for k, v in err.items()}


def _gamma(rng, n):
    return {"a": rng.uniform(1.0, 4.0, (n,)), "b": rng.uniform(0.5, 3.0, (n,))}


def _check(arrays, dtype, gpu, what):
    """the bound of the module docstring for one set of inputs -> (the kernel route's arrays, the wrapper's outputs)"""
    want = _route(_leaves(arrays, F64, CPU), False)[0]
    got, raw = _route(_leaves(arrays, dtype, gpu), True)
    err = _errors(got, want)
    base = _errors(_route(_leaves(arrays, F32, CPU), False)[0], want) if dtype == F32 else None
    print(what, _id(dtype), "kernel", ec.fmt(err), "| f32 torch route on the CPU", base and ec.fmt(base))
    _bound(dtype, err, base)
    return got, raw


B_SHAPES = ((8, 8), (9, 1), (1, 9), (16, 16), (1, 1))


@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
@pytest.mark.parametrize("shape", B_SHAPES, ids=_id)
def test_width_border_and_short_chains(shape, dtype, gpu):
    """both sides of the 8 / 16 dispatch at T = 1, 2, 3; without gradient pointers the same bits"""
    from pyro_amd.ops import torch_library
    assert torch_library.available()
    for T in ec.B_TS:
        key = ("B",) + shape + (T, False)
        arrays = dict(ec.inputs(key), **_gamma(np.random.default_rng([20241102, *shape, T]), 2))
        _, raw = _check(arrays, dtype, gpu, _id(key))
        t = _leaves(arrays, dtype, gpu)
        args = [t["a"], t["b"]] + [v.contiguous() for v in ec.parts(t)] + [t["x"]]
        quad, logdet, filt, none = kernels.gamma_gaussian_hmm_fwd_bwd(*[v.detach() for v in args], need_grads=False,
                                                                      need_filter=True)
        assert none is None and torch.equal(quad, raw[0]) and torch.equal(logdet, raw[1])
        assert torch.equal(filt[0], raw[2][0]) and torch.equal(filt[1], raw[2][1])
        # ... and the typed op is the same launch
        q2, l2, fm, fP, g2 = torch.ops.pyro_amd.gamma_gaussian_hmm(*[v.detach() for v in args], True)
        for u, v in zip([q2, l2, fm, fP, *g2], [raw[0], raw[1], *raw[2], *raw[3]]):
            assert torch.equal(u, v)
        assert torch.ops.pyro_amd.gamma_gaussian_hmm(*[v.detach() for v in args], False)[4] == []


@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
@pytest.mark.parametrize("key", [("A", "mix0", 9, 2), ("A", "series_Lq", 9, 2)], ids=_id)
def test_mixed_layouts(key, dtype, gpu):
    """two layouts of group A of tests/gaussian_hmm_edge_cases.py at the wide instantiation, B = 3, T = 5"""
    arrays = dict(ec.inputs(key), **_gamma(np.random.default_rng([20241103, ec.A_KEYS.index(key)]), ec.A_B))
    _check(arrays, dtype, gpu, _id(key))


@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
def test_gamma_shared_against_per_series(dtype, gpu):
    """``a`` shared and ``b`` per series, then the reverse, against the torch route; each also with the stride-0 axis
    expanded: bit for bit the same"""
    key = ("A", "hom_q", 3, 2)
    rng = np.random.default_rng(20241104)
    for shared in ("a", "b"):
        gam = _gamma(rng, ec.A_B)
        gam[shared] = gam[shared][:1]
        arrays = dict(ec.inputs(key), **gam)
        _, raw = _check(arrays, dtype, gpu, "shared " + shared)
        wide = dict(arrays, **{shared: np.repeat(gam[shared], ec.A_B)})
        t = _leaves(wide, dtype, gpu)
        args = [t["a"], t["b"]] + [v.contiguous() for v in ec.parts(t)] + [t["x"]]
        quad, logdet, filt, grads = kernels.gamma_gaussian_hmm_fwd_bwd(*[v.detach() for v in args], need_filter=True)
        for u, v in zip([quad, logdet, *filt, *grads], [raw[0], raw[1], *raw[2], *raw[3]]):
            assert torch.isfinite(u).all() and torch.equal(u, v)
    # per-series values that differ: series 1's weight must be its own (not series 0's)
    t = _leaves(dict(ec.inputs(key), **_gamma(rng, ec.A_B)), dtype, gpu)
    args = [v.detach() for v in [t["a"], t["b"]] + [v.contiguous() for v in ec.parts(t)] + [t["x"]]]
    g0 = kernels.gamma_gaussian_hmm_fwd_bwd(*args)[3]
    args[0] = args[0][[0, 0, 0]].contiguous()
    g1 = kernels.gamma_gaussian_hmm_fwd_bwd(*args)[3]
    assert torch.equal(g0[8][0], g1[8][0]) and not torch.equal(g0[8][1], g1[8][1])


def _mean_path(a):
    """the model's mean path of x for time-homogeneous, per-series inputs [B, 1, ...]"""
    z, xs = a["m0"], []
    for _ in range(a["x"].shape[1]):
        z = np.einsum("bi,bij->bj", z, a["F"][:, 0]) + a["q"][:, 0]
        xs.append(np.einsum("bi,bij->bj", z, a["H"][:, 0]) + a["r"][:, 0])
    return np.stack(xs, axis=1)


@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
@pytest.mark.parametrize("which", ["small_w", "large_w"])
def test_extreme_weights(which, dtype, gpu):
    """data far from the model (x = 20 randn: w below 0.05) and data on the model's mean path with a prior that expects
    large precisions (a = 1, b = 0.05: w above 5) -- by construction, asserted on the float64 torch route"""
    B, T, h, o = 2, 6, 4, 3
    rng = np.random.default_rng([20241105, int(which == "large_w")])
    arrays = ec.make_inputs(rng, B, T, h, o, (True,) * 6, (False,) * 6)
    if which == "small_w":
        arrays.update(_gamma(rng, B))
        arrays["x"] = 20.0 * rng.standard_normal((B, T, o))
    else:
        arrays.update(a=np.full((B,), 1.0), b=np.full((B,), 0.05))
        arrays["x"] = _mean_path(arrays) + 0.01 * rng.standard_normal((B, T, o))
    t = _leaves(arrays, F64, CPU)
    with torch.no_grad():
        quad = hmm._kalman_terms(*ec.parts(t), t["x"])[0]
        w = (t["a"] + 0.5 * T * o) / (t["b"] + 0.5 * quad)
    print(which, "w =", w.numpy())
    assert (w < 0.05).all() if which == "small_w" else (w > 5).all()
    _check(arrays, dtype, gpu, which)


# ---- the NaN convention --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
def test_a_bad_series_is_nan_and_alone(dtype, gpu):
    """series 1 of three with an R that is not positive definite: quad, logdet, the filter outputs and every gradient
    NaN there, the other two bit for bit what a run without it gives"""
    key = ("A", "step_q", 3, 2)
    p, x = ec.bad_pivot_parts(key, None, dtype, gpu)
    gam = _gamma(np.random.default_rng(20241106), 3)
    a, b = (torch.tensor(gam[k], dtype=dtype, device=gpu) for k in ("a", "b"))
    good = kernels.gamma_gaussian_hmm_fwd_bwd(a, b, *p, x, need_filter=True)
    assert p[7].shape[0] == 3
    p[7][1] = -40.0 * torch.eye(2, dtype=dtype, device=gpu)       # S = H^T P^p H + R loses its first pivot
    bad = kernels.gamma_gaussian_hmm_fwd_bwd(a, b, *p, x, need_filter=True)
    for u, v in zip([good[0], good[1], *good[2], *good[3]], [bad[0], bad[1], *bad[2], *bad[3]]):
        assert u.shape[0] == 3 and torch.isfinite(u).all() and torch.isnan(v[1]).all()
        assert torch.equal(u[0], v[0]) and torch.equal(u[2], v[2])


@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
@pytest.mark.parametrize("key", ec.E_KEYS, ids=_id)
def test_a_bad_q_marks_the_gradients_alone(key, dtype, gpu):
    """series 1 of three with a Q that only the backward sweep finds bad: finite quad and logdet (the torch route's),
    NaN gradients for that series, the other two bit for bit unchanged"""
    gam = _gamma(np.random.default_rng(20241107), 3)
    a, b = (torch.tensor(gam[k], dtype=dtype, device=gpu) for k in ("a", "b"))
    p, x = ec.bad_pivot_parts(key, None, dtype, gpu)
    good = kernels.gamma_gaussian_hmm_fwd_bwd(a, b, *p, x, need_filter=True)
    p, x = ec.bad_pivot_parts(key, "Q", dtype, gpu)
    quad, logdet, filt, grads = kernels.gamma_gaussian_hmm_fwd_bwd(a, b, *p, x, need_filter=True)
    n = x.shape[1] * x.shape[2]
    lp = hmm._student_log_prob(a, b, quad, logdet, n)

    def cpu_lp(dt):
        pc, xc = ec.bad_pivot_parts(key, "Q", dt, CPU)
        qd, ld, _, _ = hmm._kalman_terms(*pc, xc)
        return _np(hmm._student_log_prob(a.cpu().to(dt), b.cpu().to(dt), qd, ld, n))
    want = cpu_lp(F64)
    assert np.isfinite(want).all() and torch.isfinite(lp).all() and torch.isfinite(filt[0]).all()
    err, berr = ec.lp_err(_np(lp), want), ec.lp_err(cpu_lp(F32), want)
    print(_id(key), _id(dtype), "log_prob: kernel %.1e torch route on the CPU in float32 %.1e" % (err, berr))
    assert err < TOL64 if dtype == F64 else err <= max(4 * berr, ec.FLOOR32)
    for u, v in zip(good[3], grads):
        assert u.shape[0] == 3 and torch.isfinite(u).all()
        assert torch.isnan(v[1]).all() and torch.equal(u[0], v[0]) and torch.equal(u[2], v[2])
    for u, v in zip([good[0], good[1], *good[2]], [quad, logdet, *filt]):
        assert torch.equal(u[0], v[0]) and torch.equal(u[2], v[2])


# ---- routing through the class -------------------------------------------------------------------------------------
def test_the_class_reaches_the_entry_point_once_and_routes(gpu, monkeypatch):
    case = "b2_t9_h4_o3_het"
    g = ggc.golden(case)
    calls = _spy(monkeypatch)
    terms = []
    real = hmm._kalman_terms
    monkeypatch.setattr(hmm, "_kalman_terms", lambda *a: terms.append(a[-1].dtype) or real(*a))
    t = ggc.leaves(case, F64, gpu)
    lp = ggc.build(t, dist).log_prob(t["x"])
    assert len(calls) == 1 and calls[0].get("need_grads", True) and not terms
    # backward through the class fills .grad of concentration and rate (and of the rest)
    lp.sum().backward()
    assert len(calls) == 1
    for k in ggc.NAMES:
        assert t[k].grad is not None and gc.rel_err(_np(t[k].grad), g["g_" + k]) < TOL64, k
    # nothing requires a gradient: the forward-only launch
    t0 = ggc.leaves(case, F64, gpu, requires_grad=False)
    lp0 = ggc.build(t0, dist).log_prob(t0["x"])
    assert calls[1:] == [{"need_grads": False}] and not lp0.requires_grad and torch.equal(lp0, lp.detach())
    # only the Gamma requires one: still no backward sweep, the closed forms alone
    t1 = dict(t0, a=t0["a"].clone().requires_grad_(), b=t0["b"].clone().requires_grad_())
    ga, gb = torch.autograd.grad(ggc.build(t1, dist).log_prob(t1["x"]).sum(), [t1["a"], t1["b"]])
    assert calls[2:] == [{"need_grads": False}]
    assert gc.rel_err(_np(ga), g["g_a"]) < TOL64 and gc.rel_err(_np(gb), g["g_b"]) < TOL64
    del calls[:]
    # the torch route: the flag turned off, CPU tensors, float16, hidden 17
    monkeypatch.setattr(hmm, "FUSED_GAUSSIAN_HMM", False)
    off = ggc.build(t0, dist).log_prob(t0["x"])
    monkeypatch.setattr(hmm, "FUSED_GAUSSIAN_HMM", True)
    assert terms == [F64] and not calls and gc.rel_err(_np(off), g["log_prob"]) < TOL64
    tc = ggc.leaves(case, F64, CPU, requires_grad=False)
    assert torch.isfinite(ggc.build(tc, dist).log_prob(tc["x"])).all() and terms == [F64, F64] and not calls
    th = {k: v.to(torch.float16) for k, v in t0.items()}
    d16 = dist.GammaGaussianHMM(dist.Gamma(th["a"], th["b"]), dist.MultivariateNormal(t0["m0"], scale_tril=t0["L0"]),
                                th["F"], dist.MultivariateNormal(t0["q"], scale_tril=t0["Lq"]), th["H"],
                                dist.MultivariateNormal(t0["r"], scale_tril=t0["Lr"]))
    assert not d16._takes_kernel(th["x"])
    try:
        d16.log_prob(th["x"])
    except RuntimeError:                 # (torch has no float16 Cholesky; the torch route was entered all the same)
        pass
    assert terms == [F64, F64, torch.float16] and not calls
    h, o = kernels.GAUSSIAN_HMM_MAX_HIDDEN + 1, 2
    z = lambda *s: torch.zeros(*s, device=gpu)                                            # noqa: E731
    eye = lambda n: torch.eye(n, device=gpu)                                              # noqa: E731
    big = dist.GammaGaussianHMM(dist.Gamma(z(()) + 2.0, z(()) + 1.5), dist.MultivariateNormal(z(h), eye(h)),
                                0.5 * eye(h), dist.MultivariateNormal(z(h), eye(h)), torch.ones(h, o, device=gpu) / h,
                                dist.MultivariateNormal(z(o), eye(o)))
    assert torch.isfinite(big.log_prob(z(2, 3, o))).all() and len(terms) == 4 and not calls
    with pytest.raises(kernels.Unsupported):
        kernels.gamma_gaussian_hmm_fwd_bwd(z(1) + 2.0, z(1) + 1.5, z(1, h), eye(h)[None], 0.5 * eye(h)[None, None],
                                           z(1, 1, h), eye(h)[None, None], torch.ones(1, 1, h, o, device=gpu) / h,
                                           z(1, 1, o), eye(o)[None, None], z(2, 3, o))


# ---- the Gaussian path is untouched --------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
@pytest.mark.parametrize("case", gc.CASES)
def test_the_gaussian_instantiations_keep_their_tolerances(case, dtype, gpu):
    """the eight cases of gaussian_hmm.npz through kernels.gaussian_hmm_fwd_bwd: the tolerances of
    tests/test_gaussian_hmm_gpu.py (float64 1e-9; float32 four times the float32 torch route on the CPU, per kind)"""
    g = gc.golden(case)
    t = gc.leaves(case, dtype, gpu)
    d = gc.build(t, case, dist)
    batch, T = d._check_value(t["x"])
    graph = d._kernel_inputs(t["x"], batch, T)
    raw = [v.detach() for v in graph]
    lp, filt, grads = kernels.gaussian_hmm_fwd_bwd(*raw, need_grads=True, need_filter=True)
    outs = [gr if v.shape[0] == gr.shape[0] else gr.sum(0, keepdim=True) for v, gr in zip(raw, grads)]
    leaf = torch.autograd.grad(graph, [t[k] for k in gc.NAMES], grad_outputs=outs)
    err = {"log_prob": ec.lp_err(_np(lp), g["log_prob"]),
           "grad": max(gc.rel_err(_np(v), g["g_" + k]) for k, v in zip(gc.NAMES, leaf)),
           "filter": max(gc.rel_err(_np(filt[0]), g["filter_mean"]), gc.rel_err(_np(filt[1]), g["filter_cov"]))}
    if dtype == F64:
        assert max(err.values()) < TOL64, err
        return
    tc = gc.leaves(case, F32, CPU)
    blp, bgr = gc.value_and_grads(tc, case, dist)
    post = gc.build(tc, case, dist).filter(tc["x"])
    base = {"log_prob": ec.lp_err(blp, g["log_prob"]), "grad": max(gc.rel_err(bgr[k], g["g_" + k]) for k in gc.NAMES),
            "filter": max(gc.rel_err(_np(post.loc), g["filter_mean"]),
                          gc.rel_err(_np(post.covariance_matrix), g["filter_cov"]))}
    print(case, "f32 Gaussian kernel", ec.fmt(err), "| torch route on the CPU", ec.fmt(base))
    for kind in err:
        assert err[kind] <= 4 * base[kind], (kind, err, base)
