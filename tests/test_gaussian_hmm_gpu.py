"""csrc/gaussian_hmm.hip on the device: the one-launch Kalman filter with smoother gradients, through
kernels.gaussian_hmm_fwd_bwd and through pyro_amd.distributions.GaussianHMM, against the fixtures of the unmodified
reference (tests/golden/gaussian_hmm.npz, float64) and the float64 torch route of distributions/hmm.py.

Errors are |got - want| / (1 + |want|) per element for log_prob and max |got - want| / (1 + max |want|) for a
gradient or a filter moment.

float64: 1e-9, the project's golden tolerance.

float32: the kernel orders its operations differently from torch, so it gets FOUR times the error of the float32
torch route run on the CPU on the same float32 inputs, per case and kind (log_prob / the worst gradient / the worst
filter moment) -- the margin of the mixture-assignment tests.  The torch route's error is measured when the test
runs (never the kernel's); on the machine the fixtures were made on it was

    case                     log_prob   gradients   filter
    b3_t1_h2_o1              2.9e-08    1.4e-07     7.1e-08
    b3_t7_h3_o2_shared       7.7e-08    2.9e-07     1.1e-07
    b2_t9_h4_o3_het          1.3e-07    3.3e-07     1.6e-07
    b2_t33_h8_o5             7.8e-08    5.2e-07     2.1e-07
    b2_t40_h16_o16           6.1e-07    4.6e-07     2.0e-07
    b2_t17_h5_o16_het        3.5e-07    9.6e-07     2.5e-07
    b2_t12_h1_o1             2.2e-07    1.1e-06     1.6e-07
    b3_t6_h3_o2_indep        1.2e-07    4.0e-07     1.8e-07
    long chain (T = 2000)    1.6e-05    1.7e-06     -

The kernel has four instantiations, <float | double, padded dimension 8 | 16>, chosen by max(hidden, obs) <= 8, and
one launch path; the fixture cases reach all four in both modes (with and without gradients): dimensions that are
the padded size (4 x ., 8 x ., 16 x 16) and ones that are not (1, 2, 3, 5), time-homogeneous and heterogeneous,
batch-shared (stride 0) and per-sequence parameters.
"""
import functools

import numpy as np
import pytest
import torch

import pyro_amd as pyro
import pyro_amd.distributions as dist
from pyro_amd import kernels
from pyro_amd.distributions import hmm
from tests import gaussian_hmm_cases as gc
from tests.models import store_grads

pytestmark = pytest.mark.gpu
TOL64 = 1e-9
CPU = torch.device("cpu")


def _lp_err(got, want):
    return float(np.max(np.abs(np.asarray(got, dtype=np.float64) - want) / (1 + np.abs(want))))


def _errors(t, case, g):
    """{"log_prob", "grad", "filter"}: the errors of the class's route for the leaves ``t`` against the fixture"""
    lp, grads = gc.value_and_grads(t, case, dist)
    post = gc.build(t, case, dist).filter(t["x"])
    per = {"g_" + k: gc.rel_err(grads[k], g["g_" + k]) for k in gc.NAMES}
    per["filter_mean"] = gc.rel_err(post.loc.cpu().numpy(), g["filter_mean"])
    per["filter_cov"] = gc.rel_err(post.covariance_matrix.cpu().numpy(), g["filter_cov"])
    return {"log_prob": _lp_err(lp, g["log_prob"]), "grad": max(per["g_" + k] for k in gc.NAMES),
            "filter": max(per["filter_mean"], per["filter_cov"])}, per


@functools.lru_cache(maxsize=None)
def _torch_f32_errors(case):
    """the float32 torch route on the CPU against the float64 fixture (measured once per case)"""
    return _errors(gc.leaves(case, torch.float32, CPU), case, gc.golden(case))[0]


def _spy(monkeypatch):
    calls = []
    real = kernels.gaussian_hmm_fwd_bwd

    def spy(*a, **kw):
        calls.append(kw)
        return real(*a, **kw)
    monkeypatch.setattr(kernels, "gaussian_hmm_fwd_bwd", spy)
    return calls


def _raw(case, dtype, gpu):
    """the case in the layouts of kernels.gaussian_hmm_fwd_bwd (detached), the leaves and the graph between them"""
    t = gc.leaves(case, dtype, gpu)
    d = gc.build(t, case, dist)
    batch, T = d._check_value(t["x"])
    graph = d._kernel_inputs(t["x"], batch, T)
    return t, graph, [a.detach() for a in graph]


@pytest.mark.parametrize("case", gc.CASES)
def test_fixtures_float64(case, gpu, monkeypatch):
    g = gc.golden(case)
    calls = _spy(monkeypatch)
    err, per = _errors(gc.leaves(case, torch.float64, gpu), case, g)
    print(case, "f64", err, {k: "%.1e" % v for k, v in per.items()})
    assert len(calls) == 2                       # log_prob with its gradients, filter
    assert max(err.values()) < TOL64, (err, per)
    # ... and through kernels.gaussian_hmm_fwd_bwd itself: its gradients pushed to the leaves by torch
    t, graph, raw = _raw(case, torch.float64, gpu)
    lp, filt, grads = kernels.gaussian_hmm_fwd_bwd(*raw, need_grads=True, need_filter=True)
    assert _lp_err(lp.cpu().numpy(), g["log_prob"]) < TOL64
    assert gc.rel_err(filt[0].cpu().numpy(), g["filter_mean"]) < TOL64
    assert gc.rel_err(filt[1].cpu().numpy(), g["filter_cov"]) < TOL64
    # (a step axis of 1 is already summed by the kernel; the sum over the sequences of a shared parameter is ours)
    outs = [gr if a.shape[0] == gr.shape[0] else gr.sum(0, keepdim=True) for a, gr in zip(raw, grads)]
    leaf = torch.autograd.grad(graph, [t[k] for k in gc.NAMES], grad_outputs=outs)
    for k, v in zip(gc.NAMES, leaf):
        assert gc.rel_err(v.cpu().numpy(), g["g_" + k]) < TOL64, k


@pytest.mark.parametrize("case", gc.CASES)
def test_fixtures_float32(case, gpu, monkeypatch):
    g = gc.golden(case)
    base = _torch_f32_errors(case)
    calls = _spy(monkeypatch)
    err, per = _errors(gc.leaves(case, torch.float32, gpu), case, g)
    print(case, "f32 kernel", err, "torch route on the CPU", base, {k: "%.1e" % v for k, v in per.items()})
    assert len(calls) == 2
    for kind in ("log_prob", "grad", "filter"):
        assert err[kind] <= 4 * base[kind], (kind, err, base, per)


def _long_chain(dtype, device):
    gen = torch.Generator().manual_seed(7)
    B, T, h, o = 2, 2000, 4, 2
    r = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64)                    # noqa: E731

    def tril(n):
        A = r(B, 1, n, n)
        return torch.linalg.cholesky(A @ A.transpose(-1, -2) / n + 0.5 * torch.eye(n, dtype=torch.float64))
    F = r(B, 1, h, h)
    F = F * (0.9 / torch.linalg.matrix_norm(F, ord=2))[..., None, None]
    t = {"m0": 0.3 * r(B, h), "L0": tril(h)[:, 0], "F": F, "q": 0.3 * r(B, 1, h), "Lq": tril(h),
         "H": r(B, 1, h, o) / h ** 0.5, "r": 0.3 * r(B, 1, o), "Lr": tril(o), "x": 2.0 * r(B, T, o)}
    return {k: v.to(dtype).to(device).requires_grad_() for k, v in t.items()}


def test_long_stable_chain_float32(gpu, monkeypatch):
    """B = 2, T = 2000, hidden 4, obs 2 in float32 against the float64 torch route; the same 4x rule"""
    case = "long"
    want_lp, want_g = gc.value_and_grads(_long_chain(torch.float64, CPU), case, dist)
    base_lp, base_g = gc.value_and_grads(_long_chain(torch.float32, CPU), case, dist)
    base = (_lp_err(base_lp, want_lp), max(gc.rel_err(base_g[k], want_g[k]) for k in gc.NAMES))
    calls = _spy(monkeypatch)
    lp, grads = gc.value_and_grads(_long_chain(torch.float32, gpu), case, dist)
    err = (_lp_err(lp, want_lp), max(gc.rel_err(grads[k], want_g[k]) for k in gc.NAMES))
    print("long chain: kernel", err, "torch route on the CPU", base)
    assert len(calls) == 1
    assert err[0] <= 4 * base[0] and err[1] <= 4 * base[1], (err, base)


def test_empty_batch_and_limits(gpu, monkeypatch):
    z = lambda *s: torch.zeros(*s, device=gpu)                                            # noqa: E731
    lp, filt, grads = kernels.gaussian_hmm_fwd_bwd(z(1, 3), z(1, 3, 3), z(1, 1, 3, 3), z(1, 1, 3), z(1, 1, 3, 3),
                                                   z(1, 1, 3, 2), z(1, 1, 2), z(1, 1, 2, 2), z(0, 5, 2),
                                                   need_grads=True, need_filter=True)
    assert lp.shape == (0,) and filt[0].shape == (0, 3) and grads[2].shape == (0, 1, 3, 3) and grads[8].shape == (0, 5, 2)
    for h, o in ((kernels.GAUSSIAN_HMM_MAX_HIDDEN + 1, 2), (2, kernels.GAUSSIAN_HMM_MAX_OBS + 1)):
        eye = lambda n: torch.eye(n, device=gpu)                                          # noqa: E731
        args = (z(1, h), eye(h)[None], 0.5 * eye(h)[None, None], z(1, 1, h), eye(h)[None, None],
                torch.ones(1, 1, h, o, device=gpu) / h, z(1, 1, o), eye(o)[None, None], z(2, 3, o))
        with pytest.raises(kernels.Unsupported):
            kernels.gaussian_hmm_fwd_bwd(*args)
        # the class takes its torch route
        calls = _spy(monkeypatch)
        d = dist.GaussianHMM(dist.MultivariateNormal(z(h), eye(h)), 0.5 * eye(h), dist.MultivariateNormal(z(h), eye(h)),
                             torch.ones(h, o, device=gpu) / h, dist.MultivariateNormal(z(o), eye(o)))
        assert torch.isfinite(d.log_prob(z(2, 3, o))).all() and not calls
        monkeypatch.undo()


def test_a_bad_sequence_is_nan_and_alone(gpu):
    """one sequence of three with an R that is not positive definite: NaN there, the other two bit for bit what
    a run without it gives"""
    case = "b3_t7_h3_o2_shared"
    _, _, raw = _raw(case, torch.float32, gpu)
    m0, P0, F, q, Q, H, r, R, x = raw
    R3 = R.expand(3, *R.shape[1:]).contiguous()
    good = kernels.gaussian_hmm_fwd_bwd(m0, P0, F, q, Q, H, r, R3, x, need_filter=True)
    Rb = R3.clone()
    Rb[1] = -40.0 * torch.eye(R.shape[-1], device=gpu)          # S = H^T P^p H + R loses its first pivot
    bad = kernels.gaussian_hmm_fwd_bwd(m0, P0, F, q, Q, H, r, Rb, x, need_filter=True)
    outs_good = [good[0], *good[1], *good[2]]
    outs_bad = [bad[0], *bad[1], *bad[2]]
    for a, b in zip(outs_good, outs_bad):
        assert a.shape[0] == 3
        assert torch.isnan(b[1]).all() and torch.isfinite(a).all()
        assert torch.equal(a[0], b[0]) and torch.equal(a[2], b[2])


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_stride_zero_equals_expanded(dtype, gpu):
    """shared, time-homogeneous parameters passed with stride 0 and the same values expanded per sequence and
    per step: identical log_prob bits; the expanded gradients summed over the steps agree within the float
    tolerance (the kernel sums in its own order)"""
    case = "b3_t7_h3_o2_shared"
    _, _, raw = _raw(case, dtype, gpu)
    x = raw[-1]
    B, T, _ = x.shape
    lp0, f0, g0 = kernels.gaussian_hmm_fwd_bwd(*raw, need_filter=True)
    assert all(a.shape[0] == 1 and a.shape[1] == 1 for a in raw[2:8])
    wide = [raw[0], raw[1]] + [a.expand(B, T, *a.shape[2:]).contiguous() for a in raw[2:8]] + [x]
    lp1, f1, g1 = kernels.gaussian_hmm_fwd_bwd(*wide, need_filter=True)
    assert torch.equal(lp0, lp1) and torch.equal(f0[0], f1[0]) and torch.equal(f0[1], f1[1])
    tol = 1e-12 if dtype == torch.float64 else 16 * T * 2.0 ** -24     # T terms of either sign, f32 epsilon each
    for i, (a, b) in enumerate(zip(g0, g1)):
        if 2 <= i < 8:
            assert a.shape[1] == 1 and b.shape[1] == T
            b = b.sum(1, keepdim=True)
        assert gc.rel_err(a.cpu().numpy(), b.cpu().numpy()) <= tol, i


@pytest.mark.parametrize("case", ["b2_t33_h8_o5", "b2_t17_h5_o16_het"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_reproducible_and_forward_only(case, dtype, gpu):
    """two runs give identical bits; without gradient pointers log_prob and the filter moments keep the gradient
    run's bits, and there is no per-step workspace"""
    from pyro_amd import _lib
    _, _, raw = _raw(case, dtype, gpu)
    a = kernels.gaussian_hmm_fwd_bwd(*raw, need_filter=True)
    b = kernels.gaussian_hmm_fwd_bwd(*raw, need_filter=True)
    for u, v in zip([a[0], *a[1], *a[2]], [b[0], *b[1], *b[2]]):
        assert torch.equal(u, v)
    lp, filt, none = kernels.gaussian_hmm_fwd_bwd(*raw, need_grads=False, need_filter=True)
    assert none is None and torch.equal(lp, a[0]) and torch.equal(filt[0], a[1][0]) and torch.equal(filt[1], a[1][1])
    B, T, o = raw[-1].shape
    h = raw[0].shape[-1]
    dt = _lib.PA_F32 if dtype == torch.float32 else _lib.PA_F64
    assert _lib.load().pa_gaussian_hmm_workspace(dt, B, T, h, o, 0) == 0
    assert _lib.load().pa_gaussian_hmm_workspace(dt, B, T, h, o, 1) == B * T * (h + h * h) * raw[0].element_size()


def test_no_grad_inputs_take_the_forward_only_launch(gpu, monkeypatch):
    calls = _spy(monkeypatch)
    t = gc.leaves("b2_t9_h4_o3_het", torch.float64, gpu, requires_grad=False)
    lp = gc.build(t, "b2_t9_h4_o3_het", dist).log_prob(t["x"])
    assert calls == [{"need_grads": False}] and not lp.requires_grad
    assert _lp_err(lp.cpu().numpy(), gc.golden("b2_t9_h4_o3_het")["log_prob"]) < TOL64
    monkeypatch.setattr(hmm, "FUSED_GAUSSIAN_HMM", False)                  # the switch: the torch route on the device
    lp2 = gc.build(t, "b2_t9_h4_o3_het", dist).log_prob(t["x"])
    assert len(calls) == 1 and _lp_err(lp2.cpu().numpy(), gc.golden("b2_t9_h4_o3_het")["log_prob"]) < TOL64


def test_through_the_public_seam(gpu, monkeypatch):
    """a plate of series observed through GaussianHMM with pyro.param parameters and an empty guide: Trace_ELBO's
    loss is minus the fixture's summed log_prob, its gradients land in the param store -- on the kernel"""
    from pyro_amd.infer import Trace_ELBO
    case = "b2_t33_h8_o5"
    g = gc.golden(case)
    x = torch.tensor(g["x"], device=gpu)
    B = x.shape[0]

    def model():
        t = {k: pyro.param(k, torch.tensor(g[k], device=gpu)) for k in gc.NAMES if k != "x"}
        with pyro.plate("series", B):
            pyro.sample("y", gc.build(t, case, dist), obs=x)

    pyro.clear_param_store()
    calls = _spy(monkeypatch)
    loss = Trace_ELBO().loss_and_grads(model, lambda: None)
    assert len(calls) == 1 and calls[0].get("need_grads", True)
    np.testing.assert_allclose(loss, -g["log_prob"].sum(), rtol=TOL64)
    grads = store_grads()
    for k in gc.NAMES:
        if k != "x":
            assert gc.rel_err(-grads[k], g["g_" + k]) < TOL64, k
    pyro.clear_param_store()


@pytest.mark.parametrize("K", [3, 16])
@pytest.mark.parametrize("T", [1, 9])
def test_discrete_hmm_filter(K, T, gpu):
    """DiscreteHMM.filter against a float64 forward recursion in torch"""
    gen = torch.Generator().manual_seed(100 * K + T)
    B, V = 3, 5
    init = torch.randn(B, K, generator=gen, dtype=torch.float64)
    trans = torch.randn(B, 1, K, K, generator=gen, dtype=torch.float64)
    emit = torch.randn(K, V, generator=gen, dtype=torch.float64)
    data = torch.randint(0, V, (B, T), generator=gen)
    a = init.log_softmax(-1)
    for t in range(T):
        a = torch.logsumexp(a.unsqueeze(-1) + trans[:, 0].log_softmax(-1), dim=-2) + emit.log_softmax(-1)[:, data[:, t]].T
    want = a.softmax(-1)
    # float32: the log-potentials (|.| up to ~10) pass through T + 1 log-sum-exps over K terms, each good to a few
    # epsilon of its value: 1e-5 on a probability is ten times that
    for dtype, tol in ((torch.float64, 1e-12), (torch.float32, 1e-5)):
        d = dist.DiscreteHMM(init.to(gpu, dtype), trans.to(gpu, dtype), dist.Categorical(logits=emit.to(gpu, dtype)))
        post = d.filter(data.to(gpu))
        assert isinstance(post, dist.Categorical) and post.batch_shape == (B,)
        np.testing.assert_allclose(post.probs.cpu().double().numpy(), want.numpy(), atol=tol, rtol=0)
