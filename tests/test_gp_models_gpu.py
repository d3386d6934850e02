"""GPRegression and SparseGPRegression on the device, every step eager (nothing is captured into a graph).

float64: the fixture's models (tests/golden/gp.npz, the unmodified reference) -- losses, parameter gradients, ``forward``,
``conditional`` and the ten training losses -- within ten times the deviation the reference shows against itself under
a 1e-13 perturbation of its inputs (gp_cases.allowed).  The Cholesky factor is the device's own, hence not 1e-12.

float32: the same quantities -- losses and parameter gradients (plain and with the prior), ``forward``, ``conditional``
and the ten training losses -- within four times the error of the float32 torch route on the CPU, both against the
fixture (_f32_bound; that route's error is taken over CPU_SAMPLES float32 roundings of the same inputs, _cpu_inputs).

Models the fixture does not hold (Sum / Product kernels, the few-row sparse model) are compared with the same model on
the CPU in float64 (torch route) within 16 N 2^-52 cond (1 + |value|), cond the condition number of the factorised
matrix: first-order perturbation of a Cholesky solve, not a measurement."""
import numpy as np
import pytest
import torch

import pyro_amd as pyro
import pyro_amd.contrib.gp as gp
import pyro_amd.distributions as dist
from pyro_amd.infer import Trace_ELBO
from pyro_amd.nn import PyroSample

from . import gp_cases as gc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, F64 = torch.float32, torch.float64


@pytest.fixture(autouse=True)
def _clean():
    pyro.clear_param_store()
    yield
    pyro.clear_param_store()


def _within(got, key, g, tag=""):
    want, other = g[key], g[key.rsplit("/", 1)[0] + "/p_" + key.rsplit("/", 1)[1]]
    got = np.asarray(got)
    assert got.shape == want.shape, (key, got.shape, want.shape)
    dev, allowed = np.abs(got - want), gc.allowed(want, other)
    print("%s%s: largest deviation %.2e, allowed there %.2e" % (tag, key, dev.max(), np.broadcast_to(allowed, dev.shape).flat[dev.argmax()]))
    assert (dev <= allowed).all(), (key, dev.max(), allowed)


@pytest.mark.parametrize("name", gc.MODELS)
@pytest.mark.parametrize("variant", ["plain", "prior"])
def test_f64_loss_and_gradients_within_the_reference_sensitivity(name, variant):
    g, data = gc.golden(), gc.fixture_data()
    model = gc.build_model(gp, name, data, prior=(PyroSample, dist) if variant == "prior" else None, device=DEV)
    loss, grads = gc.loss_and_grads(model, Trace_ELBO())
    key = "model/%s/%s/" % (name, variant)
    _within(loss, key + "loss", g)
    assert sorted(grads) == sorted(k[len(key + "grad_"):] for k in g if k.startswith(key + "grad_"))
    for pname, value in grads.items():
        _within(value, key + "grad_" + pname, g)


@pytest.mark.parametrize("name", gc.MODELS)
def test_f64_forward_and_training_within_the_reference_sensitivity(name):
    g, data = gc.golden(), gc.fixture_data()
    model = gc.build_model(gp, name, data, device=DEV)
    for full, noiseless in gc.FORWARD_CASES:
        with torch.no_grad():
            loc, cov = model(data["Xnew"].to(DEV), full_cov=full, noiseless=noiseless)
        key = "model/%s/forward/%d%d/" % (name, full, noiseless)
        _within(loc.cpu().numpy(), key + "loc", g)
        _within(cov.cpu().numpy(), key + "cov", g)
    pyro.clear_param_store()          # (a second model of the same names: the store would hand it the first one's Xu)
    model = gc.build_model(gp, name, data, device=DEV)
    losses = gp.util.train(model, torch.optim.Adam(model.parameters(), lr=0.01), num_steps=gc.TRAIN_STEPS)
    _within(np.array(losses), "model/%s/train" % name, g)


@pytest.mark.parametrize("scale,whiten,full", gc.CONDITIONAL_CASES)
def test_f64_conditional_within_the_reference_sensitivity(scale, whiten, full):
    g, data = gc.golden(), gc.fixture_data()
    kern = gc.kernel_table(gp)["matern52_ard"].to(DEV)
    d = {k: v.to(DEV) for k, v in data.items()}
    with torch.no_grad():
        loc, cov = gp.util.conditional(d["Xnew"], d["X"], kern, d["f_loc"], d["f_scale_tril"] if scale else None,
                                       full_cov=full, whiten=whiten)
    key = "cond/%d%d%d/" % (scale, whiten, full)
    _within(loc.cpu().numpy(), key + "loc", g)
    _within(cov.cpu().numpy(), key + "cov", g)


def _plain_loss(model):
    """-log p(y) of a model with no priors, from torch.distributions (what Trace_ELBO's loss is for an empty guide)."""
    import torch.distributions as td
    N = model.X.size(0)
    zero = model.X.new_zeros(N)
    if isinstance(model, gp.models.SparseGPRegression):
        _, Wt = model._inducing()
        W, D = Wt.t(), model.noise.expand(N)
        residual = model.kernel(model.X, diag=True) - W.pow(2).sum(-1)
        extra = 0.0
        if model.approx == "FITC":
            D = D + residual
        elif model.approx == "VFE":
            extra = (residual.sum() / model.noise).clamp(min=0) / 2
        return extra - td.LowRankMultivariateNormal(zero, W, D).log_prob(model.y)
    return -td.MultivariateNormal(zero, scale_tril=model._factor()).log_prob(model.y)


CPU_SAMPLES = 5


def _cpu_inputs(data):
    """The fixture's inputs CPU_SAMPLES times: as they are, then with every entry moved by one float32 spacing up or
    down (seeded).  The float32 inputs are roundings of the float64 fixture already, so each of these is the same
    problem as float32 sees it, and the CPU torch route's error on them is that route's error CPU_SAMPLES times over.  One
    evaluation alone is one draw of a rounding error: the device's factorisation draws another, and a single draw
    exceeds four times another single draw of the same spread about one time in six."""
    g = np.random.default_rng(11)
    yield data
    for _ in range(CPU_SAMPLES - 1):
        yield {k: v * (1 + 2.0 ** -23 * torch.as_tensor(g.choice([-1.0, 1.0], size=tuple(v.shape)))) for k, v in data.items()}


def _f32_bound(want, cpus, spacings=1):
    """Four times the error of the float32 torch route on the CPU, entry by entry: the largest over its evaluations of
    _cpu_inputs.  Two things stand in where that error happens to vanish, neither of them a tolerance of its own: within
    an array, the largest error of the same array, unscaled (the rule of gp_cases.allowed: the entries come out of the
    same rounded arithmetic); and ``spacings`` spacings of float32 at the value's own magnitude.  One, for a quantity
    that is rounded once: below it a float32 result cannot be told from the truth.  Two for a loss: it is assembled in
    float32 from three terms of its own magnitude or larger (the quadratic form, the log-determinant, N/2 log 2 pi),
    each rounded and each sum rounded again, so float32 arithmetic promises three half-spacings of the largest, not the
    correctly rounded value -- which the CPU happens to return for the exact model in every one of its evaluations."""
    want = np.asarray(want, dtype=np.float64)
    own = np.max([np.abs(np.asarray(c, dtype=np.float64) - want) for c in cpus], axis=0)
    return own, np.maximum(np.maximum(4 * own, own.max() if own.size > 1 else 0.0),
                           spacings * np.spacing(np.abs(want).astype(np.float32)).astype(np.float64))


def _np64(t):
    return np.asarray(t.detach().cpu().double().numpy() if isinstance(t, torch.Tensor) else t, dtype=np.float64)


def _check_f32(label, got, cpus, want, spacings=1):
    got = _np64(got)
    own, bound = _f32_bound(want, [_np64(c) for c in cpus], spacings)
    dev = np.abs(got - want)
    print("%s: largest error %.2e, allowed there %.2e (CPU torch route %.2e)"
          % (label, dev.max(), np.broadcast_to(bound, dev.shape).flat[dev.argmax()], own.max()))
    assert got.shape == np.shape(want) and (dev <= bound).all(), (label, dev.max())


def _cpu_loss_and_grads(name, data, prior):
    """What Trace_ELBO's loss is for these guides, from torch.distributions on the CPU in float32: -log p(y | theta), and
    with the LogNormal(0, 1) prior under its point-mass guide, - log p(lengthscale) at the guide's point.  (The package's
    own distributions draw on the device only, so the CPU model carries the point as its plain lengthscale parameter:
    the same unconstrained leaf under another name.)"""
    import torch.distributions as td
    model = gc.build_model(gp, name, data, dtype=F32)
    if prior:
        model.kernel.lengthscale = torch.tensor(gc.LENGTHSCALE_AT, dtype=F32)
    loss = _plain_loss(model)
    if prior:
        point = model.kernel.lengthscale
        loss = loss - td.LogNormal(torch.zeros_like(point), torch.ones_like(point)).log_prob(point).sum()
    loss.backward()
    rename = {"kernel.lengthscale_unconstrained": "kernel.lengthscale_map_unconstrained"} if prior else {}
    return loss.detach(), {rename.get(n, n): p.grad.detach().clone() for n, p in model.named_parameters()}


@pytest.mark.parametrize("name", gc.MODELS)
@pytest.mark.parametrize("variant", ["plain", "prior"])
def test_f32_loss_and_gradients_within_four_times_the_cpu_torch_route(name, variant):
    g, data = gc.golden(), gc.fixture_data()
    prior = (PyroSample, dist) if variant == "prior" else None
    # (two models of one name share the parameter store: the CPU model is evaluated first, then the store is cleared)
    cpu = []
    for inputs in _cpu_inputs(data):
        pyro.clear_param_store()
        cpu.append(_cpu_loss_and_grads(name, inputs, prior))
    pyro.clear_param_store()
    loss, grads = gc.loss_and_grads(gc.build_model(gp, name, data, prior=prior, dtype=F32, device=DEV), Trace_ELBO())
    key = "model/%s/%s/" % (name, variant)
    _check_f32(key + "loss", loss, [c[0] for c in cpu], g[key + "loss"], spacings=2)
    assert sorted(grads) == sorted(cpu[0][1]) == sorted(k[len(key + "grad_"):] for k in g if k.startswith(key + "grad_"))
    for pname, value in grads.items():
        _check_f32(key + "grad_" + pname, value, [c[1][pname] for c in cpu], g[key + "grad_" + pname])


@pytest.mark.parametrize("name", gc.MODELS)
def test_f32_forward_and_training_within_four_times_the_cpu_torch_route(name):
    g, data = gc.golden(), gc.fixture_data()
    cpu_forward, cpu_losses = [], []
    for inputs in _cpu_inputs(data):
        pyro.clear_param_store()
        on_cpu = gc.build_model(gp, name, inputs, dtype=F32)
        with torch.no_grad():
            cpu_forward.append([on_cpu(inputs["Xnew"].to(F32), full_cov=full, noiseless=noiseless)
                                for full, noiseless in gc.FORWARD_CASES])
        optimizer, losses = torch.optim.Adam(on_cpu.parameters(), lr=0.01), []
        for _ in range(gc.TRAIN_STEPS):
            optimizer.zero_grad()
            loss = _plain_loss(on_cpu)
            loss.backward()
            optimizer.step()
            losses.append(loss.item())
        cpu_losses.append(np.array(losses))
    pyro.clear_param_store()
    on_dev = gc.build_model(gp, name, data, dtype=F32, device=DEV)
    with torch.no_grad():
        for n, (full, noiseless) in enumerate(gc.FORWARD_CASES):
            loc, cov = on_dev(data["Xnew"].to(DEV, F32), full_cov=full, noiseless=noiseless)
            key = "model/%s/forward/%d%d/" % (name, full, noiseless)
            _check_f32(key + "loc", loc, [c[n][0] for c in cpu_forward], g[key + "loc"])
            _check_f32(key + "cov", cov, [c[n][1] for c in cpu_forward], g[key + "cov"])
    pyro.clear_param_store()
    on_dev = gc.build_model(gp, name, data, dtype=F32, device=DEV)
    losses = gp.util.train(on_dev, torch.optim.Adam(on_dev.parameters(), lr=0.01), num_steps=gc.TRAIN_STEPS)
    _check_f32("model/%s/train" % name, np.array(losses), cpu_losses, g["model/%s/train" % name], spacings=2)


@pytest.mark.parametrize("scale,whiten,full", gc.CONDITIONAL_CASES)
def test_f32_conditional_within_four_times_the_cpu_torch_route(scale, whiten, full):
    g, data = gc.golden(), gc.fixture_data()
    key = "cond/%d%d%d/" % (scale, whiten, full)
    def run(inputs, device):
        pyro.clear_param_store()
        kern = gc.kernel_table(gp)["matern52_ard"].to(device, F32)
        d = {k: v.to(device, F32) for k, v in inputs.items()}
        with torch.no_grad():
            return gp.util.conditional(d["Xnew"], d["X"], kern, d["f_loc"], d["f_scale_tril"] if scale else None,
                                       full_cov=full, whiten=whiten)

    cpu = [run(inputs, "cpu") for inputs in _cpu_inputs(data)]
    loc, cov = run(data, DEV)
    _check_f32(key + "loc", loc, [c[0] for c in cpu], g[key + "loc"])
    _check_f32(key + "cov", cov, [c[1] for c in cpu], g[key + "cov"])


def test_launch_counts(monkeypatch):
    from pyro_amd import kernels
    calls = []
    real_fwd, real_bwd = kernels.gp_kernel_fwd, kernels.gp_kernel_bwd
    monkeypatch.setattr(kernels, "gp_kernel_fwd", lambda *a, **k: calls.append("fwd") or real_fwd(*a, **k))
    monkeypatch.setattr(kernels, "gp_kernel_bwd", lambda *a, **k: calls.append("bwd") or real_bwd(*a, **k))
    data = gc.fixture_data()
    for name, covariances in (("gpr", 1), ("sgpr_DTC", 2), ("sgpr_FITC", 2), ("sgpr_VFE", 2)):
        model = gc.build_model(gp, name, data, device=DEV)
        del calls[:]
        loss = Trace_ELBO().differentiable_loss(model.model, model.guide)
        assert calls == ["fwd"] * covariances, (name, calls)
        loss.backward()
        assert calls.count("fwd") == covariances and 1 <= calls.count("bwd") <= 2 * covariances, (name, calls)
        del calls[:]
        monkeypatch.setattr(gp.kernels, "FUSED_GP_KERNEL", False)
        Trace_ELBO().differentiable_loss(model.model, model.guide).backward()
        monkeypatch.setattr(gp.kernels, "FUSED_GP_KERNEL", True)
        assert calls == [], name


def _loss_and_grads_by_autograd(model):
    for p in model.parameters():
        p.grad = None
    loss = _plain_loss(model)
    loss.backward()
    return float(loss.detach()), {n: p.grad.detach().cpu().double().numpy() for n, p in model.named_parameters()}


def _condition_bound(model, value):
    with torch.no_grad():
        if isinstance(model, gp.models.SparseGPRegression):
            Kuu = model.kernel(model.Xu).contiguous()
            Kuu.view(-1)[::Kuu.size(0) + 1] += model.jitter
            cond = torch.linalg.cond(Kuu).item()
        else:
            L = model._factor()
            cond = torch.linalg.cond(L @ L.t()).item()
    return 16 * model.X.size(0) * gc.EPS64 * cond * (1 + np.abs(value).max())


@pytest.mark.parametrize("which", ["sum", "product"])
def test_sum_and_product_kernels_through_gpregression(which):
    data = gc.fixture_data()
    on_cpu = gc.build_model(gp, "gpr", data, which=which)
    on_dev = gc.build_model(gp, "gpr", data, which=which, device=DEV)
    want_loss, want_grads = _loss_and_grads_by_autograd(on_cpu)
    loss, grads = gc.loss_and_grads(on_dev, Trace_ELBO())
    assert abs(loss - want_loss) <= _condition_bound(on_cpu, want_loss)
    assert sorted(grads) == sorted(want_grads)
    for pname, value in grads.items():
        assert (np.abs(value - want_grads[pname]) <= _condition_bound(on_cpu, want_grads[pname])).all(), pname


def test_sparse_model_with_few_inducing_rows(monkeypatch):
    from pyro_amd import kernels
    g = np.random.default_rng(5)
    X = torch.as_tensor(g.standard_normal((300, 3)))
    data = {"X": X, "y": torch.sin(X[:, 0]) + 0.1 * torch.as_tensor(g.standard_normal(300)), "Xu": X[::43][:7] + 0.01}
    shapes = []
    real_bwd = kernels.gp_kernel_bwd
    monkeypatch.setattr(kernels, "gp_kernel_bwd", lambda x, z, *a, **k: shapes.append((x.shape[0], None if z is None else z.shape[0]))
                        or real_bwd(x, z, *a, **k))
    on_cpu = gc.build_model(gp, "sgpr_VFE", data)
    on_dev = gc.build_model(gp, "sgpr_VFE", data, device=DEV)
    want_loss, want_grads = _loss_and_grads_by_autograd(on_cpu)
    loss, grads = gc.loss_and_grads(on_dev, Trace_ELBO())
    assert (7, 300) in shapes                          # Kuf: 7 rows against 300 columns, split by the plan
    assert abs(loss - want_loss) <= _condition_bound(on_cpu, want_loss)
    for pname, value in grads.items():
        assert (np.abs(value - want_grads[pname]) <= _condition_bound(on_cpu, want_grads[pname])).all(), pname
