"""The periodic covariance kernel (csrc/gp_periodic.hip) per element on the device, f32 and f64.

Truth: the float64 restatement (tests/gp_periodic_cases.py) on the inputs AS THE KERNEL SEES THEM (f32 inputs cast up).
f64 bounds -- those of tests/test_gp_kernel_gpu.py with the angle's conditioning made explicit (derivations, not
measurements), C = max_ij sum_k (2 / l_k^2) |theta sin 2 theta| and Theta = max |theta| of the case:
    K, gx, gz                           2^-52 * 16 (D + 8) * (1 + A) * (1 + C + 2 Theta),   A the largest magnitude of that output
    lengthscale / period / variance     2^-52 (N M + 16 D) * S * (1 + C + 2 Theta),   S the sum of absolute summands
f32 bounds -- the project's rule: four times the error of the float32 twin of the restatement, with floor
4 * 2^-23 (1 + A), or 4 * 2^-23 * S for the reduced gradients.  (With sinpif in the exponent the kernel missed the f32
bound of the per-feature gradients at D = 64 by 1.7: the kernel was wrong and was changed, see its gpp_sinpi_reduced.)"""
import itertools

import numpy as np
import pytest
import torch

from . import gp_cases as gc
from . import gp_periodic_cases as pc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = {"f32": torch.float32, "f64": torch.float64}
NAMES = ("gx", "gz", "g_ls", "g_period", "g_var")
SUMS = {"g_ls": "S_ls", "g_period": "S_period", "g_var": "S_var"}


@pytest.fixture(scope="module")
def kernels():
    from pyro_amd import kernels as k
    return k


def _compare(got, x, z, ls, period, var, G, label=""):
    """``got``: name -> tensor or None (not wanted).  Asserts every output within its bound; returns the worst error /
    bound and, per output, (the worst error, the float32 twin's own)."""
    dtype, (N, D) = x.dtype, x.shape
    M = N if z is None else z.shape[0]
    up = lambda t: None if t is None else t.double()      # noqa: E731
    truth = pc.restate(up(x), up(z), up(ls), up(period), up(var), up(G))
    twin = pc.restate(x, z, ls, period, var, G) if dtype == torch.float32 else truth
    cond = 1 + truth["C"] + 2 * truth["Theta"]
    worst, errors = 0.0, {}
    for name, value in got.items():
        if value is None:
            continue
        t, S = truth[name], truth.get(SUMS.get(name))
        assert value.shape == t.shape and value.dtype == dtype and torch.isfinite(value).all(), (label, name)
        A, own = t.abs().max().item(), (twin[name].double() - t).abs()
        if dtype == torch.float64:
            bound = torch.as_tensor(gc.EPS64 * cond * (16 * (D + 8) * (1 + A) if S is None else (N * M + 16 * D) * S))
        else:
            bound = torch.maximum(4 * own, torch.as_tensor(4 * gc.EPS32 * ((1 + A) if S is None else S), dtype=torch.float64))
        err = (value.cpu().double() - t).abs()
        ratio = (err / bound.clamp(min=1e-300)).max().item()
        worst, errors[name] = max(worst, ratio), (err.max().item(), own.max().item())
        assert (err <= bound).all(), "%s %s N=%d M=%d D=%d: error / bound %.3g (error %.3g)" % (
            label, name, N, M, D, ratio, err.max().item())
    return worst, errors


def _inputs(N, M, D, dtype, mode, seed=0, shift=0.0, zmode="given", ls=None, period=None):
    x = gc.points(seed, N, D, shift).to(dtype)
    z = None if zmode == "null" else (x if zmode == "same" else gc.points(seed + 50, M, D, shift).to(dtype))
    if zmode == "given" and N >= 5 and M >= 6:
        z[5] = x[4]                                         # an exact duplicate off the diagonal
    lsv, pv, var = pc.parameters(seed, D, *mode)
    lsv = lsv if ls is None else torch.full_like(lsv, ls)
    pv = pv if period is None else torch.full_like(pv, period)
    G = torch.as_tensor(np.random.default_rng(seed + 7).standard_normal((N, N if z is None else z.shape[0])))
    return x, z, lsv.to(dtype), pv.to(dtype), var.to(dtype), G.to(dtype)


def _check(kernels, N, M, D, dtype, mode, want=(True,) * 5, forced=0, **kw):
    cpu = _inputs(N, M, D, dtype, mode, **kw)
    x, z, ls, period, var, G = (None if t is None else t.to(DEV) for t in cpu)
    z = x if kw.get("zmode") == "same" else z
    got = {"K": kernels.gp_periodic_fwd(x, z, ls, period, var)}
    for name, w, value in zip(NAMES, want, kernels.gp_periodic_bwd(x, z, ls, period, var, G, want, forced)):
        assert (value is not None) == bool(w and (name != "gz" or z is not None)), (kw, name)
        got[name] = value
    return _compare(got, *cpu, label=str((forced, kw)))


SHAPES = [(1, 1, 1), (2, 1, 2), (63, 64, 4), (64, 65, 5), (65, 63, 8), (130, 64, 16), (64, 130, 17), (130, 130, 63),
          (63, 2, 64), (130, 65, 64)]
EDGES = {      # the tiling and split edges of the stationary kernel's test; z = None and z the same tensor; extremes
    "shapes": [(s, dict(forced=f, seed=n)) for n, (s, f) in enumerate(zip(SHAPES, itertools.cycle([0, 1, 2, 7])))],
    "z": [((N, N, D), dict(forced=f, seed=n, zmode=zm)) for n, (N, D, f) in enumerate(
        zip([1, 63, 64, 65, 130], [1, 5, 8, 17, 64], [0, 2, 1, 7, 0])) for zm in ("null", "same")],
    "extreme": [((40, 33, 3), kw) for kw in ({"ls": 1e-3}, {"ls": 1e3}, {"period": 1e-2})]}


@pytest.mark.parametrize("dt,mode", list(itertools.product(sorted(DTYPES), pc.MODES)))
@pytest.mark.parametrize("group", sorted(EDGES))
def test_edges(kernels, group, dt, mode):
    worst = max(_check(kernels, *shape, DTYPES[dt], mode, **kw)[0] for shape, kw in EDGES[group])
    print("%s %s %s: worst error / bound %.3f" % (group, dt, mode, worst))


@pytest.mark.parametrize("dt", sorted(DTYPES))
def test_every_combination_of_wanted_gradients(kernels, dt):
    for want in itertools.product([False, True], repeat=5):
        _check(kernels, 65, 63, 3, DTYPES[dt], (True, True), want=want, forced=2)


@pytest.mark.parametrize("dt", sorted(DTYPES))
def test_exact_periods_a_tie_of_rint_and_a_duplicate(kernels, dt):
    """p = 0.25 and points that are multiples of 1 / 64: row 0 of z lies exactly 3.0 = 12 periods from row 0 of x in
    every feature, row 1 half a period (u = -1/2, the tie of rint), row 2 is a duplicate, row 3 two periods from x_5."""
    dtype = DTYPES[dt]
    x = torch.as_tensor(np.random.default_rng(0).integers(-64, 64, size=(6, 3)) / 64.0).to(dtype)
    z = x[:4].clone()
    z[0], z[1], z[3] = x[0] - 3.0, x[1] + 0.125, x[5] + 0.5
    ls, period, var = (torch.tensor([v], dtype=dtype) for v in (0.8, 0.25, 1.7))
    G = torch.zeros(6, 4, dtype=dtype)
    G[0, 0], G[2, 2] = 1.5, -0.75
    args = [t.to(DEV) for t in (x, z, ls, period, var)]
    K = kernels.gp_periodic_fwd(*args)
    assert K[0, 0] == var.item() and K[2, 2] == var.item() and K[5, 3] == var.item()
    grads = kernels.gp_periodic_bwd(*args, G.to(DEV))
    assert all(torch.equal(g, torch.zeros_like(g)) for g in grads[:4]) and grads[4].item() == 1.5 - 0.75
    G = torch.as_tensor(np.random.default_rng(1).standard_normal((6, 4))).to(dtype)
    _compare(dict(zip(NAMES, kernels.gp_periodic_bwd(*args, G.to(DEV))), K=K), x, z, ls, period, var, G, "exact periods")


@pytest.mark.parametrize("zmode,M", [("given", 66), ("null", 70)])
def test_shifted_inputs_do_not_lose_to_the_float32_restatement(kernels, zmode, M):
    errors = _check(kernels, 70, M, 5, torch.float32, (True, True), shift=1e3, zmode=zmode)[1]
    assert all(mine <= twins for mine, twins in errors.values()), errors


def test_peak_memory_stays_below_four_matrices():
    import pyro_amd.contrib.gp as gp
    N = M = 512
    kern = pc.build(gp, 16, *pc.parameters(0, 16, True, True, dtype=torch.float32)).to(DEV)
    X, Z = gc.points(0, N, 16).float().to(DEV).requires_grad_(), gc.points(1, M, 16).float().to(DEV)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    kern(X, Z).sum().backward()
    torch.cuda.synchronize()
    assert X.grad is not None and kern.period_unconstrained.grad is not None
    assert torch.cuda.max_memory_allocated() - before < 4 * N * M * 4      # one [N, M, D] tensor alone is 16 N M 4


@pytest.mark.parametrize("dt", sorted(DTYPES))
def test_routing_of_the_class(kernels, dt, monkeypatch):
    import pyro_amd.contrib.gp as gp
    dtype, D, calls = DTYPES[dt], 5, []
    real_fwd, real_bwd = kernels.gp_periodic_fwd, kernels.gp_periodic_bwd
    monkeypatch.setattr(kernels, "gp_periodic_fwd", lambda *a, **k: calls.append("fwd") or real_fwd(*a, **k))
    monkeypatch.setattr(kernels, "gp_periodic_bwd", lambda *a, **k: calls.append("bwd") or real_bwd(*a, **k))
    x, z, ls, period, var, G = _inputs(70, 33, D, dtype, (True, False))

    def run(device, fused):
        monkeypatch.setattr(gp.kernels, "FUSED_GP_PERIODIC", fused)
        kern = pc.build(gp, D, ls, period, var).to(device)
        X, Z = x.to(device).requires_grad_(), z.to(device).requires_grad_()
        K = kern(X, Z)
        (K * G.to(device)).sum().backward()
        assert kern(X, diag=True).shape == (70,)
        con = [getattr(kern, n).detach() for n in ("lengthscale", "period", "variance")]
        raw = [getattr(kern, n + "_unconstrained").grad for n in ("lengthscale", "period", "variance")]
        out = {"K": K.detach(), "gx": X.grad, "gz": Z.grad}
        out.update({n: (r / c).reshape(-1) for n, r, c in zip(NAMES[2:], raw, con)})
        return out, con

    fused, con = run(DEV, True)
    assert calls == ["fwd", "bwd"]
    flat = [c.reshape(-1) for c in con]
    direct = dict(zip(NAMES, real_bwd(x.to(DEV), z.to(DEV), *flat, G.to(DEV))), K=real_fwd(x.to(DEV), z.to(DEV), *flat))
    assert all(torch.equal(fused[n], direct[n]) for n in ("K", "gx", "gz"))
    cpu_con = [c.cpu() for c in flat]
    _compare(fused, x, z, *cpu_con, G, "fused")
    off = run(DEV, False)[0]
    assert calls == ["fwd", "bwd"]
    if dtype == torch.float64:                      # both torch routes against the same truth, within the same bound
        _compare(off, x, z, *cpu_con, G, "torch route on the device")
        _compare(run("cpu", False)[0], x, z, *cpu_con, G, "torch route on the CPU")
    monkeypatch.setattr(gp.kernels, "FUSED_GP_PERIODIC", True)      # D = 65, a batched period, mixed dtypes: torch route
    gp.kernels.Periodic(65).to(DEV)(torch.zeros(3, 65, device=DEV))
    gp.kernels.Periodic(5, period=torch.ones(2, 5, dtype=dtype)).to(DEV)(x[:2].to(DEV))
    gp.kernels.Periodic(5).to(DEV)(x.double().to(DEV))
    assert calls == ["fwd", "bwd"]


def test_regression_over_product_periodic_rbf_within_the_reference_sensitivity():
    import pyro_amd.contrib.gp as gp
    from pyro_amd.infer import Trace_ELBO
    pc.check_model(gp, gc, Trace_ELBO(), DEV)
