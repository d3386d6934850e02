"""The streamed sparse-GP statistics (csrc/gp_sgpr.hip) per element on the device, and SparseGPRegression on them.

Truth: the float64 restatement (tests/gp_cases.py) on the inputs as the kernel sees them: Kuf = restate(xu, x)["K"],
A = Kuf Kuf^T, b = Kuf r, G = (gA + gA^T) Kuf + gb r^T handed to ``restate`` (its gx is gxu, its gz is gx), gr = Kuf^T gb.

f64 bounds -- worst-case rounding, not measurements.  eK = 2^-52 16 (D + 8) (1 + max|Kuf|) is the per-entry bound of
tests/test_gp_kernel_gpu.py for Kuf itself.  A sum of L products of rounded factors is off by at most 2^-52 (L + 8) S
(S the sum of absolute summands: one rounding per product, at most L additions in any order, the finalize's additions
and rounding in the 8) plus what the factors' own errors carry through:
    A[i, j]   2^-52 (N + 8) sum_n |K_in K_jn|  +  eK (sum_n |K_in| + sum_n |K_jn|)
    b, gr     2^-52 (L + 8) S  +  eK sum |other factor|            (L = N, M)
    G         EG = 2^-52 (M + Q + 8) (|S| |Kuf| + |gb| |r|^T) + eK |S| 1        (entry by entry, [M, N])
    gradients 2^-52 (L + 16 (D + 8)) T(|G|) + T(EG),  T(.) the output's sum of absolute summands with that matrix in
              G's place, L = N (gxu), M (gx), N M (reduced)
f32 bounds -- the project's rule: four times the error of the same formulae in float32 torch on the CPU, floor
4 * 2^-23 times the sum of absolute summands; for the gradients the summands are those of the whole expression, the
inner sum of G included (T(|S| |Kuf| + |gb| |r|^T): G is itself a float32 sum of M + Q signed terms, and its rounding
does not shrink where they cancel).  Below float32's smallest normal number, 2^-126, the format has no
relative precision left and the matrix cores flush: a product or a Kuf entry down there is off by up to 2^-126
absolutely, so the floor carries U = 2^-126 per summand the same way eK and 2^-52 are carried above (at D = 64 whole
rows of Kuf are e^-100).

Shapes around T_M = 128 (f32) / 64 (f64) rows, T_N = 32 points, the flush length F = 4096 and the largest M."""
import itertools

import numpy as np
import pytest
import torch

from . import gp_cases as gc
from .test_gp_sgpr_host import dense_loss_and_grads, model_data as _model_data

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = {"f32": torch.float32, "f64": torch.float64}
TM, MAXM = {"f32": 128, "f64": 64}, {"f32": 512, "f64": 256}
NAMES = ("gx", "gxu", "g_ls", "g_var", "g_alpha", "gr")


@pytest.fixture(scope="module")
def kernels():
    from pyro_amd import kernels as k
    return k


def _abs_sums(family, xu, x, ls, var, al, Gm):
    d = gc.scaled_differences(xu, x, ls)
    f, df, da = gc.f_and_derivative(family, d.pow(2).sum(-1), None if al is None else al.reshape(()))
    W = (Gm * var.reshape(()) * df.abs())[:, :, None] * (2.0 / ls.reshape(-1))
    red = (0, 1) if ls.numel() > 1 else (0, 1, 2)
    return {"gxu": (W * d.abs()).sum(1), "gx": (W * d.abs()).sum(0), "g_ls": (W * d.pow(2)).sum(red).reshape(-1),
            "g_var": (Gm * f.abs()).sum().reshape(1),
            "g_alpha": None if da is None else (var.reshape(()) * Gm * da.abs()).sum().reshape(1)}


def _formulae(family, xu, x, r, ls, var, al, gA, gb):
    """Everything the two kernels return, in the dtype of the arguments, with the sums of absolute summands."""
    K = gc.restate_K(family, xu, x, ls, var, al)
    S = gA + gA.t()
    G = S @ K + gb @ r.t()
    out = gc.restate(family, xu, x, ls, var, al, G)
    res = {"A": K @ K.t(), "b": K @ r, "gr": K.t() @ gb, "gxu": out["gx"], "gx": out["gz"], "g_ls": out["g_ls"],
           "g_var": out["g_var"], "g_alpha": out["g_alpha"]}
    return res, K, S, G


def _bounds(family, x, xu, r, ls, var, al, gA, gb, dtype):
    up = lambda t: None if t is None else t.double()      # noqa: E731
    a64 = [up(t) for t in (xu, x, r, ls, var, al, gA, gb)]
    truth, K, S, G = _formulae(family, *a64)
    xu6, x6, r6, ls6, var6, al6, gA6, gb6 = a64
    (M, D), N, Q = xu.shape, x.shape[0], r.shape[1]
    Ka, rows = K.abs(), K.abs().sum(1)
    sums = {"A": Ka @ Ka.t(), "b": Ka @ r6.abs(), "gr": Ka.t() @ gb6.abs()}
    sums.update(_abs_sums(family, xu6, x6, ls6, var6, al6, G.abs()))
    if dtype == torch.float32:
        sums.update(_abs_sums(family, xu6, x6, ls6, var6, al6, S.abs() @ Ka + gb6.abs() @ r6.abs().t()))
        twin = _formulae(family, xu, x, r, ls, var, al, gA, gb)[0]
        U = 2.0 ** -126
        flushed = _abs_sums(family, xu6, x6, ls6, var6, al6,
                            (U * (M + Q + 8 + S.abs().sum(1, keepdim=True))).expand(M, N))
        flushed.update(A=U * N * (1 + 2 * Ka.max()), b=U * N * (1 + r6.abs().max()), gr=U * M * (1 + gb6.abs().max()))
        return truth, {n: torch.maximum(4 * (twin[n].double() - truth[n]).abs(),
                                        4 * (gc.EPS32 * sums[n] + flushed[n] + U * N * M))
                       for n in truth if truth[n] is not None}
    eK = gc.EPS64 * 16 * (D + 8) * (1 + Ka.max().item())
    EG = gc.EPS64 * (M + Q + 8) * (S.abs() @ Ka + gb6.abs() @ r6.abs().t()) + eK * S.abs().sum(1, keepdim=True)
    carried = _abs_sums(family, xu6, x6, ls6, var6, al6, EG)
    bound = {"A": gc.EPS64 * (N + 8) * sums["A"] + eK * (rows[:, None] + rows[None, :]),
             "b": gc.EPS64 * (N + 8) * sums["b"] + eK * r6.abs().sum(0)[None, :],
             "gr": gc.EPS64 * (M + 8) * sums["gr"] + eK * gb6.abs().sum(0)[None, :]}
    for n, L in (("gxu", N), ("gx", M), ("g_ls", N * M), ("g_var", N * M), ("g_alpha", N * M)):
        if truth[n] is not None:
            bound[n] = gc.EPS64 * (L + 16 * (D + 8)) * sums[n] + carried[n]
    return truth, bound


def _check(kernels, dt, family, M, N, D, Q, ard=False, forced=0, shift=0.0, want=(True,) * 6, seed=0):
    dtype = DTYPES[dt]
    x, xu = gc.points(seed, N, D, shift).to(dtype), gc.points(seed + 50, M, D, shift).to(dtype)
    if N >= 5 and M >= 3:
        xu[2] = x[4]                                        # a duplicate xu_i = x_n
    ls, var, al = (None if t is None else t.to(dtype) for t in gc.parameters(seed, D, ard, family))
    g = np.random.default_rng(seed + 7)
    r, gA, gb = (torch.as_tensor(g.standard_normal(s)).to(dtype) for s in ((N, Q), (M, M), (M, Q)))   # gA: NOT symmetric
    truth, bound = _bounds(family, x, xu, r, ls, var, al, gA, gb, dtype)
    dev = [None if t is None else t.to(DEV) for t in (x, xu, r, ls, var, al)]
    A, b = kernels.gp_sgpr_fwd(*dev, family, forced)
    grads = kernels.gp_sgpr_bwd(*dev, gA.to(DEV), gb.to(DEV), family, want, forced)
    assert torch.equal(A, A.t()), "A is not bit-symmetric"
    got = dict(zip(NAMES, grads), A=A, b=b)
    wanted = dict(zip(NAMES, want), A=True, b=True)
    worst = 0.0
    for name, value in got.items():
        if not wanted[name] or truth[name] is None:
            assert value is None, name
            continue
        assert value.shape == truth[name].shape and value.dtype == dtype and torch.isfinite(value).all(), name
        err = (value.cpu().double() - truth[name]).abs()
        ratio = (err / bound[name].clamp(min=1e-300)).max().item()
        worst = max(worst, ratio)
        print("%s %s %s M=%d N=%d D=%d Q=%d: error / bound %.3g" % (dt, family, name, M, N, D, Q, ratio))
        assert (err <= bound[name]).all(), "%s %s %s M=%d N=%d D=%d Q=%d splits=%d: error / bound %.3g (error %.3g)" % (
            dt, family, name, M, N, D, Q, forced, ratio, err.max().item())
    return got


# (M as a multiple of T_M plus an offset, N, D, Q, ARD, forced splits): the M and N lists of the module docstring, with
# D, Q and the lengthscale cycled through them
def _shapes(dt):
    t = TM[dt]
    ms = [1, t - 1, t, t + 1, 2 * t + 1]
    ns = [1, 31, 33, 101, 4096 + 37, 200]
    ds, qs = [1, 3, 8, 64], [1, 3, 16]
    for n, (M, N) in enumerate(zip(ms + [MAXM[dt]], ns)):
        yield M, N, ds[n % 4], qs[n % 3], bool(n & 1), 3 if N == 200 else 0
    for n, N in enumerate(ns[:4]):
        yield ms[(n + 2) % 5], N, ds[(n + 1) % 4], qs[(n + 1) % 3], not n & 1, 0


@pytest.mark.parametrize("dt", sorted(DTYPES))
@pytest.mark.parametrize("case", range(10))
def test_shapes_splits_and_flush(kernels, dt, case):
    M, N, D, Q, ard, forced = list(_shapes(dt))[case]
    _check(kernels, dt, "rbf", M, N, D, Q, ard, forced, seed=case)


@pytest.mark.parametrize("dt", sorted(DTYPES))
@pytest.mark.parametrize("family", gc.FAMILIES)
def test_families_and_shifted_inputs(kernels, family, dt):
    _check(kernels, dt, family, TM[dt] + 5, 70, 5, 2, ard=True, seed=3)
    _check(kernels, dt, family, 37, 70, 5, 2, ard=False, shift=1e3, seed=4)


@pytest.mark.parametrize("dt", sorted(DTYPES))
def test_every_subset_of_wanted_gradients_and_reproducibility(kernels, dt):
    first = None
    for want in itertools.product([False, True], repeat=6):
        got = _check(kernels, dt, "rational_quadratic", TM[dt] + 3, 67, 3, 2, ard=True, forced=2, want=want)
        if all(want):
            again = _check(kernels, dt, "rational_quadratic", TM[dt] + 3, 67, 3, 2, ard=True, forced=2, want=want)
            first = all(torch.equal(got[n], again[n]) for n in got)
    assert first, "two calls differ bit for bit"


@pytest.mark.parametrize("dt", sorted(DTYPES))
def test_limits_empty_shapes_and_typed_ops(kernels, dt):
    dtype = DTYPES[dt]
    mk = lambda *s: torch.randn(*s, dtype=dtype, device=DEV)      # noqa: E731
    ls, var = torch.ones(1, dtype=dtype, device=DEV), torch.ones(1, dtype=dtype, device=DEV)
    with pytest.raises(kernels.Unsupported):
        kernels.gp_sgpr_fwd(mk(40, 3), mk(MAXM[dt] + 1, 3), mk(40, 1), ls, var)
    with pytest.raises(kernels.Unsupported):
        kernels.gp_sgpr_fwd(mk(40, 3), mk(8, 3), mk(40, 17), ls, var)
    A, b = kernels.gp_sgpr_fwd(mk(0, 3), mk(8, 3), mk(0, 2), ls, var)
    assert A.shape == (8, 8) and b.shape == (8, 2) and not A.any() and not b.any()
    x, xu, r, gA, gb = mk(70, 3), mk(33, 3), mk(70, 2), mk(33, 33), mk(33, 2)
    from pyro_amd.ops import torch_library
    assert torch_library.available()
    ops = torch.ops.pyro_amd
    for a, want in zip(ops.gp_sgpr(x, xu, r, ls, var, None, 0, 0), kernels.gp_sgpr_fwd(x, xu, r, ls, var)):
        assert torch.equal(a, want)
    flags = (False, True, True, True, False, True)
    typed = ops.gp_sgpr_bwd(x, xu, r, ls, var, None, gA, gb, 0, *flags, 0)
    plain = kernels.gp_sgpr_bwd(x, xu, r, ls, var, None, gA, gb, "rbf", flags)
    for a, want in zip(typed, plain):
        assert a.numel() == 0 if want is None else torch.equal(a, want)
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode(allow_non_fake_inputs=False) as mode:
        fake = [mode.from_tensor(t) for t in (x, xu, r, ls, var)]
        fa, fb = ops.gp_sgpr(*fake, None, 0, 0)
        fg = ops.gp_sgpr_bwd(*fake, None, mode.from_tensor(gA), mode.from_tensor(gb), 0, *flags, 0)
    assert fa.shape == (33, 33) and fb.shape == (33, 2) and [t.shape for t in fg] == [t.shape for t in typed]


# ---- the models ---------------------------------------------------------------------------------------------------------
def _condition_bound(model, N, value):
    Kuu = model.kernel(model.Xu).detach().double().cpu()
    cond = torch.linalg.cond(Kuu + model.jitter * torch.eye(Kuu.size(0), dtype=torch.float64)).item()
    return 16 * N * gc.EPS64 * cond * (1 + np.abs(value).max())


def _quantities(gp, pyro, name, data, dtype, device, y=None, mean=None):
    pyro.clear_param_store()      # (a second model of the same names: the store would hand it the first one's Xu)
    model = gc.build_model(gp, name, data, dtype=dtype, device=device, y=y)
    if mean is not None:
        model.mean_function = mean
    out = {}
    loss, grads = dense_loss_and_grads(model) if device == "cpu" else gc.loss_and_grads(model, pyro.infer.Trace_ELBO())
    out["loss"] = np.asarray(loss)
    out.update({"grad " + n: g for n, g in grads.items()})
    Xnew = data["Xnew"].to(dtype=dtype, device=device)
    with torch.no_grad():
        for full_cov, noiseless in gc.FORWARD_CASES:
            loc, cov = model(Xnew, full_cov=full_cov, noiseless=noiseless)
            out["loc %d%d" % (full_cov, noiseless)] = loc.cpu().numpy()
            out["cov %d%d" % (full_cov, noiseless)] = cov.cpu().numpy()
    return model, out


@pytest.mark.parametrize("case", ["few_rows", "fixture", "two_outputs", "mean_function"])
@pytest.mark.parametrize("approx", ["VFE", "DTC"])
def test_models_against_the_dense_route_on_the_cpu(monkeypatch, kernels, approx, case):
    """Loss, gradients and forward(Xnew) of the streamed route on the device against the dense route on the CPU in float64.
    (A float32 model takes its statistics and its M x M algebra in float64: with float32 statistics the loss at N = 300
    was off by up to 21 times this bound, 2^-24 cond(Kuu) from rounding A = Kuf Kuf^T.)"""
    import pyro_amd as pyro
    from pyro_amd.contrib import gp
    data = _model_data("fixture" if case == "fixture" else "few_rows")
    N = data["X"].size(0)
    y = torch.stack((data["y"], data["y"].flip(0) * 0.5)) if case == "two_outputs" else None
    mean = (lambda X: 0.3 * X[:, 0] - 0.1) if case == "mean_function" else None
    name = "sgpr_" + approx
    calls = []
    for fn in ("gp_sgpr_fwd", "gp_sgpr_bwd", "gp_kernel_fwd"):
        def spy(*a, _f=getattr(kernels, fn), _n=fn, **k):
            out = _f(*a, **k)
            calls.append((_n, tuple(out.shape) if _n == "gp_kernel_fwd" else None))
            return out
        monkeypatch.setattr(kernels, fn, spy)
    monkeypatch.setattr(gp.models, "FUSED_SGPR", False)
    _, dense64 = _quantities(gp, pyro, name, data, torch.float64, "cpu", y, mean)
    _, dense32 = _quantities(gp, pyro, name, data, torch.float32, "cpu", y, mean)
    monkeypatch.setattr(gp.models, "FUSED_SGPR", True)
    monkeypatch.setattr(gp.models, "FUSED_SGPR_MIN_N", 0)
    for dtype in (torch.float64, torch.float32):
        del calls[:]
        model, got = _quantities(gp, pyro, name, data, dtype, DEV, y, mean)
        step = calls[:3]                                   # the loss and its gradient come first
        assert sorted(c[0] for c in step) == ["gp_kernel_fwd", "gp_sgpr_bwd", "gp_sgpr_fwd"], calls
        M = model.Xu.size(0)
        assert all(shape in (None, (M, M)) for _, shape in step), calls
        assert set(got) == set(dense64)
        for key, want in dense64.items():
            err = np.abs(got[key].astype(np.float64) - want).max()
            bound = _condition_bound(model, N, want) if dtype == torch.float64 else \
                4 * np.abs(dense32[key].astype(np.float64) - want).max()
            print("%s %s %s %s: error / bound %.3g" % (name, case, dtype, key, err / bound))
            assert err <= bound, (name, case, dtype, key, err, bound)


@pytest.mark.parametrize("why", ["FITC", "switch", "threshold", "sum_kernel", "M_over_limit"])
def test_other_cases_stay_on_the_dense_route_bit_for_bit(monkeypatch, kernels, why):
    import pyro_amd as pyro
    from pyro_amd import poutine
    from pyro_amd.contrib import gp
    data = _model_data("few_rows")
    if why == "M_over_limit":
        data = dict(data, X=data["X"].repeat(2, 1), y=data["y"].repeat(2), Xu=gc.points(5, 257, 3, near=False))
    name = "sgpr_FITC" if why == "FITC" else "sgpr_VFE"
    which = "sum" if why == "sum_kernel" else "rbf"
    def build():
        pyro.clear_param_store()
        return gc.build_model(gp, name, data, dtype=torch.float64, device=DEV, which=which)

    monkeypatch.setattr(gp.models, "FUSED_SGPR", False)
    want = gc.loss_and_grads(build(), pyro.infer.Trace_ELBO())
    names = list(poutine.trace(build().model).get_trace().nodes)
    monkeypatch.setattr(gp.models, "FUSED_SGPR", why != "switch")
    monkeypatch.setattr(gp.models, "FUSED_SGPR_MIN_N", 1024 if why == "threshold" else 0)
    calls = []
    for fn in ("gp_sgpr_fwd", "gp_sgpr_bwd"):
        monkeypatch.setattr(kernels, fn, lambda *a, _f=getattr(kernels, fn), **k: calls.append(1) or _f(*a, **k))
    got = gc.loss_and_grads(build(), pyro.infer.Trace_ELBO())
    assert not calls
    assert got[0] == want[0] and all(np.array_equal(got[1][n], want[1][n]) for n in want[1])
    if why == "switch":                                    # the streamed route leaves the same sites in the trace
        monkeypatch.setattr(gp.models, "FUSED_SGPR", True)
        assert list(poutine.trace(build().model).get_trace().nodes) == names and calls
