"""The streamed conditional marginals (csrc/gp_cond.hip) per element on the device, and VariationalSparseGP on them.

Truth: float64 torch on the CPU.  K = Kuf = restate_K(xu, x) (tests/gp_cases.py), loc = K^T a, s[n, j] = |P_j K[:, n]|^2,
and every gradient by autograd of sum(loc g_loc) + sum(s g_s) through those formulae.

f64 bounds -- worst-case rounding, not measurements.  eK = 2^-52 16 (D + 8) (1 + max|K|) is the per-entry bound of
tests/test_gp_kernel_gpu.py for K itself.  A sum of L products is off by at most 2^-52 (L + 8) S, S the sum of absolute
summands, plus what the factors' own errors carry through:
    loc, ga   2^-52 (L + 8) S + eK sum |other factor|                                       (L = M, N)
    Y = P_j K eY = 2^-52 (M + 8) |P_j| |K| + eK |P_j| 1;   s = sum_r Y^2:  sum_r (2 |Y| eY + eY^2) + 2^-52 (M + 8) s
    Aw_j      eA = 2^-52 (N + 8) |K| diag|g_s| |K|^T + eK (|K| |g_s| 1^T + its transpose);   gP = 2 P Aw:
              2^-52 (M + 8) 2 |P| |Aw| + 2 |P| eA
    G         EG = 2^-52 (J M + Q + M + 16) Gabs + eK sum_j (2 |P_j|^T |P_j| 1) |g_s[:, j]|^T,   Gabs = |a| |g_loc|^T +
              sum_j 2 |P_j|^T |P_j| |K| diag|g_s[:, j]|  (B2_j = 2 P_j^T P_j is itself a rounded sum of M products)
    x, xu, parameters: 2^-52 (L + 16 (D + 8)) T(|G|) + T(EG), as tests/test_gp_sgpr_gpu.py (T(.): the output's sum of
              absolute summands with that matrix in G's place, L = N (gxu), M (gx), N M (reduced))
f32 bounds -- the project's rule: four times the error of the same formulae in float32 torch on the CPU, floor 4 * 2^-23
times the sum of absolute summands of the whole expression (for s: sum_r (|P_j| |K|)^2; for the chain: T(Gabs)), and
2^-126 per summand where float32 has no relative precision left (matrix cores flush).

Shapes at the seams: the 32-row block of the forward, the 32-point tile, the chunk of 128 rows and the block of 128 (f32) /
64 (f64) rows of the backward, more than one split, the largest M."""
import numpy as np
import pytest
import torch

from . import gp_cases as gc
from .test_gp_sgpr_gpu import _abs_sums
from .test_gp_sgpr_host import model_data
from .test_gp_vsgp_host import dense_loss_and_grads, vsgp

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = {"f32": torch.float32, "f64": torch.float64}
MAXM = {"f32": 512, "f64": 256}
NAMES = ("gx", "gxu", "g_ls", "g_var", "g_alpha", "ga", "gP")


@pytest.fixture(scope="module")
def kernels():
    from pyro_amd import kernels as k
    return k


def _formulae(family, x, xu, a, P, ls, var, al, g_loc, g_s):
    """loc, s and the seven gradients in the dtype of the arguments, by autograd."""
    leaves = [t.clone().requires_grad_() for t in (x, xu, ls, var, a, P)] + ([] if al is None else [al.clone().requires_grad_()])
    x_, xu_, ls_, var_, a_, P_ = leaves[:6]
    K = gc.restate_K(family, xu_, x_, ls_, var_, leaves[6] if al is not None else None)
    loc, s = K.t() @ a_, (P_ @ K).pow(2).sum(1).t()
    grads = torch.autograd.grad((loc * g_loc).sum() + (s * g_s).sum(), leaves)
    out = dict(zip(("gx", "gxu", "g_ls", "g_var", "ga", "gP"), grads[:6]), loc=loc.detach(), s=s.detach())
    out["g_alpha"] = grads[6] if al is not None else None
    return out, K.detach()


def _bounds(family, x, xu, a, P, ls, var, al, g_loc, g_s, dtype):
    up = lambda t: None if t is None else t.double()      # noqa: E731
    a64 = [up(t) for t in (x, xu, a, P, ls, var, al, g_loc, g_s)]
    truth, K = _formulae(family, *a64)
    x6, xu6, a6, P6, ls6, var6, al6, gl6, gs6 = a64
    (M, D), N, Q = xu.shape, x.shape[0], a.shape[1]
    J = Q + 1
    Ka, Pa = K.abs(), P6.abs()
    B2a = 2 * Pa.transpose(1, 2) @ Pa
    Aabs = torch.einsum("in,nj,kn->jik", Ka, gs6.abs(), Ka)                              # |K| diag|g_s_j| |K|^T
    Gabs = a6.abs() @ gl6.abs().t() + torch.einsum("jik,kn,nj->in", B2a, Ka, gs6.abs())
    PK = Pa @ Ka                                                                         # [J, M, N]
    sums = {"loc": Ka.t() @ a6.abs(), "s": PK.pow(2).sum(1).t(), "ga": Ka @ gl6.abs(), "gP": 2 * Pa @ Aabs}
    chain = ("gx", "gxu", "g_ls", "g_var", "g_alpha")
    args = (family, xu6, x6, ls6, var6, al6)
    sums.update(_abs_sums(*args, _G(a6, gl6, P6, K, gs6).abs()))
    if dtype == torch.float32:
        sums.update(_abs_sums(*args, Gabs))
        twin = _formulae(family, x, xu, a, P, ls, var, al, g_loc, g_s)[0]
        U = 2.0 ** -126
        flushed = _abs_sums(*args, (U * (J * M + Q + 8 + B2a.sum((0, 2))[:, None])).expand(M, N))
        flushed.update(loc=U * M * (1 + a6.abs().max()), s=U * M * M * (1 + Pa.max()) ** 2 * (1 + Ka.max()),
                       ga=U * N * (1 + gl6.abs().max()), gP=U * N * M * (1 + Pa.max()) * (1 + gs6.abs().max()))
        return truth, {n: torch.maximum(4 * (twin[n].double() - truth[n]).abs(), 4 * (gc.EPS32 * sums[n] + flushed[n] + U * N * M))
                       for n in truth if truth[n] is not None}
    eK = gc.EPS64 * 16 * (D + 8) * (1 + Ka.max().item())
    eY = gc.EPS64 * (M + 8) * PK + eK * Pa.sum(2, keepdim=True)
    Y = (P6 @ K).abs()
    eA = gc.EPS64 * (N + 8) * Aabs + eK * (lambda v: v[:, :, None] + v[:, None, :])((Ka @ gs6.abs()).t())
    EG = gc.EPS64 * (J * M + Q + M + 16) * Gabs + eK * torch.einsum("ji,nj->in", B2a.sum(2), gs6.abs())
    carried = _abs_sums(*args, EG)
    bound = {"loc": gc.EPS64 * (M + 8) * sums["loc"] + eK * a6.abs().sum(0)[None, :],
             "s": (2 * Y * eY + eY.pow(2)).sum(1).t() + gc.EPS64 * (M + 8) * truth["s"],
             "ga": gc.EPS64 * (N + 8) * sums["ga"] + eK * gl6.abs().sum(0)[None, :],
             "gP": gc.EPS64 * (M + 8) * sums["gP"] + 2 * Pa @ eA}
    for n, L in zip(chain, (M, N, N * M, N * M, N * M)):
        if truth[n] is not None:
            bound[n] = gc.EPS64 * (L + 16 * (D + 8)) * sums[n] + carried[n]
    return truth, bound


def _G(a, g_loc, P, K, g_s):
    return a @ g_loc.t() + 2 * torch.einsum("jri,jrk,kn,nj->in", P, P, K, g_s)


def _inputs(dt, family, M, N, D, Q, ard, seed):
    dtype = DTYPES[dt]
    x, xu = gc.points(seed, N, D).to(dtype), gc.points(seed + 50, M, D).to(dtype)
    if N >= 5 and M >= 3:
        xu[2] = x[4]                                        # a duplicate xu_i = x_n
    ls, var, al = (None if t is None else t.to(dtype) for t in gc.parameters(seed, D, ard, family))
    g = np.random.default_rng(seed + 7)
    a, g_loc, g_s = (torch.as_tensor(g.standard_normal(s)).to(dtype) for s in ((M, Q), (N, Q), (N, Q + 1)))
    P = torch.as_tensor(g.standard_normal((Q + 1, M, M)) / np.sqrt(M)).to(dtype)
    P[0] = P[0].tril()
    return x, xu, a, P, ls, var, al, g_loc, g_s


def _check(kernels, dt, family, M, N, D, Q, ard=False, forced=0, want=(True,) * 7, seed=0):
    x, xu, a, P, ls, var, al, g_loc, g_s = _inputs(dt, family, M, N, D, Q, ard, seed)
    truth, bound = _bounds(family, x, xu, a, P, ls, var, al, g_loc, g_s, DTYPES[dt])
    dev = [None if t is None else t.to(DEV) for t in (x, xu, a, P, ls, var, al)]
    loc, s = kernels.gp_cond_fwd(*dev, family)
    grads = kernels.gp_cond_bwd(*dev, g_loc.to(DEV), g_s.to(DEV), family, want, forced)
    got = dict(zip(NAMES, grads), loc=loc, s=s)
    wanted = dict(zip(NAMES, want), loc=True, s=True)
    for name, value in got.items():
        if not wanted[name] or truth[name] is None:
            assert value is None, name
            continue
        assert value.shape == truth[name].shape and value.dtype == DTYPES[dt] and torch.isfinite(value).all(), name
        err = (value.cpu().double() - truth[name]).abs()
        ratio = (err / bound[name].clamp(min=1e-300)).max().item()
        print("%s %s %s M=%d N=%d D=%d Q=%d: error / bound %.3g" % (dt, family, name, M, N, D, Q, ratio))
        assert (err <= bound[name]).all(), "%s %s %s M=%d N=%d D=%d Q=%d splits=%d: error / bound %.3g (error %.3g)" % (
            dt, family, name, M, N, D, Q, forced, ratio, err.max().item())
    return got


# (M, N, D, Q, ARD, forced splits); M = None stands for the dtype's largest
SHAPES = [(1, 1, 1, 1, False, 0), (31, 31, 3, 3, True, 0), (33, 33, 64, 1, False, 0), (65, 4097, 3, 3, True, 0),
          (129, 33, 1, 1, True, 3), (None, 70, 3, 3, False, 0)]


@pytest.mark.parametrize("dt", sorted(DTYPES))
@pytest.mark.parametrize("case", range(len(SHAPES)))
def test_shapes_at_the_seams(kernels, dt, case):
    M, N, D, Q, ard, forced = SHAPES[case]
    _check(kernels, dt, "rbf", M or MAXM[dt], N, D, Q, ard, forced, seed=case)


@pytest.mark.parametrize("dt", sorted(DTYPES))
@pytest.mark.parametrize("family", ["rbf", "matern52", "rational_quadratic"])
def test_families_splits_masks_and_reproducibility(kernels, family, dt):
    """Per family: every gradient at 1 and at 3 splits (bit-identical gP: Aw comes from its upper triangle, sums in a
    fixed order), twice (bit-identical everything), and with everything off but gxu."""
    one = _check(kernels, dt, family, 67, 200, 5, 2, ard=True, forced=1, seed=3)
    again = _check(kernels, dt, family, 67, 200, 5, 2, ard=True, forced=1, seed=3)
    assert all(one[n] is None or torch.equal(one[n], again[n]) for n in one), "two calls differ bit for bit"
    _check(kernels, dt, family, 67, 200, 5, 2, ard=True, forced=3, seed=3)
    only = _check(kernels, dt, family, 67, 200, 5, 2, ard=True, forced=1, want=(False, True) + (False,) * 5, seed=3)
    assert torch.equal(only["gxu"], one["gxu"])


@pytest.mark.parametrize("dt", sorted(DTYPES))
def test_limits_empty_shapes_and_typed_ops(kernels, dt):
    dtype = DTYPES[dt]
    mk = lambda *s: torch.randn(*s, dtype=dtype, device=DEV)      # noqa: E731
    ls, var = torch.ones(1, dtype=dtype, device=DEV), torch.ones(1, dtype=dtype, device=DEV)
    big = MAXM[dt] + 1
    with pytest.raises(kernels.Unsupported):
        kernels.gp_cond_fwd(mk(40, 3), mk(big, 3), mk(big, 1), mk(2, big, big), ls, var)
    with pytest.raises(kernels.Unsupported):
        kernels.gp_cond_fwd(mk(40, 3), mk(8, 3), mk(8, 17), mk(18, 8, 8), ls, var)
    loc, s = kernels.gp_cond_fwd(mk(0, 3), mk(8, 3), mk(8, 2), mk(3, 8, 8), ls, var)
    assert loc.shape == (0, 2) and s.shape == (0, 3)
    loc, s = kernels.gp_cond_fwd(mk(5, 3), mk(0, 3), mk(0, 2), mk(3, 0, 0), ls, var)
    assert loc.shape == (5, 2) and s.shape == (5, 3) and not loc.any() and not s.any()
    x, xu, a, P, g_loc, g_s = mk(70, 3), mk(33, 3), mk(33, 2), mk(3, 33, 33), mk(70, 2), mk(70, 3)
    P[0] = P[0].tril()
    from pyro_amd.ops import torch_library
    assert torch_library.available()
    ops = torch.ops.pyro_amd
    for got, want in zip(ops.gp_cond(x, xu, a, P, ls, var, None, 0), kernels.gp_cond_fwd(x, xu, a, P, ls, var)):
        assert torch.equal(got, want)
    flags = (False, True, True, True, False, True, True)
    typed = ops.gp_cond_bwd(x, xu, a, P, ls, var, None, g_loc, g_s, 0, *flags, 0)
    plain = kernels.gp_cond_bwd(x, xu, a, P, ls, var, None, g_loc, g_s, "rbf", flags)
    for got, want in zip(typed, plain):
        assert got.numel() == 0 if want is None else torch.equal(got, want)
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode(allow_non_fake_inputs=False) as mode:
        fake = [mode.from_tensor(t) for t in (x, xu, a, P, ls, var)]
        floc, fs = ops.gp_cond(*fake, None, 0)
        fg = ops.gp_cond_bwd(*fake, None, mode.from_tensor(g_loc), mode.from_tensor(g_s), 0, *flags, 0)
    assert floc.shape == (70, 2) and fs.shape == (70, 3) and [t.shape for t in fg] == [t.shape for t in typed]


# ---- the model ----------------------------------------------------------------------------------------------------------
def _quantities(gp, data, dtype, device, whiten, case):
    from pyro_amd.infer import TraceMeanField_ELBO
    model = vsgp(gp, data, dtype, device, whiten, case)
    loss, grads = dense_loss_and_grads(model) if device == "cpu" else gc.loss_and_grads(model, TraceMeanField_ELBO())
    out = {"loss": np.asarray(loss)}
    out.update({"grad " + n: g for n, g in grads.items()})
    with torch.no_grad():
        loc, var = model(data["Xnew"].to(dtype=dtype, device=device))
    out.update(loc=loc.cpu().numpy(), var=var.cpu().numpy())
    return model, out


@pytest.mark.parametrize("case", ["one_output", "two_outputs", "num_data", "mean_function"])
@pytest.mark.parametrize("whiten", [False, True])
def test_model_against_the_dense_route_on_the_cpu(monkeypatch, whiten, case):
    """Loss (TraceMeanField_ELBO with the Gaussian likelihood: deterministic), every parameter's gradient and
    forward(Xnew) of the streamed route on the device against util.conditional and torch.distributions on the CPU in float64
    (tests/test_gp_vsgp_host.py: the closed form), within the conditioning bound of tests/test_gp_sgpr_gpu.py.  Float32
    models do not take the streamed route (cast up to the float64 kernels they missed four times the dense float32 route's
    own error by up to 5.0 times: README "Gaussian processes"); util.conditional must then be what runs."""
    from pyro_amd.contrib import gp
    data = model_data("few_rows")
    N = data["X"].size(0)
    dense, dense64 = _quantities(gp, data, torch.float64, "cpu", whiten, case)
    Kuu = dense.kernel(dense.Xu).detach() + dense.jitter * torch.eye(dense.Xu.size(0), dtype=torch.float64)
    cond = torch.linalg.cond(Kuu).item()
    W = torch.linalg.solve_triangular(torch.linalg.cholesky(Kuu), dense.kernel(dense.Xu, dense.X).detach(), upper=False)
    margin = (dense.kernel(dense.X, diag=True).detach() - W.pow(2).sum(0)).min().item()
    assert margin > 16 * N * gc.EPS64 * cond * (1 + W.pow(2).sum(0).max().item()), "the clamp is within the bound on s"

    def refuse(*a, **k):
        raise AssertionError("the dense route was taken")
    monkeypatch.setattr(gp.models, "FUSED_VSGP_MIN_N", 0)
    monkeypatch.setattr(gp.util, "conditional", refuse)
    _, got = _quantities(gp, data, torch.float64, DEV, whiten, case)
    assert set(got) == set(dense64)
    for key, want in dense64.items():
        err = np.abs(got[key] - want).max()
        bound = 16 * N * gc.EPS64 * cond * (1 + np.abs(want).max())
        print("vsgp %s whiten=%d %s: error / bound %.3g" % (case, whiten, key, err / bound))
        assert err <= bound, (case, whiten, key, err, bound)
    with pytest.raises(AssertionError, match="the dense route was taken"):
        _quantities(gp, data, torch.float32, DEV, whiten, case)
