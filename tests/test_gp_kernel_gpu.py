"""The stationary covariance kernels (csrc/gp_kernel.hip) per element on the device, f32 and f64.

Truth: the float64 restatement by direct differences (tests/gp_cases.py) on the inputs AS THE KERNEL SEES THEM (the f32
inputs cast up, not the f64 originals: at a shift of 1e3 the input rounding alone is 2e-5).

f64 bounds -- worst-case rounding of sums that long, not measurements:
    K, gX, gZ                 2^-52 * 16 (D + 8) * (1 + A),   A the largest magnitude of that output
    lengthscale / variance / alpha gradients    2^-52 (N M + 16 D) * S,   S the restatement's sum of absolute summands
f32 bounds -- the project's rule: four times the error of the float32 direct-difference restatement on the CPU, with
floor 4 * 2^-23 (1 + A); for the reduced gradients the floor is 4 * 2^-23 * S.

Shapes: the smallest at which tiling (64 x 64 tiles, 4 x 4 per lane) and column splitting can go wrong."""
import itertools

import numpy as np
import pytest
import torch

from . import gp_cases as gc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = {"f32": torch.float32, "f64": torch.float64}


@pytest.fixture(scope="module")
def kernels():
    from pyro_amd import kernels as k
    return k


def _inputs(family, N, M, D, dtype, ard, seed=0, shift=0.0, zmode="given", ls=None, alpha=None, G="random"):
    x = gc.points(seed, N, D, shift).to(dtype)
    z = None if zmode == "null" else (x if zmode == "same" else gc.points(seed + 50, M, D, shift).to(dtype))
    if zmode == "given" and N >= 5 and M >= 6:
        z[5] = x[4]                                         # an exact duplicate off the diagonal
    lsv, var, al = gc.parameters(seed, D, ard, family)
    if ls is not None:
        lsv = torch.full_like(lsv, ls)
    if alpha is not None and al is not None:
        al = torch.full_like(al, alpha)
    cols = N if z is None else z.shape[0]
    g = np.random.default_rng(seed + 7)
    Gt = torch.ones(N, cols, dtype=dtype) if G == "ones" else torch.as_tensor(g.standard_normal((N, cols))).to(dtype)
    return x, z, lsv.to(dtype), var.to(dtype), None if al is None else al.to(dtype), Gt


def _dev(t):
    return None if t is None else t.to(DEV)


def _bounds(name, truth, twin, S, N, M, D, dtype):
    """The allowed |got - truth| per element."""
    A = truth.abs().max().item() if truth.numel() else 0.0
    if dtype == torch.float64:
        if S is None:
            return torch.full_like(truth, gc.EPS64 * 16 * (D + 8) * (1 + A))
        return gc.EPS64 * (N * M + 16 * D) * S
    own = (twin.double() - truth).abs()
    floor = 4 * gc.EPS32 * (1 + A) if S is None else 4 * gc.EPS32 * S
    return torch.maximum(4 * own, floor if isinstance(floor, torch.Tensor) else torch.full_like(truth, floor))


def _check(kernels, family, N, M, D, dtype, ard=False, want=(True,) * 5, forced=0, label="", **kw):
    x, z, ls, var, al, G = _inputs(family, N, M, D, dtype, ard, **kw)
    up = lambda t: None if t is None else t.double()      # noqa: E731
    truth = gc.restate(family, up(x), up(z), up(ls), up(var), up(al), up(G))
    twin = gc.restate(family, x, z, ls, var, al, G) if dtype == torch.float32 else truth
    dx = _dev(x)
    dz = dx if kw.get("zmode") == "same" else _dev(z)
    K = kernels.gp_kernel_fwd(dx, dz, _dev(ls), _dev(var), _dev(al), family)
    grads = kernels.gp_kernel_bwd(dx, dz, _dev(ls), _dev(var), _dev(al), _dev(G), family, want, forced)
    cols = N if z is None else z.shape[0]
    got = {"K": K, "gx": grads[0], "gz": grads[1], "g_ls": grads[2], "g_var": grads[3], "g_alpha": grads[4]}
    sums = {"g_ls": "S_ls", "g_var": "S_var", "g_alpha": "S_alpha"}
    wanted = {"K": True, "gx": want[0], "gz": want[1] and z is not None, "g_ls": want[2], "g_var": want[3],
              "g_alpha": want[4] and al is not None}
    worst = 0.0
    for name, value in got.items():
        if not wanted[name]:
            assert value is None, (label, name)
            continue
        t = truth[name]
        assert value.shape == t.shape and value.dtype == dtype, (label, name, value.shape, t.shape)
        S = truth[sums[name]] if name in sums else None
        bound = _bounds(name, t, twin[name], S, N, cols, D, dtype)
        err = (value.cpu().double() - t).abs()
        assert torch.isfinite(value).all(), (label, name)
        ratio = (err / bound.clamp(min=1e-300)).max().item() if err.numel() else 0.0
        worst = max(worst, ratio)
        assert (err <= bound).all(), "%s %s %s N=%d M=%d D=%d: error / bound %.3g (error %.3g)" % (
            label, family, name, N, cols, D, ratio, err.max().item())
    return worst


SHAPES = [(1, 1, 1), (2, 1, 2), (1, 2, 3), (63, 64, 4), (64, 65, 5), (65, 63, 8), (130, 64, 16), (64, 130, 17),
          (130, 130, 63), (63, 2, 64), (130, 65, 64)]


@pytest.mark.parametrize("dt", sorted(DTYPES))
@pytest.mark.parametrize("family", gc.FAMILIES)
def test_shapes_splits_and_lengthscales(kernels, family, dt):
    worst = 0.0
    for n, ((N, M, D), forced) in enumerate(zip(SHAPES, itertools.cycle([0, 1, 2, 7]))):
        for ard in (False, True):
            worst = max(worst, _check(kernels, family, N, M, D, DTYPES[dt], ard, forced=forced, seed=n,
                                      label="shape %d ard %d splits %d" % (n, ard, forced)))
    print("%s %s: worst error / bound %.3f" % (family, dt, worst))


@pytest.mark.parametrize("dt", sorted(DTYPES))
@pytest.mark.parametrize("family", gc.FAMILIES)
def test_z_null_and_z_the_same_tensor(kernels, family, dt):
    worst = 0.0
    for n, (N, forced) in enumerate(zip([1, 2, 63, 64, 65, 130], itertools.cycle([0, 2, 1, 7]))):
        D = [1, 3, 5, 8, 17, 64][n]
        for zmode in ("null", "same"):
            worst = max(worst, _check(kernels, family, N, N, D, DTYPES[dt], ard=bool(n & 1), forced=forced, seed=n,
                                      zmode=zmode, label="%s N=%d" % (zmode, N)))
    print("%s %s: worst error / bound %.3f" % (family, dt, worst))


@pytest.mark.parametrize("dt", sorted(DTYPES))
@pytest.mark.parametrize("N,M", [(3, 5000), (5000, 3)])
def test_few_rows_against_many_columns_split_by_the_plan(kernels, N, M, dt):
    for family in ("matern32", "rational_quadratic"):
        for ones in (False, True):
            _check(kernels, family, N, M, 5, DTYPES[dt], ard=True, G="ones" if ones else "random", label="few rows")


@pytest.mark.parametrize("dt", sorted(DTYPES))
def test_every_combination_of_wanted_gradients(kernels, dt):
    for want in itertools.product([False, True], repeat=5):
        _check(kernels, "rational_quadratic", 65, 63, 3, DTYPES[dt], ard=True, want=want, forced=2, label=str(want))
    for want in itertools.product([False, True], repeat=5):
        if not want[1]:
            _check(kernels, "matern52", 66, 66, 4, DTYPES[dt], want=want, zmode="null", label="null " + str(want))


@pytest.mark.parametrize("dt", sorted(DTYPES))
@pytest.mark.parametrize("family", gc.FAMILIES)
def test_edges(kernels, family, dt):
    dtype = DTYPES[dt]
    _check(kernels, family, 70, 66, 5, dtype, ard=True, shift=1e3, label="shift 1e3")
    _check(kernels, family, 70, 70, 5, dtype, ard=True, shift=1e3, zmode="null", label="shift 1e3, z null")
    _check(kernels, family, 40, 33, 3, dtype, ls=1e-3, label="lengthscale 1e-3")
    _check(kernels, family, 40, 33, 3, dtype, ls=1e3, label="lengthscale 1e3")
    if family == "rational_quadratic":
        _check(kernels, family, 40, 33, 3, dtype, alpha=1e-2, label="alpha 1e-2")
        _check(kernels, family, 40, 33, 3, dtype, alpha=1e2, label="alpha 1e2")


@pytest.mark.parametrize("dt", sorted(DTYPES))
@pytest.mark.parametrize("family", gc.FAMILIES)
def test_duplicates_and_far_pairs(kernels, family, dt):
    dtype = DTYPES[dt]
    one = torch.ones(1, dtype=dtype, device=DEV)
    al = one.clone() if family == "rational_quadratic" else None
    # two identical points: every term of gX is its own or its duplicate's, d = 0 exactly
    x = torch.tensor([[0.3, -1.7, 2.9]] * 2, dtype=dtype, device=DEV)
    G = torch.tensor([[1.0, 2.0], [-3.0, 0.5]], dtype=dtype, device=DEV)
    for z in (None, x.clone()):
        gx, gz, gl, gv, ga = kernels.gp_kernel_bwd(x, z, one, one, al, G, family)
        assert torch.equal(gx, torch.zeros_like(gx)) and (z is None or torch.equal(gz, torch.zeros_like(gz)))
        assert torch.isfinite(gl).all() and torch.isfinite(gv).all()
    # pairs at r = 30: underflow gives 0 (or a tiny number), never NaN
    x = torch.zeros(3, 2, dtype=dtype, device=DEV)
    z = torch.tensor([[30.0, 0.0], [0.0, -30.0]], dtype=dtype, device=DEV)
    K = kernels.gp_kernel_fwd(x, z, one, one, al, family)
    grads = kernels.gp_kernel_bwd(x, z, one, one, al, torch.ones_like(K), family)
    assert torch.isfinite(K).all() and (K >= 0).all() and all(g is None or torch.isfinite(g).all() for g in grads)
    if family == "rbf":
        assert (K == 0).all() or dtype == torch.float64


class _SpyLib:
    """The loaded library with the GP entry points counted."""

    def __init__(self, real, calls):
        self._real, self._calls = real, calls

    def __getattr__(self, name):
        if name.startswith("pa_gp_kernel"):
            self._calls.append(name)
        return getattr(self._real, name)


def test_empty_results_make_no_launch(kernels, monkeypatch):
    one = torch.ones(1, device=DEV)
    calls = []
    spy = _SpyLib(kernels._lib.load(), calls)
    monkeypatch.setattr(kernels._lib, "load", lambda: spy)
    for N, M in ((0, 5), (5, 0), (0, 0)):
        x, z = torch.zeros(N, 3, device=DEV), torch.zeros(M, 3, device=DEV)
        K = kernels.gp_kernel_fwd(x, z, one, one, None, "rbf")
        assert K.shape == (N, M)
        gx, gz, gl, gv, ga = kernels.gp_kernel_bwd(x, z, one, one, None, K, "rbf")
        assert gx.shape == (N, 3) and gz.shape == (M, 3) and float(gl) == 0 and float(gv) == 0 and ga is None
    assert calls == []
    kernels.gp_kernel_fwd(torch.zeros(2, 3, device=DEV), None, one, one, None, "rbf")
    assert calls == ["pa_gp_kernel_fwd"]


def test_arguments_are_checked_before_any_launch(kernels):
    from pyro_amd import _lib
    one = torch.ones(1, device=DEV)
    x = torch.zeros(4, 65, device=DEV)
    with pytest.raises(_lib.Unsupported):
        kernels.gp_kernel_fwd(x, None, one, one, None, "rbf")
    x = torch.zeros(4, 3, device=DEV)
    with pytest.raises(ValueError):
        kernels.gp_kernel_fwd(x, None, torch.ones(2, device=DEV), one, None, "rbf")
    with pytest.raises(ValueError):
        kernels.gp_kernel_fwd(x, None, one, one, None, "rational_quadratic")
    with pytest.raises(ValueError):
        kernels.gp_kernel_fwd(x, None, one.double(), one, None, "rbf")
    # a workspace smaller than the plan's records is refused by the entry point
    lib = _lib.load()
    ws = torch.empty(1, dtype=torch.float64, device=DEV)
    G = torch.ones(4, 4, device=DEV)
    gx = torch.zeros_like(x)
    rc = lib.pa_gp_kernel_bwd(_lib.PA_F32, 0, x.data_ptr(), None, one.data_ptr(), 1, one.data_ptr(), None, G.data_ptr(),
                              4, 4, 3, gx.data_ptr(), None, None, None, None, 0, ws.data_ptr(), 8, None)
    assert rc == _lib.PA_ERR_INVALID and b"workspace" in lib.pa_last_error()
    need = lib.pa_gp_kernel_bwd_workspace(4, 4, 3, 1, 1, 0, 0)
    assert need == (4 * 3 + 1 * (3 + 3)) * 8


# ---- the classes -------------------------------------------------------------------------------------------------------
def _kernel_on_device(gp, family, D, dtype, ard=True, seed=0):
    ls, var, al = gc.parameters(seed, D, ard, family, dtype)
    return gc.build_stationary(gp, family, D, ls, var, al).to(DEV)


@pytest.mark.parametrize("dt", sorted(DTYPES))
def test_two_calls_are_bit_equal(kernels, dt):
    dtype = DTYPES[dt]
    x, z, ls, var, al, G = (_dev(t) for t in _inputs("rational_quadratic", 300, 130, 7, dtype, True))
    first = (kernels.gp_kernel_fwd(x, z, ls, var, al, 1),) + kernels.gp_kernel_bwd(x, z, ls, var, al, G, 1)
    again = (kernels.gp_kernel_fwd(x, z, ls, var, al, 1),) + kernels.gp_kernel_bwd(x, z, ls, var, al, G, 1)
    assert all(torch.equal(a, b) for a, b in zip(first, again))


@pytest.mark.parametrize("family", gc.FAMILIES)
def test_class_gradients_survive_an_in_place_diagonal_and_a_transposed_gradient(family):
    import pyro_amd.contrib.gp as gp
    dtype = torch.float64
    kern = _kernel_on_device(gp, family, 4, dtype)
    X = gc.points(3, 37, 4).to(DEV).requires_grad_()
    params = [p for p in kern.parameters()]

    def run(modify):
        for p in params + [X]:
            p.grad = None
        K = kern(X)
        if modify:
            K.view(-1)[::K.size(0) + 1] += 0.37
        w = torch.linspace(-1, 1, K.numel(), dtype=dtype, device=DEV).reshape(K.shape)
        got = []
        hook = K.register_hook(lambda g: got.append(g))
        (K.t() * w).sum().backward()                  # dL/dK arrives as w.t(): a transposed view
        hook.remove()
        assert not got[0].is_contiguous() and got[0].t().is_contiguous()
        return [X.grad.clone()] + [p.grad.clone() for p in params]

    plain, modified = run(False), run(True)
    assert all(torch.equal(a, b) for a, b in zip(plain, modified))
    # and they are the restatement's
    ls, var = kern.lengthscale.detach().cpu(), kern.variance.detach().cpu()
    al = kern.scale_mixture.detach().cpu() if family == "rational_quadratic" else None
    w = torch.linspace(-1, 1, 37 * 37, dtype=dtype).reshape(37, 37)
    truth = gc.restate(family, X.detach().cpu(), None, ls, var, al, w.t())
    bound = gc.EPS64 * 16 * (4 + 8) * (1 + truth["gx"].abs().max())
    assert ((plain[0].cpu() - truth["gx"]).abs() <= bound).all()


def test_routing_of_the_classes(monkeypatch):
    import pyro_amd.contrib.gp as gp
    from pyro_amd import kernels
    calls = []
    real_fwd, real_bwd = kernels.gp_kernel_fwd, kernels.gp_kernel_bwd
    monkeypatch.setattr(kernels, "gp_kernel_fwd", lambda *a, **k: calls.append("fwd") or real_fwd(*a, **k))
    monkeypatch.setattr(kernels, "gp_kernel_bwd", lambda *a, **k: calls.append("bwd") or real_bwd(*a, **k))
    dtype = torch.float64
    x, z = gc.points(0, 20, 5).to(DEV), gc.points(1, 9, 5).to(DEV)
    for family in gc.FAMILIES:
        kern = _kernel_on_device(gp, family, 5, dtype)
        del calls[:]
        K = kern(x, z)
        assert calls == ["fwd"], family
        K.sum().backward()
        assert calls == ["fwd", "bwd"], family
        assert kern(x, diag=True).shape == (20,) and calls == ["fwd", "bwd"]
        ls, var = kern.lengthscale.detach().cpu(), kern.variance.detach().cpu()
        al = kern.scale_mixture.detach().cpu() if family == "rational_quadratic" else None
        fused = K.detach().cpu()
        monkeypatch.setattr(gp.kernels, "FUSED_GP_KERNEL", False)
        del calls[:]
        off = kern(x, z).detach().cpu()
        monkeypatch.setattr(gp.kernels, "FUSED_GP_KERNEL", True)
        assert calls == []
        bound = gc.conditioning_bound(family, x.cpu(), z.cpu(), ls, var, al)
        assert ((off - fused).abs() <= bound + gc.EPS64 * 16 * 13 * (1 + fused.abs().max())).all(), family
    # D = 65 and a batched lengthscale take the torch route
    del calls[:]
    wide = gp.kernels.RBF(65, lengthscale=torch.full((65,), 3.0, dtype=dtype)).to(DEV)
    xw, zw = gc.points(0, 6, 65).to(DEV), gc.points(1, 4, 65).to(DEV)
    got = wide(xw, zw).detach().cpu()
    want = gc.restate_K("rbf", xw.cpu(), zw.cpu(), torch.full((65,), 3.0, dtype=dtype), torch.ones(1, dtype=dtype))
    assert calls == [] and ((got - want).abs() <= gc.conditioning_bound(
        "rbf", xw.cpu(), zw.cpu(), torch.full((65,), 3.0, dtype=dtype), torch.ones(1, dtype=dtype))).all()
    # (a [2, D] lengthscale divides row by row in the reference's formula: two points on each side)
    lsb = torch.as_tensor(np.random.default_rng(3).uniform(0.5, 2.0, size=(2, 5)))
    batched = gp.kernels.RBF(5, lengthscale=lsb.clone()).to(DEV)
    got = batched(x[:2], z[:2]).detach().cpu()
    one = torch.ones(1, dtype=dtype)
    xs, zs = x[:2].cpu() / lsb, z[:2].cpu() / lsb
    assert calls == [] and ((got - gc.restate_K("rbf", xs, zs, one, one)).abs()
                            <= gc.conditioning_bound("rbf", xs, zs, one, one)).all()
    mixed = gp.kernels.RBF(5).to(DEV)                      # float32 parameters, float64 inputs
    mixed(x, z)
    assert calls == []


def test_the_typed_ops_and_their_fakes(kernels):
    from pyro_amd.ops import torch_library
    assert torch_library.available()
    for dtype in (torch.float32, torch.float64):
        x, z, ls, var, al, G = (_dev(t) for t in _inputs("rational_quadratic", 70, 33, 6, dtype, True))
        K = torch.ops.pyro_amd.gp_kernel(x, z, ls, var, al, 1)
        assert torch.equal(K, kernels.gp_kernel_fwd(x, z, ls, var, al, 1))
        outs = torch.ops.pyro_amd.gp_kernel_bwd(x, z, ls, var, al, G, 1, True, True, True, True, True, 0)
        for a, b in zip(outs, kernels.gp_kernel_bwd(x, z, ls, var, al, G, 1)):
            assert torch.equal(a, b)
        outs = torch.ops.pyro_amd.gp_kernel_bwd(x, None, ls, var, al, G[:, :33].new_ones(70, 70), 1, True, True, False,
                                                False, True, 2)
        assert [tuple(o.shape) for o in outs] == [(70, 6), (0,), (0,), (0,), (1,)]
    m = lambda *sh: torch.empty(sh, device="meta")      # noqa: E731
    assert torch.ops.pyro_amd.gp_kernel(m(5, 3), m(7, 3), m(3), m(1), None, 0).shape == (5, 7)
    outs = torch.ops.pyro_amd.gp_kernel_bwd(m(5, 3), m(7, 3), m(3), m(1), None, m(5, 7), 0, True, True, False, True, True, 0)
    assert [tuple(o.shape) for o in outs] == [(5, 3), (7, 3), (0,), (1,), (0,)]
