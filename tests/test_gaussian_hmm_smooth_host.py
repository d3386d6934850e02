"""GaussianHMM.smooth without a device: the torch route of pyro_amd/distributions/hmm.py (_rts_smoother: the Kalman
filter, then the Rauch-Tung-Striebel recursion with the covariance in subtraction form; the route of CPU tensors and
of everything that needs a gradient, and the float64 restatement the kernel of csrc/gaussian_hmm_smooth.hip is tested
against).

Targets, float64, on gaussian_hmm_cases.rel_err per array (kinds ``mean``, ``cov``, ``cross``), tolerance 1e-9:

    the fixtures of the unmodified reference (tests/golden/gaussian_hmm_posterior.npz) on the eight cases;
    an INDEPENDENT oracle on the edge cases of tests/gaussian_hmm_edge_cases.py: the dense joint Gaussian of
    (z_1..z_T, x_1..x_T), built by unrolling the model, conditioned on x with torch.linalg.solve -- no filter, no
    recursion, none of hmm.py;
    the package's other two ways to the same moments: rsample_posterior with zero noise (mean) and the moments
    rebuilt from the backward-sampling maps, which hold the covariance in Joseph form (all three kinds).

Worst figures as the tests print them (x86-64 CPU): fixtures 2.8e-15; dense oracle A 8e-16, B 6e-15, D 1.8e-12 (the
first two seeds of every recipe x shape); the two other routes 3.2e-16.

Then shapes, differentiability (gradcheck on a tiny model) and bad series: a Q that is not positive definite is seen
ONLY by the backward sweep, through its factor of P^p or its check of Q's own pivots (test_a_bad_q_marks_its_series);
a bad P0 is seen by nothing on this path."""
import numpy as np
import pytest
import torch

import pyro_amd.distributions as dist
from pyro_amd.distributions import hmm
from tests import gaussian_hmm_cases as gc
from tests import gaussian_hmm_edge_cases as ec
from tests import gaussian_hmm_posterior_cases as pc

TOL = 1e-9
CPU = torch.device("cpu")
F64 = torch.float64
KINDS = pc.KINDS
_id = lambda v: "_".join(str(x) for x in v) if isinstance(v, tuple) else str(v)           # noqa: E731


def _np(v):
    return v.detach().cpu().double().numpy()


def _dist(case, requires_grad=False):
    t = gc.leaves(case, F64, CPU, requires_grad)
    return t, gc.build(t, case, dist)


def _errors(got, want):
    return {k: gc.rel_err(_np(g) if isinstance(g, torch.Tensor) else g, want[k]) for k, g in zip(KINDS, got)}


def _fmt(err):
    return " ".join("%s %.1e" % kv for kv in err.items())


def dense_conditioning(p, x):
    """{"mean", "cov", "cross"} of z_1..z_T given x from the parts in the kernels' layouts ([B | 1, T | 1, ...]) and
    x [B, T, o]: the joint Gaussian of the whole path and all the data, unrolled step by step (columns:
    z_t = F_t^T z_{t-1} + q_t + w_t, x_t = H_t^T z_t + r_t + v_t), then conditioned in one dense solve"""
    B, T, o = x.shape
    m0, P0, F, q, Q, H, r, R = (a.expand((B,) + tuple(a.shape[1:])) if i < 2 else
                                a.expand((B, T) + tuple(a.shape[2:])) for i, a in enumerate(p))
    h = m0.shape[-1]
    mu_z, mu_x = x.new_zeros(B, T * h), x.new_zeros(B, T * o)
    Szz, Hb, Rb = x.new_zeros(B, T * h, T * h), x.new_zeros(B, T * o, T * h), x.new_zeros(B, T * o, T * o)
    mu, S = m0, P0
    for t in range(T):
        A = F[:, t].transpose(-1, -2)
        zt, xt = slice(t * h, (t + 1) * h), slice(t * o, (t + 1) * o)
        mu = (A @ mu.unsqueeze(-1)).squeeze(-1) + q[:, t]
        S = A @ S @ A.transpose(-1, -2) + Q[:, t]
        Szz[:, zt, :t * h] = A @ Szz[:, (t - 1) * h:t * h, :t * h] if t else Szz[:, zt, :0]
        Szz[:, :t * h, zt] = Szz[:, zt, :t * h].transpose(-1, -2)
        Szz[:, zt, zt] = S
        mu_z[:, zt] = mu
        Hb[:, xt, zt] = H[:, t].transpose(-1, -2)
        Rb[:, xt, xt] = R[:, t]
        mu_x[:, xt] = (H[:, t].transpose(-1, -2) @ mu.unsqueeze(-1)).squeeze(-1) + r[:, t]
    Sxz = Hb @ Szz
    Sxx = Sxz @ Hb.transpose(-1, -2) + Rb
    K = torch.linalg.solve(Sxx, Sxz).transpose(-1, -2)                   # Szx Sxx^-1
    mean = mu_z + (K @ (x.reshape(B, T * o) - mu_x).unsqueeze(-1)).squeeze(-1)
    cov = Szz - K @ Sxz
    blocks = lambda k: torch.stack([cov[:, t * h:(t + 1) * h, (t + k) * h:(t + k + 1) * h]      # noqa: E731
                                    for t in range(T - k)], dim=1) if T > k else x.new_zeros(B, 0, h, h)
    return {"mean": mean.reshape(B, T, h).numpy(), "cov": blocks(0).numpy(), "cross": blocks(1).numpy()}


# ---- the fixtures of the unmodified reference ---------------------------------------------------------------------
@pytest.mark.parametrize("case", gc.CASES)
def test_fixtures(case):
    t, d = _dist(case)
    got = d.smooth(t["x"], cross=True)
    B, T, h = t["x"].shape[0], t["x"].shape[1], d.hidden_dim
    assert [tuple(v.shape) for v in got] == [(B, T, h), (B, T, h, h), (B, T - 1, h, h)]
    err = _errors(got, pc.golden(case))
    print(case, "torch route against the fixture:", _fmt(err))
    assert max(err.values()) < TOL, err
    assert torch.equal(got[1], got[1].transpose(-1, -2))
    # the other two ways to these moments: zero noise, and the maps of the backward sampler (Joseph form)
    zero = d.rsample_posterior(t["x"], noise=torch.zeros(B, T, h, dtype=F64))
    maps = pc.moments(*hmm._backward_sample_maps(*d._parts, t["x"]))
    err2 = dict(_errors(got, maps), zero_noise=gc.rel_err(_np(got[0]), _np(zero)))
    print(case, "against the backward sampler's maps:", _fmt(err2))
    assert max(err2.values()) < TOL, err2


# ---- the independent oracle ---------------------------------------------------------------------------------------
def _against_dense(key):
    t = ec.leaves(key, F64, CPU)
    p, x = ec.parts(t), t["x"]
    B, T, _ = x.shape
    got = ec.model(p, T, B).smooth(x, cross=True)
    err = _errors(got, dense_conditioning(p, x))
    print(_id(key), "torch route against dense conditioning:", _fmt(err))
    assert max(err.values()) < TOL, (key, err)


@pytest.mark.parametrize("key", ec.A_KEYS, ids=_id)
def test_dense_oracle_layouts(key):
    _against_dense(key)


@pytest.mark.parametrize("shape", ec.B_SHAPES, ids=_id)
def test_dense_oracle_width_border_and_short_chains(shape):
    for T in ec.B_TS:
        _against_dense(("B",) + shape + (T, False))


@pytest.mark.parametrize("shape", ec.D_SHAPES, ids=_id)
@pytest.mark.parametrize("recipe", ec.RECIPES)
def test_dense_oracle_ill_conditioned(recipe, shape):
    for key in ec.d_keys(recipe, shape)[:2]:
        _against_dense(key)


# ---- shapes ---------------------------------------------------------------------------------------------------------
def test_shapes():
    t, d = _dist("b3_t7_h3_o2_shared")                      # time-homogeneous: event_shape (1, 2), data of any length
    x = t["x"]
    two = d.smooth(x)
    assert isinstance(two, tuple) and len(two) == 2 and two[0].shape == (3, 7, 3) and two[1].shape == (3, 7, 3, 3)
    three = d.smooth(x, cross=True)
    assert len(three) == 3 and three[2].shape == (3, 6, 3, 3) and torch.equal(three[0], two[0])
    assert all(v.dtype == F64 and torch.isfinite(v).all() for v in three)
    for T in (4, 2):                                                                      # data of several lengths
        m, V, X = d.smooth(x[:, :T], cross=True)
        assert m.shape == (3, T, 3) and V.shape == (3, T, 3, 3) and X.shape == (3, T - 1, 3, 3)
    m, V, X = d.smooth(x[:, :1], cross=True)                                              # T = 1
    assert m.shape == (3, 1, 3) and V.shape == (3, 1, 3, 3) and X.shape == (3, 0, 3, 3)
    post = d.filter(x[:, :1])                                # ... where the smoothed marginal is the filtered one
    torch.testing.assert_close(m[:, 0], post.loc, rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(V[:, 0], post.covariance_matrix, rtol=1e-12, atol=1e-12)
    x2 = torch.stack([x, x + 1.0])                                                        # a leading batch dim
    m2, V2, X2 = d.smooth(x2, cross=True)
    assert m2.shape == (2, 3, 7, 3) and V2.shape == (2, 3, 7, 3, 3) and X2.shape == (2, 3, 6, 3, 3)
    for a, b in zip((m2, V2, X2), d.smooth(x + 1.0, cross=True)):
        torch.testing.assert_close(a[1], b, rtol=1e-12, atol=1e-12)
    # sample-free batch broadcasting: a model of batch shape () against data of batch shape (3,)
    one = dist.GaussianHMM._from_parts(tuple(a[:1] for a in d._parts[:2]) + d._parts[2:], None, None)
    assert one.batch_shape == (1,) and one.smooth(x, cross=True)[2].shape == (3, 6, 3, 3)
    th, dh = _dist("b2_t9_h4_o3_het")                                                     # a per-step model
    assert dh.smooth(th["x"], cross=True)[2].shape == (2, 8, 4, 4)
    with pytest.raises(ValueError, match="time steps"):
        dh.smooth(th["x"][:, :5])
    t1, d1 = _dist("b3_t1_h2_o1")
    assert d1.smooth(t1["x"], cross=True)[2].shape == (3, 0, 2, 2)


@pytest.mark.parametrize("shape", ec.C_SHAPES, ids=_id)
def test_through_the_constructor(shape):
    """batch shape (2, 3), leaves of every partial batch shape, a non-contiguous F and value"""
    h, o = shape
    t = ec.class_leaves(h, o, "base", F64, CPU, requires_grad=False)
    d, x = ec.class_build(t)
    assert d.batch_shape == (2, 3) and not d._parts[2].is_contiguous() and not x.is_contiguous()
    m, V, X = d.smooth(x, cross=True)
    T = ec.C_T
    assert m.shape == (2, 3, T, h) and V.shape == (2, 3, T, h, h) and X.shape == (2, 3, T - 1, h, h)
    # against dense conditioning, with every part expanded to the six series
    p = [a.expand((2, 3) + tuple(a.shape[-(nd + (1 if i >= 2 else 0)):])).reshape(
        (6,) + tuple(a.shape[-(nd + (1 if i >= 2 else 0)):])) for i, (a, nd) in
        enumerate(zip(d._parts, (1, 2, 2, 1, 2, 2, 1, 2)))]
    want = dense_conditioning(p, x.reshape(6, T, o))
    err = _errors([v.reshape((6,) + tuple(v.shape[2:])) for v in (m, V, X)], want)
    print(_id(shape), "through the constructor against dense conditioning:", _fmt(err))
    assert max(err.values()) < TOL, err


# ---- gradients ------------------------------------------------------------------------------------------------------
def test_backward_reaches_every_leaf():
    case = "b2_t9_h4_o3_het"
    t, d = _dist(case, requires_grad=True)
    out = d.smooth(t["x"], cross=True)
    assert all(v.requires_grad for v in out)
    sum((v * v).sum() for v in out).backward()
    for k in gc.NAMES:
        assert t[k].grad is not None and torch.isfinite(t[k].grad).all() and t[k].grad.abs().max() > 0, k
    with torch.no_grad():
        assert not any(v.requires_grad for v in d.smooth(t["x"], cross=True))


@pytest.mark.parametrize("kind", [0, 1], ids=["mean", "cov"])
def test_gradcheck_on_a_tiny_model(kind):
    """B = 1, T = 3, hidden 2, obs 1, float64; the covariances through their Cholesky factors"""
    rng = np.random.default_rng(11)
    t = {k: torch.tensor(v) for k, v in ec.make_inputs(rng, 1, 3, 2, 1, (True,) * 6, (False,) * 6).items()}
    names = ec.NAMES

    def smoothed(*leaves):
        u = dict(zip(names, leaves))
        # (finite differences perturb the structurally zero upper triangles: ec.parts reads the lower ones)
        return ec.model(ec.parts(u), 3, 1).smooth(u["x"])[kind]

    leaves = [t[k].clone().requires_grad_() for k in names]
    assert smoothed(*leaves).requires_grad
    assert torch.autograd.gradcheck(smoothed, leaves, eps=1e-6, atol=1e-6, rtol=1e-5)


# ---- bad series -----------------------------------------------------------------------------------------------------
def _smooth_parts(p, x):
    return ec.model(p, x.shape[1], x.shape[0]).smooth(x, cross=True)


def _smallest_predicted_eigenvalue(p, x, b):
    """the smallest eigenvalue over the backward sweep's P^p = sym(F^T P_{t-1} F + Q) of series ``b``"""
    kept = []
    hmm._kalman_filter(*p, x, keep=kept)
    low = float("inf")
    for t in range(x.shape[1] - 1, 0, -1):
        Ft, Qt = hmm._step(p[2], t, 2), hmm._step(p[4], t, 2)
        Pp = (Ft.transpose(-1, -2) @ kept[t - 1][1] @ Ft + Qt).expand(x.shape[0], -1, -1)[b]
        low = min(low, float(torch.linalg.eigvalsh(0.5 * (Pp + Pp.T)).min()))
    return low


@pytest.mark.parametrize("key", ec.E_KEYS, ids=_id)
def test_a_bad_q_marks_its_series(key):
    """Series 1 of three with a Q that is not positive definite (lowered by 0.55 I) while every innovation covariance
    is: the filter (log_prob) is finite and only the backward sweep sees it -> NaN in all three outputs for that
    series.

    The sweep's factor of P^p = sym(F^T P_{t-1} F + Q) alone would not do: F^T P_{t-1} F lifts it back above zero
    on three of the four keys, and the recursion then hands back finite numbers for a model that is none.  So the
    sweep checks the pivots of the Q it uses as well (hmm._rts_smoother; in step_q Q is time-homogeneous, in hom_q
    per-step).  The smallest eigenvalue of series 1's Q and of its P^p over the sweep, float64, as this test
    prints them:

        key                 Q          P^p
        A step_q (3, 2)     -0.020     +0.480
        A step_q (9, 2)     -0.049     +0.188
        A hom_q  (3, 2)     -0.050     -0.011
        A hom_q  (9, 2)     -0.047     +0.013"""
    p, x = ec.bad_pivot_parts(key, "Q", F64, CPU)
    assert torch.isfinite(hmm._kalman_filter(*p, x)[0]).all()
    print(_id(key), "smallest eigenvalue of series 1's Q %.3f, of its P^p over the sweep %.3f" % (
        float(torch.linalg.eigvalsh(p[4][1]).min()), _smallest_predicted_eigenvalue(p, x, 1)))
    for b in _smooth_parts(p, x):
        assert torch.isnan(b[1]).all()


@pytest.mark.parametrize("key", ec.E_KEYS, ids=_id)
def test_a_bad_q_or_p0_leaves_the_other_series_alone(key):
    good = _smooth_parts(*ec.bad_pivot_parts(key, None, F64, CPU))
    bad = _smooth_parts(*ec.bad_pivot_parts(key, "Q", F64, CPU))
    for a, b in zip(good, bad):
        assert a.shape[0] == 3 and torch.isfinite(a).all() and torch.isfinite(b[0]).all() and torch.isfinite(b[2]).all()
        assert torch.equal(a[0], b[0]) and torch.equal(a[2], b[2])
    # a P0 that is not positive definite is never factorised on this path, and the first P^p still is: all finite
    odd = _smooth_parts(*ec.bad_pivot_parts(key, "P0", F64, CPU))
    for a, b in zip(good, odd):
        assert torch.isfinite(b).all() and torch.equal(a[0], b[0]) and torch.equal(a[2], b[2])


def test_a_bad_series_in_the_filter_is_nan_and_alone():
    """one series of three with an R that is not positive definite: the filter's own pivot fails"""
    case = "b3_t7_h3_o2_shared"
    t, d = _dist(case)
    good = d.smooth(t["x"], cross=True)
    parts = list(d._parts)
    R = parts[7].expand(3, 1, 2, 2).clone()
    R[1] = -40.0 * torch.eye(2, dtype=F64)                      # S = H^T P^p H + R loses its first pivot
    parts[7] = R
    bad = dist.GaussianHMM._from_parts(tuple(parts), None, None).smooth(t["x"], cross=True)
    for a, b in zip(good, bad):
        assert torch.isfinite(a).all() and torch.isnan(b[1]).all()
        torch.testing.assert_close(b[0], a[0], rtol=1e-12, atol=1e-12)
        torch.testing.assert_close(b[2], a[2], rtol=1e-12, atol=1e-12)


# ---- routing and the layers below -----------------------------------------------------------------------------------
def test_cpu_tensors_take_the_torch_route(monkeypatch):
    from pyro_amd import kernels
    calls = []
    monkeypatch.setattr(kernels, "gaussian_hmm_smooth", lambda *a, **k: calls.append(1) or 1 / 0)
    t, d = _dist("b2_t9_h4_o3_het")
    assert all(torch.isfinite(v).all() for v in d.smooth(t["x"], cross=True)) and not calls


def test_typed_op_schema_and_c_abi_argument_errors():
    """pyro_amd::gaussian_hmm_smooth beside pyro_amd::gaussian_hmm_sample: schema and shape function; the C entry
    point's argument checks, all before any launch (no device here)"""
    from pyro_amd import _lib
    from pyro_amd.csrc.build import build_library, build_torch_ops
    from pyro_amd.ops import torch_library

    build_library()
    build_torch_ops()
    assert torch_library.available() and "pyro_amd::gaussian_hmm_smooth" in torch_library.registered_ops()
    assert str(torch.ops.pyro_amd.gaussian_hmm_smooth.default._schema) == (
        "pyro_amd::gaussian_hmm_smooth(Tensor m0, Tensor P0, Tensor trans, Tensor trans_loc, Tensor trans_cov, "
        "Tensor obs, Tensor obs_loc, Tensor obs_cov, Tensor x, bool need_cross) -> (Tensor mean, Tensor cov, "
        "Tensor[] cross)")
    m = lambda *sh: torch.empty(sh, device="meta")                                        # noqa: E731
    args = (m(1, 3), m(5, 3, 3), m(1, 1, 3, 3), m(5, 7, 3), m(1, 1, 3, 3), m(1, 7, 3, 2), m(1, 1, 2), m(5, 1, 2, 2),
            m(5, 7, 2))
    mean, cov, cross = torch.ops.pyro_amd.gaussian_hmm_smooth(*args, True)
    assert mean.shape == (5, 7, 3) and cov.shape == (5, 7, 3, 3) and [tuple(v.shape) for v in cross] == [(5, 6, 3, 3)]
    assert torch.ops.pyro_amd.gaussian_hmm_smooth(*args, False)[2] == []

    lib = _lib.load()
    none6 = [None, 0, 0] * 6

    def call(B, T, h, o, dtype=_lib.PA_F32):
        return lib.pa_gaussian_hmm_smooth(dtype, None, 0, None, 0, *none6, None, B, T, h, o, None, None, None,
                                          None, 0, None)

    assert call(0, 5, 3, 2) == _lib.PA_OK                                  # B = 0: nothing to do
    assert call(2, 0, 3, 2) == _lib.PA_ERR_INVALID and call(2, 5, 0, 2) == _lib.PA_ERR_INVALID
    assert call(2, 5, 17, 2) == _lib.PA_ERR_UNSUPPORTED and call(2, 5, 2, 17) == _lib.PA_ERR_UNSUPPORTED
    assert call(2, 5, 3, 2) == _lib.PA_ERR_INVALID and b"NULL" in lib.pa_last_error()
    assert call(2, 5, 3, 2, dtype=7) == _lib.PA_ERR_INVALID
    # the filtered moments of every step
    assert lib.pa_gaussian_hmm_smooth_workspace(_lib.PA_F32, 4, 10, 3, 2) == 4 * 10 * (3 + 9) * 4
    assert lib.pa_gaussian_hmm_smooth_workspace(_lib.PA_F64, 4, 10, 3, 2) == 4 * 10 * (3 + 9) * 8
    assert lib.pa_gaussian_hmm_smooth_workspace(_lib.PA_F64, 0, 10, 3, 2) == 0
