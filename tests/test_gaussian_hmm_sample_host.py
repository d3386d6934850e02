"""GaussianHMM.rsample_posterior without a device: the torch route of pyro_amd/distributions/hmm.py
(_backward_sample_maps and the backward-sampling loop; the route of CPU tensors and of everything that needs a
gradient, and the float64 restatement the kernels are tested against) on the fixtures of the unmodified reference
(tests/golden/gaussian_hmm_posterior.npz): the moments of the path's posterior rebuilt from the maps, the posterior
mean from zero noise, shapes, the noise argument, differentiability, a bad series.

Tolerance: 1e-9, the project's golden tolerance for float64, on gaussian_hmm_cases.rel_err (the moments measured
2e-16 .. 3e-15 when the fixtures were made)."""
import numpy as np
import pytest
import torch

import pyro_amd.distributions as dist
from pyro_amd.distributions import hmm
from tests import gaussian_hmm_cases as gc
from tests import gaussian_hmm_posterior_cases as pc

TOL = 1e-9
CPU = torch.device("cpu")
F64 = torch.float64


def _dist(case, requires_grad=False):
    t = gc.leaves(case, F64, CPU, requires_grad)
    return t, gc.build(t, case, dist)


@pytest.mark.parametrize("case", gc.CASES)
def test_maps_rebuild_the_reference_posterior(case):
    t, d = _dist(case)
    c, G, L = hmm._backward_sample_maps(*d._parts, t["x"])
    B, T, h = t["x"].shape[0], t["x"].shape[1], d.hidden_dim
    assert c.shape == (B, T, h) and G.shape == L.shape == (B, T, h, h)
    assert not G[:, -1].any() and torch.equal(L, L.tril())
    err = pc.moment_errors(c, G, L, case)
    print(case, {k: "%.1e" % v for k, v in err.items()})
    assert max(err.values()) < TOL, err
    # zero noise: the posterior mean
    mean = d.rsample_posterior(t["x"], noise=torch.zeros(B, T, h, dtype=F64))
    assert gc.rel_err(mean.numpy(), pc.golden(case)["mean"]) < TOL


def test_shapes():
    t, d = _dist("b3_t7_h3_o2_shared")                      # time-homogeneous: event_shape (1, 2), data of any length
    x = t["x"]
    for sample_shape in ((), (5,), (2, 3)):
        z = d.rsample_posterior(x, sample_shape)
        assert z.shape == sample_shape + (3, 7, 3) and z.dtype == F64 and torch.isfinite(z).all()
    assert d.rsample_posterior(x[:, :4]).shape == (3, 4, 3)
    assert d.rsample_posterior(x[:, :1], (2,)).shape == (2, 3, 1, 3)                     # T = 1
    x2 = torch.stack([x, x + 1.0])                                                        # a leading batch dim
    noise = torch.randn(2, 3, 7, 3, dtype=F64)
    z2 = d.rsample_posterior(x2, noise=noise)
    assert z2.shape == (2, 3, 7, 3)
    torch.testing.assert_close(z2[1], d.rsample_posterior(x + 1.0, noise=noise[1]), rtol=1e-12, atol=1e-12)
    th, dh = _dist("b2_t9_h4_o3_het")
    assert dh.rsample_posterior(th["x"], (4,)).shape == (4, 2, 9, 4)
    with pytest.raises(ValueError, match="time steps"):
        dh.rsample_posterior(th["x"][:, :5])
    t1, d1 = _dist("b3_t1_h2_o1")
    assert d1.rsample_posterior(t1["x"]).shape == (3, 1, 2)


def test_noise_argument():
    t, d = _dist("b2_t9_h4_o3_het")
    for k, sample_shape in ((3, ()), (4, (5,))):
        torch.manual_seed(k)
        a = d.rsample_posterior(t["x"], sample_shape)
        torch.manual_seed(k)
        noise = torch.randn(sample_shape + (2, 9, 4), dtype=F64)
        assert torch.equal(a, d.rsample_posterior(t["x"], sample_shape, noise=noise))
    for shape in ((2, 10, 4), (9, 4), (5, 2, 9, 4)):
        with pytest.raises(ValueError, match="noise"):
            d.rsample_posterior(t["x"], noise=torch.zeros(shape, dtype=F64))
    with pytest.raises(ValueError, match="noise"):
        d.rsample_posterior(t["x"], (5,), noise=torch.zeros(2, 9, 4, dtype=F64))


def test_draws_have_the_posterior_moments():
    """the sample mean of 20 000 paths within 5 standard errors of the fixture's mean, at every step"""
    case = "b3_t7_h3_o2_shared"
    t, d = _dist(case)
    torch.manual_seed(0)
    n = 20000
    z = d.rsample_posterior(t["x"], (n,))
    g = pc.golden(case)
    var = np.diagonal(g["cov"], axis1=-2, axis2=-1)
    assert (np.abs(z.mean(0).numpy() - g["mean"]) < 5 * np.sqrt(var / n)).all()
    assert np.abs(z.var(0).numpy() / var - 1).max() < 5 * np.sqrt(2.0 / n)


def test_draws_are_differentiable():
    case = "b3_t7_h3_o2_shared"
    t = gc.leaves(case, F64, CPU, requires_grad=False)
    noise = pc.fixed_noise(case, 1)[0]
    names = ("m0", "F", "Lq", "H", "x")

    def draws(*leaves):
        u = dict(t, **dict(zip(names, leaves)))
        u["Lq"] = u["Lq"].tril()                 # (finite differences perturb the structurally zero upper triangle)
        return gc.build(u, case, dist).rsample_posterior(u["x"], noise=noise)

    leaves = [t[k].clone().requires_grad_() for k in names]
    assert draws(*leaves).requires_grad
    # (fast mode: the 63 x 75 Jacobian checked along random directions instead of entry by entry)
    assert torch.autograd.gradcheck(draws, leaves, eps=1e-6, atol=1e-6, rtol=1e-5, fast_mode=True)


def test_a_bad_series_is_nan_and_alone():
    """one series of three with an R that is not positive definite: NaN there, the other two as without it"""
    case = "b3_t7_h3_o2_shared"
    t, d = _dist(case)
    noise = pc.fixed_noise(case, 2)
    good = d.rsample_posterior(t["x"], (2,), noise=noise)
    parts = list(d._parts)
    R = parts[7].expand(3, 1, 2, 2).clone()
    R[1] = -40.0 * torch.eye(2, dtype=F64)                      # S = H^T P^p H + R loses its first pivot
    parts[7] = R
    bad = dist.GaussianHMM._from_parts(tuple(parts), None, None).rsample_posterior(t["x"], (2,), noise=noise)
    assert torch.isnan(bad[:, 1]).all() and torch.isfinite(good).all()
    torch.testing.assert_close(bad[:, 0], good[:, 0], rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(bad[:, 2], good[:, 2], rtol=1e-12, atol=1e-12)


def test_cpu_tensors_take_the_torch_route(monkeypatch):
    from pyro_amd import kernels
    calls = []
    monkeypatch.setattr(kernels, "gaussian_hmm_sample", lambda *a, **k: calls.append(1) or 1 / 0)
    t, d = _dist("b2_t9_h4_o3_het")
    assert torch.isfinite(d.rsample_posterior(t["x"])).all() and not calls


def test_typed_op_schema_and_c_abi_argument_errors():
    """pyro_amd::gaussian_hmm_sample beside pyro_amd::gaussian_hmm: schema and shape function; the C entry point's
    argument checks, all before any launch (no device here)"""
    from pyro_amd import _lib
    from pyro_amd.csrc.build import build_library, build_torch_ops
    from pyro_amd.ops import torch_library

    build_library()
    build_torch_ops()
    assert torch_library.available() and "pyro_amd::gaussian_hmm_sample" in torch_library.registered_ops()
    assert str(torch.ops.pyro_amd.gaussian_hmm_sample.default._schema) == (
        "pyro_amd::gaussian_hmm_sample(Tensor m0, Tensor P0, Tensor trans, Tensor trans_loc, Tensor trans_cov, "
        "Tensor obs, Tensor obs_loc, Tensor obs_cov, Tensor x, Tensor eps, bool need_maps) -> (Tensor z, Tensor[] maps)")
    m = lambda *sh: torch.empty(sh, device="meta")                                        # noqa: E731
    args = (m(1, 3), m(5, 3, 3), m(1, 1, 3, 3), m(5, 7, 3), m(1, 1, 3, 3), m(1, 7, 3, 2), m(1, 1, 2), m(5, 1, 2, 2),
            m(5, 7, 2), m(4, 5, 7, 3))
    z, maps = torch.ops.pyro_amd.gaussian_hmm_sample(*args, True)
    assert z.shape == (4, 5, 7, 3) and [tuple(v.shape) for v in maps] == [(5, 7, 3), (5, 7, 3, 3), (5, 7, 3, 3)]
    assert torch.ops.pyro_amd.gaussian_hmm_sample(*args, False)[1] == []

    lib = _lib.load()
    none6 = [None, 0, 0] * 6

    def call(B, T, h, o, S, dtype=_lib.PA_F32, maps=(None, None, None)):
        return lib.pa_gaussian_hmm_sample(dtype, None, 0, None, 0, *none6, None, B, T, h, o, S, None, None, *maps,
                                          None, 0, None)

    one = torch.zeros(1)
    p = one.data_ptr()
    assert call(0, 5, 3, 2, 4) == _lib.PA_OK                               # B = 0: nothing to do
    assert call(2, 5, 3, 2, 0) == _lib.PA_OK                               # S = 0 and no maps asked for: nothing to do
    assert call(2, 5, 3, 2, 0, maps=(p, p, p)) == _lib.PA_ERR_INVALID and b"NULL" in lib.pa_last_error()
    assert call(2, 0, 3, 2, 4) == _lib.PA_ERR_INVALID and call(2, 5, 3, 2, -1) == _lib.PA_ERR_INVALID
    assert call(2, 5, 17, 2, 4) == _lib.PA_ERR_UNSUPPORTED and call(2, 5, 2, 17, 4) == _lib.PA_ERR_UNSUPPORTED
    assert call(2, 5, 3, 2, 4) == _lib.PA_ERR_INVALID and b"NULL" in lib.pa_last_error()
    assert call(2, 5, 3, 2, 4, dtype=7) == _lib.PA_ERR_INVALID
    assert call(2, 5, 3, 2, 4, maps=(p, None, p)) == _lib.PA_ERR_INVALID and b"maps" in lib.pa_last_error()
    # the filtered moments of every step, and the maps of a caller that does not keep them
    assert lib.pa_gaussian_hmm_sample_workspace(_lib.PA_F32, 4, 10, 3, 2) == 4 * 10 * ((3 + 9) + (3 + 18)) * 4
    assert lib.pa_gaussian_hmm_sample_workspace(_lib.PA_F64, 4, 10, 3, 2) == 4 * 10 * ((3 + 9) + (3 + 18)) * 8
    assert lib.pa_gaussian_hmm_sample_workspace(_lib.PA_F64, 0, 10, 3, 2) == 0
