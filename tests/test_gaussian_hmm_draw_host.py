"""GaussianHMM.rsample on the host: the torch route (the generative loop, now with ``noise=``) in float64 on the CPU
against the fixtures of the unmodified reference (tests/golden/gaussian_hmm_prior.npz) and against the float64 numpy
restatement of the three equations (tests/gaussian_hmm_prior_cases.restate, shared with the device tests), its
random stream against a copy of the loop as it was, its gradients, and which route a call takes.

The common tool is the affine map: one call with zero noise plus the h + T (h + o) unit vectors as its sample dimension
gives the mean a and the linear part M of x, and M M^T.  Errors are gaussian_hmm_cases.rel_err; the tolerance is 1e-12
(gaussian_hmm_prior_cases.TOL64)."""
import numpy as np
import pytest
import torch

import pyro_amd.distributions as dist
from pyro_amd import kernels
from pyro_amd.distributions import hmm
from tests import gaussian_hmm_cases as gc
from tests import gaussian_hmm_prior_cases as pr

F64 = torch.float64
CPU = torch.device("cpu")


def _build(case, dtype=F64, requires_grad=False, duration=True):
    t = gc.leaves(case, dtype, CPU, requires_grad=requires_grad)
    d = gc.build(t, case, dist)
    B, T, o = t["x"].shape
    if d.duration is None and duration:
        d = dist.GaussianHMM._from_parts(d._parts, T, None)
    return t, d, (B, T, d.hidden_dim, o)


def _fmt(err):
    return {k: "%.1e" % v for k, v in err.items()}


@pytest.mark.parametrize("case", gc.CASES)
def test_affine_map_against_the_reference(case):
    _, d, (B, T, h, o) = _build(case)
    x = d.rsample((1 + h + T * (h + o),), noise=pr.unit_noise(B, T, h, o))
    assert x.shape == (1 + h + T * (h + o), B, T, o)
    err = pr.moment_errors(x, pr.golden(case), "x_")
    print(case, "torch route f64 against the reference", _fmt(err))
    assert max(err.values()) <= pr.TOL64, err


@pytest.mark.parametrize("case", gc.CASES)
def test_draws_against_the_restatement(case):
    _, d, (B, T, h, o) = _build(case)
    noise = pr.seeded_noise(case, 3, B, T, h, o)
    x = d.rsample((3,), noise=noise)
    want, _ = pr.restate(pr.model(case), *(e.numpy() for e in noise))
    err = gc.rel_err(x.numpy(), want)
    print(case, "torch route f64 against the restatement %.1e" % err)
    assert err <= pr.TOL64
    # zeros give the mean path
    zero = [torch.zeros_like(e[:1]) for e in noise]
    assert gc.rel_err(d.rsample((1,), noise=zero).numpy()[0], pr.golden(case)["x_mean"]) <= pr.TOL64


@pytest.mark.parametrize("case", [c for c in gc.CASES if gc.golden(c)["x"].shape[1] >= 2])
def test_forecast_against_the_reference(case):
    t, d, (B, T, h, o) = _build(case)
    t0, f = T // 2, T - T // 2
    fc = d.prefix_condition(t["x"][:, :t0])
    assert fc.duration == f and fc.batch_shape == (B,)
    x = fc.rsample((1 + h + f * (h + o),), noise=pr.unit_noise(B, f, h, o))
    g = pr.golden(case)
    want = pr.push_through({k: g["fc_z_" + k] for k in ("mean", "cov", "cross")}, pr.model(case), t0)
    err = pr.moment_errors(x, want, "x_")
    print(case, "forecast, torch route f64 against the reference", _fmt(err))
    assert max(err.values()) <= pr.TOL64, err


def test_bad_noise_shapes_raise():
    _, d, (B, T, h, o) = _build("b2_t9_h4_o3_het")
    e0, ez, ex = pr.seeded_noise("b2_t9_h4_o3_het", 3, B, T, h, o)
    assert d.rsample((3,), noise=(e0, ez, ex)).shape == (3, B, T, o)
    for bad in ((e0[:2], ez, ex), (e0, ez[:, :, 1:], ex), (e0, ez, ex[..., :2]), (e0, ez), (e0, ex, ez),
                (e0[0], ez[0], ex[0])):
        with pytest.raises(ValueError, match="expected noise"):
            d.rsample((3,), noise=bad)
    assert d.rsample(noise=(e0[0], ez[0], ex[0])).shape == (B, T, o)
    # a time-homogeneous model without a duration still cannot be drawn from
    _, nod, _ = _build("b2_t33_h8_o5", duration=False)
    with pytest.raises(ValueError, match="duration"):
        nod.rsample()


def _loop_as_it_was(d, sample_shape=torch.Size()):
    """GaussianHMM.rsample before it took ``noise``: the calls to torch.randn, their order and their shapes"""
    m0, P0, F, q, Q, H, r, R = d._parts
    shape = torch.Size(sample_shape) + d.batch_shape

    def draw(loc, cov):
        L = torch.linalg.cholesky(cov)
        eps = torch.randn(shape + loc.shape[-1:], dtype=loc.dtype, device=loc.device)
        return loc + (L @ eps.unsqueeze(-1)).squeeze(-1)

    z = draw(m0, P0)
    xs = []
    for t in range(d.duration):
        z = (z.unsqueeze(-2) @ hmm._step(F, t, 2)).squeeze(-2) + draw(hmm._step(q, t, 1), hmm._step(Q, t, 2))
        xs.append((z.unsqueeze(-2) @ hmm._step(H, t, 2)).squeeze(-2) + draw(hmm._step(r, t, 1), hmm._step(R, t, 2)))
    return torch.stack(xs, dim=-2)


@pytest.mark.parametrize("case", ["b3_t7_h3_o2_shared", "b2_t9_h4_o3_het", "b3_t6_h3_o2_indep"])
@pytest.mark.parametrize("dtype", [torch.float32, F64])
def test_cpu_draws_for_a_seed_are_unchanged(case, dtype):
    _, d, (B, T, h, o) = _build(case, dtype)
    torch.manual_seed(11)
    want = _loop_as_it_was(d, (2, 3))
    after = torch.rand(())
    torch.manual_seed(11)
    got = d.rsample((2, 3), noise=None)
    assert got.shape == (2, 3, B, T, o) and torch.equal(got, want)
    assert torch.equal(torch.rand(()), after)                    # the generator stands where it stood


def test_gradients_reach_the_parts_and_the_noise():
    case = "b2_t9_h4_o3_het"
    t, d, (B, T, h, o) = _build(case, requires_grad=True)
    noise = [e.requires_grad_(True) for e in pr.seeded_noise(case, 2, B, T, h, o)]
    x = d.rsample((2,), noise=noise)
    assert x.requires_grad
    names = [k for k in gc.NAMES if k != "x"]
    grads = torch.autograd.grad(x.square().sum(), [t[k] for k in names] + noise)
    for k, g in zip(names + ["eps0", "eps_z", "eps_x"], grads):
        assert torch.isfinite(g).all() and g.abs().max() > 0, k
    # d x / d e'_t = L_R,t: the last step's observation noise reaches the last step's x alone
    gx, = torch.autograd.grad(d.rsample((2,), noise=noise)[0, 0, -1, 0], noise[2])
    LR = np.linalg.cholesky(pr.model(case)["R"][0, -1])
    assert gc.rel_err(gx[0, 0, -1].numpy(), LR[0]) <= pr.TOL64 and not gx[0, 0, :-1].any() and not gx[1].any()
    # without noise the draws are still reparameterised in the parts
    assert d.rsample((2,)).requires_grad


def test_route_choice(monkeypatch):
    """the kernel route is taken for device tensors alone: with the device test and the wrapper patched, a CPU model
    goes to the wrapper exactly when the switch is on, the dimensions are within the limits and nothing needs a
    gradient"""
    case = "b2_t9_h4_o3_het"
    t, d, (B, T, h, o) = _build(case)
    noise = pr.seeded_noise(case, 3, B, T, h, o)
    calls = []

    def fake(*args, **kw):
        calls.append((args, kw))
        eps0 = args[-3]
        return eps0.new_zeros(eps0.shape[:2] + (T, o)), None
    monkeypatch.setattr(kernels, "gaussian_hmm_draw", fake)
    assert d.rsample((3,), noise=noise).abs().sum() > 0 and not calls            # CPU tensors: the loop
    monkeypatch.setattr(kernels, "on_device", lambda t: True)
    x = d.rsample((3,), noise=noise)
    assert len(calls) == 1 and x.shape == (3, B, T, o) and not x.any()
    args, kw = calls[0]
    assert len(args) == 12 and args[8] == T and not kw
    assert [tuple(a.shape) for a in args[9:]] == [(3, B, h), (3, B, T, h), (3, B, T, o)]
    assert torch.equal(args[9], noise[0]) and all(a.is_contiguous() for a in args[:8] + args[9:])
    # noise drawn inside: one torch.randn of the total size, split in order
    torch.manual_seed(5)
    assert d.rsample((2, 2)).shape == (2, 2, B, T, o) and len(calls) == 2
    torch.manual_seed(5)
    flat = torch.randn(4 * B * (h + T * (h + o)), dtype=F64)
    e0, ez, ex = flat.split([4 * B * h, 4 * B * T * h, 4 * B * T * o])
    got = calls[1][0][9:]
    assert torch.equal(got[0], e0.reshape(4, B, h)) and torch.equal(got[1], ez.reshape(4, B, T, h))
    assert torch.equal(got[2], ex.reshape(4, B, T, o))
    # the switch
    monkeypatch.setattr(hmm, "FUSED_GAUSSIAN_HMM", False)
    assert d.rsample((3,), noise=noise).any() and len(calls) == 2
    monkeypatch.setattr(hmm, "FUSED_GAUSSIAN_HMM", True)
    # something needs a gradient under grad mode: the loop; under no_grad: the kernel
    tg, dg, _ = _build(case, requires_grad=True)
    assert dg.rsample((3,), noise=noise).requires_grad and len(calls) == 2
    with torch.no_grad():
        assert not dg.rsample((3,), noise=noise).requires_grad and len(calls) == 3
    noisy = [e.clone().requires_grad_(True) for e in noise]
    assert d.rsample((3,), noise=noisy).requires_grad and len(calls) == 3
    # noise of another dtype than the parts, and dimensions over the limit: the loop
    with pytest.raises(RuntimeError):
        d.rsample((3,), noise=[e.float() for e in noise])
    assert len(calls) == 3
    n = kernels.GAUSSIAN_HMM_MAX_HIDDEN + 1
    eye, z = torch.eye(n, dtype=F64), torch.zeros(n, dtype=F64)
    wide = dist.GaussianHMM(dist.MultivariateNormal(z, eye), 0.5 * eye, dist.MultivariateNormal(z, eye),
                            torch.ones(n, 2, dtype=F64) / n, dist.MultivariateNormal(z[:2], eye[:2, :2]), duration=3)
    assert wide.rsample((4,)).shape == (4, 3, 2) and len(calls) == 3


def test_wrapper_and_op_are_declared():
    """the new entry point is in the ctypes table and, where the typed ops are built, among the dispatcher ops"""
    from pyro_amd import _lib
    from pyro_amd.ops import torch_library
    assert "pa_gaussian_hmm_draw" in _lib._SIGNATURES and "pa_gaussian_hmm_draw_workspace" in _lib._SIGNATURES
    assert callable(kernels.gaussian_hmm_draw)
    assert torch_library.available() and "pyro_amd::gaussian_hmm_draw" in torch_library.registered_ops()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        z = torch.zeros
        kernels.gaussian_hmm_draw(z(1, 2), z(1, 2, 2), z(1, 1, 2, 2), z(1, 1, 2), z(1, 1, 2, 2), z(1, 1, 2, 1),
                                  z(1, 1, 1), z(1, 1, 1, 1), 3, z(4, 1, 2), z(4, 1, 3, 2), z(4, 1, 3, 1))
