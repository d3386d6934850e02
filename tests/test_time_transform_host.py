"""Host side of the time transforms: the torch route of pyro_amd.ops.tensor_utils, the two transform classes, the
reparameterisers and the ``periodic_*`` helpers against the UNMODIFIED reference (tests/golden/time_transforms.npz,
made by tests/golden/make_golden_time_transforms.py), and the contract around them.  No GPU: CPU tensors take the torch
route by construction."""
import numpy as np
import pytest
import torch

import pyro_amd as pyro
import pyro_amd.distributions as dist
from pyro_amd import poutine
from pyro_amd.contrib.forecast import Forecaster, util
from pyro_amd.distributions import hmm
from pyro_amd.infer.autoguide import guides
from pyro_amd.infer.reparam import DiscreteCosineReparam, HaarReparam, UnitJacobianReparam
from pyro_amd.ops import stats, tensor_utils
from tests import forecast_cases as fc
from tests import time_transform_cases as ttc

FIXTURE_CASES = [c for c in ttc.CASES if c[0] <= max(ttc.SMALL_N) and c[1:3] == ttc.FIXTURE_SHAPE]


@pytest.fixture
def cpu_backend(oracle_backend, monkeypatch):
    """The numpy oracle for the element-wise families, which declares every tensor to be on the device: the kernels it
    does not answer are switched off."""
    monkeypatch.setattr(hmm, "FUSED_GAUSSIAN_HMM", False)
    monkeypatch.setattr(hmm, "FUSED_LINEAR_HMM", False)
    monkeypatch.setattr(stats, "FUSED_FORECAST_SCORES", False)
    monkeypatch.setattr(tensor_utils, "FUSED_TIME_TRANSFORM", False)
    torch.set_default_dtype(torch.float64)
    yield
    torch.set_default_dtype(torch.float32)


def close(got, want, rtol=1e-12):
    want = torch.as_tensor(np.array(want), dtype=got.dtype)
    got = got.detach()
    assert got.shape == want.shape, (got.shape, want.shape)
    scale = max(float(want.abs().max()), 1e-300) if want.numel() else 1.0
    err = float((got - want).abs().max()) if want.numel() else 0.0
    assert err <= rtol * scale, (err, scale)


@pytest.mark.parametrize("case", FIXTURE_CASES, ids=ttc.case_id)
def test_torch_route_against_the_reference(case):
    x = ttc.make(case)
    want = ttc.golden("ops/" + ttc.case_id(case))
    for op in ttc.OPS:
        close(ttc.along_time(getattr(tensor_utils, op), x), want[op])


@pytest.mark.parametrize("n", ttc.SMALL_N + (300,))
def test_torch_route_inverts_itself_and_differentiates(n):
    x = ttc.make((n, 2, 3, "normal")).transpose(-1, -2).contiguous().requires_grad_()
    for op in ttc.OPS:
        fwd, inv = getattr(tensor_utils, op), getattr(tensor_utils, ttc.INVERSE[op])
        y = fwd(x)
        close(inv(y), x.detach(), rtol=1e-12 * max(1, n))
        w = torch.randn_like(y)
        g, = torch.autograd.grad((w * y).sum(), x)
        close(g, inv(w), rtol=1e-12 * max(1, n))           # orthonormal: the adjoint is the inverse


def test_edges_of_the_functions():
    empty = torch.zeros(3, 0)
    for op in ttc.OPS:
        fn = getattr(tensor_utils, op)
        assert fn(empty).shape == (3, 0)
        assert torch.equal(fn(torch.zeros(2, 7)), torch.zeros(2, 7))          # all zero -> exact zeros
    one = torch.tensor([[1.5], [-2.0]])
    assert torch.equal(tensor_utils.haar_transform(one), one)
    assert torch.equal(tensor_utils.inverse_haar_transform(one), one)
    x = torch.randn(4, 6, dtype=torch.float16)
    assert tensor_utils.haar_transform(x).dtype == torch.float16
    assert [tensor_utils.next_fast_len(n) for n in (1, 7, 11, 16, 17, 121)] == [1, 8, 12, 16, 18, 125]
    assert tensor_utils.TIME_TRANSFORM_MAX_STEPS == 2048
    from pyro_amd import kernels
    assert kernels.TIME_TRANSFORM_MAX_STEPS == tensor_utils.TIME_TRANSFORM_MAX_STEPS


def test_positive_dim_and_other_dims():
    x = torch.randn(2, 9, 3, dtype=torch.float64)
    for fn in (tensor_utils.dct, tensor_utils.idct):
        assert torch.equal(fn(x, dim=1), fn(x, dim=-2))
        close(fn(x, dim=0), fn(x.transpose(0, -1)).transpose(0, -1))


@pytest.mark.parametrize("case", ttc.TRANSFORM_CASES, ids=ttc.transform_id)
def test_transform_classes_against_the_reference(case):
    x = ttc.transform_input()
    want = ttc.golden("transforms/" + ttc.transform_id(case))
    t = ttc.build_transform(dist.transforms, case)
    y = t(x)
    close(y, want["y"])
    close(t.inv(x), want["inv"])
    ladj = t.log_abs_det_jacobian(x, y)
    assert ladj.shape == want["ladj"].shape and not ladj.any()
    close(t.inv(y), x, rtol=1e-13)


def test_transform_contract():
    T = dist.transforms
    assert T.AffineTransform is torch.distributions.transforms.AffineTransform      # torch's module, re-exported
    a, b = T.DiscreteCosineTransform(dim=-2, smooth=1.0), T.DiscreteCosineTransform(dim=-2, smooth=1)
    assert a == b and hash(a) == hash(b)
    assert a != T.DiscreteCosineTransform(dim=-1, smooth=1.0) and a != T.DiscreteCosineTransform(dim=-2)
    assert a != T.HaarTransform(dim=-2)
    h, g = T.HaarTransform(dim=-3, flip=True), T.HaarTransform(dim=-3, flip=True)
    assert h == g and hash(h) == hash(g) and h != T.HaarTransform(dim=-3)
    for t in (a, h):
        assert t.bijective and t.domain.event_dim == -t.dim == t.codomain.event_dim == t.event_dim
        cached = t.with_cache()
        assert cached == t and cached._cache_size == 1 and cached.with_cache() is cached
        assert t.forward_shape((4, 5, 6)) == (4, 5, 6) == t.inverse_shape((4, 5, 6))
        with pytest.raises(ValueError):
            t.forward_shape((5,))
        assert t.log_abs_det_jacobian(torch.zeros(4, 5, 6, 7), None).shape == (4, 5, 6, 7)[:t.dim]
    with pytest.raises(AssertionError):
        T.HaarTransform(dim=0)
    # smooth weights frequency k + 1/2 by (k + 1/2) ** smooth, normalised to unit geometric mean
    x = torch.randn(3, 8, dtype=torch.float64)
    w = torch.linspace(0.5, 7.5, 8, dtype=torch.float64) ** 1.5
    w = w / w.log().mean().exp()
    close(T.DiscreteCosineTransform(smooth=1.5)(x), tensor_utils.dct(x) * w, rtol=1e-14)
    assert abs(float(w.log().sum())) < 1e-12
    # flip reverses time first
    close(T.HaarTransform(flip=True)(x), tensor_utils.haar_transform(x.flip(-1)), rtol=0)
    # registered with reshape_transform_batch
    assert util.reshape_transform_batch(h, (2, 3), (2, 1, 3)) is h


@pytest.mark.parametrize("noise", ttc.DRIFT_NOISES)
@pytest.mark.parametrize("which", ttc.REPARAMS)
@pytest.mark.parametrize("config", fc.CONFIGS, ids=[c[0] for c in fc.CONFIGS])
def test_reparameterised_traces_against_the_reference(noise, which, config, cpu_backend):
    name, particles, nesting = config
    want = ttc.golden(ttc.trace_key(noise, which, name))
    t = fc.tensors(fc.golden("inputs"))
    tr = ttc.run_reparam_trace(ttc.namespace(), noise, which, t, particles, nesting, ttc.drift_coefficients())
    sites = fc.sample_sites(tr)
    assert sites == list(want["sites"])
    for s in sites:
        close(tr.nodes[s]["log_prob"].detach(), want["log_prob_" + s])
    close(tr.nodes["drift"]["value"], want["value_drift"])
    assert tr.nodes["drift"]["is_observed"] and not tr.nodes["drift"]["log_prob"].any()


def test_unit_jacobian_reparam_refuses_a_batch_dim_without_the_flag(cpu_backend):
    def model():
        with pyro.plate("time", 6, dim=-1):
            return pyro.sample("x", dist.Normal(torch.zeros(6), 1.0))

    for rep in (HaarReparam(dim=-1), DiscreteCosineReparam(dim=-1),
                UnitJacobianReparam(dist.transforms.HaarTransform(dim=-1))):
        with pytest.raises(ValueError, match="batch dimension"):
            poutine.reparam(model, config={"x": rep})()
    tr = poutine.trace(poutine.reparam(model, config={"x": HaarReparam(dim=-1, experimental_allow_batch=True)})
                       ).get_trace()
    assert tr.nodes["x_haar"]["value"].shape == (1, 6) and tr.nodes["x"]["value"].shape == (6,)
    close(tensor_utils.haar_transform(tr.nodes["x"]["value"]), tr.nodes["x_haar"]["value"][0], rtol=1e-6)
    # an event dim needs no flag; the suffix of the general class
    def event_model():
        return pyro.sample("x", dist.Normal(torch.zeros(6), 1.0).to_event(1))
    rep = UnitJacobianReparam(dist.transforms.DiscreteCosineTransform(dim=-1))
    tr = poutine.trace(poutine.reparam(event_model, config={"x": rep})).get_trace()
    assert "x_transformed" in tr.nodes


def test_time_reparam_configs_pick_their_own_class(cpu_backend):
    seen = {}

    def model():
        pyro.sample("scale", dist.LogNormal(torch.zeros(()), 1.0))
        with pyro.plate("time", 5, dim=-1):
            pyro.sample("drift", dist.Normal(torch.zeros(5, 2), 1.0).to_event(1))
            pyro.sample("obs", dist.Normal(torch.zeros(5), 1.0), obs=torch.zeros(5))

    for config, cls in ((util.time_reparam_dct, DiscreteCosineReparam), (util.time_reparam_haar, HaarReparam)):
        def spy(msg, config=config):
            seen[msg["name"]] = config(msg)
            return None
        poutine.reparam(model, config=spy)()
        assert seen["scale"] is None and seen["obs"] is None
        assert type(seen["drift"]) is cls and seen["drift"].transform.dim == -2
        assert seen["drift"].experimental_allow_batch
    assert "slip" in util.time_reparam_dct.__doc__ and "slip" in util.time_reparam_haar.__doc__


def test_periodic_helpers_against_the_reference():
    want, inputs = ttc.golden("periodic"), ttc.periodic_inputs()
    for k, args in enumerate(inputs["repeat"]):
        close(tensor_utils.periodic_repeat(*args), want["repeat_%d" % k], rtol=0)
    for k, args in enumerate(inputs["cumsum"]):
        close(tensor_utils.periodic_cumsum(*args), want["cumsum_%d" % k])
    for k, args in enumerate(inputs["features"]):
        close(tensor_utils.periodic_features(*args, dtype=torch.float64), want["features_%d" % k])
    assert guides.periodic_repeat is tensor_utils.periodic_repeat


def test_forecaster_trains_a_model_reparameterised_by_hand(cpu_backend):
    """Forecaster's own options stay refused; the route to SVI with a time reparameteriser is poutine.reparam around
    the model's ``model`` method."""
    pyro.clear_param_store()
    pyro.set_rng_seed(5)
    t = fc.tensors(fc.golden("inputs"))
    with pytest.raises(NotImplementedError):
        Forecaster(ttc.make_drift_model(ttc.namespace(), "normal0", t), t["data"], t["covariates"][:fc.T_OBS],
                   time_reparam="haar", num_steps=0)
    model = ttc.make_drift_model(ttc.namespace(), "normal0", t)
    model.model = poutine.reparam(model.model, config=util.time_reparam_haar)
    forecaster = Forecaster(model, t["data"], t["covariates"][:fc.T_OBS], num_steps=5, log_every=0)
    assert len(forecaster.losses) == 5 and all(np.isfinite(forecaster.losses))
    with poutine.block(), poutine.trace() as seen:
        forecaster.guide(t["data"], t["covariates"][:fc.T_OBS])
    guide_sites = [name for name, site in seen.trace.nodes.items() if site["type"] == "sample"]
    assert "drift_haar" in guide_sites and "drift" not in guide_sites
    assert any(name.endswith("drift_haar") for name in pyro.get_param_store().keys())
    out = forecaster(t["data"], t["covariates"], num_samples=3)
    assert out.shape == (3, fc.T_AHEAD, fc.OBS) and torch.isfinite(out).all()
