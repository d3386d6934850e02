"""The time-transform kernels (csrc/time_transform.hip) on the device: kernels.time_transform, the typed op
pyro_amd::time_transform, pyro_amd.ops.tensor_utils and what sits on them (the transform classes, the
reparameterisers, HMCForecaster), over the cases of tests/time_transform_cases.py.

Bounds (derived in that module, u the unit roundoff of the dtype, A = max |x|): DCT / IDCT (N + 2) u sqrt(2 N) A, Haar
4 max(1, ceil(log2 N)) u sqrt(N) A, against the reference's float64 results (the fixture, N <= 129) and against the
float64 torch route on the CPU (every case); twice that for a round trip."""
import warnings

import numpy as np
import pytest
import torch

import pyro_amd as pyro
import pyro_amd.distributions as dist
from pyro_amd import kernels, poutine
from pyro_amd.contrib.forecast import HMCForecaster, util
from pyro_amd.ops import tensor_utils
from tests import forecast_cases as fc
from tests import time_transform_cases as ttc

pytestmark = pytest.mark.gpu
F64, F32 = torch.float64, torch.float32
DTYPES = pytest.mark.parametrize("dtype", (F64, F32), ids=("f64", "f32"))
OP_CODE = {"dct": 0, "idct": 1, "haar_transform": 2, "inverse_haar_transform": 3}
MAX = tensor_utils.TIME_TRANSFORM_MAX_STEPS


@pytest.fixture(autouse=True, scope="module")
def _typed_ops():
    from pyro_amd.ops import torch_library
    assert torch_library.available()


def _spy(monkeypatch):
    calls = []
    real = kernels.time_transform

    def spy(x, op, dim=-1):
        calls.append((tuple(x.shape), op, dim))
        return real(x, op, dim)
    monkeypatch.setattr(kernels, "time_transform", spy)
    return calls


def _apply(op, x, dim=-2):
    return getattr(tensor_utils, op)(x, dim=dim)


def _cpu64(op, x):
    """The float64 torch route on the CPU along dim -2 (``x``: a CPU tensor, already rounded to the dtype under test)."""
    return _apply(op, x.to(F64))


def _err(got, want):
    return float((got.detach().cpu().to(F64) - want).abs().max())


@DTYPES
@pytest.mark.parametrize("case", ttc.CASES, ids=ttc.case_id)
def test_cases(case, dtype, gpu, monkeypatch):
    calls = _spy(monkeypatch)
    n = case[0]
    x = ttc.make(case).to(dtype)
    xd = x.to(gpu)
    amax = float(x.abs().max())
    in_fixture = dtype == F64 and n <= max(ttc.SMALL_N) and case[1:3] == ttc.FIXTURE_SHAPE
    want_ref = ttc.golden("ops/" + ttc.case_id(case)) if in_fixture else {}
    for op in ttc.OPS:
        before = len(calls)
        got = _apply(op, xd)
        assert len(calls) == before + 1 and calls[-1] == (tuple(x.shape), OP_CODE[op], -2)     # ONE launch, no transpose
        assert got.dtype == dtype and got.shape == x.shape and got.is_contiguous()
        bound = ttc.bound(op, n, dtype, amax)
        err = _err(got, _cpu64(op, x))
        print("%s %s %s: err %.3e bound %.3e" % (ttc.case_id(case), op, dtype, err, bound))
        assert err <= bound, (op, err, bound)
        if in_fixture:
            err = _err(got, torch.tensor(np.array(want_ref[op])))
            assert err <= bound, ("fixture", op, err, bound)
        # there and back again
        back = _apply(ttc.INVERSE[op], got)
        assert _err(back, x.to(F64)) <= 2 * bound, (op, "round trip")
        # all zero -> exact zeros (no -0 + rounding artefacts)
        zeros = _apply(op, torch.zeros_like(xd))
        assert not zeros.any()


@DTYPES
def test_raw_kernel_typed_op_and_functions_agree_bit_for_bit(dtype, gpu):
    for case in ((7, 2, 3, "normal"), (64, 3, 5, "walk"), (129, 1, 17, "offset"), (1000, 2, 4, "normal")):
        xd = ttc.make(case).to(dtype).to(gpu)
        for op in ttc.OPS:
            a = kernels.time_transform(xd, OP_CODE[op], -2)
            b = torch.ops.pyro_amd.time_transform(xd, OP_CODE[op], -2)
            c = _apply(op, xd)
            again = kernels.time_transform(xd, OP_CODE[op], 1)
            assert torch.equal(a, b) and torch.equal(a, c) and torch.equal(a, again), (case, op)
    # the last dim: inner = 1
    x = ttc.make((33, 3, 1, "normal")).to(dtype).to(gpu).squeeze(-1)
    assert torch.equal(tensor_utils.dct(x), tensor_utils.dct(x.unsqueeze(-1), dim=-2).squeeze(-1))
    assert torch.equal(tensor_utils.haar_transform(x), kernels.time_transform(x, "haar"))
    assert torch.ops.pyro_amd.time_transform(torch.empty((3, 0), device="meta"), 0, -1).shape == (3, 0)


@DTYPES
@pytest.mark.parametrize("n", (5, 8, 65, 1000))
def test_backward_is_the_inverse_kernel(n, dtype, gpu, monkeypatch):
    calls = _spy(monkeypatch)
    x = ttc.make((n, 2, 3, "normal")).to(dtype)
    w = ttc.make((n, 2, 3, "walk")).to(dtype)
    wd = w.to(gpu)
    for op in ttc.OPS:
        xd = x.to(gpu).requires_grad_()
        before = len(calls)
        y = _apply(op, xd)
        assert len(calls) == before + 1
        (wd * y).sum().backward()
        assert len(calls) == before + 2 and calls[-1][1] == OP_CODE[ttc.INVERSE[op]]     # one more launch, the inverse
        bound = ttc.bound(op, n, dtype, float(w.abs().max()))
        assert _err(xd.grad, _cpu64(ttc.INVERSE[op], w)) <= bound, op
    if dtype == F64 and n <= 8:
        for op in ttc.OPS:
            xd = x.to(gpu).requires_grad_()
            assert torch.autograd.gradcheck(lambda t: _apply(op, t), (xd,))
            assert torch.autograd.gradcheck(lambda t: _apply(op, t, dim=0), (xd,))


def test_routing(gpu, monkeypatch):
    calls = _spy(monkeypatch)
    x = ttc.make((MAX + 1, 1, 3, "normal"))
    xd = x.to(gpu)
    for op in ttc.OPS:
        got = _apply(op, xd)                                          # over the limit: the torch route, on the device
        assert not calls
        assert _err(got, _cpu64(op, x)) <= ttc.bound(op, MAX + 1, F64, float(x.abs().max()))
    monkeypatch.undo()
    for op in ttc.OPS:
        with pytest.raises(kernels.Unsupported):
            kernels.time_transform(xd, OP_CODE[op], -2)
    calls = _spy(monkeypatch)
    x = ttc.make((64, 2, 3, "normal"))
    xd = x.to(gpu)
    want = _apply("dct", xd)
    assert len(calls) == 1
    monkeypatch.setattr(tensor_utils, "FUSED_TIME_TRANSFORM", False)
    off = _apply("dct", xd)
    assert len(calls) == 1 and _err(off, want.cpu()) <= 2 * ttc.bound("dct", 64, F64, float(x.abs().max()))
    monkeypatch.setattr(tensor_utils, "FUSED_TIME_TRANSFORM", True)
    _apply("haar_transform", xd.half())                               # another dtype
    _apply("idct", x)                                                 # CPU tensors
    assert _apply("dct", xd[:, :, :0]).shape == (2, 64, 0)            # empty: no launch, no error
    assert _apply("haar_transform", xd[:, :0]).shape == (2, 0, 3)
    assert len(calls) == 1
    # the measured crossover: f64, over 1024 steps, more than 128 series -> the torch route's FFT (the DCT only)
    long = torch.randn(43, 1025, 3, dtype=F64, device=gpu)
    _apply("idct", long)
    assert len(calls) == 1
    _apply("idct", long[:42])
    _apply("idct", long.float())
    _apply("inverse_haar_transform", long)
    assert len(calls) == 4
    del calls[1:]
    # a double backward takes the torch route when asked for one: create_graph through the kernel route is refused
    q = xd.clone().requires_grad_()
    g, = torch.autograd.grad(_apply("dct", q).sum(), q, create_graph=True)
    with pytest.raises(RuntimeError):
        g.sum().backward()
    monkeypatch.setattr(tensor_utils, "FUSED_TIME_TRANSFORM", False)
    q = xd.clone().requires_grad_()
    g, = torch.autograd.grad((_apply("dct", q) ** 2).sum(), q, create_graph=True)
    g.sum().backward()
    assert q.grad is not None


@DTYPES
def test_other_dims_and_views(dtype, gpu, monkeypatch):
    calls = _spy(monkeypatch)
    base = ttc.make((33, 5, 12, "normal")).to(dtype)                   # [5, 33, 12]
    views = {-2: base.to(gpu)[:, :, ::3],                              # [5, 33, 4], strided
             -3: base.to(gpu).transpose(0, 1)[:, 1:4, :5],             # [33, 3, 5], transposed and cut
             -1: base.to(gpu).transpose(1, 2)[::2]}                    # [3, 12, 33]
    host = {-2: base[:, :, ::3], -3: base.transpose(0, 1)[:, 1:4, :5], -1: base.transpose(1, 2)[::2]}
    amax = float(base.abs().max())
    for dim, v in views.items():
        assert not v.is_contiguous()
        for op in ttc.OPS:
            before = len(calls)
            got = _apply(op, v, dim=dim)
            assert len(calls) == before + 1 and calls[-1][2] == dim
            want = _apply(op, host[dim].to(F64), dim=dim)
            assert got.shape == want.shape and _err(got, want) <= ttc.bound(op, 33, dtype, amax), (dim, op)


@DTYPES
def test_a_nan_stays_in_its_column(dtype, gpu):
    for case in ((31, 2, 5, "normal"), (1000, 1, 5, "normal"), (2048, 1, 3, "normal")):
        x = ttc.make(case).to(dtype).to(gpu)
        bad = x.clone()
        bad[-1, case[0] // 2, 1] = float("nan")
        keep = torch.ones(x.shape[0], x.shape[2], dtype=torch.bool, device=gpu)
        keep[-1, 1] = False
        for op in ttc.OPS:
            clean, got = _apply(op, x), _apply(op, bad)
            assert torch.equal(got.transpose(1, 2)[keep], clean.transpose(1, 2)[keep]), (case, op)
            assert torch.isnan(got[-1, :, 1]).any()
            if op in ("dct", "idct"):
                assert torch.isnan(got[-1, :, 1]).all()


def test_transform_classes_on_the_device(gpu, monkeypatch):
    calls = _spy(monkeypatch)
    x = ttc.transform_input()
    for case in ttc.TRANSFORM_CASES:
        want = ttc.golden("transforms/" + ttc.transform_id(case))
        t = ttc.build_transform(dist.transforms, case)
        before = len(calls)
        y = t(x.to(gpu))
        assert len(calls) == before + 1 and calls[-1][2] == case[2]
        assert _err(y, torch.tensor(np.array(want["y"]))) <= 1e-12 * float(np.abs(want["y"]).max())
        assert _err(t.inv(x.to(gpu)), torch.tensor(np.array(want["inv"]))) <= 1e-12 * float(np.abs(want["inv"]).max())
        assert t.log_abs_det_jacobian(x.to(gpu), y).shape == want["ladj"].shape


@pytest.mark.parametrize("noise", ttc.DRIFT_NOISES)
@pytest.mark.parametrize("which", ttc.REPARAMS)
@pytest.mark.parametrize("config", fc.CONFIGS, ids=[c[0] for c in fc.CONFIGS])
def test_reparameterised_traces_on_the_device(noise, which, config, gpu, monkeypatch):
    calls = _spy(monkeypatch)
    name, particles, nesting = config
    want = ttc.golden(ttc.trace_key(noise, which, name))
    torch.set_default_dtype(F64)
    try:
        t = fc.tensors(fc.golden("inputs"), device=gpu)
        tr = ttc.run_reparam_trace(ttc.namespace(), noise, which, t, particles, nesting,
                                   ttc.drift_coefficients(device=gpu))
    finally:
        torch.set_default_dtype(F32)
    assert calls and all(c[2] == -2 for c in calls)
    sites = fc.sample_sites(tr)
    assert sites == [str(s) for s in want["sites"]]
    for s in sites + ["value_drift"]:
        got = tr.nodes["drift"]["value"] if s == "value_drift" else tr.nodes[s]["log_prob"]
        ref = torch.tensor(np.array(want[s if s == "value_drift" else "log_prob_" + s]))
        assert got.shape == ref.shape, s
        assert _err(got, ref) <= 1e-12 * max(float(ref.abs().max()), 1e-300), s


def test_one_captured_svi_step_under_time_reparam_dct(gpu, monkeypatch):
    """A Normal-noise model (no GaussianHMM launch) whose ``model`` method is wrapped in
    poutine.reparam(config=time_reparam_dct), stepped by an SVI with the default hip_graph setting: the step is captured
    after its eager warm-up and its loss is the eager step's."""
    from pyro_amd.infer import SVI, Trace_ELBO
    from pyro_amd.infer.autoguide import AutoNormal
    from pyro_amd.infer.svi import CapturedStepWarning
    calls = _spy(monkeypatch)
    torch.set_default_dtype(F64)
    try:
        t = fc.tensors(fc.golden("inputs"), device=gpu)
        data, cov = t["data"], t["covariates"][:fc.T_OBS]

        def run(**options):
            pyro.clear_param_store()
            pyro.set_rng_seed(11)
            model = ttc.make_drift_model(ttc.namespace(), "normal0", t)
            model.model = poutine.reparam(model.model, config=util.time_reparam_dct)
            svi = SVI(model, AutoNormal(model, init_scale=0.1), pyro.optim.Adam({"lr": 0.01}),
                      Trace_ELBO(max_plate_nesting=1), **options)
            return svi, [svi.step(data, cov) for _ in range(8)]

        with warnings.catch_warnings():
            warnings.simplefilter("ignore", CapturedStepWarning)
            captured, losses = run()
        assert captured.hip_graph and len(captured._graphs) == 1, "the step was not captured"
        n_captured = len(calls)
        eager, want = run(hip_graph=False)
        assert not eager._graphs and len(calls) - n_captured > n_captured        # replays make no Python-side call
        assert any("drift_dct" in name for name in pyro.get_param_store().keys())
        for got, ref in zip(losses, want):
            assert abs(got - ref) <= 1e-12 * abs(ref), (losses, want)
    finally:
        torch.set_default_dtype(F32)
        pyro.clear_param_store()


# ---- HMCForecaster ---------------------------------------------------------------------------------------------------
_RUNS = {}


def _hmc_run(time_reparam, gpu):
    if time_reparam not in _RUNS:
        pyro.clear_param_store()
        pyro.set_rng_seed(20261020)
        data, cov = ttc.hmc_data(device=gpu)
        _RUNS[time_reparam] = HMCForecaster(ttc.make_hmc_model(), data, cov[:ttc.HMC_T], num_warmup=100,
                                            num_samples=200, max_tree_depth=5, time_reparam=time_reparam)
    return _RUNS[time_reparam]


@pytest.mark.parametrize("time_reparam", (None, "dct", "haar"))
def test_hmc_forecaster_recovers_the_exact_posterior(time_reparam, gpu):
    forecaster = _hmc_run(time_reparam, gpu)
    data, cov = ttc.hmc_data(device=gpu)
    draws = forecaster.samples["drift"]
    assert set(forecaster.samples) == {"drift"} and draws.shape == (200, ttc.HMC_T, 1)
    mean, sd = draws.mean(0).squeeze(-1).cpu(), draws.std(0).squeeze(-1).cpu()
    exact = (data.squeeze(-1) / 1.25).cpu()
    print(time_reparam, "mean error %.3f" % float((mean - exact).abs().max()),
          "sd ratio %.3f .. %.3f" % (float(sd.min() / ttc.HMC_POSTERIOR_SD), float(sd.max() / ttc.HMC_POSTERIOR_SD)))
    assert float((mean - exact).abs().max()) <= 0.3
    assert float(sd.max()) <= 1.5 * ttc.HMC_POSTERIOR_SD and float(sd.min()) >= ttc.HMC_POSTERIOR_SD / 1.5
    out = forecaster(data, cov, 7)
    assert out.shape == (7, ttc.HMC_AHEAD, 1) and torch.isfinite(out).all()
    out = forecaster(data, cov, 7, batch_size=3)
    assert out.shape == (7, ttc.HMC_AHEAD, 1) and torch.isfinite(out).all()


def test_hmc_forecaster_refuses_an_unknown_time_reparam(gpu):
    data, cov = ttc.hmc_data(device=gpu)
    with pytest.raises(ValueError, match="time_reparam"):
        HMCForecaster(ttc.make_hmc_model(), data, cov[:ttc.HMC_T], num_warmup=1, num_samples=1, time_reparam="fft")


def test_hmc_forecaster_with_a_gaussian_hmm_noise_model(gpu):
    pyro.clear_param_store()
    pyro.set_rng_seed(3)
    data, cov = ttc.hmc_data(device=gpu)
    forecaster = HMCForecaster(ttc.make_hmc_model("hmm"), data, cov[:ttc.HMC_T], num_warmup=20, num_samples=20,
                               max_tree_depth=4, time_reparam="dct")                  # eager: no jit_compile
    assert torch.isfinite(forecaster.samples["drift"]).all()
    out = forecaster(data, cov, 5)
    assert out.shape == (5, ttc.HMC_AHEAD, 1) and torch.isfinite(out).all()
