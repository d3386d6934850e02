"""The one-pass forecast-score kernel (csrc/forecast_scores.hip) on the device: kernels.forecast_scores, the
dispatcher op, stats.crps_empirical and stats.forecast_scores over every case of tests/forecast_scores_cases.py.

Every S of fsc.SAMPLES with every input kind, each at every M of fsc.COLUMNS (1, C - 1, C, C + 1, 3 C + 5 for both strip
widths the kernel instantiates).  The bounds are fsc's: the median bit-equal to torch's; float64 mean and crps within
S * 2^-52 * (1 + A) of the float64 torch formula (run on the CPU) and of the reference's results in the fixture;
float32 within four times the error of the float32 torch formula on the CPU, both against float64, with floor
4 * 2^-23 * (1 + A).  A NaN sample or a NaN truth makes its column NaN in all three outputs and leaves the others as
they are without it.  S = 1025 takes the torch route, as a spy shows."""
import pytest
import torch

from pyro_amd import kernels
from pyro_amd.ops import stats
from tests import forecast_scores_cases as fsc

pytestmark = pytest.mark.gpu
F64, F32 = torch.float64, torch.float32


@pytest.fixture(autouse=True, scope="module")
def _typed_ops():
    from pyro_amd.ops import torch_library
    assert torch_library.available()


def _spy(monkeypatch):
    calls = []
    real = kernels.forecast_scores

    def spy(*a, **kw):
        calls.append((a, kw))
        return real(*a, **kw)
    monkeypatch.setattr(kernels, "forecast_scores", spy)
    return calls


def _check(got, pred, truth, dtype, S):
    """``got``: (mean, median, crps) of the device for the float64 CPU case (pred [S, M], truth [M]) run in ``dtype``."""
    A = fsc.magnitude(pred, truth)
    want = fsc.torch_formula(pred, truth)                              # float64
    same = fsc.torch_formula(pred.to(dtype), truth.to(dtype))         # the same dtype, on the CPU
    for name, g, w, s in zip(("mean", "median", "crps"), got, want, same):
        assert g.dtype == dtype and g.shape == truth.shape, name
        assert fsc.same_nonfinite(g, s), name
        if name == "median":
            assert torch.equal(g.cpu().nan_to_num(nan=0.5), s.nan_to_num(nan=0.5)), name
            continue
        err = fsc.max_err(g, w)
        if dtype == F64:
            bound = fsc.bound64(S, A)
        else:
            bound = max(4 * fsc.max_err(s, w), fsc.floor32(A))
        print("%s S=%d M=%d %s: err %.3e bound %.3e" % (name, S, truth.numel(), dtype, err, bound))
        assert err <= bound, (name, err, bound)


@pytest.mark.parametrize("dtype", (F64, F32), ids=("f64", "f32"))
@pytest.mark.parametrize("kind", fsc.KINDS)
@pytest.mark.parametrize("S", fsc.SAMPLES)
def test_cases(S, kind, dtype, gpu, monkeypatch):
    calls = _spy(monkeypatch)
    for M in fsc.COLUMNS:
        pred, truth = fsc.make(kind, S, M)
        p, y = pred.to(dtype).to(gpu), truth.to(dtype).to(gpu)
        if kind == "transposed" and min(S, M) > 1:
            assert not p.is_contiguous()                              # (still a view when it reaches the route)
        n = len(calls)
        got = stats.forecast_scores(p, y)
        assert len(calls) == n + 1                                    # ONE launch for the three
        crps = stats.crps_empirical(p, y)
        assert len(calls) == n + 2 and torch.equal(crps.nan_to_num(nan=0.5), got[2].nan_to_num(nan=0.5))
        flat = pred.reshape(S, M)
        _check(got, flat, truth, dtype, S)
        if kind in ("nan_sample", "nan_truth"):
            j = fsc.bad_column(M)
            assert all(bool(torch.isnan(g[j])) for g in got)
            # the neighbours are what they are without the NaN
            clean_p, clean_y = flat.clone(), truth.clone()
            clean_p[:, j], clean_y[j] = 0.0, 0.0
            clean = kernels.forecast_scores(clean_p.to(dtype).to(gpu).contiguous(), clean_y.to(dtype).to(gpu))
            keep = torch.arange(M) != j
            for g, c in zip(got, clean):
                assert torch.equal(g.cpu()[keep], c.cpu()[keep])


@pytest.mark.parametrize("dtype", (F64, F32), ids=("f64", "f32"))
def test_dispatcher_op_and_raw_kernel_agree(dtype, gpu):
    for S, M in ((3, 17), (129, 33)):
        pred, truth = fsc.make("random", S, M)
        p, y = pred.to(dtype).to(gpu), truth.to(dtype).to(gpu)
        a, b = kernels.forecast_scores(p, y), torch.ops.pyro_amd.forecast_scores(p, y)
        assert all(torch.equal(u, v) for u, v in zip(a, b))
        again = kernels.forecast_scores(p, y)
        assert all(torch.equal(u, v) for u, v in zip(a, again))      # no atomics: bit-reproducible


@pytest.mark.parametrize("kind,S,M", fsc.GOLDEN, ids=lambda v: str(v))
def test_fixture_float64(kind, S, M, gpu):
    """the reference's crps_empirical, median(0).values and mean(0)"""
    g = fsc.golden("scores/%s_%d_%d" % (kind, S, M))
    pred, truth = fsc.make(kind, S, M)
    assert torch.equal(pred, torch.tensor(g["pred"])) and torch.equal(truth, torch.tensor(g["truth"]))
    got = stats.forecast_scores(pred.to(gpu), truth.to(gpu))
    bound = fsc.bound64(S, fsc.magnitude(pred, truth))
    assert torch.equal(got[1].cpu(), torch.tensor(g["median"]))
    assert fsc.max_err(got[0], torch.tensor(g["mean"])) <= bound
    assert fsc.max_err(got[2], torch.tensor(g["crps"])) <= bound


def test_routing(gpu, monkeypatch):
    calls = _spy(monkeypatch)
    pred, truth = fsc.make("random", fsc.OVER, 17)
    p, y = pred.to(gpu), truth.to(gpu)
    got = stats.forecast_scores(p, y)
    assert not calls                                                   # S = 1025: the torch formula
    want = fsc.torch_formula(pred, truth)
    bound = fsc.bound64(fsc.OVER, fsc.magnitude(pred, truth))
    assert torch.equal(got[1].cpu(), want[1])
    assert fsc.max_err(got[0], want[0]) <= bound and fsc.max_err(got[2], want[2]) <= bound
    with pytest.raises(kernels.Unsupported):
        kernels.forecast_scores(p, y)
    calls.clear()

    pred, truth = fsc.make("random", 64, 17)
    p, y = pred.to(gpu), truth.to(gpu)
    stats.crps_empirical(p, y)
    assert len(calls) == 1
    monkeypatch.setattr(stats, "FUSED_FORECAST_SCORES", False)
    stats.crps_empirical(p, y)
    assert len(calls) == 1
    monkeypatch.setattr(stats, "FUSED_FORECAST_SCORES", True)
    stats.crps_empirical(p.half(), y.half())                          # another dtype
    stats.crps_empirical(pred, truth)                                 # CPU tensors
    assert len(calls) == 1
    q = p.clone().requires_grad_()
    crps = stats.crps_empirical(q, y)                                 # a gradient asked for: differentiable
    assert len(calls) == 1
    crps.sum().backward()
    assert q.grad is not None and bool(torch.isfinite(q.grad).all())
    with torch.no_grad():
        stats.crps_empirical(q, y)
    assert len(calls) == 2
    assert stats.crps_empirical(p[:, :0], y[:0]).shape == (0,)        # no columns: no launch, no error
