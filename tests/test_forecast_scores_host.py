"""stats.crps_empirical and stats.forecast_scores on the CPU, which is the torch route: against the O(S^2) definition
E|p - y| - E|p - p'| / 2, against the reference's results in tests/golden/forecast.npz, the shape rule, and the wiring
of the kernel (which needs no device to be looked at).

The O(S^2) check runs in float64.  Both sides carry the rounding of an S-term sum of terms up to A (the definition's
S^2-term mean is summed pairwise by torch), so they agree within twice fsc.bound64 = 2 S 2^-52 (1 + A)."""
import pytest
import torch

from pyro_amd import _lib, kernels
from pyro_amd.ops import stats, torch_library
from tests import forecast_scores_cases as fsc

FINITE = tuple(k for k in fsc.KINDS if k not in ("nan_sample", "nan_truth", "inf_sample"))


def _definition(pred, truth):
    return (pred - truth).abs().mean(0) - (pred - pred.unsqueeze(1)).abs().mean([0, 1]) / 2


@pytest.mark.parametrize("kind", FINITE)
@pytest.mark.parametrize("S", tuple(s for s in fsc.SAMPLES if s <= 129))
def test_torch_route_is_the_definition(S, kind):
    for M in (1, 17, 33):
        pred, truth = fsc.make(kind, S, M)
        got = stats.crps_empirical(pred, truth)
        assert got.shape == truth.shape and got.dtype == torch.float64
        flat = pred.reshape(S, M)
        err = fsc.max_err(got, _definition(flat, truth))
        assert err <= 2 * fsc.bound64(S, fsc.magnitude(pred, truth)), (M, err)
        mean, median, crps = stats.forecast_scores(pred, truth)
        assert torch.equal(crps, got) and torch.equal(mean, flat.mean(0)) and torch.equal(median, flat.median(0).values)


def test_large_sample_counts_against_the_definition():
    for S in (1000, 1024, fsc.OVER):
        pred, truth = fsc.make("random", S, 1)
        err = fsc.max_err(stats.crps_empirical(pred, truth), _definition(pred, truth))
        assert err <= 2 * fsc.bound64(S, fsc.magnitude(pred, truth))


@pytest.mark.parametrize("kind,S,M", fsc.GOLDEN, ids=lambda v: str(v))
def test_fixture(kind, S, M):
    g = fsc.golden("scores/%s_%d_%d" % (kind, S, M))
    pred, truth = fsc.make(kind, S, M)
    assert torch.equal(pred, torch.tensor(g["pred"])) and torch.equal(truth, torch.tensor(g["truth"]))
    mean, median, crps = stats.forecast_scores(pred, truth)
    bound = fsc.bound64(S, fsc.magnitude(pred, truth))
    assert torch.equal(median, torch.tensor(g["median"]))
    assert fsc.max_err(mean, torch.tensor(g["mean"])) <= bound
    assert fsc.max_err(crps, torch.tensor(g["crps"])) <= bound


def test_nonfinite_follow_the_formula():
    for kind in ("nan_sample", "nan_truth", "inf_sample"):
        pred, truth = fsc.make(kind, 65, 17)
        crps = stats.crps_empirical(pred, truth)
        j = fsc.bad_column(17)
        assert not bool(torch.isfinite(crps[j])) and bool(torch.isfinite(crps[torch.arange(17) != j]).all())
    pred, truth = fsc.make("inf_sample", 1, 17)
    assert float(stats.crps_empirical(pred, truth)[fsc.bad_column(17)]) == float("inf")


def test_shapes():
    pred, truth = torch.randn(5, 1, 1, 2, 3), torch.randn(2, 3)
    assert stats.crps_empirical(pred, truth).shape == (2, 3)
    assert all(t.shape == (2, 3) for t in stats.forecast_scores(pred, truth))
    assert stats.crps_empirical(torch.randn(5), torch.tensor(0.3)).shape == ()
    for bad_pred, bad_truth in ((torch.randn(5, 3), torch.randn(4)), (torch.randn(5, 2, 3), torch.randn(3)),
                                (torch.randn(3), torch.randn(3)), (torch.randn(5, 1, 3), torch.randn(1, 1, 3))):
        with pytest.raises(ValueError, match="one extra sample dim"):
            stats.crps_empirical(bad_pred, bad_truth)
        with pytest.raises(ValueError, match="one extra sample dim"):
            stats.forecast_scores(bad_pred, bad_truth)


def test_torch_route_is_differentiable():
    pred, truth = fsc.make("random", 7, 3)
    pred = pred.requires_grad_()
    stats.crps_empirical(pred, truth).sum().backward()
    assert pred.grad.shape == pred.shape and bool(torch.isfinite(pred.grad).all())


def test_wiring():
    assert "pa_forecast_scores" in _lib._SIGNATURES and callable(kernels.forecast_scores)
    assert torch_library.available() and "pyro_amd::forecast_scores" in torch_library.registered_ops()
    assert kernels.FORECAST_SCORES_MAX_SAMPLES == 1024
    assert tuple(c for _, c in kernels.FORECAST_SCORES_STRIPS) == fsc.STRIPS
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        kernels.forecast_scores(torch.zeros(3, 2), torch.zeros(2))
