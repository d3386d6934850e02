"""Scores of sample forecasts and the moving-window backtest (reference: pyro/contrib/forecast/evaluate.py).

eval_mae (the sample median as point estimate), eval_rmse (the sample mean) and eval_crps each reduce
``stats.forecast_scores``: for device samples that is ONE launch reading ``pred`` once where the reference sorts,
selects and averages in three passes.  ``backtest`` with the default metrics makes that one call per window and
shares it among the three numbers.
"""
import logging
import warnings
from timeit import default_timer

import torch

from ... import primitives
from ...ops import stats
from .forecaster import Forecaster

logger = logging.getLogger(__name__)


def _fits(pred, truth):
    """crps_empirical's shape rule; the point estimates of other shapes broadcast against the truth as they may."""
    return pred.dim() >= 1 and pred.shape[1:] == (1,) * (pred.dim() - truth.dim() - 1) + truth.shape


def _mae(median, truth):
    return (median - truth).abs().mean().cpu().item()


def _rmse(mean, truth):
    error = mean - truth
    return (error * error).mean().cpu().item() ** 0.5


@torch.no_grad()
def eval_mae(pred, truth):
    """Mean absolute error of the sample median -> float."""
    return _mae(stats.forecast_scores(pred, truth)[1] if _fits(pred, truth) else pred.median(0).values, truth)


@torch.no_grad()
def eval_rmse(pred, truth):
    """Root mean squared error of the sample mean -> float."""
    return _rmse(stats.forecast_scores(pred, truth)[0] if _fits(pred, truth) else pred.mean(0), truth)


@torch.no_grad()
def eval_crps(pred, truth):
    """Continuous ranked probability score averaged over all data elements -> float."""
    return stats.crps_empirical(pred, truth).mean().cpu().item()


DEFAULT_METRICS = {"mae": eval_mae, "rmse": eval_rmse, "crps": eval_crps}
_SHARED = {eval_mae: lambda s, truth: _mae(s[1], truth), eval_rmse: lambda s, truth: _rmse(s[0], truth),
           eval_crps: lambda s, truth: s[2].mean().cpu().item()}


@torch.no_grad()
def _evaluate(metrics, pred, truth):
    """{name: metric(pred, truth)}; the metrics of this module share one pass over ``pred``."""
    out, scores = {}, None
    for name, fn in metrics.items():
        if fn in _SHARED and _fits(pred, truth):
            if scores is None:
                scores = stats.forecast_scores(pred, truth)
            out[name] = _SHARED[fn](scores, truth)
        else:
            out[name] = fn(pred, truth)
    return out


def _windows(duration, train_window, min_train_window, test_window, min_test_window, stride):
    """(t0, t1, t2) of every window: training on [t0, t1), testing on [t1, t2).  A fixed ``train_window`` slides with
    the split, otherwise training starts at 0; a fixed ``test_window`` ends the test there, otherwise it runs to the
    end of the data."""
    first = min_train_window if train_window is None else train_window
    shortest_test = min_test_window if test_window is None else test_window
    for split in range(first, duration - shortest_test + 1, stride):
        begin = 0 if train_window is None else split - train_window
        end = duration if test_window is None else split + test_window
        if not 0 <= begin < split < end <= duration:
            raise ValueError("window [{}, {}, {}] does not fit {} steps".format(begin, split, end, duration))
        yield begin, split, end


def _forecast(forecaster, data, covariates, num_samples, batch_size):
    """(the forecast, the batch size it was drawn with): a batch that does not fit the device is halved until it
    does."""
    while True:
        try:
            return forecaster(data, covariates, num_samples=num_samples, batch_size=batch_size), batch_size
        except RuntimeError as error:
            if "out of memory" not in str(error) or batch_size is None or batch_size <= 1:
                raise
            batch_size = (batch_size + 1) // 2
            warnings.warn("the forecast ran out of memory: drawing {} samples at a time".format(batch_size),
                          RuntimeWarning)


def backtest(data, covariates, model_fn, *, forecaster_fn=Forecaster, metrics=None, transform=None,
             train_window=None, min_train_window=1, test_window=None, min_test_window=1, stride=1,
             seed=1234567890, num_samples=100, batch_size=None, forecaster_options={}):
    """Trains and scores ``model_fn()`` on a moving (train, test) window over ``data`` [..., duration, obs] and
    ``covariates`` [..., duration, features].  Keywords as the reference's: ``forecaster_fn(model, data, covariates,
    **options)`` builds the forecaster; ``forecaster_options`` is a dict or a callable of ``t0, t1, t2`` returning one;
    ``metrics`` maps names to functions of ``(pred, truth)``; ``transform(pred, truth)`` is applied before them.
    -> a list with one dict per window: "t0", "t1", "t2" (train begin, split, test end), "seed", "num_samples",
    "train_walltime", "test_walltime", "params" (the scalar parameters of the param store) and one entry per metric."""
    duration = data.size(-2)
    if covariates.size(-2) != duration:
        raise ValueError("data and covariates differ in duration: {} against {}".format(duration, covariates.size(-2)))
    for name, value in (("min_train_window", min_train_window), ("min_test_window", min_test_window)):
        if not isinstance(value, int) or value < 1:
            raise ValueError("{} must be a positive int, got {!r}".format(name, value))
    metrics = DEFAULT_METRICS if metrics is None else metrics
    if not metrics:
        raise ValueError("backtest needs at least one metric")
    options_for = forecaster_options if callable(forecaster_options) else (lambda **window: forecaster_options)
    if train_window is not None and options_for().get("warm_start"):
        raise ValueError("a warm start needs a training window that grows: pass train_window=None or warm_start=False")

    records = []
    primitives.clear_param_store()
    for t0, t1, t2 in _windows(duration, train_window, min_train_window, test_window, min_test_window, stride):
        logger.info("window %d: train on [%d, %d), test on [%d, %d)", len(records), t0, t1, t1, t2)
        options = options_for(t0=t0, t1=t1, t2=t2)
        primitives.set_rng_seed(seed)
        if not options.get("warm_start"):
            primitives.clear_param_store()
        train = (data[..., t0:t1, :], covariates[..., t0:t1, :])
        clock = default_timer()
        forecaster = forecaster_fn(model_fn(), *train, **options)
        train_walltime = default_timer() - clock
        clock = default_timer()
        pred, batch_size = _forecast(forecaster, train[0], covariates[..., t0:t2, :], num_samples, batch_size)
        test_walltime = default_timer() - clock
        del forecaster                               # sample forecasts are large: nothing else should stay alive
        truth = data[..., t1:t2, :]
        if transform is not None:
            pred, truth = transform(pred, truth)
        record = dict(t0=t0, t1=t1, t2=t2, seed=seed, num_samples=num_samples, train_walltime=train_walltime,
                      test_walltime=test_walltime,
                      params={name: value.cpu().item() for name, value in primitives.get_param_store().items()
                              if value.numel() == 1})
        record.update(_evaluate(metrics, pred, truth))
        del pred
        records.append(record)
        logger.debug("window %d: %s", len(records) - 1,
                     {k: v for k, v in {**record["params"], **record}.items() if isinstance(v, (int, float))})
    return records
