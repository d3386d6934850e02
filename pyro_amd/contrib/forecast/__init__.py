"""Forecasting with state-space noise models (reference: pyro/contrib/forecast): ForecastingModel, Forecaster,
HMCForecaster, the scores and the backtest; ``util.time_reparam_dct`` / ``util.time_reparam_haar`` are the configs
that sample time-local latents in a frequency or wavelet basis."""
from .evaluate import backtest, eval_crps, eval_mae, eval_rmse
from .forecaster import Forecaster, ForecastingModel, HMCForecaster

__all__ = ["Forecaster", "ForecastingModel", "HMCForecaster", "backtest", "eval_crps", "eval_mae", "eval_rmse"]
