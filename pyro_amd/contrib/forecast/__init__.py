"""Forecasting with state-space noise models (reference: pyro/contrib/forecast): ForecastingModel, Forecaster, the
scores and the backtest."""
from .evaluate import backtest, eval_crps, eval_mae, eval_rmse
from .forecaster import Forecaster, ForecastingModel

__all__ = ["Forecaster", "ForecastingModel", "backtest", "eval_crps", "eval_mae", "eval_rmse"]
