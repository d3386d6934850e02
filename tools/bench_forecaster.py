"""Training and forecasting through contrib.forecast (developer tool, report only): B = 256 series of T = 512 steps,
obs 4, a GaussianHMM noise model with hidden 8 whose transition and observation scales are latent per series, a bias
and a weight on 2 covariates, AutoNormal guide, f32.

    python tools/bench_forecaster.py [--shape B:T:H:O] [--steps 20] [--ahead 64] [--samples 100]

``train_step_ms``: milliseconds per SVI step (Forecaster's eager steps: model and guide in Python, ONE launch of the
Kalman kernel per step), median of 5 blocks of --steps steps after a first Forecaster that warms everything up, with
the fastest and slowest block.  ``forecast_ms``: one call drawing --samples forecasts --ahead steps ahead (the
filter's launch, then the fused draw), median of 5 calls after one.  ``score_ms``: the three default metrics of that
forecast (one launch).  The same with ``hmm.FUSED_GAUSSIAN_HMM = False`` (the torch loop over T) for one block, as
the same-tree baseline.  One line of JSON."""
import argparse
import json
import statistics
import sys
import time

import torch

sys.path.insert(0, ".")
import pyro_amd as pyro  # noqa: E402
import pyro_amd.distributions as dist  # noqa: E402
from pyro_amd.contrib.forecast import Forecaster, ForecastingModel, evaluate  # noqa: E402
from pyro_amd.distributions import hmm  # noqa: E402


class Model(ForecastingModel):
    def __init__(self, hidden):
        super().__init__()
        self.hidden = hidden

    def model(self, zero_data, covariates):
        B, duration, o = zero_data.shape
        h, f = self.hidden, covariates.size(-1)
        with pyro.plate("series", B, dim=-2):
            slot = zero_data[..., :1, :]                                     # [B, 1, o]
            bias = pyro.sample("bias", dist.Normal(slot, 10.0).to_event(1))
            weight = pyro.sample("weight", dist.Normal(zero_data.new_zeros(B, 1, f, o), 1.0).to_event(2))
            trans_scale = pyro.sample("trans_scale", dist.LogNormal(zero_data.new_full((B, 1, h), -2.0), 1.0).to_event(1))
            obs_scale = pyro.sample("obs_scale", dist.LogNormal(slot - 1.0, 1.0).to_event(1))
            prediction = bias + (covariates.unsqueeze(-1) * weight).sum(-2)
            F = 0.9 * torch.eye(h, dtype=zero_data.dtype, device=zero_data.device)
            H = zero_data.new_ones(h, o) / h
            noise = dist.GaussianHMM(dist.Normal(zero_data.new_zeros(h), 1.0).to_event(1), F,
                                     dist.Normal(zero_data.new_zeros(h), trans_scale).to_event(1), H,
                                     dist.Normal(zero_data.new_zeros(o), obs_scale).to_event(1), duration=duration)
            self.predict(noise, prediction)


def timed(fn, nblk=5):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(nblk):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return ts


def summary(ts, per=1):
    return {"median": round(statistics.median(ts) / per, 3), "min": round(min(ts) / per, 3),
            "max": round(max(ts) / per, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="256:512:8:4")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--ahead", type=int, default=64)
    ap.add_argument("--samples", type=int, default=100)
    args = ap.parse_args()
    B, T, h, o = (int(v) for v in args.shape.split(":"))
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(0)
    cov = torch.randn(T + args.ahead, 2, generator=gen).to(dev)
    data = (cov[:T] @ torch.randn(2, o, generator=gen).to(dev) + 0.3 * torch.randn(B, T, o, generator=gen).to(dev))
    truth = torch.randn(B, args.ahead, o, generator=gen).to(dev)
    out = {"shape": {"B": B, "T": T, "hidden": h, "obs": o}, "dtype": "f32", "steps_per_block": args.steps,
           "ahead": args.ahead, "samples": args.samples}
    keep = {}

    def train():
        pyro.clear_param_store()
        pyro.set_rng_seed(0)
        keep["f"] = Forecaster(Model(h), data, cov[:T], num_steps=args.steps, log_every=0)

    for route, fused in (("kernel", True), ("same_tree_torch", False)):
        hmm.FUSED_GAUSSIAN_HMM = fused
        try:
            out[route + "_train_step_ms"] = summary(timed(train, 5 if fused else 1), args.steps)
            forecast = lambda: keep.__setitem__("pred", keep["f"](data, cov, num_samples=args.samples))  # noqa: E731
            with torch.no_grad():
                out[route + "_forecast_ms"] = summary(timed(forecast, 5 if fused else 1))
        finally:
            hmm.FUSED_GAUSSIAN_HMM = True
    out["losses"] = [round(keep["f"].losses[0], 4), round(keep["f"].losses[-1], 4)]
    pred = keep["pred"]
    out["forecast_shape"] = list(pred.shape)
    out["score_ms"] = summary(timed(lambda: evaluate._evaluate(evaluate.DEFAULT_METRICS, pred, truth)))
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
