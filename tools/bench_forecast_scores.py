"""Scoring a sample forecast (developer tool): one call each of eval_mae, eval_rmse and eval_crps of
pyro_amd.contrib.forecast on ``pred`` [S, 336, 2500] against ``truth`` [336, 2500] -- 336 steps ahead for 2500
series -- at
    S = 100, f32      S = 1000, f32      S = 100, f64
by the kernel (csrc/forecast_scores.hip: one launch per call, ``pred`` read once) and with
``stats.FUSED_FORECAST_SCORES = False`` in the same tree (the same-tree baseline: the reference's torch formulas --
a sort along the sample axis for the crps, a median selection for the mae, a mean for the rmse).

    python tools/bench_forecast_scores.py [--shape S:dtype ...] [--columns 336:2500]

Per route: milliseconds for the three calls together as the median of 5 blocks after one warm-up block, with the
fastest and slowest block; a block is the three calls and ends where the last score has reached the host (each eval_*
returns a float), so a number covers the host work, every launch and the device time.  Peak memory: what torch's
allocator held at most during one block, above what ``pred`` and ``truth`` occupy.  ``one_launch_ms``: the kernel
alone, from device events around kernels.forecast_scores (5 blocks of five: median, fastest, slowest), and the rate
``pred`` is read at.  ``backtest_window_ms``: what evaluate.backtest spends per window on its three default metrics
(ONE launch shared by the three).  One line of JSON per shape."""
import argparse
import json
import statistics
import sys
import time

import torch

sys.path.insert(0, ".")
from pyro_amd import kernels  # noqa: E402
from pyro_amd.contrib.forecast import evaluate  # noqa: E402
from pyro_amd.ops import stats  # noqa: E402


def blocks(fn, nblk=5):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(nblk):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return {"median": round(statistics.median(ts), 3), "min": round(min(ts), 3), "max": round(max(ts), 3)}


def device_ms(fn, per=5, nblk=5):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(nblk):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(per):
            fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) / per)
    return ts


def one_shape(S, name, steps, series, dev):
    dtype = torch.float32 if name == "f32" else torch.float64
    gen = torch.Generator(device=dev).manual_seed(0)
    pred = torch.randn(S, steps, series, generator=gen, dtype=dtype, device=dev)
    truth = torch.randn(steps, series, generator=gen, dtype=dtype, device=dev)

    def three():
        return evaluate.eval_mae(pred, truth), evaluate.eval_rmse(pred, truth), evaluate.eval_crps(pred, truth)

    out = {"shape": {"S": S, "M": steps * series}, "dtype": name, "pred_mib": round(pred.numel() * pred.element_size() / 2 ** 20, 1)}
    results = {}
    for route, fused in (("kernel", True), ("same_tree_torch", False)):
        stats.FUSED_FORECAST_SCORES = fused
        try:
            out[route + "_ms"] = blocks(three)
            torch.cuda.synchronize()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            results[route] = three()
            torch.cuda.synchronize()
            out[route + "_peak_mib"] = round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1)
        finally:
            stats.FUSED_FORECAST_SCORES = True
        torch.cuda.empty_cache()
    out["speedup"] = round(out["same_tree_torch_ms"]["median"] / out["kernel_ms"]["median"], 2)
    out["scores"] = {k: [round(v, 7) for v in vs] for k, vs in results.items()}
    flat, y = pred.reshape(S, -1), truth.reshape(-1)
    ts = device_ms(lambda: kernels.forecast_scores(flat, y))
    out["one_launch_ms"] = {"median": round(statistics.median(ts), 3), "min": round(min(ts), 3), "max": round(max(ts), 3)}
    out["one_launch_gbps"] = round(flat.numel() * flat.element_size() / statistics.median(ts) / 1e6, 1)
    out["backtest_window_ms"] = blocks(lambda: evaluate._evaluate(evaluate.DEFAULT_METRICS, pred, truth))
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", nargs="+", default=["100:f32", "1000:f32", "100:f64"])
    ap.add_argument("--columns", default="336:2500")
    args = ap.parse_args()
    steps, series = (int(v) for v in args.columns.split(":"))
    dev = torch.device("cuda:0")
    for shape in args.shape:
        S, name = shape.split(":")
        one_shape(int(S), name, steps, series, dev)


if __name__ == "__main__":
    main()
