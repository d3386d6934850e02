"""The time transforms under a gradient (developer tool): one forward plus backward of ``idct`` and of
``inverse_haar_transform`` along dim -2 -- what a time reparameteriser runs in every evaluation of a model -- at
    [1, 512, 4]   [1024, 512, 4]   [1, 2048, 4]   [64, 2048, 4]        f32 and f64
by three routes of the same tree:
    kernel   csrc/time_transform.hip: one launch forward, one backward
    torch    ``tensor_utils.FUSED_TIME_TRANSFORM = False`` (the baseline: the parent commit has no such function)
    matmul   the DCT only: a product with the [N, N] cosine matrix, built once outside the timed region

    python tools/bench_time_transform.py [--shape O:N:I ...] [--iters 20]
    python tools/bench_time_transform.py --end-to-end

Per route: microseconds per forward-plus-backward as the median of 5 blocks after one warm-up block, with the fastest
and slowest block; a block is ``--iters`` iterations and ends with a device synchronisation, so a number covers the
host work, every launch and the device time.  ``launches``: device kernels of one forward plus backward, counted by
torch.profiler.  One line of JSON per (op, shape, dtype).

``--end-to-end``, a run of its own: one evaluation of the log-density and its gradient of a tiny forecasting model with
T = 512 steps and three time-local latents under ``poutine.reparam(config=time_reparam_dct)``, kernel route against
torch route."""
import argparse
import json
import math
import statistics
import sys
import time

import torch

sys.path.insert(0, ".")
from pyro_amd.ops import tensor_utils  # noqa: E402


def blocks(fn, iters, nblk=5):
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(nblk):
        t0 = time.perf_counter()
        for _ in range(iters):
            fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e6 / iters)
    return {"median": round(statistics.median(ts), 1), "min": round(min(ts), 1), "max": round(max(ts), 1)}


def launches(fn):
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA)


def cosine_matrix(n, dtype, dev):
    """C[k, j] = s_k cos(pi (2j + 1) k / 2n) in float64, rounded once: dct(x) = C x, idct(y) = C^T y."""
    k = torch.arange(n, dtype=torch.float64, device=dev).unsqueeze(-1)
    j = torch.arange(n, dtype=torch.float64, device=dev)
    c = torch.cos(math.pi * (2 * j + 1) * k / (2 * n)) * math.sqrt(2.0 / n)
    c[0] *= math.sqrt(0.5)
    return c.to(dtype)


def one(op, outer, n, inner, dtype, iters, dev):
    gen = torch.Generator(device=dev).manual_seed(0)
    x = torch.randn(outer, n, inner, generator=gen, dtype=dtype, device=dev, requires_grad=True)
    w = torch.randn(outer, n, inner, generator=gen, dtype=dtype, device=dev)
    fn = getattr(tensor_utils, op)

    def step():
        x.grad = None
        (fn(x, dim=-2) * w).sum().backward()

    out = {"op": op, "shape": [outer, n, inner], "dtype": str(dtype).replace("torch.", "")}
    for route, fused in (("kernel", True), ("torch", False)):
        tensor_utils.FUSED_TIME_TRANSFORM = fused
        try:
            out[route + "_us"] = blocks(step, iters)
            out[route + "_launches"] = launches(step)
        finally:
            tensor_utils.FUSED_TIME_TRANSFORM = True
    if op == "idct":
        ct = cosine_matrix(n, dtype, dev).t().contiguous()

        def matmul_step():
            x.grad = None
            (torch.matmul(ct, x) * w).sum().backward()
        out["matmul_us"] = blocks(matmul_step, iters)
        out["matmul_launches"] = launches(matmul_step)
        out["matmul_matrix_mib"] = round(ct.numel() * ct.element_size() / 2 ** 20, 2)
    print(json.dumps(out), flush=True)


def end_to_end(iters, dev):
    import pyro_amd as pyro
    import pyro_amd.distributions as dist
    from pyro_amd import poutine
    from pyro_amd.contrib.forecast import ForecastingModel, util

    T, OBS = 512, 2
    torch.set_default_dtype(torch.float64)

    class Model(ForecastingModel):
        def model(self, zero_data, covariates):
            with self.time_plate:
                drift = pyro.sample("drift", dist.Normal(zero_data, 0.1).to_event(1))
                level = pyro.sample("level", dist.Normal(zero_data, 1.0).to_event(1))
                season = pyro.sample("season", dist.Normal(zero_data, 0.5).to_event(1))
            self.predict(dist.Normal(zero_data, 0.5), drift.cumsum(-2) + level + season)

    gen = torch.Generator(device=dev).manual_seed(0)
    data = torch.randn(T, OBS, generator=gen, device=dev)
    cov = torch.zeros(T, 0, device=dev)
    model = poutine.reparam(Model(), config=util.time_reparam_dct)
    z = {name + "_dct": torch.randn(1, T, OBS, generator=gen, device=dev, requires_grad=True)
         for name in ("drift", "level", "season")}

    def step():
        tr = poutine.trace(poutine.condition(model, data=z)).get_trace(data, cov)
        return torch.autograd.grad(tr.log_prob_sum(), list(z.values()))

    out = {"end_to_end": "log-density and gradient, T=512, 3 time-local latents, time_reparam_dct, f64"}
    for route, fused in (("kernel", True), ("torch", False)):
        tensor_utils.FUSED_TIME_TRANSFORM = fused
        try:
            out[route + "_us"] = blocks(step, iters)
            out[route + "_launches"] = launches(step)
        finally:
            tensor_utils.FUSED_TIME_TRANSFORM = True
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", nargs="+", default=["1:512:4", "1024:512:4", "1:2048:4", "64:2048:4"])
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--end-to-end", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    if args.end_to_end:
        return end_to_end(args.iters, dev)
    for shape in args.shape:
        outer, n, inner = (int(v) for v in shape.split(":"))
        for dtype in (torch.float32, torch.float64):
            for op in ("idct", "inverse_haar_transform"):
                one(op, outer, n, inner, dtype, args.iters, dev)


if __name__ == "__main__":
    main()
