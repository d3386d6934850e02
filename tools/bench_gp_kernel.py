"""Gaussian-process covariance matrices and models under a gradient (developer tool; not part of bench.py), by the two
routes of the same tree:
    kernel   csrc/gp_kernel.hip: one launch forward, one pass over dL/dK per side backward
    torch    ``kernels.FUSED_GP_KERNEL = False``: the reference's expansion in torch operators (the baseline: the parent
             commit has no GP route at all)

    python tools/bench_gp_kernel.py [--iters 5] [--only covariance|sgpr|gpr]

covariance   K(Xu, X) forward plus backward, Matern52 with ARD lengthscales, [512, 8] against [100000, 8], f32
sgpr         one differentiable_loss + backward of SparseGPRegression, N = 1e5, M = 512, D = 8, f32, VFE
gpr          one differentiable_loss + backward of GPRegression, N = 4096, D = 8, f32 and f64

Per route: milliseconds per step as the median of 5 blocks after one warm-up block, with the fastest and slowest
block (a block is ``--iters`` steps and ends with a device synchronisation), and ``peak_mib``: the allocator's peak
during one step above what was allocated before it (the inputs and parameters).  One line of JSON per case."""
import argparse
import json
import statistics
import sys
import time

import torch

sys.path.insert(0, ".")
import pyro_amd as pyro  # noqa: E402
import pyro_amd.contrib.gp as gp  # noqa: E402
from pyro_amd.infer import Trace_ELBO  # noqa: E402


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
        ts.append((time.perf_counter() - t0) * 1e3 / iters)
    return {"median": round(statistics.median(ts), 3), "min": round(min(ts), 3), "max": round(max(ts), 3)}


def peak_mib(fn):
    fn()
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1)


def both_routes(out, step, iters):
    for route, fused in (("kernel", True), ("torch", False)):
        gp.kernels.FUSED_GP_KERNEL = fused
        try:
            out[route + "_ms"] = blocks(step, iters)
            out[route + "_peak_mib"] = peak_mib(step)
        finally:
            gp.kernels.FUSED_GP_KERNEL = True
    print(json.dumps(out), flush=True)


def data(N, D, dtype, dev):
    gen = torch.Generator(device=dev).manual_seed(0)
    X = torch.randn(N, D, generator=gen, dtype=dtype, device=dev)
    y = torch.sin(X[:, 0]) + 0.1 * torch.randn(N, generator=gen, dtype=dtype, device=dev)
    return X, y


def covariance(iters, dev):
    dtype = torch.float32
    X, _ = data(100000, 8, dtype, dev)
    Xu = X[::195][:512].clone().requires_grad_()
    kern = gp.kernels.Matern52(8, lengthscale=torch.linspace(0.5, 2.0, 8, dtype=dtype)).to(dev)
    w = torch.randn(512, 100000, dtype=dtype, device=dev)

    def step():
        Xu.grad = None
        for p in kern.parameters():
            p.grad = None
        (kern(Xu, X) * w).sum().backward()

    both_routes({"case": "covariance", "family": "matern52", "shape": [512, 100000, 8], "dtype": "float32"}, step, iters)


def model_step(model):
    elbo = Trace_ELBO()

    def step():
        for p in model.parameters():
            p.grad = None
        elbo.differentiable_loss(model.model, model.guide).backward()
    return step


def sgpr(iters, dev):
    dtype = torch.float32
    X, y = data(100000, 8, dtype, dev)
    pyro.clear_param_store()
    kern = gp.kernels.RBF(8, lengthscale=torch.ones(8, dtype=dtype)).to(dev)
    model = gp.models.SparseGPRegression(X, y, kern, X[::195][:512].clone(), noise=torch.tensor(0.1, dtype=dtype, device=dev),
                                         approx="VFE", jitter=1e-4)
    both_routes({"case": "sgpr", "approx": "VFE", "N": 100000, "M": 512, "D": 8, "dtype": "float32"}, model_step(model), iters)


def gpr(iters, dev):
    for dtype in (torch.float32, torch.float64):
        X, y = data(4096, 8, dtype, dev)
        pyro.clear_param_store()
        kern = gp.kernels.RBF(8, lengthscale=torch.ones(8, dtype=dtype)).to(dev)
        model = gp.models.GPRegression(X, y, kern, noise=torch.tensor(0.1, dtype=dtype, device=dev),
                                       jitter=1e-4 if dtype == torch.float32 else 1e-6)
        both_routes({"case": "gpr", "N": 4096, "D": 8, "dtype": str(dtype).replace("torch.", "")}, model_step(model), iters)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--only", choices=["covariance", "sgpr", "gpr"])
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    for name, fn in (("covariance", covariance), ("sgpr", sgpr), ("gpr", gpr)):
        if args.only in (None, name):
            fn(args.iters, dev)


if __name__ == "__main__":
    main()
