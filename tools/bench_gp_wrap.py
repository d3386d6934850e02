"""Derived Gaussian-process kernels under a gradient (developer tool; not part of bench.py), by the two routes of the same
tree:
    kernel   csrc/gp_wrap.hip: one launch forward, one pass over dL/dK per side backward (``kernels.FUSED_GP_WRAP = True``)
    torch    ``kernels.FUSED_GP_WRAP = False``: the child's own kernel route, then the reference's element-wise torch
             operators on its [N, M] matrix (the parent commit has no such classes to compare against)

    python tools/bench_gp_wrap.py [--iters 5]

Cases: Exponent(RBF), Warping(Matern52, None, [1, 0, 2]) and VerticalScaling(RBF, fn), ARD lengthscales, f32; [4096, 8]
against itself and [512, 8] against [100000, 8].  A step is K, sum(K w) and its backward to the points, the parameters
and fn's weights.  Per route: milliseconds per step as the median of 5 blocks after one warm-up block, with the fastest
and slowest block (a block is ``--iters`` steps and ends with a device synchronisation; the blocks of the two routes
alternate), and ``peak_mib``: the allocator's peak during one step above what was allocated before it (the inputs, the
parameters and w).  One line of JSON per case."""
import argparse
import json
import statistics
import sys
import time

import torch

sys.path.insert(0, ".")
import pyro_amd.contrib.gp as gp  # noqa: E402

ROUTES = (("kernel", True), ("torch", False))


def block(step, iters):
    t0 = time.perf_counter()
    for _ in range(iters):
        step()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / iters


def peak_mib(step):
    step()
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    step()
    torch.cuda.synchronize()
    return round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1)


def measure(out, step, iters, nblk=5):
    times = {route: [] for route, _ in ROUTES}
    try:
        for n in range(nblk + 1):                       # (block 0 warms both routes up)
            for route, fused in ROUTES:
                gp.kernels.FUSED_GP_WRAP = fused
                t = block(step, iters)
                if n:
                    times[route].append(t)
        for route, fused in ROUTES:
            gp.kernels.FUSED_GP_WRAP = fused
            ts = times[route]
            out[route + "_ms"] = {"median": round(statistics.median(ts), 3), "min": round(min(ts), 3), "max": round(max(ts), 3)}
            out[route + "_peak_mib"] = peak_mib(step)
    finally:
        gp.kernels.FUSED_GP_WRAP = True
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    args = ap.parse_args()
    dev, dtype, k = torch.device("cuda:0"), torch.float32, gp.kernels
    gen = torch.Generator(device=dev).manual_seed(0)
    ls = lambda: torch.linspace(0.5, 2.0, 8, dtype=dtype)      # noqa: E731
    v = (0.3 * torch.randn(8, generator=gen, dtype=dtype, device=dev)).requires_grad_()
    fn = lambda x: 1.0 + 0.5 * torch.tanh(x @ v)               # noqa: E731
    trees = {"exponent_rbf": k.Exponent(k.RBF(8, lengthscale=ls())),
             "warping_matern52": k.Warping(k.Matern52(8, lengthscale=ls()), None, [1, 0, 2]),
             "vscaling_rbf": k.VerticalScaling(k.RBF(8, lengthscale=ls()), fn)}
    for name, kern in trees.items():
        kern = kern.to(dev)
        for n, m in ((4096, None), (512, 100000)):
            X = torch.randn(m or n, 8, generator=gen, dtype=dtype, device=dev)
            A, B = X[:n].clone().requires_grad_(), None if m is None else X
            w = torch.randn(n, m or n, generator=gen, dtype=dtype, device=dev)

            def step():
                A.grad = v.grad = None
                for p in kern.parameters():
                    p.grad = None
                (kern(A, B) * w).sum().backward()

            measure({"case": name, "shape": [n, m or n, 8], "z": "given" if m else "x", "dtype": "float32"}, step, args.iters)


if __name__ == "__main__":
    main()
