"""One GaussianHMM.smooth(x, cross=True) under no_grad (developer tool): the smoothed marginals -- mean, covariance and
lag-one cross covariance of every state -- of B series of T steps, hidden 8, obs 4, time-homogeneous parameters shared
by the series, at the two shapes
    B = 1024, T = 512      (many series)
    B = 1,    T = 512      (one series: the latency of a single wave)
in f32 and f64, three ways:

    kernel            csrc/gaussian_hmm_smooth.hip, one launch, one wave per series
    maps_then_loop    what the tree offered before that kernel for the same result: kernels.gaussian_hmm_sample with
                      S = 0 and need_maps=True (the maps kernel), then the moments of the chain rebuilt from the maps
                      (mu_t = c_t + G_t mu_{t+1}, V_t = G_t V_{t+1} G_t^T + L_t L_t^T, X_t = G_t V_{t+1}) as a loop of
                      torch ops over T on the device
    same_tree_torch   ``hmm.FUSED_GAUSSIAN_HMM = False``: the sequential torch filter and Rauch-Tung-Striebel loop of
                      distributions/hmm.py

    python tools/bench_gaussian_hmm_smooth.py [--shape B:T:H:O ...] [--dtype f32|f64 ...]

Per route: milliseconds per call as the median of 5 blocks after one warm-up call (ten calls per block on the kernel,
one on the two loops), with the fastest and slowest block; each block ends with a device synchronisation, so a number
covers the host work, every launch and the device time.  Peak memory: what torch's allocator held at most during one
call, above what the inputs occupy.  ``kernel_device_ms``: the kernel's own time from device events around
kernels.gaussian_hmm_smooth, median of 5 blocks of ten, with and without the cross covariances.  ``rel_diff``: the
largest gaussian_hmm_cases-style difference between the kernel and each of the other two.  One line of JSON per shape
and dtype."""
import argparse
import json
import statistics
import sys
import time

import torch

sys.path.insert(0, ".")
import pyro_amd.distributions as dist  # noqa: E402
from pyro_amd import kernels  # noqa: E402
from pyro_amd.distributions import hmm  # noqa: E402


def blocks(fn, per, warm=1, nblk=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(nblk):
        t0 = time.perf_counter()
        for _ in range(per):
            fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) / per * 1e3)
    return statistics.median(ts), min(ts), max(ts)


def device_ms(fn, per=10, nblk=5):
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
    return statistics.median(ts)


def inputs(B, T, h, o, dtype, dev):
    """the recipe of tests/golden/make_golden_gaussian_hmm.py"""
    gen = torch.Generator().manual_seed(0)
    r = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64)                    # noqa: E731

    def tril(n):
        A = r(n, n)
        return torch.linalg.cholesky(A @ A.T / n + 0.5 * torch.eye(n, dtype=torch.float64))
    F = r(h, h)
    F = F * (0.9 / torch.linalg.matrix_norm(F, ord=2))
    t = {"m0": 0.3 * r(h), "L0": tril(h), "F": F, "q": 0.3 * r(h), "Lq": tril(h), "H": r(h, o) / h ** 0.5,
         "r": 0.3 * r(o), "Lr": tril(o)}
    t = {k: v.to(dtype).to(dev) for k, v in t.items()}
    return t, (2.0 * r(B, T, o)).to(dtype).to(dev)


def moments_loop(c, G, L):
    """the moments of the chain z_T = c_T + L_T eps_T, z_t = c_t + G_t z_{t+1} + L_t eps_t from its maps [B, T, ...],
    on their device and in their dtype (the recursion of tests/gaussian_hmm_posterior_cases.moments)"""
    T = c.shape[1]
    mu, V = c[:, T - 1], L[:, T - 1] @ L[:, T - 1].transpose(-1, -2)
    mus, Vs, Xs = [mu], [V], []
    for t in range(T - 2, -1, -1):
        Xs.append(G[:, t] @ V)
        mu = c[:, t] + (G[:, t] @ mu.unsqueeze(-1)).squeeze(-1)
        V = G[:, t] @ V @ G[:, t].transpose(-1, -2) + L[:, t] @ L[:, t].transpose(-1, -2)
        mus.append(mu)
        Vs.append(V)
    return torch.stack(mus[::-1], dim=1), torch.stack(Vs[::-1], dim=1), torch.stack(Xs[::-1], dim=1)


def rel_diff(a, b):
    return max(float((u.double() - v.double()).abs().max() / (1 + v.double().abs().max())) for u, v in zip(a, b))


def one_shape(B, T, h, o, name, dev):
    dtype = torch.float32 if name == "f32" else torch.float64
    t, x = inputs(B, T, h, o, dtype, dev)
    d = dist.GaussianHMM(dist.MultivariateNormal(t["m0"], scale_tril=t["L0"]), t["F"],
                         dist.MultivariateNormal(t["q"], scale_tril=t["Lq"]), t["H"],
                         dist.MultivariateNormal(t["r"], scale_tril=t["Lr"]), validate_args=False)
    batch, _ = d._check_value(x)
    args = d._kernel_inputs(x, batch, T)
    none = torch.empty(0, B, T, h, dtype=dtype, device=dev)

    def smooth():
        with torch.no_grad():
            return d.smooth(x, cross=True)

    def maps_then_loop():
        with torch.no_grad():
            return moments_loop(*kernels.gaussian_hmm_sample(*args, none, need_maps=True)[1])

    out = {"shape": {"B": B, "T": T, "hidden": h, "obs": o}, "dtype": name}
    results = {}
    for route, fn, fused in (("kernel", smooth, True), ("maps_then_loop", maps_then_loop, True),
                             ("same_tree_torch", smooth, False)):
        hmm.FUSED_GAUSSIAN_HMM = fused
        try:
            med, lo, hi = blocks(fn, 10 if route == "kernel" else 1)
            torch.cuda.synchronize()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            results[route] = fn()
            torch.cuda.synchronize()
            peak = torch.cuda.max_memory_allocated() - base
        finally:
            hmm.FUSED_GAUSSIAN_HMM = True
        out[route + "_ms"] = {"median": round(med, 3), "min": round(lo, 3), "max": round(hi, 3)}
        out[route + "_peak_mib"] = round(peak / 2 ** 20, 1)
    out["speedup_over_maps_then_loop"] = round(out["maps_then_loop_ms"]["median"] / out["kernel_ms"]["median"], 1)
    out["speedup_over_same_tree_torch"] = round(out["same_tree_torch_ms"]["median"] / out["kernel_ms"]["median"], 1)
    out["rel_diff"] = {k: rel_diff(results["kernel"], results[k]) for k in ("maps_then_loop", "same_tree_torch")}
    out["kernel_device_ms"] = {
        "with_cross": round(device_ms(lambda: kernels.gaussian_hmm_smooth(*args, need_cross=True)), 3),
        "without": round(device_ms(lambda: kernels.gaussian_hmm_smooth(*args)), 3)}
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", nargs="+", default=["1024:512:8:4", "1:512:8:4"])
    ap.add_argument("--dtype", nargs="+", default=["f32", "f64"], choices=("f32", "f64"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    for shape in args.shape:
        B, T, h, o = (int(v) for v in shape.split(":"))
        for name in args.dtype:
            one_shape(B, T, h, o, name, dev)


if __name__ == "__main__":
    main()
